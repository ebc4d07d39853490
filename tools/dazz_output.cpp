// dazz_output.cpp -- `dentist output` (commands/output.d; tests/test-commands.sh:184-230 ends with it): insertions.db in,
// gap-closed FASTA, AGP and closed-gaps BED out.  An executable of its own (tools/output) over the helpers of the multi-call
// binary: the table of names of dazz_main.cpp stays as the recorded command-line replay knows it.
#include <cmath>

#include "dazz_tools.h"

namespace {
const char *const kUsage =
    "usage: output [--agp=<f>] [--agp-dazzler] [--agp-skip-read-ids] [--closed-gaps-bed=<f>] [--fasta-line-width=<n>] "
    "[--no-highlight-insertions] [--join-policy=scaffoldGaps|scaffolds|contigs] [--only=spanning|extending|both] "
    "[--min-extension-length=<n>] [--max-insertion-error=<f>] [--skip-gaps=<a>-<b>[,...]] [--skip-gaps-file=<f>] "
    "[--revert=<option>[,...]] <ref-db> <reads-db> <insertions.db> [<result.fasta>]";

struct OutputCli {
    std::string agp, bed, skip_gaps_file;
    bool agp_dazzler = false, agp_skip_read_ids = false, highlight = true;
    int32_t line_width = 50, join_policy = 0, only = 1, min_extension_length = 100;
    double max_insertion_error = 0.1;
    std::vector<std::pair<long long, long long>> skip_gaps;  // 1-based contig ids as given
};

// <contigA>-<contigB> (parseGapSpec, commandline.d:2559-2566: "%d-%d" and nothing behind it)
bool parse_gap_spec(const std::string &s, std::pair<long long, long long> &out)
{
    const char *p = s.c_str();
    char *end = nullptr;
    if (!(*p >= '0' && *p <= '9')) return false;
    out.first = strtoll(p, &end, 10);
    if (*end != '-' || !(end[1] >= '0' && end[1] <= '9')) return false;
    out.second = strtoll(end + 1, &end, 10);
    return *end == 0;
}

// --revert=<option>: the named option back to its default (revertOption, commandline.d:2435-2484)
void revert_option(OutputCli &o, const std::string &name)
{
    const OutputCli d;
    if (name == "agp")
        o.agp = d.agp;
    else if (name == "agp-dazzler")
        o.agp_dazzler = d.agp_dazzler;
    else if (name == "agp-skip-read-ids")
        o.agp_skip_read_ids = d.agp_skip_read_ids;
    else if (name == "closed-gaps-bed")
        o.bed = d.bed;
    else if (name == "fasta-line-width" || name == "w")
        o.line_width = d.line_width;
    else if (name == "no-highlight-insertions" || name == "H")
        o.highlight = d.highlight;
    else if (name == "join-policy")
        o.join_policy = d.join_policy;
    else if (name == "only")
        o.only = d.only;
    else if (name == "min-extension-length")
        o.min_extension_length = d.min_extension_length;
    else if (name == "max-insertion-error")
        o.max_insertion_error = d.max_insertion_error;
    else if (name == "skip-gaps")
        o.skip_gaps.clear();
    else if (name == "skip-gaps-file")
        o.skip_gaps_file = d.skip_gaps_file;
    else if (name == "scaffolding")
        ;  // (known to the reference; never set here)
    else
        fail("invalid value for --revert: unknown option " + std::string(name.size() > 1 ? "--" : "-") + name);
}

// the name of read i in the AGP: the first word of its FASTA header (output.d:284-290)
std::string read_name(const dh_dazz *d, int32_t i, bool dam)
{
    std::string s = dh_dazz_header(d, i);
    if (!s.empty() && s[0] == '>') s.erase(0, 1);
    const size_t e = s.find_first_of(" \t\n");
    if (e != std::string::npos) s.resize(e);
    if (!dam)  // a .db keeps the prolog only: <prolog>/<well>/<begin>_<end> (dazzler.d:1389-1393)
        s += "/" + std::to_string(dh_dazz_origin(d)[i]) + "/" + std::to_string(dh_dazz_fpulse(d)[i]) + "_" +
             std::to_string(dh_dazz_fpulse(d)[i] + (dh_dazz_offsets(d)[i + 1] - dh_dazz_offsets(d)[i]));
    return s;
}
}  // namespace

// ---------------------------------------------------------------------------------- output
// `dentist output`: dh_dazz_open (both DBs, trimmed view) -> dh_db_create -> dh_insertions_from_db -> dh_output_db, which
// formats the FASTA on the device.  The scaffolds, their headers and the gap lengths come from the .dam (getScaffoldStructure);
// the read names only when the AGP needs them.  The options are read first, --revert acts on them afterwards, the gap specs
// are checked against the .dam before a device is opened.
int tool_output(const Args &args)
{
    OutputCli o;
    Args pos, reverts;
    std::string v_width, v_minext, v_err, v;
    bool ignored = false;
    auto list_of = [](const std::string &s) {
        Args out;
        size_t at = 0;
        while (at <= s.size()) {
            const size_t comma = std::min(s.find(',', at), s.size());
            out.push_back(s.substr(at, comma - at));
            at = comma + 1;
        }
        return out;
    };
    for (const std::string &a : args) {
        if (long_value(a, "--agp=", &o.agp) || long_value(a, "--closed-gaps-bed=", &o.bed) || long_value(a, "--fasta-line-width=", &v_width) ||
            short_value(a, 'w', &v_width) || long_value(a, "--min-extension-length=", &v_minext) || long_value(a, "--max-insertion-error=", &v_err) ||
            long_value(a, "--skip-gaps-file=", &o.skip_gaps_file))
            continue;
        else if (a == "--agp-dazzler")
            o.agp_dazzler = true;
        else if (a == "--agp-skip-read-ids")
            o.agp_skip_read_ids = true;
        else if (a == "--no-highlight-insertions" || a == "-H")
            o.highlight = false;
        else if (long_value(a, "--join-policy=", &v)) {
            if (v == "scaffoldGaps")
                o.join_policy = 0;
            else if (v == "scaffolds")
                o.join_policy = 1;
            else if (v == "contigs")
                o.join_policy = 2;
            else
                die("unknown or malformed option " + a + "\n" + kUsage);
        } else if (long_value(a, "--only=", &v)) {
            if (v == "spanning")
                o.only = 1;
            else if (v == "extending")
                o.only = 2;
            else if (v == "both")
                o.only = 3;
            else
                die("unknown or malformed option " + a + "\n" + kUsage);
        } else if (long_value(a, "--skip-gaps=", &v)) {
            for (const std::string &spec : list_of(v)) {
                std::pair<long long, long long> g;
                if (!parse_gap_spec(spec, g)) fail("ill-formatted <gap-spec> (" + spec + "): should be <contigA>-<contigB>");
                o.skip_gaps.push_back(g);
            }
        } else if (long_value(a, "--revert=", &v)) {
            for (const std::string &name : list_of(v)) reverts.push_back(name);
        } else if (long_value(a, "--scaffolding="))
            fail("--scaffolding (the assembly graph as an insertions.db) is not built");
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + kUsage);
        else
            pos.push_back(a);
    }
    if (pos.size() < 3 || pos.size() > 4) die(kUsage);
    if (ignored) notice_ignored();
    lenient_number(v_width, &o.line_width), lenient_number(v_minext, &o.min_extension_length), lenient_number(v_err, &o.max_insertion_error);
    // the reference reverts in a PreValidate hook, behind the parser: an option that is given and reverted ends reverted
    for (const std::string &name : reverts) revert_option(o, name);
    if (!(o.max_insertion_error >= 0 && o.max_insertion_error <= 1)) fail("--max-insertion-error must lie in [0, 1]");
    if (o.min_extension_length < 0) fail("--min-extension-length must not be negative");
    if (!o.skip_gaps_file.empty()) {  // hookReadSkipGapsFile, commandline.d:2542-2556
        FILE *f = fopen(o.skip_gaps_file.c_str(), "r");
        if (!f) fail("cannot open " + o.skip_gaps_file);
        const std::string text = slurp(f);
        fclose(f);
        size_t at = 0;
        for (int line = 1; at < text.size(); line++) {
            const size_t nl = std::min(text.find('\n', at), text.size());
            const std::string spec = text.substr(at, nl - at);
            at = nl + 1;
            if (spec.empty() || spec[0] == '#') continue;
            std::pair<long long, long long> g;
            if (!parse_gap_spec(spec, g))
                fail("ill-formatted <gap-spec> (" + spec + ") in " + o.skip_gaps_file + ":" + std::to_string(line) + ": should be <contigA>-<contigB>");
            o.skip_gaps.push_back(g);
        }
    }
    Dazz da;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    const int32_t ncontigs = dh_dazz_nreads(da.get());
    std::vector<int32_t> skip2;
    for (const auto &g : o.skip_gaps) {  // validatePileUpSkipGap, commandline.d:2578-2596; hookSortSkipGaps :2598-2604
        if (!(0 < g.first && g.first <= ncontigs))
            fail("invalid <gap-spec>: <contigA> == " + std::to_string(g.first) + " is out of bounds [1, " + std::to_string(ncontigs) + "]");
        if (!(0 < g.second && g.second <= ncontigs))
            fail("invalid <gap-spec>: <contigB> == " + std::to_string(g.second) + " is out of bounds [1, " + std::to_string(ncontigs) + "]");
        if (g.first == g.second) fail("invalid <gap-spec>: <contigA> mut not be equal to <contigB>");
        skip2.push_back((int32_t)std::min(g.first, g.second) - 1);
        skip2.push_back((int32_t)std::max(g.first, g.second) - 1);
    }
    Dazz dr;
    must(dh_dazz_open(pos[1].c_str(), into(dr)));
    // the scaffolds of the .dam: contigs that follow each other under one header; the gap behind a contig from the positions
    const int64_t *off = dh_dazz_offsets(da.get());
    std::vector<int32_t> scaffold_of((size_t)std::max(ncontigs, 1), 0), gap_len((size_t)std::max(ncontigs, 1), 0);
    std::vector<std::string> header_text;
    for (int32_t c = 0; c < ncontigs; c++) {
        if (c == 0 || !scaffold_neighbours(da.get(), c - 1)) {
            std::string h = dh_dazz_header(da.get(), c);
            if (!h.empty() && h[0] == '>') h.erase(0, 1);
            header_text.push_back(h);
        } else
            gap_len[(size_t)c - 1] = dh_dazz_fpulse(da.get())[c] - (int32_t)(dh_dazz_fpulse(da.get())[c - 1] + (off[c] - off[c - 1]));
        scaffold_of[(size_t)c] = (int32_t)header_text.size() - 1;
    }
    std::vector<const char *> headers;
    for (const std::string &h : header_text) headers.push_back(h.c_str());
    if (headers.empty()) headers.push_back("");
    const bool want_names = !o.agp.empty() && !o.agp_dazzler && !o.agp_skip_read_ids;
    const int32_t nreads = dh_dazz_nreads(dr.get());
    std::vector<std::string> name_text;
    std::vector<const char *> names;
    if (want_names) {
        const bool dam = parse_db_path(pos[1]).ext == "dam";
        for (int32_t i = 0; i < nreads; i++) name_text.push_back(read_name(dr.get(), i, dam));
        for (const std::string &s : name_text) names.push_back(s.c_str());
    }
    Handle<dh_insertions, dh_insertions_destroy> ins;
    must(dh_insertions_from_db(pos[2].c_str(), off, ncontigs, into(ins)));
    Ctx ctx;
    must(dh_ctx_create(0, nullptr, into(ctx)));
    Db A;
    must(dh_db_create(ctx.get(), dh_dazz_bases(da.get()), off, ncontigs, nullptr, into(A)));
    dh_output_opts oo;
    dh_default_output_opts(&oo);
    oo.line_width = o.line_width, oo.highlight = o.highlight ? 1 : 0, oo.join_policy = o.join_policy, oo.only = o.only;
    oo.agp_dazzler = o.agp_dazzler ? 1 : 0, oo.agp_skip_read_ids = o.agp_skip_read_ids ? 1 : 0, oo.min_extension_length = o.min_extension_length;
    oo.input_assembly = pos[0].c_str();
    dh_output_filter flt;
    // (0 means "no cut" to the library; a limit of 0 keeps error-free overlaps only, which 1 ppm does for any overlap below 1 Mb)
    flt.max_insertion_error_ppm = std::max<int32_t>((int32_t)llround(o.max_insertion_error * 1e6), 1);
    flt.nskip = (int32_t)skip2.size() / 2;
    flt.skip_gaps2 = skip2.empty() ? nullptr : skip2.data();
    int32_t dropped = 0;
    must(dh_output_db(ctx.get(), A.get(), pos.size() == 4 ? pos[3].c_str() : nullptr, o.bed.empty() ? nullptr : o.bed.c_str(),
                      o.agp.empty() ? nullptr : o.agp.c_str(), scaffold_of.data(), headers.data(), gap_len.data(), ins.get(),
                      want_names ? nreads : (nreads > 0 ? nreads : -1), want_names ? names.data() : nullptr, &oo, &flt, &dropped));
    if (dropped) fprintf(stderr, "output: the join policy skipped %d insertion(s)\n", dropped);
    return 0;
}

int main(int argc, char **argv)
{
    g_tool = "output";
    return tool_output(Args(argv + 1, argv + argc));
}
