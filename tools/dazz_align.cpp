// dazz_align.cpp -- the tools that show or compute base-level alignments (LApaf, LAtranspose, DBnw, stretcher) and exact
// matches (fm-index).
#include <sys/stat.h>

#include "dazz_tools.h"

// a trailing `first-last` (or `n`) behind at least two positionals: taken off `pos`; r1 stays -1 without one
static void pop_range(Args &pos, const char *what, long long *r0, long long *r1)
{
    if (pos.size() < 3 || pos.back().find_first_not_of("0123456789-") != std::string::npos) return;
    if (sscanf(pos.back().c_str(), "%lld-%lld", r0, r1) != 2) {
        if (sscanf(pos.back().c_str(), "%lld", r0) != 1) die(std::string("bad ") + what + " range " + pos.back());
        *r1 = *r0;
    }
    pos.pop_back();
}

// the extended cigar (= X I D) of an edit path, in `text`
static const char *cigar_text(const uint8_t *o, int64_t no, std::vector<char> &text)
{
    const int64_t clen = dh_format_cigar(o, no, 1, nullptr, 0);
    if (clen < 0) die(dh_last_error());
    text.resize((size_t)clen + 1);
    text[0] = 0;
    dh_format_cigar(o, no, 1, text.data(), clen + 1);
    return text.data();
}

// -a: the alignment text of dh_format_alignment, every line prefixed '#'
static void print_alignment(const uint8_t *a, const uint8_t *b, const uint8_t *o, int64_t no, int width, std::vector<char> &text)
{
    const int64_t tl = dh_format_alignment(a, b, o, no, width, nullptr, 0);
    if (tl < 0) die(dh_last_error());
    text.resize((size_t)tl + 1);
    text[0] = 0;
    dh_format_alignment(a, b, o, no, width, text.data(), tl + 1);
    putchar('#');
    for (int64_t k = 0; k < tl; k++) {
        putchar(text[(size_t)k]);
        if (text[(size_t)k] == '\n') putchar('#');
    }
    putchar('\n');
}

// ---------------------------------------------------------------------------------- LApaf
// LApaf [-a] [-c] [-w<int(100)>] <A:db|dam> [<B:db|dam>] <align:las> [first-last]: base-level alignments of the records of a
// .las as PAF with an extended cigar (dh_la_edit_paths: getExactAlignment's per-trace-point part, dazzler.d:2405-2426); -a adds
// the alignment text (SequenceAlignment.toString).
// One PAF line per record: the query is the B read (strand '-' and coordinates turned back to the forward strand for
// complement records), the target the A sequence; names are the first word of the FASTA header (DAM) or the prolog (DB)
// followed by /<1-based read number>.  Tags: NM:i the exact edit distance summed over the trace tiles, tp:i the sum of the
// trace's diffs (what the aligner's band found), cg:Z the extended cigar (= X I D).
// -c: one line per CHAIN of the file (a record without the NEXT flag starts a chain, file order), from dh_la_chain_paths: the
// query range is the chain's B range, the target range its A range; NM:i the non-zero ops, nl:i the records of the chain, nf:i
// the fillers aligned between them, cg:Z the cigar of the whole chain; fk:i:1 on a chain with a faked filler; a nested chain
// prints 0 matches, * for the cigar and st:Z:nested.  first-last counts chains then.
static std::string paf_name(const dh_dazz *d, int32_t i)
{
    const char *h = dh_dazz_header(d, i);
    std::string s = h ? h : "";
    if (!s.empty() && s[0] == '>') s.erase(0, 1);
    const size_t e = s.find_first_of(" \t\n");
    if (e != std::string::npos) s.resize(e);
    if (s.empty()) s = "read";
    return s + "/" + std::to_string(dh_dazz_first_id(d) + i + 1);
}

int tool_lapaf(const Args &args)
{
    bool show = false, chains = false;
    int width = 100;
    Args pos;
    for (const std::string &a : args) {
        if (a == "-a")
            show = true;
        else if (a == "-c")
            chains = true;
        else if (a.compare(0, 2, "-w") == 0)
            width = atoi(a.c_str() + 2);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    long long r0 = 1, r1 = -1;
    pop_range(pos, "record", &r0, &r1);
    if (pos.size() < 2 || pos.size() > 3 || width < 1) die("usage: LApaf [-a] [-c] [-w<int(100)>] <A:db|dam> [<B:db|dam>] <align:las> [first-last]");
    const Dev va(pos[0]);
    std::unique_ptr<Dev> second;
    if (pos.size() == 3 && pos[1] != pos[0]) second.reset(new Dev(va.ctx, pos[1]));
    const Dev &vb = second ? *second : va;
    const dh_dazz *da = va.dz.get(), *dbz = vb.dz.get();
    const LaSet set = read_las(pos.back());
    const std::vector<dh_la> las = shifted_records(set.get(), dh_dazz_first_id(da), dh_dazz_first_id(dbz));
    const int64_t n = (int64_t)las.size();
    // the entries of the output: records, or (-c) chains by flags as record ranges
    std::vector<int64_t> coff;
    if (chains) {
        for (int64_t i = 0; i < n; i++)
            if (i == 0 || !(las[(size_t)i].flags & DH_FLAG_NEXT)) coff.push_back(i);
        coff.push_back(n);
    }
    const int64_t nent = chains ? (int64_t)coff.size() - 1 : n;
    if (r1 < 0) r1 = nent;
    if (r0 < 1 || r1 > nent || r0 > r1 + 1)
        die(std::string(chains ? "chain" : "record") + " range outside the file (" + std::to_string(nent) + (chains ? " chains)" : " records)"));
    const uint16_t *trace = dh_la_set_trace(set.get());
    const int32_t ts = dh_la_set_tspace(set.get());
    EditPaths ep;
    std::vector<int32_t> cstatus;
    if (chains) {
        const int64_t cnt = r1 - r0 + 1, rec0 = coff[(size_t)(r0 - 1)];
        std::vector<int64_t> off((size_t)cnt + 1);
        for (int64_t k = 0; k <= cnt; k++) off[(size_t)k] = coff[(size_t)(r0 - 1 + k)] - rec0;
        cstatus.assign((size_t)cnt + 1, 0);
        CHK(dh_la_chain_paths(va.ctx, va.db.get(), vb.db.get(), las.data() + rec0, n - rec0, trace, ts, off.data(), cnt, into(ep), cstatus.data()));
    } else {
        CHK(dh_la_edit_paths(va.ctx, va.db.get(), vb.db.get(), las.data(), n, trace, ts, r0 - 1, r1 - r0 + 1, into(ep)));
    }
    const int64_t *op_off = dh_edit_paths_op_off(ep.get());
    const uint8_t *ops = dh_edit_paths_ops(ep.get());
    const int32_t *score = dh_edit_paths_score(ep.get());
    const int32_t *nfill = dh_edit_paths_entry_fillers(ep.get());
    const int64_t *aoff = dh_dazz_offsets(da), *boff = dh_dazz_offsets(dbz);
    std::vector<char> text;
    std::vector<uint8_t> brc;
    for (int64_t i = 0; i < dh_edit_paths_count(ep.get()); i++) {
        // the entry as one record: a chain from the begin of its first record to the end of its last
        const int64_t f = chains ? coff[(size_t)(r0 - 1 + i)] : r0 - 1 + i, e = chains ? coff[(size_t)(r0 + i)] : f + 1;
        dh_la l = las[(size_t)f];
        l.aepos = las[(size_t)(e - 1)].aepos;
        l.bepos = las[(size_t)(e - 1)].bepos;
        const uint8_t *o = ops + op_off[i];
        const int64_t no = op_off[i + 1] - op_off[i];
        const int64_t alen = aoff[l.aread + 1] - aoff[l.aread], blen = boff[l.bread + 1] - boff[l.bread];
        const bool comp = (l.flags & DH_FLAG_COMP) != 0;
        const bool nested = chains && cstatus[(size_t)i] == DH_CP_NESTED;
        int64_t nmatch = 0, tdiffs = 0;
        for (int64_t k = 0; k < no; k++) nmatch += o[k] == 0;
        for (int32_t t = 0; t < l.tlen; t += 2) tdiffs += trace[l.toff + t];
        const char *cigar = cigar_text(o, no, text);
        printf("%s\t%lld\t%lld\t%lld\t%c\t%s\t%lld\t%d\t%d\t%lld\t%lld\t255\tNM:i:%d", paf_name(dbz, l.bread).c_str(), (long long)blen,
               (long long)(comp ? blen - l.bepos : l.bbpos), (long long)(comp ? blen - l.bbpos : l.bepos), comp ? '-' : '+',
               paf_name(da, l.aread).c_str(), (long long)alen, l.abpos, l.aepos, (long long)nmatch, (long long)no, score[i]);
        if (!chains) {
            printf("\ttp:i:%lld\tcg:Z:%s\n", (long long)tdiffs, cigar);
        } else {
            printf("\tnl:i:%lld\tnf:i:%d\tcg:Z:%s", (long long)(e - f), nfill ? nfill[i] : 0, nested ? "*" : cigar);
            if (cstatus[(size_t)i] == DH_CP_FAKED) printf("\tfk:i:1");
            if (nested) printf("\tst:Z:nested");
            putchar('\n');
        }
        if (!show || nested) continue;
        const uint8_t *a = dh_dazz_bases(da) + aoff[l.aread] + l.abpos, *b = dh_dazz_bases(dbz) + boff[l.bread] + l.bbpos;
        if (comp) {  // the B side of the record in the reverse-complement frame
            brc.resize((size_t)(l.bepos - l.bbpos));
            const uint8_t *fwd = dh_dazz_bases(dbz) + boff[l.bread];
            for (int32_t x = l.bbpos; x < l.bepos; x++) {
                const uint8_t c = fwd[blen - 1 - x];
                brc[(size_t)(x - l.bbpos)] = c < 4 ? (uint8_t)(3 - c) : c;
            }
            b = brc.data();
        }
        print_alignment(a, b, o, no, width, text);
    }
    return 0;
}

// ---------------------------------------------------------------------------------- LAtranspose
// LAtranspose [-b] <A:db|dam> <B:db|dam> <in:las> <out:las>: the same alignments with the roles of the sequences exchanged
// (dh_la_transpose: the file `damapper -C` names <B>.<A>.las, dazzler.d:6158-6170, as the exact transposition of <in>); -b sets
// the chain flags
int tool_latranspose(const Args &args)
{
    bool best = false;
    Args pos;
    for (const std::string &a : args) {
        if (a == "-b")
            best = true;
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    if (pos.size() != 4) die("usage: LAtranspose [-b] <A:db|dam> <B:db|dam> <in:las> <out:las>");
    const Dev va(pos[0]);
    std::unique_ptr<Dev> second;
    if (pos[1] != pos[0]) second.reset(new Dev(va.ctx, pos[1]));
    const Dev &vb = second ? *second : va;
    const int32_t first_a = dh_dazz_first_id(va.dz.get()), first_b = dh_dazz_first_id(vb.dz.get());
    const LaSet set = read_las(pos[2]);
    std::vector<dh_la> las = shifted_records(set.get(), first_a, first_b);
    LaSet transposed;
    CHK(dh_la_transpose(va.ctx, va.db.get(), vb.db.get(), las.data(), (int64_t)las.size(), dh_la_set_trace(set.get()), dh_la_set_tspace(set.get()),
                        best ? 1 : 0, into(transposed), nullptr));
    las = shifted_records(transposed.get(), -first_b, -first_a);  // (the id offsets exchanged with the reads)
    CHK(dh_las_write(pos[3].c_str(), las.data(), (int64_t)las.size(), dh_la_set_trace(transposed.get()), dh_la_set_tspace(transposed.get())));
    return 0;
}

// ---------------------------------------------------------------------------------- DBnw
// DBnw [-f] [-a] [-w<int(100)>] <A:db|dam> <B:db|dam> [first-last]
// Read i of A against read i of B, globally (dh_nw_batch: findAlignment, util/string.d:478-520; -f: free shift).  One line per
// pair, tab separated: pair number (1-based), length of the A read, length of the B read, score, matches, alignment columns
// (the two numbers `check-results` reads from stretcher's "# Identity:" line), extended cigar; -a adds the alignment text.
// A pair whose band the kernel does not serve prints score -1, 0 matches, 0 columns and the cigar "*".
int tool_dbnw(const Args &args)
{
    bool show = false, fs = false;
    int width = 100;
    Args pos;
    for (const std::string &a : args) {
        if (a == "-a")
            show = true;
        else if (a == "-f")
            fs = true;
        else if (a.compare(0, 2, "-w") == 0)
            width = atoi(a.c_str() + 2);
        else if (a[0] == '-')
            die("unknown option " + a);
        else
            pos.push_back(a);
    }
    long long r0 = 1, r1 = -1;
    pop_range(pos, "pair", &r0, &r1);
    if (pos.size() != 2 || width < 1) die("usage: DBnw [-f] [-a] [-w<int(100)>] <A:db|dam> <B:db|dam> [first-last]");
    Ctx ctx;
    CHK(dh_ctx_create(0, nullptr, into(ctx)));
    const Dazz dza = open_dazz(pos[0]), dzb = open_dazz(pos[1]);
    const dh_dazz *da = dza.get(), *dbz = dzb.get();
    const int64_t n = std::min(dh_dazz_nreads(da), dh_dazz_nreads(dbz));
    if (r1 < 0) r1 = n;
    if (r0 < 1 || r1 > n || r0 > r1 + 1) die("pair range outside the DBs (" + std::to_string(n) + " pairs)");
    const int64_t cnt = r1 - r0 + 1;
    const int64_t *aoff = dh_dazz_offsets(da) + (r0 - 1), *boff = dh_dazz_offsets(dbz) + (r0 - 1);
    EditPaths ep;
    std::vector<int32_t> status((size_t)cnt + 1);
    CHK(dh_nw_batch(ctx.get(), dh_dazz_bases(da), aoff, dh_dazz_bases(dbz), boff, cnt, fs ? 1 : 0, into(ep), status.data()));
    const int64_t *op_off = dh_edit_paths_op_off(ep.get());
    const uint8_t *ops = dh_edit_paths_ops(ep.get());
    const int32_t *score = dh_edit_paths_score(ep.get());
    std::vector<char> text;
    for (int64_t i = 0; i < cnt; i++) {
        const uint8_t *o = ops + op_off[i];
        const int64_t no = op_off[i + 1] - op_off[i];
        const long long alen = aoff[i + 1] - aoff[i], blen = boff[i + 1] - boff[i];
        if (status[(size_t)i] != DH_NW_OK) {
            printf("%lld\t%lld\t%lld\t-1\t0\t0\t*\n", (long long)(r0 + i), alen, blen);
            continue;
        }
        int64_t nmatch = 0;
        for (int64_t k = 0; k < no; k++) nmatch += o[k] == 0;
        printf("%lld\t%lld\t%lld\t%d\t%lld\t%lld\t%s\n", (long long)(r0 + i), alen, blen, score[i], (long long)nmatch, (long long)no,
               cigar_text(o, no, text));
        if (show) print_alignment(dh_dazz_bases(da) + aoff[i], dh_dazz_bases(dbz) + boff[i], o, no, width, text);
    }
    return 0;
}

// ---------------------------------------------------------------------------------- stretcher
// stretcher [--auto] [--stdout | --outfile=<file>] [--aformat=pair] [--awidth=<int(50)>] [--sreverse2] [--gapopen=<int(16)>]
//           [--gapextend=<int(4)>] <a:fasta> <b:fasta>   (one dash or two) the first record of each file aligned end to end
// with affine gap costs (dh_nw_affine_batch), written as EMBOSS `pair` text (dh_format_pair): the call of `dentist
// check-results` (commands/checkResults.d:2091-2100).
// The first record of a FASTA file: its name (the header's first word) and its bases as codes 0..4 (letters outside ACGT
// become N).
static void first_fasta_record(const std::string &path, std::string &name, std::vector<uint8_t> &seq)
{
    FILE *f = fopen(path.c_str(), "r");
    if (!f) die("cannot open " + path);
    const std::string text = slurp(f);
    fclose(f);
    size_t p = text.find('>');
    if (p == std::string::npos || (p > 0 && text[p - 1] != '\n')) die("no FASTA record in " + path);
    size_t eol = text.find('\n', p);
    if (eol == std::string::npos) eol = text.size();
    const std::string header = text.substr(p + 1, eol - p - 1);
    name = header.substr(0, header.find_first_of(" \t\r"));
    for (size_t k = eol; k < text.size(); k++) {
        const char c = text[k];
        if (c == '>' && text[k - 1] == '\n') break;
        if (c == '\n' || c == '\r' || c == ' ' || c == '\t') continue;
        switch (c | 32) {
            case 'a': seq.push_back(0); break;
            case 'c': seq.push_back(1); break;
            case 'g': seq.push_back(2); break;
            case 't': seq.push_back(3); break;
            default: seq.push_back(4);
        }
    }
}

int tool_stretcher(const Args &args)
{
    const char *usage = "usage: stretcher [--auto] [--stdout | --outfile=<file>] [--aformat=pair] [--awidth=<int(50)>] [--sreverse2] "
                        "[--gapopen=<int(16)>] [--gapextend=<int(4)>] <a:fasta> <b:fasta>";
    dh_nw_scoring sc = {5, -4, 16, 4};
    long long width = 50;
    bool rev2 = false;
    std::string outfile;
    Args pos;
    for (const std::string &a : args) {
        if (a.size() < 2 || a[0] != '-') {
            pos.push_back(a);
            continue;
        }
        const std::string opt = a.substr(a[1] == '-' ? 2 : 1);
        const size_t eq = opt.find('=');
        const std::string key = opt.substr(0, eq), val = eq == std::string::npos ? "" : opt.substr(eq + 1);
        char *end = nullptr;
        const long long num = strtoll(val.c_str(), &end, 10);
        const bool is_num = !val.empty() && *end == 0;
        if ((key == "auto" || key == "stdout") && eq == std::string::npos)
            ;
        else if (key == "sreverse2" && eq == std::string::npos)
            rev2 = true;
        else if (key == "aformat") {
            if (val != "pair") die("--aformat=" + val + ": only the pair format is written");
        } else if (key == "awidth" && is_num && num >= 1)
            width = num;
        else if (key == "gapopen" && is_num && num >= 0 && num <= INT32_MAX)
            sc.gap_open = (int32_t)num;
        else if (key == "gapextend" && is_num && num >= 0 && num <= INT32_MAX)
            sc.gap_extend = (int32_t)num;
        else if (key == "outfile" && !val.empty())
            outfile = val;
        else
            die("unknown or malformed option " + a + "\n" + usage);
    }
    if (pos.size() != 2) die(usage);
    std::string name[2];
    std::vector<uint8_t> seq[2];
    for (int k = 0; k < 2; k++) first_fasta_record(pos[(size_t)k], name[k], seq[k]);
    if (rev2) {
        std::reverse(seq[1].begin(), seq[1].end());
        for (uint8_t &c : seq[1]) c = c < 4 ? (uint8_t)(3 - c) : c;
    }
    Ctx ctx;
    CHK(dh_ctx_create(0, nullptr, into(ctx)));
    const int64_t aoff[2] = {0, (int64_t)seq[0].size()}, boff[2] = {0, (int64_t)seq[1].size()};
    EditPaths ep;
    int32_t status = 0;
    CHK(dh_nw_affine_batch(ctx.get(), seq[0].data(), aoff, seq[1].data(), boff, 1, &sc, into(ep), &status));
    if (status != DH_NW_OK)
        fail("the alignment of " + name[0] + " (" + std::to_string(seq[0].size()) + " bases) and " + name[1] + " (" +
             std::to_string(seq[1].size()) + " bases) cannot be proven optimal inside " + std::to_string(DH_NWA_MAX_BAND) +
             " diagonals, the widest band the kernel serves; nothing was written");
    const uint8_t *ops = dh_edit_paths_ops(ep.get());
    const int64_t nops = dh_edit_paths_op_off(ep.get())[1];
    const int32_t score = dh_edit_paths_score(ep.get())[0];
    const int64_t tl = dh_format_pair(name[0].c_str(), seq[0].data(), aoff[1], name[1].c_str(), seq[1].data(), boff[1], ops, nops, score,
                                      &sc, width, nullptr, 0);
    if (tl < 0) die(dh_last_error());
    std::vector<char> text((size_t)tl + 1);
    dh_format_pair(name[0].c_str(), seq[0].data(), aoff[1], name[1].c_str(), seq[1].data(), boff[1], ops, nops, score, &sc, width,
                   text.data(), tl + 1);
    FILE *o = outfile.empty() ? stdout : fopen(outfile.c_str(), "w");
    if (!o) die("cannot write " + outfile);
    const bool ok = fwrite(text.data(), 1, (size_t)tl, o) == (size_t)tl;
    if ((o != stdout ? fclose(o) : fflush(o)) != 0 || !ok) die("write error");
    return 0;
}

// ---------------------------------------------------------------------------------- fm-index
// fm-index [-P<dir>] [-r] <reference> [<queries>...]: every exact occurrence of every query line (-r: and of its reverse
// complement) in the records (lines) of <reference>, one TAB-separated line per hit (dh_exact_locate): the reference's
// external/fm-index.cpp as `dentist check-results` calls it (commands/checkResults.d:511-565, 654-687); leaves <reference>.fm9.
// The contract is the reference program's (external/fm-index.cpp), restated: records and queries are lines; record ids are
// 0-based line numbers, empty lines included; empty query lines are skipped and do not advance the 0-based query id, which
// restarts for every source; per query all forward occurrences ascending by (record, begin), then with -r those of the
// reverse complement; coordinates 0-based, right-open, relative to the record.  Deviations: no index is built --
// <reference>.fm9 is a small file of our own that says so (check-results asserts that it exists, checkResults.d:684), and
// <reference>.idx is not written; a last line without '\n' is a record (the reference program throws on a hit in it);
// the alphabet is acgt, or ACGT if every letter of the reference and of all queries is upper case -- any other byte, or
// mixed case, ends the run (the reference program matches bytes, so nothing is case-folded silently).
namespace {
const char kFm9Magic[8] = {'d', 'h', 'f', 'm', '9', '\n', 0, 0};
const int64_t kFm9Version = 1;

struct FmLetters {  // the case of the first letter seen, and where
    int upper = -1;
    std::string file;
    long long line = 0;
};

// the lines of `text` as codes appended to `seq`, their ends to `off`; keep_empty: empty lines are records
void fm_lines(const std::string &text, const std::string &file, bool keep_empty, FmLetters &lt, std::vector<uint8_t> &seq,
              std::vector<int64_t> &off, std::vector<int64_t> *text_starts)
{
    long long line = 1;
    size_t p = 0;
    while (p < text.size()) {
        size_t eol = text.find('\n', p);
        const bool last_open = eol == std::string::npos;
        if (last_open) eol = text.size();
        if (text_starts) text_starts->push_back((int64_t)p);
        for (size_t k = p; k < eol; k++) {
            const unsigned char c = (unsigned char)text[k];
            const unsigned char l = (unsigned char)(c | 32);
            const bool letter = (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z');
            if (!letter || (l != 'a' && l != 'c' && l != 'g' && l != 't')) {
                char msg[256];
                snprintf(msg, sizeof(msg), "%s: line %lld: byte 0x%02x%s is not one of acgt (or ACGT)", file.c_str(), line, c,
                         c == 'n' || c == 'N' ? " (n)" : "");
                fail(msg);
            }
            const int upper = c < 'a';
            if (lt.upper < 0) {
                lt.upper = upper;
                lt.file = file;
                lt.line = line;
            } else if (lt.upper != upper) {
                char msg[512];
                snprintf(msg, sizeof(msg), "%s: line %lld: %s-case letter, but %s line %lld is %s case: bytes are matched as they are, mixed "
                         "case is refused", file.c_str(), line, upper ? "upper" : "lower", lt.file.c_str(), lt.line, lt.upper ? "upper" : "lower");
                fail(msg);
            }
            seq.push_back((uint8_t)(l == 'a' ? 0 : l == 'c' ? 1 : l == 'g' ? 2 : 3));
        }
        if (keep_empty || eol > p) off.push_back((int64_t)seq.size());
        p = eol + 1;
        line++;
    }
}

bool fm9_current(const std::string &path, int64_t size)
{
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    char magic[8];
    int64_t head[2] = {0, 0};
    const bool ok = fread(magic, 1, 8, f) == 8 && fread(head, 8, 2, f) == 2 && memcmp(magic, kFm9Magic, 8) == 0 &&
                    head[0] == kFm9Version && head[1] == size;
    fclose(f);
    return ok;
}
}  // namespace

int tool_fm_index(const Args &args)
{
    auto usage = [](const std::string &err) {
        fprintf(stderr,
                "error: %s\n\nUsage fm-index [-P<dir>] [-r] <in:reference> [<in:queries> ...]\n"
                "    Locates every exact occurrence of the <queries> (one per line) in <reference>\n"
                "    (one record per line) on the GPU; reads standard input if no <queries> is given.\n\n"
                "    -P<dir>   temporary directory (must exist; unused)\n"
                "    -r        search the reverse complement of each query as well\n\n"
                "    Output, TAB-separated: refName refId refLength queryId hitBegin hitEnd revComp\n"
                "    Ids and coordinates are zero-based, coordinates right-open.  Leaves <reference>.fm9.\n",
                err.c_str());
        return 1;
    };
    bool both = false;
    std::string tmpdir;
    size_t i = 0;
    for (; i < args.size() && !args[i].empty() && args[i][0] == '-'; i++) {
        const std::string &a = args[i];
        if (a.size() >= 2 && a[1] == 'P') {
            tmpdir = a.substr(2);
            if (tmpdir.empty()) return usage("Missing value for -P.");
        } else if (a == "-r")
            both = true;
        else if (a.size() >= 2 && a[1] == 'r')
            return usage("Flag -r takes no value.");
        else
            return usage("Invalid option " + a + ".");
    }
    if (!tmpdir.empty()) {
        struct stat sb;
        if (stat(tmpdir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode)) return usage("Cannot open temporary directory: " + tmpdir);
    }
    if (i >= args.size()) return usage("Missing arguments.");
    const std::string ref_path = args[i];
    const Args qfiles(args.begin() + (long)i + 1, args.end());
    // ---- the reference: records, alphabet, <reference>.fm9
    FILE *f = fopen(ref_path.c_str(), "rb");
    if (!f) fail("File `" + ref_path + "` does not exist.");
    const std::string ref_text = slurp(f);
    fclose(f);
    FmLetters lt;
    std::vector<uint8_t> rseq, qseq;
    std::vector<int64_t> roff{0}, qoff{0}, text_starts;
    fm_lines(ref_text, ref_path, true, lt, rseq, roff, &text_starts);
    text_starts.push_back((int64_t)ref_text.size());
    const int64_t nref = (int64_t)roff.size() - 1;
    const std::string fm9 = ref_path + ".fm9";
    if (!fm9_current(fm9, (int64_t)ref_text.size())) {
        fprintf(stderr, "{\"level\":\"info\",\"info\":\"Writing the record list (no index is needed).\",\"file\":\"%s\"}\n", fm9.c_str());
        FILE *o = fopen(fm9.c_str(), "wb");
        if (!o) fail("cannot write " + fm9);
        const int64_t head[3] = {kFm9Version, (int64_t)ref_text.size(), nref};
        const bool ok = fwrite(kFm9Magic, 1, 8, o) == 8 && fwrite(head, 8, 3, o) == 3 &&
                        fwrite(text_starts.data(), 8, text_starts.size(), o) == text_starts.size();
        if (fclose(o) != 0 || !ok) fail("write error on " + fm9);
    }
    // ---- the queries of every source
    struct Source {
        std::string name;
        int64_t first;  // its first query in the call
    };
    std::vector<Source> sources;
    auto add_source = [&](const std::string &name, const std::string &text) {
        sources.push_back(Source{name, (int64_t)qoff.size() - 1});
        fm_lines(text, name, false, lt, qseq, qoff, nullptr);
    };
    if (qfiles.empty())
        add_source("stdin", slurp(stdin));
    else
        for (const std::string &q : qfiles) {
            FILE *qf = fopen(q.c_str(), "rb");
            if (!qf) {
                fprintf(stderr, "{\"level\":\"warning\",\"info\":\"File does not exist. Skipping.\",\"file\":\"%s\"}\n", q.c_str());
                continue;
            }
            add_source(q, slurp(qf));
            fclose(qf);
        }
    const int64_t nqry = (int64_t)qoff.size() - 1;
    Ctx ctx;
    CHK(dh_ctx_create(0, nullptr, into(ctx)));
    ExactHits hits;
    CHK(dh_exact_locate(ctx.get(), rseq.data(), roff.data(), nref, qseq.data(), qoff.data(), nqry, both ? 1 : 0, into(hits)));
    const dh_exact_hit *h = dh_exact_hits_records(hits.get());
    const int64_t nh = dh_exact_hits_count(hits.get());
    size_t s = 0;
    std::string line;
    for (int64_t k = 0; k < nh; k++) {
        while (s + 1 < sources.size() && h[k].query >= sources[s + 1].first) s++;
        char buf[160];
        snprintf(buf, sizeof(buf), "\t%d\t%lld\t%lld\t%lld\t%lld\t%s\n", h[k].ref, (long long)(roff[(size_t)h[k].ref + 1] - roff[(size_t)h[k].ref]),
                 (long long)(h[k].query - sources[s].first), (long long)h[k].begin, (long long)h[k].end, h[k].complement ? "yes" : "no");
        line = sources[s].name + buf;
        if (fwrite(line.data(), 1, line.size(), stdout) != line.size()) fail("write error");
    }
    if (fflush(stdout) != 0) fail("write error");
    return 0;
}
