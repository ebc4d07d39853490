// dazz_check.cpp -- check-results [--crop-alignment=<n>] [--crop-ambiguous=<n>] [--dust=<mask>] [--gap-details=<json>] [--json]
//                   <true-assembly> <mapped-regions-mask> <reference> <result>
// `dentist check-results` (commands/checkResults.d), the subset tools/README.md states: the input contigs are placed in the result
// by exact search (dh_exact_locate, findReferenceContigs :399-565), every gap goes through dh_check_gaps, and the stats that need
// only the mask, the DB lengths, the mappings and the summaries are printed.  Unknown options: the usage and exit 1.  Everything
// that fails behind the options: the library's message and exit 2.
#include <cmath>
#include <fstream>

#include "dazz_tools.h"

namespace {
struct Options {
    Args pos;  // <true-assembly> <mapped-regions-mask> <reference> <result>
    bool json = false, dust_given = false;
    long long crop = 0, crop_amb = 100;
    std::string dust_name = "dust", details;
};

Options parse_options(const Args &args)
{
    const std::string usage = "usage: check-results [--crop-alignment=<n>] [--crop-ambiguous=<n>] [--dust=<mask>] [--gap-details=<json>] "
                              "[--gap-details-context=0] [--json] [--config=<file>] [-v] [--quiet] [-T<n>] "
                              "<true-assembly> <mapped-regions-mask> <reference> <result>";
    Options o;
    bool ignored = false;
    long long context = 0;
    for (const std::string &a : args) {
        if (strict_number(a, "--crop-alignment=", &o.crop, usage) || strict_number(a, "--crop-ambiguous=", &o.crop_amb, usage) ||
            strict_number(a, "--gap-details-context=", &context, usage) || long_value(a, "--gap-details=", &o.details))
            continue;
        if (long_value(a, "--dust=", &o.dust_name))
            o.dust_given = true;
        else if (a == "--json" || a == "-j")
            o.json = true;
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown option " + a + "\n" + usage);
        else
            o.pos.push_back(a);
    }
    if (o.pos.size() != 4) die(usage);
    if (o.crop > o.crop_amb) die("--crop-alignment must be <= --crop-ambiguous\n" + usage);
    if (context != 0) die("--gap-details-context: only 0 is served (the sequence is null)\n" + usage);
    if (ignored) notice_ignored();
    return o;
}

// the cutoff of the reference DB's stub, else its shortest contig
long long contig_cutoff(const std::string &stub_path, const int64_t *off, int32_t n)
{
    long long cutoff = -1;
    std::ifstream stub(stub_path);
    std::string line;
    while (std::getline(stub, line)) {
        const size_t at = line.find("cutoff = ");
        if (at != std::string::npos) cutoff = atoll(line.c_str() + at + strlen("cutoff = "));
    }
    if (cutoff < 0)
        for (int32_t c = 0; c < n; c++) cutoff = cutoff < 0 ? off[c + 1] - off[c] : std::min<long long>(cutoff, off[c + 1] - off[c]);
    return cutoff;
}

// findReferenceContigs: duplicates by the self search at --crop-ambiguous, mappings by the search in the result
std::vector<dh_contig_mapping> find_reference_contigs(dh_ctx *ctx, const dh_dazz *dr, const dh_dazz *ds, long long crop, long long crop_amb)
{
    const int32_t n_ref = dh_dazz_nreads(dr), n_res = dh_dazz_nreads(ds);
    const int64_t *qoff = dh_dazz_offsets(dr), *soff = dh_dazz_offsets(ds);
    std::vector<uint8_t> qb;
    std::vector<int64_t> qo;
    auto cropped = [&](long long by) {
        qb.clear();
        qo.assign(1, 0);
        for (int32_t c = 0; c < n_ref; c++) {
            const int64_t len = qoff[c + 1] - qoff[c];
            if (len > 2 * by) qb.insert(qb.end(), dh_dazz_bases(dr) + qoff[c] + by, dh_dazz_bases(dr) + qoff[c + 1] - by);
            qo.push_back((int64_t)qb.size());
        }
    };
    std::vector<char> dup((size_t)n_ref + 1, 0);
    ExactHits hits;
    cropped(crop_amb);
    must(dh_exact_locate(ctx, dh_dazz_bases(dr), qoff, n_ref, qb.data(), qo.data(), n_ref, 1, into(hits)));
    for (int64_t k = 0; k < dh_exact_hits_count(hits.get()); k++) {
        const dh_exact_hit &h = dh_exact_hits_records(hits.get())[k];
        if (h.ref != h.query && qo[(size_t)h.query + 1] > qo[(size_t)h.query]) dup[(size_t)h.query] = 1;
    }
    hits.reset();
    cropped(crop);
    must(dh_exact_locate(ctx, dh_dazz_bases(ds), soff, n_res, qb.data(), qo.data(), n_ref, 1, into(hits)));
    std::vector<dh_contig_mapping> maps;
    for (int64_t k = 0; k < dh_exact_hits_count(hits.get()); k++) {
        const dh_exact_hit &h = dh_exact_hits_records(hits.get())[k];
        if (qo[(size_t)h.query + 1] == qo[(size_t)h.query]) continue;  // (a contig the crop leaves empty is not searched)
        maps.push_back(dh_contig_mapping{h.ref + 1, (int32_t)h.begin, (int32_t)h.end, (int32_t)(soff[h.ref + 1] - soff[h.ref]), h.query + 1,
                                         dup[(size_t)h.query], h.complement, 0.0f});
    }
    return maps;
}

double ratio(double a, double b) { return b > 0 ? a / b : std::nan(""); }
std::string json_number(double x)  // (NaN has no JSON text: null)
{
    char buf[40];
    snprintf(buf, sizeof(buf), "%.17g", x);
    return std::isnan(x) ? std::string("null") : std::string(buf);
}

// --gap-details: one object per gap that is not ignored (writeGapDetailsJson :1203-1239)
void write_gap_details(FILE *f, const dh_gap_report *rep, int32_t n_input, const dh_dazz *dt, const dh_dazz *ds, const std::vector<int32_t> &result_gap,
                       long long crop)
{
    static const char *const state_name[6] = {"unkown", "broken", "unclosed", "partiallyClosed", "closed", "ignored"};
    const dh_gap_summary *gs = dh_gap_report_summaries(rep);
    const dh_edit_paths *paths = dh_gap_report_paths(rep);
    const int64_t *toff = dh_dazz_offsets(dt), *soff = dh_dazz_offsets(ds);
    for (int32_t g = 0; g < n_input; g++) {
        const dh_gap_summary &s = gs[g];
        if (s.state == DH_GAP_IGNORED) continue;
        fprintf(f, "{\"leftContig\":%d,\"rightContig\":%d,\"state\":\"%s\",\"gapLength\":%d,\"details\":", g + 1, g + 2, state_name[s.state], s.gap_length);
        if (s.state == DH_GAP_CLOSED || s.state == DH_GAP_PARTIALLY_CLOSED) {
            std::string l[3];
            if (s.align_status == DH_CG_OK) {
                const uint8_t *ops = dh_edit_paths_ops(paths) + dh_edit_paths_op_off(paths)[g];
                const uint8_t *rb = dh_dazz_bases(dt) + toff[s.true_contig - 1] + s.true_begin;
                // the query as the aligner saw it
                std::vector<uint8_t> q;
                const uint8_t *sb = dh_dazz_bases(ds);
                if (s.result_begin_contig == s.result_end_contig)
                    q.assign(sb + soff[s.result_begin_contig - 1] + s.result_begin, sb + soff[s.result_begin_contig - 1] + s.result_end);
                else {
                    q.assign(sb + soff[s.result_begin_contig - 1] + s.result_begin, sb + soff[s.result_begin_contig]);
                    q.insert(q.end(), (size_t)result_gap[(size_t)s.result_begin_contig - 1], (uint8_t)4);
                    q.insert(q.end(), sb + soff[s.result_end_contig - 1], sb + soff[s.result_end_contig - 1] + s.result_end);
                }
                if (s.complement) {
                    std::reverse(q.begin(), q.end());
                    for (auto &b : q) b = b < 4 ? (uint8_t)(3 - b) : b;
                }
                int64_t i = 0, j = 0;
                for (int32_t k = 0; k < s.col_end; k++) {
                    const uint8_t op = ops[k];
                    const char rc_ = op == 2 ? '-' : base_char(rb[i++]), qc = op == 1 ? '-' : base_char(q[(size_t)j++]);
                    if (k < s.col_begin) continue;
                    l[0] += rc_, l[1] += op == 0 ? '|' : (op == 3 ? '.' : '-'), l[2] += qc;
                }
            }
            // (cropReference does not carry the complement over: false at crop > 0, as in the reference)
            fprintf(f, "{\"referenceLength\":%d,\"queryLength\":%d,\"complement\":%s,\"percentIdentity\":%s,\"dustPercentIdentity\":%s,"
                       "\"noneDustPercentIdentity\":%s,\"alignment\":[\"%s\",\"%s\",\"%s\"]}",
                    s.reference_length, s.query_length, s.complement && crop == 0 ? "true" : "false",
                    json_number(ratio(s.matches, s.col_end - s.col_begin)).c_str(), json_number(ratio(s.dust_matches, s.dust_ops)).c_str(),
                    json_number(ratio(s.none_dust_matches, s.none_dust_ops)).c_str(), l[0].c_str(), l[1].c_str(), l[2].c_str());
        } else
            fprintf(f, "null");
        fprintf(f, ",\"sequence\":null}\n");
    }
}

// the stats table, as text or --json
void print_stats(const dh_gap_summary *gs, const std::vector<int32_t> &mapped, const std::vector<dh_contig_mapping> &maps, const dh_dazz *ds, bool json)
{
    const int32_t n_input = (int32_t)(mapped.size() / 3), n_res = dh_dazz_nreads(ds);
    const int64_t *soff = dh_dazz_offsets(ds);
    const unsigned long long none = ~0ull;
    unsigned long long bps_expected = 0, bps_known = 0, bps_result = (unsigned long long)soff[n_res], bps_gaps = 0;
    std::vector<unsigned long long> scaffolds, inputs, results, gap_len, closed_len;
    for (int32_t c = 0; c < n_input; c++) {
        const unsigned long long len = (unsigned long long)(mapped[3 * (size_t)c + 2] - mapped[3 * (size_t)c + 1]);
        bps_known += len, inputs.push_back(len);
        if (c == 0 || mapped[3 * (size_t)c] != mapped[3 * (size_t)c - 3]) scaffolds.push_back(0);
        int32_t first = c;
        while (first > 0 && mapped[3 * (size_t)first - 3] == mapped[3 * (size_t)c]) first--;
        scaffolds.back() = (unsigned long long)(mapped[3 * (size_t)c + 2] - mapped[3 * (size_t)first + 1]);
    }
    for (unsigned long long x : scaffolds) bps_expected += x;
    for (int32_t c = 0; c < n_res; c++) results.push_back((unsigned long long)(soff[c + 1] - soff[c]));
    double weighted = 0;
    long long correct = 0, closed = 0, partially = 0;
    for (int32_t g = 0; g < n_input; g++) {
        const dh_gap_summary &s = gs[g];
        if (s.state == DH_GAP_IGNORED) continue;
        const double identity = ratio(s.matches, s.col_end - s.col_begin);
        bps_gaps += (unsigned long long)s.gap_length, gap_len.push_back((unsigned long long)s.gap_length);
        weighted += identity * s.gap_length;
        partially += s.state == DH_GAP_PARTIALLY_CLOSED;
        if (s.state == DH_GAP_CLOSED) closed++, closed_len.push_back((unsigned long long)s.gap_length), correct += 1.0 <= identity;
    }
    std::vector<int32_t> per_contig((size_t)n_input + 1, 0);
    for (const dh_contig_mapping &m : maps) per_contig[(size_t)m.query_contig] += !m.duplicate;
    const long long mapped_contigs = std::count(per_contig.begin(), per_contig.end(), 1);
    auto n50 = [&](std::vector<unsigned long long> v) -> unsigned long long {  // util/math.d N!50 against numBpsExpected
        std::sort(v.begin(), v.end());
        double cum = 0;
        for (size_t k = v.size(); k-- > 0;)
            if ((cum += (double)v[k]) >= 0.5 * (double)bps_expected) return v[k];
        return 0;
    };
    auto median = [&](std::vector<unsigned long long> v) -> unsigned long long {
        if (v.empty()) return none;
        std::sort(v.begin(), v.end());
        return v.size() > 1 && v.size() % 2 == 0 ? (v[v.size() / 2 - 1] + v[v.size() / 2]) / 2 : v[v.size() / 2];
    };
    const double avg_err = bps_gaps ? weighted / (double)bps_gaps : std::nan("");
    const std::pair<const char *, unsigned long long> rows[] = {
        {"numContigsExpected", (unsigned long long)n_input}, {"numMappedContigs", (unsigned long long)mapped_contigs},
        {"numClosedGaps", (unsigned long long)closed}, {"numPartiallyClosedGaps", (unsigned long long)partially},
        {"numCorrectGaps", (unsigned long long)correct}, {"numBpsExpected", bps_expected}, {"numBpsKnown", bps_known},
        {"numBpsResult", bps_result}, {"numBpsInGaps", bps_gaps}, {"maximumN50", n50(scaffolds)}, {"inputN50", n50(inputs)},
        {"resultN50", n50(results)}, {"gapMedian", median(gap_len)}, {"closedGapMedian", median(closed_len)},
        {"minClosedGap", closed_len.empty() ? none : *std::min_element(closed_len.begin(), closed_len.end())},
        {"maxClosedGap", closed_len.empty() ? none : *std::max_element(closed_len.begin(), closed_len.end())}};
    if (json) {
        printf("{");
        for (const auto &r : rows) printf("\"%s\":%llu,", r.first, r.second);
        printf("\"averageInsertionError\":%s}\n", json_number(avg_err).c_str());
    } else {
        for (const auto &r : rows) printf("%-24s%20llu\n", (std::string(r.first) + ":").c_str(), r.second);
        printf("%-24s%20.3e\n", "averageInsertionError:", avg_err);
    }
}
}  // namespace

int tool_check_results(const Args &args)
{
    const Options opt = parse_options(args);
    const Args &pos = opt.pos;
    Ctx ctx;
    Dazz dt, dr, ds;
    must(dh_dazz_open(pos[0].c_str(), into(dt)));
    must(dh_dazz_open(pos[2].c_str(), into(dr)));
    must(dh_dazz_open(pos[3].c_str(), into(ds)));
    const int32_t n_true = dh_dazz_nreads(dt.get()), n_ref = dh_dazz_nreads(dr.get()), n_res = dh_dazz_nreads(ds.get());
    const int64_t *toff = dh_dazz_offsets(dt.get()), *soff = dh_dazz_offsets(ds.get());
    const long long cutoff = contig_cutoff(pos[2], dh_dazz_offsets(dr.get()), n_ref);
    if (n_ref > 0 && (2 * opt.crop >= cutoff || 2 * opt.crop_amb >= cutoff))
        fail("--crop-alignment and --crop-ambiguous: twice the crop must stay below the contig cutoff of " + std::to_string(cutoff));
    // ---- the mapped intervals are the input contigs, in order
    std::vector<int64_t> mptr, dptr;
    std::vector<int32_t> miv, div;
    std::string err = read_mask_track(dt.get(), pos[0], pos[1], mptr, miv);
    if (!err.empty()) fail(err);
    std::vector<int32_t> mapped;
    for (int32_t t = 0; t < n_true; t++)
        for (int64_t k = mptr[(size_t)t]; k < mptr[(size_t)t + 1]; k++) mapped.insert(mapped.end(), {t + 1, miv[(size_t)(2 * k)], miv[(size_t)(2 * k + 1)]});
    const int32_t n_input = (int32_t)(mapped.size() / 3);
    if (n_input != n_ref) fail("the mask " + pos[1] + " has " + std::to_string(n_input) + " intervals, " + pos[2] + " has " + std::to_string(n_ref) + " contigs");
    bool have_dust = true;
    err = read_mask_track(dt.get(), pos[0], opt.dust_name, dptr, div);
    if (!err.empty()) {
        if (opt.dust_given) fail(err);
        have_dust = false;  // (the default track is used when it is there)
    }
    std::vector<int32_t> result_gap((size_t)n_res + 1, 0);
    for (int32_t c = 0; c + 1 < n_res; c++)
        if (scaffold_neighbours(ds.get(), c))
            result_gap[(size_t)c] = dh_dazz_fpulse(ds.get())[c + 1] - (int32_t)(dh_dazz_fpulse(ds.get())[c] + (soff[c + 1] - soff[c]));
    must(dh_ctx_create(0, nullptr, into(ctx)));
    const std::vector<dh_contig_mapping> maps = find_reference_contigs(ctx.get(), dr.get(), ds.get(), opt.crop, opt.crop_amb);
    // ---- the gaps
    Db T, S;
    must(dh_db_create(ctx.get(), dh_dazz_bases(dt.get()), toff, n_true, nullptr, into(T)));
    must(dh_db_create(ctx.get(), dh_dazz_bases(ds.get()), soff, n_res, nullptr, into(S)));
    GapReport rep;
    must(dh_check_gaps(ctx.get(), T.get(), S.get(), mapped.data(), n_input, maps.data(), (int32_t)maps.size(), result_gap.data(),
                       have_dust ? dptr.data() : nullptr, have_dust ? div.data() : nullptr, (int32_t)opt.crop, nullptr, 1, n_input, into(rep)));
    if (!opt.details.empty()) {
        FILE *f = fopen(opt.details.c_str(), "w");
        if (!f) fail("cannot write " + opt.details);
        write_gap_details(f, rep.get(), n_input, dt.get(), ds.get(), result_gap, opt.crop);
        fclose(f);
    }
    print_stats(dh_gap_report_summaries(rep.get()), mapped, maps, ds.get(), opt.json);
    return 0;
}
