// dazz_dentist.cpp -- DENTIST's own sub-commands over the library's batched calls.  In all of them an unknown or malformed
// option prints the usage and exits 1; everything that fails behind the options exits 2 with the library's message.
#include <cmath>

#include "dazz_tools.h"

// ---------------------------------------------------------------------------------- chain-local-alignments
// chain-local-alignments [--max-indel=<bps>] [--max-chain-gap=<bps>] [--max-relative-overlap=<f>] [--min-relative-score=<f>]
//           [--min-score=<n>] <ref-db> [<reads-db>] <in:las> <out:las>
// The local alignments of every (A, B) pair chained (dh_la_chain: chainLocalAlignments, common/alignments/chaining.d:122-334):
// every accepted chain as one run of records, alternate chains included -- the command of the same name
// (commands/chainLocalAlignments.d; options commandline.d:945-951, 1813-2165).  The numbers are checked after the .las is
// read: their defaults depend on its trace spacing.
int tool_chain(const Args &args)
{
    const char *usage = "usage: chain-local-alignments [--max-indel=<bps>] [--max-chain-gap=<bps>] [--max-relative-overlap=<f>] "
                        "[--min-relative-score=<f>] [--min-score=<n>] <ref-db> [<reads-db>] <in:las> <out:las>";
    Args pos;
    std::string v_indel, v_gap, v_ovl, v_rel, v_min;
    for (const std::string &a : args) {
        if (long_value(a, "--max-indel=", &v_indel) || long_value(a, "--max-chain-gap=", &v_gap) || long_value(a, "--max-relative-overlap=", &v_ovl) ||
            long_value(a, "--min-relative-score=", &v_rel) || long_value(a, "--min-score=", &v_min))
            continue;
        if (is_option(a)) die(std::string("unknown or malformed option ") + a + "\n" + usage);
        pos.push_back(a);
    }
    if (pos.size() != 3 && pos.size() != 4) die(usage);
    const std::string &in = pos[pos.size() - 2], &out = pos[pos.size() - 1];
    Ctx ctx;
    LaSet set, chained;
    must(dh_las_read(in.c_str(), into(set)));
    dh_chain_opts o;
    dh_default_chain_opts(&o, dh_la_set_tspace(set.get()));
    lenient_number(v_indel, &o.max_indel), lenient_number(v_gap, &o.max_chain_gap), lenient_number(v_min, &o.min_score);
    lenient_number(v_ovl, &o.max_relative_overlap), lenient_number(v_rel, &o.min_relative_score);
    // the DBs only say which read ids exist
    Dazz da, db;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    if (pos.size() == 4) must(dh_dazz_open(pos[1].c_str(), into(db)));
    const dh_dazz *dbz = db ? db.get() : da.get();
    const int64_t n = dh_la_set_count(set.get());
    const dh_la *las = dh_la_set_records(set.get());
    for (int64_t i = 0; i < n; i++) {
        const int64_t a = (int64_t)las[i].aread - dh_dazz_first_id(da.get()), b = (int64_t)las[i].bread - dh_dazz_first_id(dbz);
        if (a < 0 || a >= dh_dazz_nreads(da.get()) || b < 0 || b >= dh_dazz_nreads(dbz))
            fail("record " + std::to_string(i) + " of " + in + ": a read id outside the DB");
    }
    must(dh_ctx_create(0, nullptr, into(ctx)));
    LaChains chains;
    must(dh_la_chain(ctx.get(), las, n, &o, into(chains)));
    must(dh_la_chains_to_set(chains.get(), las, n, dh_la_set_trace(set.get()), dh_la_set_tspace(set.get()), into(chained)));
    static const uint16_t no_trace = 0;
    const uint16_t *tr = dh_la_set_trace(chained.get());
    must(dh_las_write(out.c_str(), dh_la_set_records(chained.get()), dh_la_set_count(chained.get()), tr ? tr : &no_trace, dh_la_set_tspace(chained.get())));
    return 0;
}

// readMasks (propagateMask.d:136-142, collectPileUps/package.d:100-110): the union of the mask tracks `masks` of the opened DB,
// per contig sorted with intersecting or touching intervals merged.  Returns "" or what failed.
static std::string read_united_masks(const dh_dazz *da, const std::string &db_path, const Args &masks, std::vector<int64_t> &mask_ptr,
                                     std::vector<int32_t> &mask_iv)
{
    const int32_t ncontigs = dh_dazz_nreads(da);
    std::vector<std::vector<std::pair<int32_t, int32_t>>> per((size_t)ncontigs);
    for (const std::string &m : masks) {
        std::vector<int64_t> ptr;
        std::vector<int32_t> iv;
        const std::string err = read_mask(da, db_path, m, ptr, iv);
        if (!err.empty()) return err;
        for (int32_t c = 0; c < ncontigs; c++)
            for (int64_t j = ptr[(size_t)c]; j < ptr[(size_t)c + 1]; j++)
                if (iv[(size_t)(2 * j + 1)] > iv[(size_t)(2 * j)]) per[(size_t)c].push_back({iv[(size_t)(2 * j)], iv[(size_t)(2 * j + 1)]});
    }
    merge_intervals(per, mask_ptr, mask_iv);
    mask_iv.push_back(0);  // (never an empty array)
    return "";
}

// ---------------------------------------------------------------------------------- propagate-mask
// propagate-mask -m <mask> [-m <mask>]... <ref-db> [<reads-db>] <db-alignment> <out-mask>
// The union of the masks of <ref-db> carried through the alignments to <reads-db> (to <ref-db> itself when it is omitted) and
// written there as <out-mask> (dh_la_propagate_mask: `dentist propagate-mask`, commands/propagateMask.d:136-305;
// snakemake/Snakefile:1218-1255).
int tool_propagate_mask(const Args &args)
{
    const char *usage = "usage: propagate-mask -m <mask> [-m <mask>]... [--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> [<reads-db>] "
                        "<db-alignment> <out-mask>";
    Args pos, masks;
    bool ignored = false;
    for (size_t i = 0; i < args.size(); i++) {
        const std::string &a = args[i];
        std::string v;
        if (a == "-m" && i + 1 < args.size())
            masks.push_back(args[++i]);
        else if (short_value(a, 'm', &v) || long_value(a, "--mask=", &v))
            masks.push_back(v);
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (masks.empty() || (pos.size() != 3 && pos.size() != 4)) die(usage);
    if (ignored) notice_ignored();
    const std::string &in = pos[pos.size() - 2], &out_name = pos[pos.size() - 1], &dest_path = pos.size() == 4 ? pos[1] : pos[0];
    Ctx ctx;
    Dazz da, db;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    if (pos.size() == 4) must(dh_dazz_open(pos[1].c_str(), into(db)));
    const dh_dazz *dest = db ? db.get() : da.get();
    const int32_t ncontigs = dh_dazz_nreads(da.get()), nreads = dh_dazz_nreads(dest);
    std::vector<int64_t> mask_ptr;
    std::vector<int32_t> mask_iv;
    const std::string mask_err = read_united_masks(da.get(), pos[0], masks, mask_ptr, mask_iv);
    if (!mask_err.empty()) fail(mask_err);
    LaSet set;
    must(dh_las_read(in.c_str(), into(set)));
    const std::vector<dh_la> las = shifted_records(set.get(), dh_dazz_first_id(da.get()), dh_dazz_first_id(dest));
    must(dh_ctx_create(0, nullptr, into(ctx)));
    MaskResult res;
    must(dh_la_propagate_mask(ctx.get(), las.data(), (int64_t)las.size(), dh_la_set_trace(set.get()), dh_la_set_trace_len(set.get()),
                              dh_la_set_tspace(set.get()), mask_ptr.data(), mask_iv.data(), ncontigs, dh_dazz_offsets(dest), nreads, into(res)));
    must(write_mask(dest_path, out_name, nreads, dh_mask_result_ptr(res.get()), dh_mask_result_iv(res.get()), dh_mask_result_count(res.get())));
    return 0;
}

// ---------------------------------------------------------------------------------- validate-regions
// validate-regions [--min-coverage-reads=<n> | --read-coverage=<f> --ploidy=<n>] [--min-spanning-reads=<n>]
//                  [--region-context=<bps>] [--weak-coverage-window=<bps>] [--weak-coverage-mask=<mask>] [--report-all]
//                  <ref-db> <reads-db> <in.las> <regions-mask>
// One JSON line per invalid region (per region with --report-all) of the mask <regions-mask> of <ref-db>, the weak-coverage
// mask written on request (dh_la_validate_regions: `dentist validate-regions`, commands/validateRegions.d:141-512;
// snakemake/Snakefile:1425-1466).  A mask that carries the track extras `contigs` and `reads` (bed2mask --data-comments) also
// gives every region its contig pair and consensus read ids, which the workflow's skip-gaps file is made from.
int tool_validate_regions(const Args &args)
{
    const char *usage = "usage: validate-regions [--min-coverage-reads=<n> | --read-coverage=<f> --ploidy=<n>] [--min-spanning-reads=<n>] "
                        "[--region-context=<bps>] [--weak-coverage-window=<bps>] [--weak-coverage-mask=<mask>] [--report-all] "
                        "[--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> <reads-db> <in.las> <regions-mask>";
    Args pos;
    std::string v_min_cov, v_cov, v_ploidy, v_span, v_context, v_window, out_mask;
    bool ignored = false, report_all = false;
    for (const std::string &a : args) {
        if (long_value(a, "--min-coverage-reads=", &v_min_cov) || long_value(a, "--read-coverage=", &v_cov) || long_value(a, "--ploidy=", &v_ploidy) ||
            long_value(a, "--min-spanning-reads=", &v_span) || long_value(a, "--region-context=", &v_context) ||
            long_value(a, "--weak-coverage-window=", &v_window) || long_value(a, "--weak-coverage-mask=", &out_mask))
            continue;
        if (a == "--report-all")
            report_all = true;
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 4) die(usage);
    if (ignored) notice_ignored();
    // the defaults of commandline.d:2187, 2411, 2497; the coverage options of :2060-2088
    int32_t min_cov = 0, min_span = 3, context = 1000, window = 500, ploidy = 0;
    double read_cov = 0;
    lenient_number(v_min_cov, &min_cov), lenient_number(v_cov, &read_cov), lenient_number(v_ploidy, &ploidy);
    lenient_number(v_span, &min_span), lenient_number(v_context, &context), lenient_number(v_window, &window);
    if (v_min_cov.empty() == v_cov.empty()) fail("exactly one of --min-coverage-reads and --read-coverage must be given");
    if (!v_cov.empty()) {
        if (ploidy <= 0) fail("--read-coverage needs --ploidy > 0");
        min_cov = (int32_t)(0.5 * read_cov / ploidy);
    }
    Ctx ctx;
    Dazz da, db;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    must(dh_dazz_open(pos[1].c_str(), into(db)));
    const int32_t ncontigs = dh_dazz_nreads(da.get());
    LaSet set;
    must(dh_las_read(pos[2].c_str(), into(set)));
    const int64_t n = dh_la_set_count(set.get());
    if (n == 0) {  // (:151-159)
        fprintf(stderr, "validate-regions: warning: empty reads-alignment %s\n", pos[2].c_str());
        return 0;
    }
    const std::vector<dh_la> las = shifted_records(set.get(), dh_dazz_first_id(da.get()), dh_dazz_first_id(db.get()));
    // the regions of the contigs between the first and the last aread of the file (:259-271)
    std::vector<int64_t> ptr;
    std::vector<int32_t> iv;
    const std::string mask_err = read_mask(da.get(), pos[0], pos[3], ptr, iv);
    if (!mask_err.empty()) fail(mask_err);
    // the track extras `contigs` and `reads` of the mask, where bed2mask --data-comments stored them (:204-256): positional,
    // one pair and one list per interval of the whole mask
    std::vector<int64_t> contig_ids, read_ids, read_off;
    const bool has_contigs = read_extra(pos[0], pos[3], "contigs", contig_ids), has_reads = read_extra(pos[0], pos[3], "reads", read_ids);
    const int64_t nmask = ptr[(size_t)ncontigs];
    if (has_contigs && (int64_t)contig_ids.size() != 2 * nmask)
        fail("mask " + pos[3] + ": the extra `contigs` has " + std::to_string(contig_ids.size()) + " entries, not two for each of the " +
             std::to_string(nmask) + " intervals of the mask (<ref-db> must be the whole DB)");
    if (has_reads) {  // per interval the count, then the ids
        std::vector<int64_t> ids;
        read_off.push_back(0);
        for (size_t at = 0; at < read_ids.size();) {
            const int64_t k = read_ids[at++];
            if (k < 0 || k > (int64_t)(read_ids.size() - at)) fail("mask " + pos[3] + ": the extra `reads` ends inside a list of read ids");
            ids.insert(ids.end(), read_ids.begin() + (ptrdiff_t)at, read_ids.begin() + (ptrdiff_t)(at + (size_t)k));
            at += (size_t)k;
            read_off.push_back((int64_t)ids.size());
        }
        if ((int64_t)read_off.size() - 1 != nmask)
            fail("mask " + pos[3] + ": the extra `reads` holds " + std::to_string(read_off.size() - 1) + " lists, not one for each of the " +
                 std::to_string(nmask) + " intervals of the mask (<ref-db> must be the whole DB)");
        read_ids.swap(ids);
    }
    // ... sliced with the regions (:259-271)
    std::vector<dh_region> regions;
    std::vector<int64_t> region_interval;
    for (int32_t c = std::max(0, las.front().aread); c < ncontigs && c <= las.back().aread; c++)
        for (int64_t j = ptr[(size_t)c]; j < ptr[(size_t)c + 1]; j++) {
            regions.push_back(dh_region{c, iv[(size_t)(2 * j)], iv[(size_t)(2 * j + 1)]});
            region_interval.push_back(j);
        }
    must(dh_ctx_create(0, nullptr, into(ctx)));
    RegionResult res;
    must(dh_la_validate_regions(ctx.get(), las.data(), n, dh_dazz_offsets(da.get()), ncontigs, regions.data(), (int32_t)regions.size(), context, window,
                                min_cov, min_span, into(res)));
    const dh_region_report *rep = dh_region_result_reports(res.get());
    const int64_t *span_off = dh_region_result_span_off(res.get());
    const int32_t *span_ids = dh_region_result_span_ids(res.get());
    const int32_t first_contig = dh_dazz_first_id(da.get()) + 1, first_read = dh_dazz_first_id(db.get()) + 1;  // the ids of the report are 1-based
    for (size_t r = 0; r < regions.size(); r++) {
        if (rep[r].is_valid && !report_all) continue;
        printf("{\"region\":{\"contigId\":%d,\"begin\":%d,\"end\":%d},\"regionWithContext\":{\"contigId\":%d,\"begin\":%d,\"end\":%d},"
               "\"isValid\":%s,\"numSpanningReads\":%d,\"spanningReadIds\":[",
               regions[r].contig + first_contig, regions[r].begin, regions[r].end, regions[r].contig + first_contig, rep[r].ctx_begin,
               rep[r].ctx_end, rep[r].is_valid ? "true" : "false", rep[r].num_spanning_reads);
        for (int64_t k = span_off[r]; k < span_off[r + 1]; k++) printf("%s%d", k > span_off[r] ? "," : "", span_ids[k] + first_read);
        printf("],\"weakCoverageMaskBps\":%d", rep[r].weak_bp);
        const int64_t j = region_interval[r];
        if (has_contigs && contig_ids[(size_t)(2 * j)] > 0) {  // the ids as stored (:373-377)
            printf(",\"contigIds\":[%lld,%lld],\"consensusReadIds\":[", (long long)contig_ids[(size_t)(2 * j)], (long long)contig_ids[(size_t)(2 * j + 1)]);
            if (has_reads)
                for (int64_t k = read_off[(size_t)j]; k < read_off[(size_t)j + 1]; k++)
                    printf("%s%lld", k > read_off[(size_t)j] ? "," : "", (long long)read_ids[(size_t)k]);
            printf("]");
        }
        printf("}\n");
    }
    if (!out_mask.empty())
        must(write_mask(pos[0], out_mask, ncontigs, dh_region_result_mask_ptr(res.get()), dh_region_result_mask_iv(res.get()),
                        dh_region_result_mask_count(res.get())));
    return 0;
}

// ---------------------------------------------------------------------------------- collect
// collect [--mask=<name>[,<name>...]]... [--max-alignment-error=<f>] [--min-anchor-length=<n>] [--proper-alignment-allowance=<n>]
//         [--min-spanning-reads=<n>] [--best-pile-up-margin=<f>] [--existing-gap-bonus=<f>] [--no-merge-extension]
//         <ref-db> <reads-db> <ref-vs-reads.las> <pile-ups.db>
// `dentist collect` (commands/collectPileUps/package.d:88-206; snakemake/Snakefile:1257-1290): the six alignment filters on the
// device (dh_la_collect_filter), the scaffold graph with resolveBubbles, every pile-up written to <pile-ups.db>.  The numbers
// are checked after the .las is read: the allowance defaults to its trace spacing.
int tool_collect(const Args &args)
{
    const char *usage = "usage: collect [--mask=<name>[,<name>...]]... [--max-alignment-error=<f>] [--min-anchor-length=<n>] "
                        "[--proper-alignment-allowance=<n>] [--min-spanning-reads=<n>] [--best-pile-up-margin=<f>] "
                        "[--existing-gap-bonus=<f>] [--no-merge-extension] <ref-db> <reads-db> <ref-vs-reads.las> <pile-ups.db>";
    Args pos, masks;
    std::string v_err, v_anchor, v_allow, v_span, v_margin, v_bonus;
    bool ignored = false, merge_extensions = true;
    auto add_masks = [&](const std::string &list) {  // <name>[,<name>...]
        size_t at = 0;
        while (at <= list.size()) {
            const size_t comma = std::min(list.find(',', at), list.size());
            if (comma > at) masks.push_back(list.substr(at, comma - at));
            at = comma + 1;
        }
    };
    for (size_t i = 0; i < args.size(); i++) {
        const std::string &a = args[i];
        std::string v;
        if ((a == "-m" || a == "-e") && i + 1 < args.size()) {
            if (a == "-m")
                add_masks(args[++i]);
            else
                v_err = args[++i];
        } else if (long_value(a, "--mask=", &v) || short_value(a, 'm', &v))
            add_masks(v);
        else if (long_value(a, "--max-alignment-error=", &v_err) || short_value(a, 'e', &v_err) || long_value(a, "--min-anchor-length=", &v_anchor) ||
                 long_value(a, "--proper-alignment-allowance=", &v_allow) || long_value(a, "--min-spanning-reads=", &v_span) ||
                 long_value(a, "--best-pile-up-margin=", &v_margin) || long_value(a, "--existing-gap-bonus=", &v_bonus))
            continue;
        else if (a == "--no-merge-extension")
            merge_extensions = false;
        else if (ignored_option(a) || long_value(a, "--auxiliary-threads=") || long_value(a, "--tmpdir=") || long_value(a, "--damapper-ref-vs-reads=") ||
                 short_value(a, 'A') || short_value(a, 'P'))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (masks.empty() || pos.size() != 4) die(usage);  // (at least one mask: commandline.d:1789)
    if (ignored) notice_ignored("--config, -v, --quiet, -T / --threads, -A / --auxiliary-threads, -P / --tmpdir and --damapper-ref-vs-reads");
    Ctx ctx;
    LaSet set;
    must(dh_las_read(pos[2].c_str(), into(set)));
    const int64_t n = dh_la_set_count(set.get());
    if (n == 0) fail("empty ref vs. reads alignment");  // (:127)
    const int32_t tspace = dh_la_set_tspace(set.get());
    // the defaults of commandline.d:1336, 1681, 1799-1808, 2024-2036, 2183, 2317-2332
    double max_err = 0.3;
    int32_t min_anchor = 500, allowance = tspace;
    dh_scaffold_opts so;
    dh_default_scaffold_opts(&so);
    so.min_spanning_reads = 3, so.best_pile_up_margin = 3.0, so.existing_gap_bonus = 6.0, so.merge_extensions = merge_extensions ? 1 : 0;
    lenient_number(v_err, &max_err), lenient_number(v_anchor, &min_anchor), lenient_number(v_allow, &allowance);
    lenient_number(v_span, &so.min_spanning_reads), lenient_number(v_margin, &so.best_pile_up_margin), lenient_number(v_bonus, &so.existing_gap_bonus);
    if (!(max_err > 0 && max_err <= 0.3)) fail("--max-alignment-error must lie in (0, 0.3]");
    Dazz da, db;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    must(dh_dazz_open(pos[1].c_str(), into(db)));
    const int32_t ncontigs = dh_dazz_nreads(da.get()), nreads = dh_dazz_nreads(db.get());
    std::vector<int64_t> mask_ptr;
    std::vector<int32_t> mask_iv;
    const std::string mask_err = read_united_masks(da.get(), pos[0], masks, mask_ptr, mask_iv);
    if (!mask_err.empty()) fail(mask_err);
    std::vector<dh_la> las = shifted_records(set.get(), dh_dazz_first_id(da.get()), dh_dazz_first_id(db.get()));
    must(dh_ctx_create(0, nullptr, into(ctx)));
    dh_process_opts po;
    dh_default_process_opts(&po);
    po.max_align_err_ppm = (int32_t)llround(max_err * 1e6), po.allowance = allowance, po.min_anchor = min_anchor;
    int64_t dropped[6];
    must(dh_la_collect_filter(ctx.get(), las.data(), n, dh_dazz_offsets(da.get()), ncontigs, dh_dazz_offsets(db.get()), nreads, mask_ptr.data(),
                              mask_iv.data(), &po, dropped, nullptr));
    static const char *const stage[6] = {"LQ", "Improper", "WeaklyAnchored", "Contained", "Ambiguous", "Redundant"};
    for (int k = 0; k < 6; k++) fprintf(stderr, "collect: filter %s dropped %lld alignment chains\n", stage[k], (long long)dropped[k]);
    int64_t left = 0;
    for (const dh_la &l : las) left += l.flags & DH_FLAG_DISABLED ? 0 : 1;
    if (left == 0) fail("no alignment chains left after filtering");  // (:153-156)
    // the gaps of the input assembly: contigs that follow each other in one scaffold of the .dam
    std::vector<int32_t> gaps;
    for (int32_t c = 0; c + 1 < ncontigs; c++)
        if (scaffold_neighbours(da.get(), c)) gaps.insert(gaps.end(), {c, c + 1});
    Db A, B;
    must(dh_db_create(ctx.get(), dh_dazz_bases(da.get()), dh_dazz_offsets(da.get()), ncontigs, nullptr, into(A)));
    must(dh_db_create(ctx.get(), dh_dazz_bases(db.get()), dh_dazz_offsets(db.get()), nreads, nullptr, into(B)));
    dh_align_opts ao;
    dh_default_align_opts(&ao);
    ao.tspace = tspace;
    Scaffold sc;
    LaSet extra;
    must(dh_scaffold_pileups_resolved(ctx.get(), A.get(), B.get(), las.data(), n, gaps.data(), (int32_t)gaps.size() / 2, &so, &ao, allowance, 0, 0,
                                      into(sc), into(extra), nullptr));
    // the records and traces of *extra behind the file's: LA index n + i is record i of *extra
    std::vector<uint16_t> trace(dh_la_set_trace(set.get()), dh_la_set_trace(set.get()) + dh_la_set_trace_len(set.get()));
    const int64_t nx = extra ? dh_la_set_count(extra.get()) : 0;
    for (int64_t i = 0; i < nx; i++) {
        dh_la l = dh_la_set_records(extra.get())[i];
        l.toff += (int64_t)trace.size();
        las.push_back(l);
    }
    if (nx) trace.insert(trace.end(), dh_la_set_trace(extra.get()), dh_la_set_trace(extra.get()) + dh_la_set_trace_len(extra.get()));
    Pileups piles;
    must(dh_scaffold_all_pileups(sc.get(), las.data(), (int64_t)las.size(), 3, into(piles), nullptr));
    trace.push_back(0);  // (never an empty array)
    must(dh_pileups_write_db(piles.get(), las.data(), (int64_t)las.size(), trace.data(), dh_dazz_offsets(da.get()), ncontigs, dh_dazz_offsets(db.get()),
                             nreads, tspace, pos[3].c_str()));
    return 0;
}

// ---------------------------------------------------------------------------------- mask-repetitive-regions
// mask-repetitive-regions [--read-coverage=<f> | --max-coverage-reads=<n>] [--max-improper-coverage-reads=<n>]
//         [--max-coverage-self=<n>] [--proper-alignment-allowance=<n>] [--debug-repeat-masks] <ref-db> [<reads-db>] <db-alignment>
//         <repeat-mask>
// The mask of the contig bases whose coverage by alignment chains (with <reads-db>: also by the improper ones) leaves its
// bounds, written as a mask track of <ref-db> (dh_la_repeat_mask: `dentist mask-repetitive-regions`,
// commands/maskRepetitiveRegions.d:129-430).  The reference's option validation (commandline.d:1840-1972) exits 1 like an
// unknown option.
int tool_mask_repetitive_regions(const Args &args)
{
    const std::string usage = "usage: mask-repetitive-regions [--read-coverage=<f> | --max-coverage-reads=<n>] [--max-improper-coverage-reads=<n>] "
                              "[--max-coverage-self=<n>] [--proper-alignment-allowance=<n>] [--debug-repeat-masks] [--config=<file>] [-v] "
                              "[--quiet] [-T<n>] <ref-db> [<reads-db>] <db-alignment> <repeat-mask>";
    Args pos;
    bool ignored = false, debug_masks = false, has_cov = false, has_max = false, has_max_improper = false, has_allowance = false;
    double read_coverage = 0.0;
    long long max_reads = 0, max_improper = 0, max_self = 4, allowance = 0;
    for (const std::string &a : args) {
        std::string v;
        if (long_value(a, "--read-coverage=", &v)) {
            char *end = nullptr;
            read_coverage = strtod(v.c_str(), &end);
            if (*end || !(read_coverage > 0.0)) die("unknown or malformed option " + a + "\n" + usage);
            has_cov = true;
        } else if (strict_number(a, "--max-coverage-reads=", &max_reads, usage))
            has_max = true;
        else if (strict_number(a, "--max-improper-coverage-reads=", &max_improper, usage))
            has_max_improper = true;
        else if (strict_number(a, "--max-coverage-self=", &max_self, usage))
            ;
        else if (strict_number(a, "--proper-alignment-allowance=", &allowance, usage))
            has_allowance = true;
        else if (a == "--debug-repeat-masks")
            debug_masks = true;
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 3 && pos.size() != 4) die(usage);
    const bool reads_case = pos.size() == 4;
    if (reads_case) {  // commandline.d:1868-1875, 1948-1955
        if (!has_max && !has_cov) die("must provide either --read-coverage or --max-coverage-reads");
        if (has_max && has_cov) die("must not provide both --read-coverage and --max-coverage-reads");
        if (!has_max_improper && !has_cov) die("must provide either --read-coverage or --max-improper-coverage-reads");
        if (has_max_improper && has_cov) die("must not provide both --read-coverage and --max-improper-coverage-reads");
    } else if (max_self < 1)
        die("--max-coverage-self must be positive");
    if (ignored) notice_ignored();
    const std::string &in = pos[pos.size() - 2], &out_name = pos[pos.size() - 1];
    Ctx ctx;
    Dazz da, db;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    if (reads_case) must(dh_dazz_open(pos[1].c_str(), into(db)));
    const dh_dazz *other = db ? db.get() : da.get();  // (a self alignment has the contigs on both sides)
    const int32_t ncontigs = dh_dazz_nreads(da.get()), nreads = dh_dazz_nreads(other);
    LaSet set;
    must(dh_las_read(in.c_str(), into(set)));
    const int64_t n = dh_la_set_count(set.get());
    if (n == 0) fprintf(stderr, "mask-repetitive-regions: warning: empty %s-alignment\n", reads_case ? "reads" : "self");
    const std::vector<dh_la> las = shifted_records(set.get(), dh_dazz_first_id(da.get()), dh_dazz_first_id(other));
    dh_repeat_opts o;
    o.lower = 0, o.improper_lower = 0, o.with_improper = reads_case ? 1 : 0;
    o.upper = reads_case ? (has_cov ? dh_max_coverage_reads(read_coverage) : (int32_t)max_reads) : (int32_t)max_self;
    o.improper_upper = reads_case ? (has_cov ? dh_max_improper_coverage_reads(read_coverage) : (int32_t)max_improper) : 0;
    o.allowance = has_allowance ? (int32_t)allowance : dh_la_set_tspace(set.get());
    // an empty .las: empty masks, without a device (count 0: the arrays are not looked at)
    RepeatResult res;
    const std::vector<int64_t> no_ptr((size_t)ncontigs + 1, 0);
    if (n > 0) {
        must(dh_ctx_create(0, nullptr, into(ctx)));
        must(dh_la_repeat_mask(ctx.get(), las.data(), n, dh_dazz_offsets(da.get()), ncontigs, dh_dazz_offsets(other), nreads, &o, into(res)));
    }
    const dh_repeat_result *r = res.get();
    must(write_mask(pos[0], out_name, ncontigs, r ? dh_repeat_result_mask_ptr(r) : no_ptr.data(), r ? dh_repeat_result_mask_iv(r) : nullptr,
                    r ? dh_repeat_result_mask_count(r) : 0));
    if (debug_masks && reads_case) {  // maskRepetitiveRegions.d:225-237
        must(write_mask(pos[0], out_name + "-all", ncontigs, r ? dh_repeat_result_all_ptr(r) : no_ptr.data(), r ? dh_repeat_result_all_iv(r) : nullptr,
                        r ? dh_repeat_result_all_count(r) : 0));
        must(write_mask(pos[0], out_name + "-improper", ncontigs, r ? dh_repeat_result_improper_ptr(r) : no_ptr.data(),
                        r ? dh_repeat_result_improper_iv(r) : nullptr, r ? dh_repeat_result_improper_count(r) : 0));
    }
    return 0;
}

// ---------------------------------------------------------------------------------- merge-masks, filter-mask
// `<block>.<mask>` with a block of the DB names the track of that block (Snakefile:583-584): its reads are shifted by the
// block's first id into the whole DB's contig range.
std::string read_mask_track(const dh_dazz *da, const std::string &db_path, const std::string &name, std::vector<int64_t> &ptr,
                            std::vector<int32_t> &iv)
{
    const std::string err = read_mask(da, db_path, name, ptr, iv);
    if (!err.empty()) return err;
    const int32_t ncontigs = dh_dazz_nreads(da);
    const size_t dot = name.find('.');
    if (dot == std::string::npos || dot == 0 || name.find_first_not_of("0123456789") != dot) return "";
    const DbPath d = parse_db_path(db_path);
    const int32_t block = atoi(name.c_str());
    if (block < 1 || block > stub_blocks(d)) return "";
    Dazz blk;  // opened as TANmask opens the block of its .las
    if (dh_dazz_open(d.block_db(block).c_str(), into(blk))) return "mask " + name + ": " + dh_last_error();
    const int32_t first = dh_dazz_first_id(blk.get()) - dh_dazz_first_id(da), nb = dh_dazz_nreads(blk.get());
    if (first < 0 || first + nb > ncontigs) return "mask " + name + ": the block lies outside the DB";
    const std::vector<int64_t> in(ptr);  // (entries 0 .. nb: the block's reads)
    for (int32_t c = 0; c <= ncontigs; c++) ptr[(size_t)c] = c < first ? 0 : in[(size_t)std::min(c - first, nb)];
    return "";
}

// merge-masks <ref-db> <merged-mask> <input-mask>...: `dentist merge-masks` (commands/mergeMasks.d:47-53), the union of the
// input masks
int tool_merge_masks(const Args &args)
{
    const std::string usage = "usage: merge-masks [--config=<file>] [-v] [--quiet] [-T<n>] <ref-db> <merged-mask> <input-mask>...";
    Args pos;
    bool ignored = false;
    for (const std::string &a : args) {
        if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() < 3) die(usage);
    if (ignored) notice_ignored();
    Ctx ctx;
    Dazz da;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    const int32_t ncontigs = dh_dazz_nreads(da.get()), nmasks = (int32_t)pos.size() - 2;
    std::vector<std::vector<int64_t>> ptr((size_t)nmasks);
    std::vector<std::vector<int32_t>> iv((size_t)nmasks);
    std::vector<const int64_t *> pp;
    std::vector<const int32_t *> pi;
    for (int32_t k = 0; k < nmasks; k++) {
        const std::string err = read_mask_track(da.get(), pos[0], pos[(size_t)k + 2], ptr[(size_t)k], iv[(size_t)k]);
        if (!err.empty()) fail(err);
        pp.push_back(ptr[(size_t)k].data()), pi.push_back(iv[(size_t)k].data());
    }
    MaskSet res;
    dh_mask_opts o;
    dh_default_mask_opts(&o);
    must(dh_ctx_create(0, nullptr, into(ctx)));
    must(dh_mask_combine(ctx.get(), pp.data(), pi.data(), nmasks, nullptr, nullptr, dh_dazz_offsets(da.get()), ncontigs, &o, into(res)));
    must(write_mask(pos[0], pos[1], ncontigs, dh_mask_set_ptr(res.get()), dh_mask_set_iv(res.get()), dh_mask_set_count(res.get())));
    return 0;
}

// filter-mask [--min-gap-size=<n>] [--min-interval-size=<n>] <ref-db> <in-mask> <out-mask>: `dentist filter-mask`
// (commands/filterMask.d:124-159): gaps up to --min-gap-size closed, then intervals below --min-interval-size dropped.  An
// empty input mask gives an empty mask (the reference indexes an empty array there).
int tool_filter_mask(const Args &args)
{
    const std::string usage = "usage: filter-mask [--min-gap-size=<n>] [--min-interval-size=<n>] [--config=<file>] [-v] [--quiet] [-T<n>] "
                              "<ref-db> <in-mask> <out-mask>";
    Args pos;
    bool ignored = false;
    long long min_gap = 0, min_interval = 0;
    for (const std::string &a : args) {
        if (strict_number(a, "--min-gap-size=", &min_gap, usage) || strict_number(a, "--min-interval-size=", &min_interval, usage))
            continue;
        if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 3) die(usage);
    if (ignored) notice_ignored();
    Ctx ctx;
    Dazz da;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    const int32_t ncontigs = dh_dazz_nreads(da.get());
    std::vector<int64_t> ptr;
    std::vector<int32_t> iv;
    const std::string err = read_mask_track(da.get(), pos[0], pos[1], ptr, iv);
    if (!err.empty()) fail(err);
    if (ptr[(size_t)ncontigs] == 0) {  // an empty mask, without a device
        must(write_mask(pos[0], pos[2], ncontigs, ptr.data(), nullptr, 0));
        return 0;
    }
    MaskSet res;
    const dh_mask_opts o{1, (int32_t)min_gap, (int32_t)min_interval, 0};
    const int64_t *pp = ptr.data();
    const int32_t *pi = iv.data();
    must(dh_ctx_create(0, nullptr, into(ctx)));
    must(dh_mask_combine(ctx.get(), &pp, &pi, 1, nullptr, nullptr, dh_dazz_offsets(da.get()), ncontigs, &o, into(res)));
    must(write_mask(pos[0], pos[2], ncontigs, dh_mask_set_ptr(res.get()), dh_mask_set_iv(res.get()), dh_mask_set_count(res.get())));
    return 0;
}

// ---------------------------------------------------------------------------------- process, process-pile-ups
// process [options] <ref-db> <reads-db> <pile-ups.db> <insertions.db>
// `dentist process` / `dentist process-pile-ups` (commands/processPileUps/package.d:123-159; the options of
// DentistCommand.processPileUps, commandline.d:1048-1054, 1088-1101, 1171-1281 and the other blocks that name it;
// snakemake/Snakefile:1292-1334): the batches of <pile-ups.db> through dh_process_pileups_db_batches -- only the reads the
// pile-ups name are loaded from <reads-db>, which is never opened whole -- and the closed pile-ups written sorted to
// <insertions.db> with the trace spacing of the pile-up alignments.  Everything that fails before the batches are known
// fails before a device is opened.
namespace {
const char *const kProcessUsage =
    "usage: process [--mask=<name>[,<name>...]]... [--batch=<idx-spec>[,<idx-spec>...]]... [--min-anchor-length=<n>] "
    "[--min-reads-per-pile-up=<n>] [--max-insertion-error=<f>] [--max-alignment-error=<f>] [--bad-fraction=<f>] "
    "[--proper-alignment-allowance=<n>] [--min-relative-score=<f>] [--only=spanning|extending|both] <ref-db> <reads-db> "
    "<pile-ups.db> <insertions.db>";

// <idx> | <from>..<to> | <from>..$ (parsePileUpIdxSpec, commandline.d:1195-1215); an end of -1 stands for `$`
bool parse_idx_spec(const std::string &spec, long long &from, long long &to)
{
    const char *p = spec.c_str();
    char *end = nullptr;
    if (!(*p >= '0' && *p <= '9')) return false;
    from = strtoll(p, &end, 10);
    if (*end == 0) {
        to = from + 1;
        return true;
    }
    if (end[0] != '.' || end[1] != '.') return false;
    p = end + 2;
    if (p[0] == '$' && p[1] == 0) {
        to = -1;
        return true;
    }
    if (!(*p >= '0' && *p <= '9')) return false;
    to = strtoll(p, &end, 10);
    return *end == 0;
}

const char *pile_status_name(int32_t st)
{
    static const char *const names[] = {"ok", "noCommonTracePoint", "tooSmall", "emptyAlignment", "flanksNotUnique", "orientation",
                                        "maxInsertionError", "negativeInsertion", "alignOverflow", "unsupportedJoin"};
    return st >= 0 && st < (int32_t)(sizeof(names) / sizeof(names[0])) ? names[st] : "unknown";
}
}  // namespace

int tool_process(const Args &args)
{
    Args pos, masks;
    std::string v_anchor, v_reads, v_ins, v_err, v_bad, v_allow, v_score;
    std::vector<std::pair<long long, long long>> batches;
    bool ignored = false;
    int32_t only = 0;
    auto add_masks = [&](const std::string &list) {  // <name>[,<name>...]
        size_t at = 0;
        while (at <= list.size()) {
            const size_t comma = std::min(list.find(',', at), list.size());
            if (comma > at) masks.push_back(list.substr(at, comma - at));
            at = comma + 1;
        }
    };
    auto add_batches = [&](const std::string &list) {
        size_t at = 0;
        while (at <= list.size()) {
            const size_t comma = std::min(list.find(',', at), list.size());
            long long from = 0, to = 0;
            if (!parse_idx_spec(list.substr(at, comma - at), from, to)) fail("ill-formatted batch range");
            batches.push_back({from, to});
            at = comma + 1;
        }
    };
    for (size_t i = 0; i < args.size(); i++) {
        const std::string &a = args[i];
        std::string v;
        if ((a == "-m" || a == "-e" || a == "-b") && i + 1 < args.size()) {
            if (a == "-m")
                add_masks(args[++i]);
            else if (a == "-b")
                add_batches(args[++i]);
            else
                v_err = args[++i];
        } else if (long_value(a, "--mask=", &v) || short_value(a, 'm', &v))
            add_masks(v);
        else if (long_value(a, "--batch=", &v) || short_value(a, 'b', &v))
            add_batches(v);
        else if (long_value(a, "--min-anchor-length=", &v_anchor) || long_value(a, "--min-reads-per-pile-up=", &v_reads) ||
                 long_value(a, "--max-insertion-error=", &v_ins) || long_value(a, "--max-alignment-error=", &v_err) || short_value(a, 'e', &v_err) ||
                 long_value(a, "--bad-fraction=", &v_bad) || long_value(a, "--proper-alignment-allowance=", &v_allow) ||
                 long_value(a, "--min-relative-score=", &v_score))
            continue;
        else if (long_value(a, "--only=", &v)) {
            if (v == "both")
                only = 0;
            else if (v == "spanning")
                only = 1;
            else if (v == "extending")
                only = 2;
            else
                die("unknown or malformed option " + a + "\n" + kProcessUsage);
        } else if (a == "--allow-single-reads")
            fail("--allow-single-reads (single reads instead of a consensus) is not built");
        else if (ignored_option(a) || short_value(a, 'A') || long_value(a, "--auxiliary-threads=") || long_value(a, "--aux-threads=") || short_value(a, 'P') ||
                 long_value(a, "--tmpdir=") || a == "--keep-temp" || a == "-k" || long_value(a, "--daccord=") || long_value(a, "--daligner-consensus=") ||
                 long_value(a, "--daligner-reads-vs-reads=") || long_value(a, "--daligner-self=") || long_value(a, "--datander-ref=") ||
                 long_value(a, "--dust-reads="))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + kProcessUsage);
        else
            pos.push_back(a);
    }
    if (masks.empty() || pos.size() != 4) die(kProcessUsage);  // (at least one mask: commandline.d:1789)
    if (ignored)
        notice_ignored("--config, -v, --quiet, -T / --threads, -A / --auxiliary-threads, -P / --tmpdir, --keep-temp and the pass-through options of "
                       "the aligners");
    dh_process_opts po;
    dh_default_process_opts(&po);
    po.max_reads = 0;  // (the reference knows minimum counts only, commandline.d:2125-2187)
    double max_ins = 0.1, max_err = 0.3, bad_fraction = 0.08, min_score = 1.0;
    int32_t allowance = -1;
    lenient_number(v_anchor, &po.min_anchor), lenient_number(v_reads, &po.min_reads), lenient_number(v_ins, &max_ins), lenient_number(v_err, &max_err);
    lenient_number(v_bad, &bad_fraction), lenient_number(v_allow, &allowance), lenient_number(v_score, &min_score);
    if (!(max_err > 0 && max_err <= 0.3)) fail("--max-alignment-error must lie in (0, 0.3]");
    if (!(max_ins >= 0 && max_ins <= 1)) fail("--max-insertion-error must lie in [0, 1]");
    if (!(bad_fraction >= 0 && bad_fraction < 0.5)) fail("--bad-fraction must be within [0, 0.5)");
    if (!(min_score > 0 && min_score <= 1)) fail("--min-relative-score must lie in (0, 1]");
    if (po.min_anchor < 0 || po.min_reads < 1 || (!v_allow.empty() && allowance < 0)) fail("an option's value is out of range");
    po.max_ins_err_ppm = (int32_t)llround(max_ins * 1e6), po.max_align_err_ppm = (int32_t)llround(max_err * 1e6);
    po.bad_fraction_ppm = (int32_t)llround(bad_fraction * 1e6), po.min_relative_score_ppm = std::max<int32_t>((int32_t)llround(min_score * 1e6), 1);
    // the batches against the file (validatePileUpBatches, commandline.d:1234-1271; without one: the whole file)
    Handle<dh_chaindb, dh_chaindb_destroy> pdb;
    must(dh_pileupdb_read(pos[2].c_str(), into(pdb)));
    const long long npiles = dh_chaindb_npiles(pdb.get());
    int32_t file_tspace = 0;
    if (dh_chaindb_nseeded(pdb.get()) > 0) file_tspace = dh_chaindb_seeded(pdb.get())[0].tspace;
    pdb.reset();
    if (batches.empty()) batches.push_back({0, -1});
    std::vector<int32_t> ranges;
    for (size_t i = 0; i < batches.size(); i++) {
        const long long from = batches[i].first, to = batches[i].second;
        const bool whole_empty = npiles == 0 && from == 0 && to == -1;  // (an empty file has no valid range but the whole)
        if (!whole_empty && !(from < (to < 0 ? npiles : to) && (to < 0 || to <= npiles)))
            fail("invalid batch range; check that 0 <= <from> < <to> <= " + std::to_string(npiles));
        ranges.push_back((int32_t)from);
        ranges.push_back(to < 0 ? -1 : (int32_t)to);
    }
    for (size_t i = 0; i < batches.size(); i++)  // (validatePileUpBatchesDontIntersect, :1255-1271: the first pair in its order)
        for (size_t j = i + 1; j < batches.size(); j++) {
            const long long a1 = batches[i].second < 0 ? npiles : batches[i].second, b1 = batches[j].second < 0 ? npiles : batches[j].second;
            if (std::max(batches[i].first, batches[j].first) < std::min(a1, b1))
                fail("invalid --batch: <idx-spec>'s at indices " + std::to_string(i) + " and " + std::to_string(j) + " intersect");
        }
    po.allowance = allowance >= 0 ? allowance : (file_tspace > 0 ? file_tspace : po.allowance);
    Dazz da;
    must(dh_dazz_open(pos[0].c_str(), into(da)));
    const int32_t ncontigs = dh_dazz_nreads(da.get());
    std::vector<int64_t> mask_ptr;
    std::vector<int32_t> mask_iv;
    const std::string mask_err = read_united_masks(da.get(), pos[0], masks, mask_ptr, mask_iv);
    if (!mask_err.empty()) fail(mask_err);
    // the pile-ups are read before a device is asked for: a file that contradicts the reference fails here
    {
        Pileups probe;
        LaSet probe_set;
        for (size_t k = 0; k + 1 < ranges.size(); k += 2)
            must(dh_pileups_from_db(pos[2].c_str(), ranges[k], ranges[k + 1] < 0 ? -1 : ranges[k + 1] - ranges[k], dh_dazz_offsets(da.get()), ncontigs,
                                    into(probe), into(probe_set), nullptr));
    }
    Ctx ctx;
    Db A;
    Handle<dh_insertions, dh_insertions_destroy> ins;
    int32_t *file_index = nullptr, *skipped = nullptr, nskipped = 0;
    const bool need_device = npiles > 0;  // (an empty file: an empty insertions.db, and no device is asked for)
    if (need_device) {
        must(dh_ctx_create(0, nullptr, into(ctx)));
        must(dh_db_create(ctx.get(), dh_dazz_bases(da.get()), dh_dazz_offsets(da.get()), ncontigs, nullptr, into(A)));
        must(dh_process_pileups_db_batches(ctx.get(), A.get(), pos[1].c_str(), pos[2].c_str(), ranges.data(), (int32_t)ranges.size() / 2, mask_ptr.data(),
                                           mask_iv.data(), &po, only, 1, into(ins), &file_index, &skipped, &nskipped));
    }
    for (int32_t k = 0; k < nskipped; k++)
        fprintf(stderr, "process: pile-up %d skipped by --only=%s\n", skipped[k], only == 1 ? "spanning" : "extending");
    const int32_t nrec = ins ? dh_insertions_count(ins.get()) : 0;
    for (int32_t i = 0; i < nrec; i++) {
        const int32_t st = dh_insertions_records(ins.get())[i].status;
        if (st != DH_PILE_OK) fprintf(stderr, "process: pile-up %d not closed: %s\n", file_index[i], pile_status_name(st));
    }
    dh_shard_free(file_index);
    dh_shard_free(skipped);
    if (ins)
        must(dh_insertions_write_db(ins.get(), dh_dazz_offsets(da.get()), ncontigs, po.tspace_pile, pos[3].c_str()));
    else
        must(dh_insertiondb_write(pos[3].c_str(), 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    return 0;
}

// ---------------------------------------------------------------------------------- show-pile-ups
// show-pile-ups [-j] <pile-ups.db>
// `dentist show-pile-ups` (commands/showPileUps.d:46-115): the size of the file and the number of its pile-ups, read
// alignments, seeded alignments, local alignments and trace points (pairs), as the table of :105-115 or with -j / --json as one
// JSON object (the Snakefile sizes the batches of `process` from it).  The whitespace of the JSON is not pinned.  Host only.
int tool_show_pile_ups(const Args &args)
{
    const char *usage = "usage: show-pile-ups [-j] [--config=<file>] [-v] [--quiet] [-T<n>] <pile-ups.db>";
    Args pos;
    bool json = false, ignored = false;
    for (const std::string &a : args) {
        if (a == "-j" || a == "--json")
            json = true;
        else if (ignored_option(a))
            ignored = true;
        else if (is_option(a))
            die("unknown or malformed option " + a + "\n" + usage);
        else
            pos.push_back(a);
    }
    if (pos.size() != 1) die(usage);
    if (ignored) notice_ignored();
    FILE *f = fopen(pos[0].c_str(), "rb");
    if (!f) fail("cannot open " + pos[0]);
    fseek(f, 0, SEEK_END);
    const long long size = ftell(f);
    fclose(f);
    Handle<dh_chaindb, dh_chaindb_destroy> db;
    must(dh_pileupdb_read(pos[0].c_str(), into(db)));
    const char *const key[6] = {"totalDbSize", "numPileUps", "numReadAlignments", "numSeededAlignments", "numLocalAlignments", "numTracePoints"};
    const long long val[6] = {size,
                              dh_chaindb_npiles(db.get()),
                              dh_chaindb_nread_alignments(db.get()),
                              (long long)dh_chaindb_nseeded(db.get()),
                              (long long)dh_chaindb_nlas(db.get()),
                              (long long)dh_chaindb_ntrace(db.get()) / 2};  // (the container counts u16 values, the reference pairs)
    if (json) {
        printf("{");
        for (int i = 0; i < 6; i++) printf("%s\"%s\":%lld", i ? "," : "", key[i], val[i]);
        printf("}\n");
        return 0;
    }
    const long long most = *std::max_element(val, val + 6);
    const int width = most > 0 ? (int)std::ceil(std::log10((double)most)) : 0;  // (columnWidth, :88-102: log10 rounded up)
    for (int i = 0; i < 6; i++) {
        const std::string label = std::string(key[i]) + ":";
        printf("%-20s %*lld%s\n", label.c_str(), width, val[i], i == 0 ? " bytes" : "");
    }
    return 0;
}
