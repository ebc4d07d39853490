// dh_scaffold.cpp -- the C entry points of the scaffold-graph pile-up builder of `dentist collect`
// (collectPileUps/pileups.d:173-208 build) over one driver: raw joins of every read (dh_scaffold_joins.cpp), the graph
// pipeline (dh_scaffold_graph.cpp), with resolveBubbles (dh_scaffold_bubbles.cpp) where the caller supplies the
// re-mapping of the skipping reads -- dh_remap_skipping_reads on the device (dh_scaffold_pileups_resolved) or the
// caller's (dh_scaffold_pileups_cb).  dh_scaffold_pileups itself runs without it: the forks of a bubble then go through
// the read-support rule like any other fork.  The result is read through the accessors here and the views of
// dh_scaffold_views.cpp.
#include <cstring>
#include <memory>

#include "dh_scaffold.h"

using namespace dh_scaffold_detail;

extern "C" void dh_default_scaffold_opts(dh_scaffold_opts *o)
{
    if (!o) return;
    memset(o, 0, sizeof(*o));
    o->min_spanning_reads = 3;     // commandline.d:2125, 2187
    o->merge_extensions = 1;       // commandline.d:2217-2222
    o->best_pile_up_margin = 3.0;  // commandline.d:1345
    o->existing_gap_bonus = 6.0;   // commandline.d:1688
}

extern "C" int32_t dh_scaffold_npiles(const dh_scaffold *s) { return s ? (int32_t)s->joins.size() : 0; }
extern "C" int64_t dh_scaffold_nentries(const dh_scaffold *s) { return s ? (int64_t)s->entries.size() : 0; }
extern "C" const dh_join *dh_scaffold_joins(const dh_scaffold *s) { return s ? s->joins.data() : nullptr; }
extern "C" const dh_read_alignment *dh_scaffold_entries(const dh_scaffold *s) { return s ? s->entries.data() : nullptr; }
extern "C" void dh_scaffold_destroy(dh_scaffold *s) { delete s; }

// The builder.  rs: resolveBubbles (pileups.d:1124-1315) runs between the raw scaffold and discardAmbiguousJoins, as
// build() runs it (pileups.d:186); the alignments the resolver adds are returned in *rs->extra: LA index n + i of the
// result's read alignments = record i of it (ids of the full DBs; traces for the cropper when the device maps).
static int scaffold_resolved(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                             const int32_t *input_gaps, int32_t ngaps, const dh_scaffold_opts *opts, dh_scaffold **out, Resolver *rs = nullptr)
{
    if (int rc = check_input_gaps("dh_scaffold_pileups", input_gaps, ngaps, ncontigs)) return rc;
    // alignment chains are the unit (SeededAlignment.from(AlignmentChain), base.d:1964-2050: first.begin .. last.end): the
    // builder runs on one pseudo record per chain, the read alignments then name the chain's first record (the re-mapped
    // alignments are taken record by record: they cover a whole intermediate contig)
    dh_chain_view cv;
    dh_chain_view_build(las, n, cv);
    const dh_la *u = cv.trivial ? las : cv.unit.data();
    const int64_t nu = cv.trivial ? n : (int64_t)cv.unit.size();
    std::vector<std::vector<RawJoin>> found;
    if (int rc = collect_raw_joins("dh_scaffold_pileups", u, nu, contig_off, ncontigs, read_off, 0, nreads, &found)) return rc;
    if (rs) {
        rs->c = Ctx{u, contig_off, read_off};
        rs->c.n = nu;
        rs->c.extra = rs->extra;
    }
    if (int rc = scaffold_from_runs(found, ncontigs, input_gaps, ngaps, opts, out, rs)) return rc;
    if (!cv.trivial) {
        // unit index -> record index: the first record of the chain; the added alignments follow the n records
        auto rec_of = [&](int32_t x) { return x < nu ? (int32_t)cv.first[(size_t)x] : (int32_t)(n + (x - nu)); };
        for (dh_read_alignment &ra : (*out)->entries) {
            ra.la0 = rec_of(ra.la0);
            if (ra.n == 2) ra.la1 = rec_of(ra.la1);
        }
    }
    return DH_OK;
}

extern "C" int dh_scaffold_pileups(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                                   const int64_t *read_off, int32_t nreads, const int32_t *input_gaps, int32_t ngaps,
                                   const dh_scaffold_opts *opts, dh_scaffold **out)
{
    if ((n > 0 && !las) || !contig_off || !read_off || !opts || !out || ncontigs < 0 || nreads < 0 || n < 0 ||
        n >= (1ll << 31) || (ngaps > 0 && !input_gaps) || ngaps < 0)
        return dh_fail(DH_EINVAL, "dh_scaffold_pileups: bad argument");
    return scaffold_resolved(las, n, contig_off, ncontigs, read_off, nreads, input_gaps, ngaps, opts, out);
}

// the frame of the two resolving entry points: the builder with a resolver whose re-mapping is `remap` (it may keep
// what belongs to its alignments, their trace values, in the set handed to it), the added alignments as a set in *extra
typedef std::function<int(const std::vector<int32_t> &, const std::vector<int32_t> &, std::vector<dh_la> &, dh_la_set &)> RemapInto;
static int resolved_into_set(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                             const int32_t *input_gaps, int32_t ngaps, const dh_scaffold_opts *opts, int32_t max_bubble_size, int32_t max_iterations,
                             int32_t tspace, const RemapInto &remap, dh_scaffold **out, dh_la_set **extra, int32_t *resolved)
{
    std::unique_ptr<dh_la_set> ex(new dh_la_set());
    ex->tspace = tspace;
    std::vector<dh_la> added;
    Resolver rs;
    rs.extra = &added;
    rs.remap = [&](const std::vector<int32_t> &cids, const std::vector<int32_t> &rids, std::vector<dh_la> &fresh) -> int {
        if (int rc = remap(cids, rids, fresh, *ex)) return rc;
        for (const dh_la &l : fresh)
            if (l.aread < 0 || l.aread >= ncontigs || l.bread < 0 || l.bread >= nreads)
                return dh_fail(DH_EINVAL, "resolveBubbles: the re-mapping returned an id outside the DBs");
        return DH_OK;
    };
    rs.max_bubble_size = max_bubble_size > 0 ? max_bubble_size : 8;
    rs.max_iterations = max_iterations > 0 ? max_iterations : 4;
    const int rc = scaffold_resolved(las, n, contig_off, ncontigs, read_off, nreads, input_gaps, ngaps, opts, out, &rs);
    if (resolved) *resolved = rs.resolved;
    if (rc) return rc;
    ex->la.assign(added.begin(), added.end());
    *extra = ex.release();
    return DH_OK;
}

// host only: the re-mapping is the caller's (tests feed the oracle's alignments; a D host could spawn damapper)
extern "C" int dh_scaffold_pileups_cb(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                                      int32_t nreads, const int32_t *input_gaps, int32_t ngaps, const dh_scaffold_opts *opts,
                                      int32_t max_bubble_size, int32_t max_iterations, dh_remap_fn remap, void *user,
                                      dh_scaffold **out, dh_la_set **extra, int32_t *resolved)
{
    if ((n > 0 && !las) || !contig_off || !read_off || !opts || !out || !extra || !remap || ncontigs < 0 || nreads < 0 || n < 0 ||
        n >= (1ll << 30) || (ngaps > 0 && !input_gaps) || ngaps < 0)
        return dh_fail(DH_EINVAL, "dh_scaffold_pileups_cb: bad argument");
    return resolved_into_set(
        las, n, contig_off, ncontigs, read_off, nreads, input_gaps, ngaps, opts, max_bubble_size, max_iterations, 0,
        [&](const std::vector<int32_t> &cids, const std::vector<int32_t> &rids, std::vector<dh_la> &fresh, dh_la_set &) -> int {
            dh_la *p = nullptr;
            int64_t cnt = 0;
            if (int rc2 = remap(user, cids.data(), (int32_t)cids.size(), rids.data(), (int32_t)rids.size(), &p, &cnt)) {
                free(p);
                return dh_fail(rc2, "resolveBubbles: the re-mapping callback failed");
            }
            if (cnt < 0 || (cnt > 0 && !p)) return dh_fail(DH_EINVAL, "resolveBubbles: bad callback result");
            fresh.assign(p, p + cnt);
            free(p);
            return DH_OK;
        },
        out, extra, resolved);
}

// the device maps: dh_remap_skipping_reads with the mapping options of the caller, no mask
extern "C" int dh_scaffold_pileups_resolved(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const dh_la *las, int64_t n,
                                            const int32_t *input_gaps, int32_t ngaps, const dh_scaffold_opts *opts,
                                            const dh_align_opts *map_opts, int32_t allowance, int32_t max_bubble_size,
                                            int32_t max_iterations, dh_scaffold **out, dh_la_set **extra, int32_t *resolved)
{
    if (!ctx || !contigs || !reads || (n > 0 && !las) || !opts || !map_opts || !out || !extra || n < 0 || n >= (1ll << 30) ||
        (ngaps > 0 && !input_gaps) || ngaps < 0 || allowance < 0)
        return dh_fail(DH_EINVAL, "dh_scaffold_pileups_resolved: bad argument");
    return resolved_into_set(
        las, n, contigs->h_off.data(), contigs->n, reads->h_off.data(), reads->n, input_gaps, ngaps, opts, max_bubble_size,
        max_iterations, map_opts->tspace,
        [&](const std::vector<int32_t> &cids, const std::vector<int32_t> &rids, std::vector<dh_la> &fresh, dh_la_set &ex) -> int {
            dh_la_set *set = nullptr;
            if (int rc2 = dh_remap_skipping_reads(ctx, contigs, reads, cids.data(), (int32_t)cids.size(), rids.data(), (int32_t)rids.size(),
                                                  map_opts, allowance, &set))
                return rc2;
            const int64_t t0 = (int64_t)ex.trace.size();
            fresh.assign(set->la.begin(), set->la.end());
            for (dh_la &l : fresh) l.toff += t0;
            ex.trace.insert(ex.trace.end(), set->trace.begin(), set->trace.end());
            dh_la_set_destroy(set);
            return DH_OK;
        },
        out, extra, resolved);
}
