// dh_vreg.h -- region validation (dh_la_validate_regions; `dentist validate-regions`, commands/validateRegions.d:141-512): the
// layouts, the lane code shared by the kernels of dh_vreg.hip and the CPU harness of tests/native/vreg_host.cpp, and the
// host-side plan (the checks made before anything is launched, the regions in plan order, the launch groups).  Driver:
// dh_vreg.cpp.
//
// Every record is bound to the regions it touches in one pass instead of every region walking its contig's records:
//   plan     the regions of a contig sorted by the begin of their extended interval (cb), with the prefix maximum of its end (ce)
//   bind     one lane per record: two binary searches give the regions [lo, hi) that can intersect [abpos, aepos) (exact for
//            disjoint regions, a superset for nested ones: every candidate is tested).  Counted per region first: the pairs
//            (abpos < ce && cb < aepos), those of them that span a window start, and the spanning records; then, per launch
//            group of regions, written: (w0, w1 + 1) of every pair that spans a window start, the index of every spanning record
//   span     one workgroup per region: its spanning records ordered by record index, written as their bread
//   region   one workgroup per region: +1 / -1 of its pairs into a difference array (LDS, or a slab of global memory for a
//            region of more than DH_VREG_LDS_WINDOWS entries), then chunks of 256 window starts with a carry: coverage (a sum
//            scan), the last weak start in front of every start (a max scan), "opens an interval" (the start is weak and lies
//            more than wlen behind the last weak one), the interval's rank (a sum scan).  Counted, placed by the host, emitted.
// The order in which the atomics of `bind` claim their slots reaches no result: the pairs are summed, the spanning records sorted.
#ifndef DH_VREG_H
#define DH_VREG_H

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <vector>

#include "../../include/dentist_hip.h"

#if defined(__HIPCC__)
#define VR_HD __host__ __device__ __forceinline__
#else
#define VR_HD inline
#endif

#define VR_BLOCK 256       // threads of a region's workgroup = window starts of one chunk of its scan
#define VR_SPAN_LDS 2048   // a region's spanning records are ranked in LDS up to that many, in global memory beyond
#define VR_SLAB_ALIGN 64   // a region's part of the slab starts at a multiple of that many entries (no cache line is shared)

namespace vr {

struct Rec {  // what is uploaded per record (16 bytes)
    int32_t abpos, aepos, aread, bread;
};
struct Reg {  // a region in plan order (24 bytes); nw = window starts (0: wlen <= 0), pmax = max ce of the contig's regions up to it
    int32_t contig, cb, ce, wlen, nw, pmax;
};
struct Pair {  // a record that spans the window starts [w0, w1e) of a region
    int32_t w0, w1e;
};
struct Job {  // a region of a launch group (48 bytes); nw = 0: no window is considered
    int32_t cb, wlen, nw, pad;
    int64_t pair_at, npairs, slab_at, out_at;  // its pairs, its part of the slab, its first interval in the group's output
};
enum { PAIR = 1, WINDOWS = 2, SPANS = 4 };

// ---- bind.  The regions of the record's contig that can intersect it: from the first whose prefix maximum of ce lies behind
// abpos to the first whose cb is not in front of aepos
VR_HD void candidates(const Rec &r, const int64_t *rptr, const Reg *regs, int64_t *lo_out, int64_t *hi_out)
{
    int64_t lo = rptr[r.aread], hi = rptr[r.aread + 1];
    const int64_t end = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (regs[mid].pmax <= r.abpos)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int64_t first = lo;
    hi = end;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (regs[mid].cb < r.aepos)
            lo = mid + 1;
        else
            hi = mid;
    }
    *lo_out = first;
    *hi_out = lo;
}
// what the record is to the region: PAIR (:458), WINDOWS with the window starts [w0, w1e) it spans (it spans [w, w + wlen) iff
// abpos <= w && w + wlen <= aepos), SPANS (:409-420, both strict)
VR_HD uint32_t classify(const Rec &r, const Reg &g, Pair *p)
{
    uint32_t what = 0;
    if (r.abpos < g.ce && g.cb < r.aepos) {
        what = PAIR;
        const int64_t w0 = (int64_t)(r.abpos > g.cb ? r.abpos : g.cb) - g.cb, w1 = (int64_t)r.aepos - g.wlen - g.cb;
        if (g.nw > 0 && w1 >= w0 && w0 < g.nw) {
            what |= WINDOWS;
            p->w0 = (int32_t)w0;
            p->w1e = (int32_t)(w1 + 1 < g.nw ? w1 + 1 : g.nw);
        }
    }
    if (r.abpos < g.cb && g.ce < r.aepos) what |= SPANS;
    return what;
}

// ---- region.  A window start w is weak below min_cov; `last` is the last weak start in front of it (-1: none).  The weak
// windows [w, w + wlen) fuse while a begin is <= the end before it (:485-498): w opens an interval iff it is weak and lies
// more than wlen behind `last` (a weak start right behind a weak one never does: wlen >= 1)
VR_HD bool opens(int64_t w, int64_t last, int32_t wlen) { return last < 0 || w > last + wlen; }

// ---- span.  The place of a record among the spanning records of its region: the indices are distinct
VR_HD int64_t rank_of(const int64_t *idx, int64_t m, int64_t x)
{
    int64_t k = 0;
    for (int64_t j = 0; j < m; j++) k += idx[j] < x ? 1 : 0;
    return k;
}

// ------------------------------------------------------------------------------------------------------------ host plan
struct Fault {
    int64_t record = -1;  // >= 0: the lowest offending record
    int32_t region = -1;  // >= 0: the lowest offending region
    int32_t contig = -1;  // >= 0: the lowest contig whose length is malformed
    const char *what = "";
    bool any() const { return record >= 0 || region >= 0 || contig >= 0; }
};
struct Plan {
    std::vector<Rec> recs;
    std::vector<Reg> regs;       // plan order: by (contig, cb, ce, input index)
    std::vector<int32_t> perm;   // plan order -> input index
    std::vector<int64_t> rptr;   // ncontigs + 1: the regions of a contig in plan order
};
struct Group {  // regions [s0, s1) of the plan
    int64_t s0, s1;
};
typedef std::function<void(int64_t, const std::function<void(int64_t, int64_t)> &)> ParallelFor;

inline const char *check_record(const dh_la *las, int64_t i, const int64_t *contig_off, int32_t ncontigs)
{
    const dh_la &l = las[i];
    if (l.aread < 0 || l.aread >= ncontigs) return "aread out of range";
    if (i > 0 && l.aread < las[i - 1].aread) return "reads-alignment must be sorted at least by a-read ID";
    if (l.abpos < 0 || l.abpos > l.aepos) return "abpos < 0 or abpos > aepos";
    if ((int64_t)l.aepos > contig_off[l.aread + 1] - contig_off[l.aread]) return "aepos lies behind the end of the contig";
    return nullptr;
}

inline void extended(const dh_region &rg, int64_t clen, int32_t region_context, int32_t *cb, int32_t *ce)
{
    *cb = rg.begin > region_context ? rg.begin - region_context : 0;
    *ce = (int32_t)std::min<int64_t>((int64_t)rg.end + region_context, clen);
}

// everything the host can check, the compact records and the regions in plan order
inline void build_plan(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const dh_region *regions, int32_t nregions,
                       int32_t region_context, int32_t window, const ParallelFor &pfor, Plan &pl, Fault &f)
{
    for (int32_t c = 0; c < ncontigs; c++)
        if (contig_off[c + 1] < contig_off[c] || contig_off[c + 1] - contig_off[c] > (int64_t)INT32_MAX) {
            f.contig = c, f.what = "contig_off decreases or a contig is longer than 2^31 - 1";
            return;
        }
    std::atomic<int64_t> bad{INT64_MAX};
    pl.recs.resize((size_t)n);
    Rec *recs = pl.recs.data();
    pfor(n, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            if (check_record(las, i, contig_off, ncontigs)) {
                int64_t cur = bad.load();
                while (i < cur && !bad.compare_exchange_weak(cur, i)) {
                }
                break;  // (records behind it in this chunk have higher indices)
            }
            recs[i] = Rec{las[i].abpos, las[i].aepos, las[i].aread, las[i].bread};
        }
    });
    if (bad.load() != INT64_MAX) {
        f.record = bad.load();
        f.what = check_record(las, f.record, contig_off, ncontigs);
        return;
    }
    for (int32_t r = 0; r < nregions; r++)
        if (regions[r].contig < 0 || regions[r].contig >= ncontigs || regions[r].begin < 0 || regions[r].end < regions[r].begin) {
            f.region = r, f.what = "bad region";
            return;
        }
    std::vector<Reg> in((size_t)nregions);
    for (int32_t r = 0; r < nregions; r++) {
        Reg &g = in[(size_t)r];
        g.contig = regions[r].contig;
        extended(regions[r], contig_off[g.contig + 1] - contig_off[g.contig], region_context, &g.cb, &g.ce);
        g.wlen = (int32_t)std::min<int64_t>(window, (int64_t)g.ce - g.cb);
        g.nw = g.wlen > 0 ? (g.ce - g.cb) - g.wlen + 1 : 0;
        g.pmax = 0;
    }
    pl.perm.resize((size_t)nregions);
    for (int32_t r = 0; r < nregions; r++) pl.perm[(size_t)r] = r;
    std::sort(pl.perm.begin(), pl.perm.end(), [&](int32_t x, int32_t y) {
        const Reg &p = in[(size_t)x], &q = in[(size_t)y];
        if (p.contig != q.contig) return p.contig < q.contig;
        if (p.cb != q.cb) return p.cb < q.cb;
        if (p.ce != q.ce) return p.ce < q.ce;
        return x < y;
    });
    pl.regs.resize((size_t)nregions);
    pl.rptr.assign((size_t)ncontigs + 1, 0);
    for (int32_t s = 0; s < nregions; s++) {
        Reg &g = pl.regs[(size_t)s];
        g = in[(size_t)pl.perm[(size_t)s]];
        g.pmax = s > 0 && pl.regs[(size_t)s - 1].contig == g.contig ? std::max(pl.regs[(size_t)s - 1].pmax, g.ce) : g.ce;
        pl.rptr[(size_t)g.contig + 1]++;
    }
    for (int32_t c = 0; c < ncontigs; c++) pl.rptr[(size_t)c + 1] += pl.rptr[(size_t)c];
}

// the window starts a region is scanned over once its pairs are counted: none without a pair (:458)
inline int32_t live_windows(const Reg &g, uint64_t pairs) { return pairs > 0 ? g.nw : 0; }
inline bool is_big(int32_t nw, int64_t lds_windows) { return nw > 0 && (int64_t)nw + 1 > lds_windows; }
inline int64_t slab_entries(int32_t nw) { return ((int64_t)nw + 1 + VR_SLAB_ALIGN - 1) / VR_SLAB_ALIGN * VR_SLAB_ALIGN; }
// the launch groups: consecutive regions of the plan whose pair lists, spanning lists and slab parts fit `budget` bytes (one
// region always fits).  cnt: per region its pairs, its pairs with windows, its spanning records
inline void build_groups(const Plan &pl, const uint64_t *cnt, int64_t lds_windows, int64_t budget, std::vector<Group> &groups)
{
    groups.clear();
    const int64_t nreg = (int64_t)pl.regs.size();
    int64_t acc = 0, s0 = 0;
    for (int64_t s = 0; s < nreg; s++) {
        const int32_t nw = live_windows(pl.regs[(size_t)s], cnt[3 * s]);
        const int64_t cost = (int64_t)cnt[3 * s + 1] * (int64_t)sizeof(Pair) + (int64_t)cnt[3 * s + 2] * 12 +
                             (is_big(nw, lds_windows) ? slab_entries(nw) * 4 : 0);
        if (acc + cost > budget && s > s0) {
            groups.push_back(Group{s0, s});
            s0 = s, acc = 0;
        }
        acc += cost;
    }
    if (nreg > s0) groups.push_back(Group{s0, nreg});
}

// the report of a region from its counts (validateRegions.d:384-407)
inline void fill_report(const Reg &g, int64_t spanning, int64_t weak_bp, int32_t min_spanning_reads, dh_region_report *rep)
{
    rep->num_spanning_reads = (int32_t)spanning;
    rep->weak_bp = (int32_t)weak_bp;
    rep->is_valid = spanning >= min_spanning_reads && weak_bp == 0;
    rep->ctx_begin = g.cb;
    rep->ctx_end = g.ce;
}

// the command's mask: per contig the union of the weak (contig, begin, end) triples, sorted, intersecting or touching
// intervals merged (util/region.d:776-816)
inline void merge_mask(const std::vector<int32_t> &weak, int32_t ncontigs, std::vector<int64_t> &ptr, std::vector<int32_t> &iv)
{
    std::vector<size_t> order(weak.size() / 3);
    for (size_t k = 0; k < order.size(); k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
        for (int k = 0; k < 3; k++)
            if (weak[3 * x + k] != weak[3 * y + k]) return weak[3 * x + k] < weak[3 * y + k];
        return false;
    });
    ptr.assign((size_t)ncontigs + 1, 0);
    iv.clear();
    int32_t cur = -1;
    for (size_t k : order) {
        const int32_t c = weak[3 * k], b = weak[3 * k + 1], e = weak[3 * k + 2];
        if (e <= b) continue;
        if (c == cur && b <= iv.back())
            iv.back() = std::max(iv.back(), e);
        else {
            iv.push_back(b);
            iv.push_back(e);
            ptr[(size_t)c + 1]++;
            cur = c;
        }
    }
    for (int32_t c = 0; c < ncontigs; c++) ptr[(size_t)c + 1] += ptr[(size_t)c];
}

}  // namespace vr

#endif
