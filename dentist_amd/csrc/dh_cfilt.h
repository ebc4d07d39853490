// dh_cfilt.h -- the alignment filters of `dentist collect` on the device (dh_la_collect_filter; collectPileUps/filter.d:122-356
// in the order of collectPileUps/package.d:130-141): the layouts, the lane code shared by the kernels of dh_cfilt.hip and the
// CPU harness of tests/native/cfilt_host.cpp, and the host-side plan (the checks made before anything is launched, the compact
// records, the mask's prefix sums).  Driver: dh_cfilt.cpp.  The contract is dh_collect_filter (dh_filter.cpp).
//
//   scan     one lane per record: "starts a chain" (dh_continues_chain), scanned: the unit of every record, the first record of
//            every unit
//   unit     one lane per chain: walks its members -- the unit's fields, covered, unmasked (two binary searches into the prefix
//            sums of the mask's interval lengths per member) -- and judges it by the first of LQ, Improper, WeaklyAnchored it
//            fails; counts the units of its read
//   group    the counts scanned; every unit claims a slot of its read's segment (atomicAdd: the order reaches no result, the
//            sort of Contained has the unit's index as its last key and Ambiguous / Redundant are order-free); one lane per read
//            handles a read of one unit and puts the others on the list of their tier
//   tiers    2..64 units: one wavefront, the units in registers; up to the LDS cap: one workgroup, the order of the units in
//            LDS; above: the same code, the order in a slab of global memory
//   finish   one lane per record: its flag from its unit's; the six counts per wavefront, one atomic each
//
// Contained runs in its order-free form: in the sorted order of a read's units, y is dropped iff it is enabled after stage 3 and
// some x in front of it, enabled after stage 3, reaches it with its scan (every unit of (x, y] has x's aread and lies inside x
// on A), has its strand and contains its forward read interval.  It equals the sequential loop of the host: an x that the loop
// skips was dropped by an x' in front of it whose scan reached x, with x's strand and x's read interval inside its own; then
// every unit x reaches lies inside x' on A as well (x'.abpos <= x.abpos, x.aepos <= x'.aepos, nothing in between ended the
// scan of x'), and what x would drop has x's strand and lies inside x on the read, hence inside x': x' has dropped it already.
// By induction over x' the loop drops what the order-free form drops; the converse is immediate.
#ifndef DH_CFILT_H
#define DH_CFILT_H

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <vector>

#include "../../include/dentist_hip.h"

#if defined(__HIPCC__)
#define CF_HD __host__ __device__ __forceinline__
#else
#define CF_HD inline
#endif

#define CF_BLOCK 256          // threads of a workgroup
#define CF_WAVE_UNITS 64      // a read of up to that many units is one wavefront's
#define CF_LDS_UNITS 8192     // default (and largest) LDS cap: 32 KB of order per workgroup, five workgroups per CU of 160 KB

namespace cf {

struct Rec {  // what is uploaded per record (32 bytes)
    int32_t abpos, aepos, bbpos, bepos, diffs, aread, bread;
    uint32_t flags;
};
struct Unit {  // a chain (40 bytes): the first member's fields, the last member's ends; bfb / bfe: the forward read interval
    int32_t aread, bread, abpos, aepos, bbpos, bepos, bfb, bfe;
    uint32_t st;  // COMP, DIS (disabled on entry or by stages 1-3), RED (the trigger of Redundant holds)
    int32_t pad;
};
enum : uint32_t { COMP = 0x1u, START = 0x4u, NEXT = 0x8u, DIS = 0x20u, RED = 0x100u };
// why[unit]: the stage that dropped the unit, 0 = none (disabled on entry, or enabled)
enum : uint8_t { W_NONE = 0, W_LQ = 1, W_IMPROPER = 2, W_WEAK = 3, W_CONTAINED = 4, W_AMBIGUOUS = 5, W_REDUNDANT = 6 };
struct Opts {
    int32_t ppm, allowance, min_anchor, pad;
};
struct Mask {  // ptr == nullptr: no mask.  pre[j]: the bases of the intervals in front of interval j (all contigs)
    const int64_t *ptr;
    const int32_t *iv;
    const int64_t *pre;
};
// the counters of a call (uint32 each); the number of chains is the 64-bit total of the flag scan, kept behind the six counts
enum { C_WAVE = 0, C_LDS = 1, C_GLOBAL = 2, C_SLAB = 3, C_COUNT = 4 };

// dh_continues_chain (dh_internal.h)
CF_HD bool continues(const Rec &prev, const Rec &cur)
{
    return (cur.flags & NEXT) && !(cur.flags & START) && cur.aread == prev.aread && cur.bread == prev.bread &&
           (cur.flags & COMP) == (prev.flags & COMP);
}

// the masked bases of [b, e) on contig c, b < e; the contig's intervals are sorted and disjoint
CF_HD int64_t masked(const Mask &m, int32_t c, int32_t b, int32_t e)
{
    const int64_t p0 = m.ptr[c], p1 = m.ptr[c + 1];
    int64_t lo = p0, hi = p1;
    while (lo < hi) {  // the first interval that ends behind b
        const int64_t mid = (lo + hi) >> 1;
        if (m.iv[2 * mid + 1] <= b)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int64_t first = lo;
    hi = p1;
    while (lo < hi) {  // the first interval that does not begin in front of e
        const int64_t mid = (lo + hi) >> 1;
        if (m.iv[2 * mid] < e)
            lo = mid + 1;
        else
            hi = mid;
    }
    if (lo <= first) return 0;
    int64_t s = m.pre[lo] - m.pre[first];
    if (m.iv[2 * first] < b) s -= (int64_t)b - m.iv[2 * first];
    if (m.iv[2 * lo - 1] > e) s -= (int64_t)m.iv[2 * lo - 1] - e;
    return s;
}

// the unit of the records [i0, i1) and the stage of 1-3 it fails (dh_filter.cpp:77-92, 116-151, 188-219).  trivial: every
// chain of the input is one record -- the host then takes the record's own length where a chain takes the union of its members
CF_HD uint8_t make_unit(const Rec *recs, int64_t i0, int64_t i1, bool trivial, const Mask &m, const int32_t *alen_of, const int32_t *blen_of,
                        const Opts &o, Unit *out)
{
    const Rec f = recs[i0];
    Unit u;
    u.aread = f.aread, u.bread = f.bread, u.abpos = f.abpos, u.bbpos = f.bbpos, u.aepos = f.aepos, u.bepos = f.bepos;
    uint32_t diffs = 0u, dis = 0u;
    int64_t covered = 0, unmasked = 0;
    int32_t done = -1;
    for (int64_t i = i0; i < i1; i++) {
        const Rec r = recs[i];
        u.aepos = r.aepos, u.bepos = r.bepos;
        diffs += (uint32_t)r.diffs;
        dis |= r.flags & DIS;
        covered += r.aepos - r.abpos;
        if (trivial) {
            unmasked = r.aepos - r.abpos;
            if (m.ptr && r.aepos > r.abpos) unmasked -= masked(m, r.aread, r.abpos, r.aepos);
        } else {
            const int32_t b0 = r.abpos > done ? r.abpos : done;
            if (r.aepos > b0) {
                unmasked += (int64_t)r.aepos - b0 - (m.ptr ? masked(m, r.aread, b0, r.aepos) : 0);
                done = r.aepos;
            }
        }
    }
    const int32_t alen = alen_of[u.aread], blen = blen_of[u.bread];
    const bool comp = (f.flags & COMP) != 0;
    u.bfb = comp ? blen - u.bepos : u.bbpos;
    u.bfe = comp ? blen - u.bbpos : u.bepos;
    u.pad = 0;
    u.st = (f.flags & COMP) | dis;
    uint8_t why = W_NONE;
    if (!dis) {
        const bool begins = u.abpos <= o.allowance || u.bbpos <= o.allowance;
        const bool ends = (int64_t)u.aepos + o.allowance >= alen || (int64_t)u.bepos + o.allowance >= blen;
        if ((int64_t)(int32_t)diffs * 1000000 > (int64_t)o.ppm * covered)
            why = W_LQ;
        else if (!(begins && ends))
            why = W_IMPROPER;
        else if (unmasked <= o.min_anchor)
            why = W_WEAK;
        if (why) u.st |= DIS;
    }
    if (u.bbpos <= u.abpos && (int64_t)u.aepos + blen - u.bepos < alen) u.st |= RED;
    *out = u;
    return why;
}

// ---- stages 4-6 on the units of one read
// AlignmentChain.opCmp within a read (base.d:766-777), the unit's index (= its place in the input) last
CF_HD bool key_less(const Unit &p, int32_t ip, const Unit &q, int32_t iq)
{
    if (p.aread != q.aread) return p.aread < q.aread;
    if (p.abpos != q.abpos) return p.abpos < q.abpos;
    if (p.bbpos != q.bbpos) return p.bbpos < q.bbpos;
    if (p.aepos != q.aepos) return p.aepos < q.aepos;
    if (p.bepos != q.bepos) return p.bepos < q.bepos;
    return ip < iq;
}
// the scan of x goes on over y (sliceUntil, filter.d:178-211)
CF_HD bool scan_goes_on(const Unit &x, const Unit &y) { return y.aread == x.aread && x.abpos <= y.abpos && y.aepos <= x.aepos; }
// y on the scan of x is dropped (if it is still enabled)
CF_HD bool drops(const Unit &x, const Unit &y) { return ((x.st ^ y.st) & COMP) == 0 && x.bfb <= y.bfb && y.bfe <= x.bfe; }
CF_HD bool intersect(const Unit &p, const Unit &q) { return p.bfb < q.bfe && q.bfb < p.bfe; }
CF_HD bool enabled(const Unit &u, uint8_t why) { return !(u.st & DIS) && why == W_NONE; }
CF_HD int32_t pow2ceil(int32_t x)
{
    int32_t p = 1;
    while (p < x) p <<= 1;
    return p;
}
// 0: no unit, 1: one lane, 2: a wavefront, 3: a workgroup with the order in LDS, 4: in the slab
CF_HD int tier_of(int32_t units, int32_t lds_units)
{
    return units <= 1 ? units : units <= CF_WAVE_UNITS ? 2 : units <= lds_units ? 3 : 4;
}
// a read of one unit: only Redundant can apply
CF_HD bool single(const Unit &u, uint8_t *why)
{
    if (!enabled(u, *why) || !(u.st & RED)) return false;
    *why = W_REDUNDANT;
    return true;
}

// the workgroup tiers: ord[0, P) holds the read's units (indices; -1 behind the last, which sorts last), P = pow2ceil(size).
// Every function is what one thread does between two barriers.
CF_HD bool ord_less(const Unit *units, int32_t a, int32_t b)
{
    if (a < 0) return false;
    if (b < 0) return true;
    return key_less(units[a], a, units[b], b);
}
// step (k, j) of the bitonic network, comparator t of P / 2
CF_HD void bt_compare(int32_t *ord, const Unit *units, int32_t t, int32_t k, int32_t j)
{
    const int32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const int32_t a = ord[i], b = ord[l];
    const bool up = (i & k) == 0;
    if (up ? ord_less(units, b, a) : ord_less(units, a, b)) ord[i] = b, ord[l] = a;
}
// the scan of the unit at sorted place x (order-free: x as it left stage 3)
CF_HD void bt_contained(const int32_t *ord, int32_t size, const Unit *units, uint8_t *why, int32_t x)
{
    const Unit ux = units[ord[x]];
    if (ux.st & DIS) return;
    for (int32_t y = x + 1; y < size; y++) {
        const Unit uy = units[ord[y]];
        if (!scan_goes_on(ux, uy)) break;
        if (drops(ux, uy) && !(uy.st & DIS)) why[ord[y]] = W_CONTAINED;
    }
}
// an enabled unit behind place x intersects the enabled unit at x on the read
CF_HD bool bt_ambiguous(const int32_t *ord, int32_t size, const Unit *units, const uint8_t *why, int32_t x)
{
    const Unit ux = units[ord[x]];
    if (!enabled(ux, why[ord[x]])) return false;
    for (int32_t y = x + 1; y < size; y++) {
        const Unit uy = units[ord[y]];
        if (enabled(uy, why[ord[y]]) && intersect(ux, uy)) return true;
    }
    return false;
}

// ------------------------------------------------------------------------------------------------------------ host plan
struct Fault {
    int64_t record = -1;  // >= 0: the lowest record with an id out of range
    int32_t contig = -1;  // >= 0: the lowest contig whose mask is malformed
    const char *what = "";
    bool any() const { return record >= 0 || contig >= 0; }
};
struct Plan {  // recs / alen / blen are the caller's (the driver keeps them in page-locked memory): n, ncontigs, nreads entries
    Rec *recs = nullptr;
    int32_t *alen = nullptr, *blen = nullptr;  // per contig, per read
    std::vector<int64_t> pre;                  // intervals + 1 (empty without a mask)
};
typedef std::function<void(int64_t, const std::function<void(int64_t, int64_t)> &)> ParallelFor;

inline const char *check_mask(const int64_t *ptr, const int32_t *iv, int32_t c, int64_t clen)
{
    if (ptr[c] < 0 || ptr[c + 1] < ptr[c]) return "rep_ptr decreases";
    for (int64_t j = ptr[c]; j < ptr[c + 1]; j++) {
        if (iv[2 * j] < 0 || iv[2 * j + 1] < iv[2 * j] || (int64_t)iv[2 * j + 1] > clen) return "a mask interval lies outside the contig";
        if (j > ptr[c] && iv[2 * j] < iv[2 * j - 1]) return "the mask intervals are not sorted and disjoint";
    }
    return nullptr;
}

// everything the host checks, the compact records, the lengths and the prefix sums of the mask
inline void build_plan(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                       const int64_t *rep_ptr, const int32_t *rep_iv, const ParallelFor &pfor, Plan &pl, Fault &f)
{
    std::atomic<int64_t> bad{INT64_MAX};
    Rec *recs = pl.recs;
    pfor(n, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            const dh_la &l = las[i];
            if (l.aread < 0 || l.aread >= ncontigs || l.bread < 0 || l.bread >= nreads) {
                int64_t cur = bad.load();
                while (i < cur && !bad.compare_exchange_weak(cur, i)) {
                }
                break;  // (records behind it in this chunk have higher indices)
            }
            recs[i] = Rec{l.abpos, l.aepos, l.bbpos, l.bepos, l.diffs, l.aread, l.bread, l.flags};
        }
    });
    if (bad.load() != INT64_MAX) {
        f.record = bad.load();
        f.what = las[f.record].aread < 0 || las[f.record].aread >= ncontigs ? "aread out of range" : "bread out of range";
        return;
    }
    if (rep_ptr)
        for (int32_t c = 0; c < ncontigs; c++)
            if (const char *w = check_mask(rep_ptr, rep_iv, c, contig_off[c + 1] - contig_off[c])) {
                f.contig = c, f.what = w;
                return;
            }
    for (int32_t c = 0; c < ncontigs; c++) pl.alen[c] = (int32_t)(contig_off[c + 1] - contig_off[c]);
    int32_t *blen = pl.blen;
    pfor(nreads, [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; r++) blen[r] = (int32_t)(read_off[r + 1] - read_off[r]);
    });
    pl.pre.clear();
    if (rep_ptr) {
        const int64_t m = ncontigs > 0 ? rep_ptr[ncontigs] : 0;
        pl.pre.assign((size_t)m + 1, 0);
        for (int64_t j = 0; j < m; j++) {
            const bool used = ncontigs > 0 && j >= rep_ptr[0];  // (intervals in front of the first contig's belong to no contig)
            pl.pre[(size_t)j + 1] = pl.pre[(size_t)j] + (used ? (int64_t)rep_iv[2 * j + 1] - rep_iv[2 * j] : 0);
        }
    }
}

}  // namespace cf

#endif
