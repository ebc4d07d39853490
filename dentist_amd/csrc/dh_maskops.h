// dh_maskops.h -- mask algebra on the device (dh_mask_combine: `dentist merge-masks` commands/mergeMasks.d:47-53, `dentist
// filter-mask` commands/filterMask.d:124-159, the ReferenceRegion operators util/region.d:776-1149; dh_la_tandem_mask: TANmask):
// the key layout, the lane code shared by the kernels of dh_maskops.hip and the CPU harness of tests/native/maskops_host.cpp,
// and the host-side plan (the checks made before anything is launched, the launch groups).  Driver: dh_maskops.cpp.  The
// contract is stated at dh_mask_combine in include/dentist_hip.h.
//
// Nothing here is organised per contig: every step is one lane per interval, event, boundary or run of the whole launch group.
//
//   events   one lane per interval: a non-empty one writes two keys  unit << (posbits + 2) | pos << 2 | is_subtract << 1 | is_end
//            (count, scan, place).  `unit` is the contig of the group, or mask * contigs + contig when the masks are normalised
//            on their own first (min_count > 1: each mask counts once per base).
//   sort     rx::  a device-wide stable LSD radix sort of 64-bit keys, 8-bit digits, only the digits in use; nothing of it
//            knows about masks.  Per pass: a histogram per tile, one scan over hist[digit][tile], a scatter whose in-tile rank
//            comes from ballots per digit bit (the lanes of a wavefront with the same digit, counted below the lane), a count
//            per wavefront through LDS and a running count per digit over the rounds of the tile -- never from an atomic.
//   sweep    two deltas per event from the low key bits, two scans: the coverage and the subtract depth behind every event;
//            only the last event of a distinct (unit, pos) is a boundary; the boundaries are compacted, an edge is a boundary
//            whose kept state differs from the boundary before it; edges alternate begin, end: edge 2r and 2r + 1 are run r.
//   filter   head flags (not joinable with the run before), a scan, the head writes begin and the tail end; a size flag, a scan,
//            compaction.
//   ptr      one lane per unit boundary: a binary search in the runs.
#ifndef DH_MASKOPS_H
#define DH_MASKOPS_H

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <string>
#include <vector>

#include "../../include/dentist_hip.h"

#if defined(__HIPCC__)
#define MO_HD __host__ __device__ __forceinline__
#else
#define MO_HD inline
#endif

#define MO_BLOCK 256        // threads of a workgroup
#define RX_TILE_KEYS 2048   // keys of a workgroup tile of the sort: 8 rounds of 256
#define RX_TILE_KEYS_MIN 256
// what a launch group takes on the device per input interval (the pair, its flag, two keys in two buffers, per event three
// scanned words and a boundary, per run three stages of two words) and per contig and mask (offsets)
#define MO_BYTES_PER_INTERVAL 192
#define MO_BYTES_PER_CONTIG 16

namespace rx {
typedef unsigned long long u64;
// pass p sorts by bits [8p, 8p + 8)
MO_HD int32_t digit(u64 key, int32_t pass) { return (int32_t)((key >> (8 * pass)) & 255u); }
MO_HD int32_t passes_of_bits(int32_t bits) { return (bits + 7) / 8; }
// ball[b]: the lanes of the wavefront whose digit has bit b set; active: the lanes that hold a key.  The lanes with `digit`.
MO_HD u64 peers(const u64 *ball, int32_t digit, u64 active)
{
    u64 m = active;
    for (int b = 0; b < 8; b++) m &= ((digit >> b) & 1) ? ball[b] : ~ball[b];
    return m;
}
MO_HD int32_t below(u64 m, int32_t lane) { return (int32_t)__builtin_popcountll(m & (((u64)1 << lane) - 1)); }
MO_HD bool leads(u64 m, int32_t lane) { return (m & (((u64)1 << lane) - 1)) == 0; }
}  // namespace rx

namespace mo {

typedef unsigned long long u64;

struct Opts {  // dh_mask_opts
    int32_t min_count, min_gap, min_interval, pad_;
};

MO_HD int32_t bits_of(u64 v)  // the bits needed for values 0 .. v
{
    int32_t b = 0;
    while (v) b++, v >>= 1;
    return b;
}
MO_HD u64 event_key(u64 unit, int32_t pos, bool is_sub, bool is_end, int32_t posbits)
{
    return (unit << (posbits + 2)) | ((u64)(uint32_t)pos << 2) | (is_sub ? 2u : 0u) | (is_end ? 1u : 0u);
}
MO_HD u64 key_at(u64 k) { return k >> 2; }  // unit << posbits | pos
MO_HD u64 at_unit(u64 at, int32_t posbits) { return at >> posbits; }
MO_HD int32_t at_pos(u64 at, int32_t posbits) { return (int32_t)(at & (((u64)1 << posbits) - 1)); }
MO_HD uint32_t delta_add(u64 k) { return (k & 2u) ? 0u : (k & 1u) ? 0xFFFFFFFFu : 1u; }
MO_HD uint32_t delta_sub(u64 k) { return (k & 2u) ? ((k & 1u) ? 0xFFFFFFFFu : 1u) : 0u; }
// the state behind a boundary
MO_HD bool kept(uint32_t cov, uint32_t sub, int32_t min_count) { return cov >= (uint32_t)min_count && sub == 0; }
// event i of n sorted keys is the last of its (unit, pos); next: key i + 1
MO_HD bool boundary(u64 k, u64 next, bool is_last) { return is_last || key_at(k) != key_at(next); }
// runs a and b (a in front): b starts a group of its own (filterMask.d:131-143 joins iff same contig && a.end + min_gap >= b.begin)
MO_HD bool heads(u64 a_end, u64 b_begin, int32_t posbits, int32_t min_gap)
{
    return at_unit(a_end, posbits) != at_unit(b_begin, posbits) || (int64_t)at_pos(a_end, posbits) + min_gap < (int64_t)at_pos(b_begin, posbits);
}
MO_HD bool long_enough(u64 b, u64 e, int32_t posbits, int32_t min_interval) { return at_pos(e, posbits) - at_pos(b, posbits) >= min_interval; }
// the tandem rule (tools/TANmask): the record's interval on its read, whether it counts
MO_HD bool tandem_interval(const dh_la &l, int32_t min_len, int32_t *b, int32_t *e)
{
    if (l.aread != l.bread || (l.flags & DH_FLAG_COMP)) return false;
    *b = l.abpos < l.bbpos ? l.abpos : l.bbpos;
    *e = l.aepos > l.bepos ? l.aepos : l.bepos;
    return *e > *b && (int64_t)*e - *b >= min_len;
}
// the first index of v[0 .. n) with v[i] > x
template <class T>
MO_HD int64_t upper_bound(const T *v, int64_t n, T x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] <= x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}
// the first index of v[0 .. n) with v[i] >= x
MO_HD int64_t lower_bound(const u64 *v, int64_t n, u64 x)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (v[mid] < x)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------------------ host plan
struct Fault {
    int32_t mask = -1;  // >= 0: the lowest offending mask (nmasks: the subtract mask)
    int32_t contig = -1;
    int64_t interval = -1;  // of that mask
    const char *what = "";
    bool any() const { return mask >= 0 || contig >= 0 || interval >= 0; }
};
struct Group {  // contigs [c0, c1), `intervals` of all masks, `nonempty` of them; the subtract mask's share of both
    int32_t c0, c1;
    int64_t intervals, nonempty, maxlen, sub_intervals, sub_nonempty;
};
struct Plan {
    std::vector<Group> groups;
    int64_t intervals = 0;
};

inline const char *check_opts(const Opts &o, int32_t nmasks)
{
    if (o.min_count < 1) return "min_count < 1";
    if (o.min_count > nmasks) return "min_count > nmasks";
    if (o.min_gap < 0) return "a negative min_gap";
    if (o.min_interval < 0) return "a negative min_interval";
    return nullptr;
}

typedef std::function<void(int64_t, const std::function<void(int64_t, int64_t)> &)> ParallelFor;

inline const char *check_interval(int32_t b, int32_t e, int64_t len)
{
    return b < 0 ? "begin < 0" : b > e ? "begin > end" : e > len ? "end behind the contig's end" : nullptr;
}

// masks 0 .. nmasks - 1 are the inputs, mask nmasks the subtract mask (ptr NULL: none).  The lowest mask with a fault wins, in it
// the ptr faults in front of the interval faults, the lowest index each.  The intervals of a mask are walked in chunks by pfor
// (a chunk finds its contig by a binary search); on the way the non-empty intervals of every contig are counted: ne_in over the
// input masks, ne_sub of the subtract mask (ncontigs entries each).
inline void check_masks(const int64_t *const *ptr, const int32_t *const *iv, int32_t nmasks, const int64_t *contig_off, int32_t ncontigs,
                        const ParallelFor &pfor, std::vector<int64_t> &ne_in, std::vector<int64_t> &ne_sub, Fault &f)
{
    ne_in.assign((size_t)ncontigs, 0), ne_sub.assign((size_t)ncontigs, 0);
    for (int32_t c = 0; c < ncontigs; c++) {
        const int64_t len = contig_off[c + 1] - contig_off[c];
        if (len < 0 || len > INT32_MAX) {
            f.contig = c, f.what = len < 0 ? "contig_off decreases" : "longer than 2^31 - 1";
            return;
        }
    }
    for (int32_t k = 0; k <= nmasks; k++) {
        const int64_t *p = ptr[k];
        if (!p) continue;
        if (p[0] != 0) {
            f.mask = k, f.what = "ptr does not start at 0";
            return;
        }
        for (int32_t c = 0; c < ncontigs; c++)
            if (p[c + 1] < p[c]) {
                f.mask = k, f.contig = c, f.what = "ptr decreases";
                return;
            }
        std::atomic<int64_t> bad_at{INT64_MAX};
        int64_t *ne = (k == nmasks ? ne_sub : ne_in).data();
        const int32_t *v = iv[k];
        pfor(p[ncontigs], [&](int64_t lo, int64_t hi) {
            int32_t c = (int32_t)upper_bound(p, (int64_t)ncontigs + 1, lo) - 1;  // p[c] <= lo < p[c + 1]
            int64_t len = contig_off[c + 1] - contig_off[c], count = 0;
            for (int64_t i = lo; i < hi; i++) {
                if (i >= p[c + 1]) {
                    if (count) __atomic_fetch_add(&ne[c], count, __ATOMIC_RELAXED);
                    count = 0;
                    while (i >= p[c + 1]) c++;
                    len = contig_off[c + 1] - contig_off[c];
                }
                if (check_interval(v[2 * i], v[2 * i + 1], len)) {
                    int64_t cur = bad_at.load();
                    while (i < cur && !bad_at.compare_exchange_weak(cur, i)) {
                    }
                    break;  // (the intervals behind it in this chunk have higher indices)
                }
                count += v[2 * i] < v[2 * i + 1];
            }
            if (count) __atomic_fetch_add(&ne[c], count, __ATOMIC_RELAXED);
        });
        if (bad_at.load() != INT64_MAX) {
            const int64_t i = bad_at.load();
            const int32_t c = (int32_t)upper_bound(p, (int64_t)ncontigs + 1, i) - 1;
            f.mask = k, f.contig = c, f.interval = i, f.what = check_interval(v[2 * i], v[2 * i + 1], contig_off[c + 1] - contig_off[c]);
            return;
        }
    }
}

// dh_la_tandem_mask: the reads' lengths, then every counted record, the lowest offending index each; returns the counted records
inline int64_t check_tandem(const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads, int32_t first_read, int32_t min_len,
                            int64_t *maxlen, std::string &why)
{
    *maxlen = 0;
    for (int32_t r = 0; r < nreads; r++) {
        const int64_t len = read_off[r + 1] - read_off[r];
        if (len < 0 || len > INT32_MAX) {
            why = "read " + std::to_string(r) + (len < 0 ? ": read_off decreases" : ": longer than 2^31 - 1");
            return -1;
        }
        *maxlen = std::max(*maxlen, len);
    }
    int64_t counted = 0;
    for (int64_t i = 0; i < n; i++) {
        int32_t b, e;
        if (!tandem_interval(las[i], min_len, &b, &e)) continue;
        const int64_t r = (int64_t)las[i].aread - first_read;
        const char *w = r < 0 || r >= nreads ? "aread outside the reads" : b < 0 ? "begin < 0" : e > read_off[r + 1] - read_off[r] ? "end behind the read's end" : nullptr;
        if (w) {
            why = "record " + std::to_string(i) + ": " + w;
            return -1;
        }
        counted++;
    }
    return counted;
}

inline std::string fault_text(const Fault &f, int32_t nmasks)
{
    std::string s;
    if (f.mask >= 0) s += f.mask == nmasks ? "subtract mask: " : "mask " + std::to_string(f.mask) + ": ";
    if (f.contig >= 0) s += "contig " + std::to_string(f.contig) + ": ";
    if (f.interval >= 0) s += "interval " + std::to_string(f.interval) + ": ";
    return s + f.what;
}

// the launch groups: whole contigs, as many as chunk_bytes hold; one contig always fits.  ne_in / ne_sub: check_masks' counts
inline void make_groups(const int64_t *const *ptr, int32_t nmasks, const int64_t *contig_off, int32_t ncontigs, const std::vector<int64_t> &ne_in,
                        const std::vector<int64_t> &ne_sub, int64_t chunk_bytes, Plan &pl)
{
    pl.groups.clear(), pl.intervals = 0;
    int32_t c0 = 0;
    while (c0 < ncontigs) {
        Group g{c0, c0, 0, 0, 0, 0, 0};
        int64_t bytes = 0;
        while (g.c1 < ncontigs) {
            int64_t all = 0, sub = 0;
            for (int32_t k = 0; k <= nmasks; k++)
                if (ptr[k]) all += ptr[k][g.c1 + 1] - ptr[k][g.c1], sub += k == nmasks ? ptr[k][g.c1 + 1] - ptr[k][g.c1] : 0;
            const int64_t add = all * MO_BYTES_PER_INTERVAL + (int64_t)(nmasks + 1) * MO_BYTES_PER_CONTIG;
            if (g.c1 > g.c0 && bytes + add > chunk_bytes) break;
            bytes += add, g.intervals += all, g.sub_intervals += sub;
            g.nonempty += ne_in[(size_t)g.c1] + ne_sub[(size_t)g.c1], g.sub_nonempty += ne_sub[(size_t)g.c1];
            g.maxlen = std::max(g.maxlen, contig_off[g.c1 + 1] - contig_off[g.c1]);
            g.c1++;
        }
        pl.intervals += g.intervals;
        pl.groups.push_back(g);
        c0 = g.c1;
    }
}

// the elements of every device buffer of a launch group: n_in lanes of input, no sweep with more than cap_ev events (even)
struct Sizes {
    size_t idx, ev1, hist, sums, ctr, ptr, keys, runs, bkept, iv;
    Sizes(int64_t n_in, int64_t cap_ev, int32_t ncg, int32_t tile_keys)
    {
        const size_t ev = (size_t)cap_ev, ntiles = (ev + (size_t)tile_keys - 1) / (size_t)tile_keys;
        idx = (size_t)n_in + 1, ev1 = ev + 1, hist = 256 * ntiles;
        sums = std::max(std::max(hist, ev1), idx) / 2048 + 1;  // (dhk_scan: one per 2048 values)
        ctr = 4, ptr = (size_t)ncg + 1, keys = ev, runs = ev / 2 + 1, bkept = ev, iv = 2 * (ev / 2 + 1);
    }
};

// a decimal number of MiB (default 1024)
inline int64_t chunk_bytes_of(const char *e)
{
    double mb = 1024.0;
    if (e) mb = atof(e);
    if (!(mb > 0.0)) mb = 1024.0;
    return std::max<int64_t>(1, (int64_t)(std::min(mb, 1048576.0) * 1048576.0));
}

}  // namespace mo

#endif
