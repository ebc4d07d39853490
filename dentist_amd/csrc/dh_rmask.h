// dh_rmask.h -- `dentist mask-repetitive-regions` on the device (dh_la_repeat_mask; commands/maskRepetitiveRegions.d:129-430):
// the layouts, the lane code shared by the kernels of dh_rmask.hip and the CPU harness of tests/native/rmask_host.cpp, and the
// host-side plan (the checks made before anything is launched, the compact records, the launch groups).  Driver: dh_rmask.cpp.
// The contract is stated at dh_la_repeat_mask in include/dentist_hip.h.
//
//   start    one lane per record: "starts a chain" (cf::continues; k_cf_start of dh_cfilt.hip, shared), scanned: the unit of every
//            chain start.  Records are grouped by aread and a contig's first record starts a chain, so the units of contig c are
//            the consecutive numbers [uid[first record of c], uid[first record of c + 1]) and its events the slots at twice those:
//            no count, no partition, no atomics.
//   events   the lane of a chain start walks its members: the unit's interval, its improper bit, two 64-bit keys
//            position << 2 | is_end << 1 | improper at slots 2u and 2u + 1.  Keys need no payload.
//   classify one lane per contig: its segment and the list of its tier by the number of events.
//   sort     up to 64 events: one wavefront ranks the keys in registers; up to the LDS cap: one workgroup, a bitonic network in
//            LDS; more: the same network on a slab of global memory, every step a launch over all workgroups.  The sorted keys go
//            back to the segment.
//   cover    one wavefront per contig walks the sorted keys in tiles of 64 with two running sums (all, improper) carried from
//            tile to tile.  At the last key of each distinct position both coverages behind it are known; the state in front of
//            it is that of the distinct position before (a ballot).  Run once to count the runs of a contig and, after a scan of
//            the counts, once to place them: the k-th start and the k-th end of a contig are one interval, no atomics.
//   union    one lane per contig merges its two sorted disjoint lists (count, scan, place).
#ifndef DH_RMASK_H
#define DH_RMASK_H

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <string>
#include <vector>

#include "dh_cfilt.h"

#define RM_BLOCK 256        // threads of a workgroup
#define RM_WAVE_EVENTS 64   // a contig of up to that many events is sorted by one wavefront
#define RM_LDS_EVENTS 8192  // default (and largest) LDS cap: 64 KB of keys per workgroup
#define RM_LDS_EVENTS_MIN 1024
// what a launch group takes on the device, per record (compact record, flag, unit, two keys, their share of the slab, the three
// interval lists) and per contig (offsets, segment, tier lists, counts)
#define RM_BYTES_PER_RECORD 120
#define RM_BYTES_PER_CONTIG 64

namespace rm {

using cf::Rec;
typedef unsigned long long u64;

struct Opts {  // dh_repeat_opts
    int32_t lower, upper, improper_lower, improper_upper, allowance, with_improper;
};
// the counters of a launch group (64 bits each): contigs per tier, the slab's keys, the improper units
enum { C_ZERO = 0, C_WAVE = 1, C_LDS = 2, C_GLOBAL = 3, C_SLAB = 4, C_IMPROPER = 5, C_COUNT = 6 };

const u64 PAD = ~0ull;  // sorts behind every key; its position equals no contig position

CF_HD u64 event_key(int32_t pos, bool is_end, bool improper) { return ((u64)(uint32_t)pos << 2) | (is_end ? 2u : 0u) | (improper ? 1u : 0u); }
CF_HD int64_t key_pos(u64 k) { return (int64_t)(k >> 2); }
CF_HD int32_t delta_all(u64 k) { return k == PAD ? 0 : (k & 2u) ? -1 : 1; }
CF_HD int32_t delta_improper(u64 k) { return (k & 1u) ? delta_all(k) : 0; }
CF_HD bool bad(int32_t cov, int32_t lower, int32_t upper) { return cov < lower || cov > upper; }
// 0: no event, 1: a wavefront, 2: a workgroup with the keys in LDS, 3: in the slab
CF_HD int tier_of(int32_t events, int32_t lds_events) { return events == 0 ? 0 : events <= RM_WAVE_EVENTS ? 1 : events <= lds_events ? 2 : 3; }

// the unit whose first record is recs[i] (of m): its two keys; returns whether it is improper (false without with_improper)
CF_HD bool unit_events(const Rec *recs, int64_t i, int64_t m, const int32_t *alen_of, const int32_t *blen_of, const Opts &o, u64 *begin_key,
                       u64 *end_key)
{
    const Rec f = recs[i];
    Rec l = f;
    for (int64_t j = i + 1; j < m && cf::continues(l, recs[j]); j++) l = recs[j];
    bool improper = false;
    if (o.with_improper) {
        const bool begins = f.abpos <= o.allowance || f.bbpos <= o.allowance;
        const bool ends = (int64_t)l.aepos + o.allowance >= alen_of[f.aread] || (int64_t)l.bepos + o.allowance >= blen_of[f.bread];
        improper = !(begins && ends);
    }
    *begin_key = event_key(f.abpos, false, improper);
    *end_key = event_key(l.aepos, true, improper);
    return improper;
}

// the wave tier: lane `lane` holds `me`; key `kz` of lane z lies in front of it
CF_HD int32_t ranks_before(u64 kz, int32_t z, u64 me, int32_t lane) { return kz < me || (kz == me && z < lane) ? 1 : 0; }

// the workgroup tiers: step (k, j) of the bitonic network over P keys (PAD behind the last), comparator t of P / 2
CF_HD void bt_compare(u64 *key, int32_t t, int32_t k, int32_t j)
{
    const int32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
    const u64 a = key[i], b = key[l];
    const bool up = (i & k) == 0;
    if (up ? b < a : a < b) key[i] = b, key[l] = a;
}

// cover, one tile of 64 sorted keys.  last: the lanes with the last key of a distinct position; badb: those of them behind which
// the coverage is bad (a position at the contig's end has nothing behind it: never bad); prev_bad: the state in front of the
// tile's first position.  A run starts at the lane's position iff the zone behind it is bad and the zone in front of it is not,
// and ends there in the opposite case.
CF_HD void lane_edges(int32_t lane, u64 last, u64 badb, bool prev_bad, bool *starts, bool *ends)
{
    const bool mine = (last >> lane) & 1u;
    const u64 below = last & (((u64)1 << lane) - 1);
    const bool before = below ? ((badb >> (63 - __builtin_clzll(below))) & 1u) != 0 : prev_bad;
    const bool after = (badb >> lane) & 1u;
    *starts = mine && after && !before;
    *ends = mine && before && !after;
}
// the state behind the tile
CF_HD bool state_behind(u64 last, u64 badb, bool prev_bad) { return last ? ((badb >> (63 - __builtin_clzll(last))) & 1u) != 0 : prev_bad; }
CF_HD int32_t lanes_below(u64 b, int32_t lane) { return (int32_t)__builtin_popcountll(b & (((u64)1 << lane) - 1)); }

// union: the ReferenceRegion union (util/region.d:776-816) of two ascending disjoint lists of one contig; intersecting or
// touching intervals are merged.  out == nullptr: count only.
CF_HD int32_t merge_union(const int32_t *a, int32_t na, const int32_t *b, int32_t nb, int32_t *out)
{
    int32_t ia = 0, ib = 0, n = 0, cb = 0, ce = 0;
    bool open = false;
    while (ia < na || ib < nb) {
        const bool take_a = ib >= nb || (ia < na && a[2 * ia] <= b[2 * ib]);
        const int32_t s = take_a ? a[2 * ia] : b[2 * ib], e = take_a ? a[2 * ia + 1] : b[2 * ib + 1];
        if (take_a)
            ia++;
        else
            ib++;
        if (open && s <= ce) {
            if (e > ce) ce = e;
            continue;
        }
        if (open) {
            if (out) out[2 * n] = cb, out[2 * n + 1] = ce;
            n++;
        }
        open = true, cb = s, ce = e;
    }
    if (open) {
        if (out) out[2 * n] = cb, out[2 * n + 1] = ce;
        n++;
    }
    return n;
}

// ------------------------------------------------------------------------------------------------------------ host plan
struct Fault {
    int64_t record = -1;  // >= 0: the lowest offending record
    int32_t contig = -1;  // >= 0: the lowest offending contig
    const char *what = "";
    bool any() const { return record >= 0 || contig >= 0; }
};
struct Group {  // contigs [c0, c1), records [r0, r1)
    int32_t c0, c1;
    int64_t r0, r1;
};
struct Plan {  // recs / alen / blen are the caller's: n, ncontigs, nreads entries (blen unused without with_improper)
    Rec *recs = nullptr;
    int32_t *alen = nullptr, *blen = nullptr;
    std::vector<int64_t> rec_off;  // ncontigs + 1: the records of every contig
    std::vector<Group> groups;
};
typedef cf::ParallelFor ParallelFor;

inline const char *check_opts(const Opts &o)
{
    if (o.lower < 0 || o.upper < 0 || o.allowance < 0) return "a negative bound or allowance";
    if (o.lower > o.upper) return "lower > upper";
    if (o.with_improper && (o.improper_lower < 0 || o.improper_upper < 0)) return "a negative bound or allowance";
    if (o.with_improper && o.improper_lower > o.improper_upper) return "improper_lower > improper_upper";
    return nullptr;
}

// what is wrong with record i, nullptr if nothing (the records in front of it are fine)
inline const char *check_record(const dh_la *las, int64_t i, int64_t n, const int64_t *contig_off, int32_t ncontigs, int32_t nreads,
                                bool with_improper)
{
    const dh_la &l = las[i];
    if (l.aread < 0 || l.aread >= ncontigs) return "aread out of range";
    if (with_improper && (l.bread < 0 || l.bread >= nreads)) return "bread out of range";
    if (i > 0 && l.aread < las[i - 1].aread) return "aread below the record before it (the records must be sorted by aread)";
    if (l.abpos < 0) return "abpos < 0";
    if (l.abpos > l.aepos) return "abpos > aepos";
    if ((int64_t)l.aepos > contig_off[l.aread + 1] - contig_off[l.aread]) return "aepos behind the contig's end";
    auto rec = [&](int64_t k) { return Rec{0, 0, 0, 0, 0, las[k].aread, las[k].bread, las[k].flags}; };
    if (i == 0 || !cf::continues(rec(i - 1), rec(i))) {  // a chain start
        int64_t e = i;
        while (e + 1 < n && cf::continues(rec(e), rec(e + 1))) e++;
        if (las[e].aepos < l.abpos) return "the chain that starts here ends before it begins";
    }
    return nullptr;
}

// the launch groups: whole contigs, as many as chunk_bytes hold; one contig always fits
inline void make_groups(const std::vector<int64_t> &rec_off, int32_t ncontigs, int64_t chunk_bytes, std::vector<Group> &groups)
{
    groups.clear();
    int32_t c0 = 0;
    while (c0 < ncontigs) {
        int32_t c1 = c0;
        int64_t bytes = 0;
        while (c1 < ncontigs) {
            const int64_t add = (rec_off[c1 + 1] - rec_off[c1]) * RM_BYTES_PER_RECORD + RM_BYTES_PER_CONTIG;
            if (c1 > c0 && bytes + add > chunk_bytes) break;
            bytes += add, c1++;
        }
        groups.push_back(Group{c0, c1, rec_off[c0], rec_off[c1]});
        c0 = c1;
    }
}

// everything the host checks, the compact records, the lengths, the records of every contig and the launch groups
inline void build_plan(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                       const Opts &o, int64_t chunk_bytes, const ParallelFor &pfor, Plan &pl, Fault &f)
{
    for (int32_t c = 0; c < ncontigs; c++) {
        const int64_t len = contig_off[c + 1] - contig_off[c];
        if (len < 0 || len > INT32_MAX) {
            f.contig = c, f.what = len < 0 ? "contig_off decreases" : "longer than 2^31 - 1";
            return;
        }
        pl.alen[c] = (int32_t)len;
    }
    std::atomic<int64_t> bad_at{INT64_MAX};
    Rec *recs = pl.recs;
    pfor(n, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            if (check_record(las, i, n, contig_off, ncontigs, nreads, o.with_improper != 0)) {
                int64_t cur = bad_at.load();
                while (i < cur && !bad_at.compare_exchange_weak(cur, i)) {
                }
                break;  // (records behind it in this chunk have higher indices)
            }
            const dh_la &l = las[i];
            recs[i] = Rec{l.abpos, l.aepos, l.bbpos, l.bepos, l.diffs, l.aread, l.bread, l.flags};
        }
    });
    if (bad_at.load() != INT64_MAX) {
        f.record = bad_at.load();
        f.what = check_record(las, f.record, n, contig_off, ncontigs, nreads, o.with_improper != 0);
        return;
    }
    if (o.with_improper) {
        int32_t *blen = pl.blen;
        pfor(nreads, [&](int64_t lo, int64_t hi) {
            for (int64_t r = lo; r < hi; r++) blen[r] = (int32_t)std::min<int64_t>(read_off[r + 1] - read_off[r], INT32_MAX);
        });
    }
    pl.rec_off.assign((size_t)ncontigs + 1, n);
    int64_t i = 0;
    for (int32_t c = 0; c < ncontigs; c++) {
        pl.rec_off[(size_t)c] = i;
        while (i < n && las[i].aread == c) i++;
    }
    for (int32_t c = 0; c < ncontigs; c++)
        if (pl.rec_off[(size_t)c + 1] - pl.rec_off[(size_t)c] > ((int64_t)1 << 29)) {  // (its padded keys are counted in 32 bits)
            f.contig = c, f.what = "more than 2^29 records";
            return;
        }
    make_groups(pl.rec_off, ncontigs, chunk_bytes, pl.groups);
}

// DH_RMASK_CHUNK_MB: a decimal number of MiB (default 1024)
inline int64_t chunk_bytes_of_env()
{
    double mb = 1024.0;
    if (const char *e = getenv("DH_RMASK_CHUNK_MB")) mb = atof(e);
    if (!(mb > 0.0)) mb = 1024.0;
    return std::max<int64_t>(1, (int64_t)(std::min(mb, 1048576.0) * 1048576.0));
}

}  // namespace rm

#endif
