// dh_pmask.h -- mask propagation (dh_la_propagate_mask; `dentist propagate-mask`, commands/propagateMask.d:136-305): the
// layouts, the lane code shared by the kernels of dh_pmask.hip and the CPU harness of tests/native/pmask_host.cpp, and the
// host-side plan (the checks made before anything is launched, the launch groups, the bit offsets of the destination
// sequences and the destination ranges).  Driver: dh_pmask.cpp.
//
// The union per destination sequence is taken on a bitmap with one bit per destination base, not by sorting:
//   plan       one lane per record: the mask intervals of its A sequence that intersect [abpos, aepos) -> lo, cnt
//   translate  one wavefront per record with cnt > 0: the trace is walked once in chunks of 64 tiles (a wave scan of the
//              tiles' b-bases plus the carry of the chunks before); the lanes hold 64 intervals per batch and pick the prefix
//              up at the trace-point index of their cut begin (floor) and cut end (ceil) -> (read, begin, end) at a position
//              the input fixes
//   paint      atomicOr of the bits [boff[read] + begin, boff[read] + end)
//   runs       starts and ends of the runs of set bits per word, counted, scanned, emitted: the k-th start and the k-th end
//              of the bitmap are the same run
// Sequence r starts at bit boff[r], a multiple of 32, and boff[r + 1] = roundup32(boff[r] + len_r + 1): the last bit in front
// of a sequence is never set, so no run crosses into the next sequence, every run ends inside its own sequence's words, and
// the carry into the first word of a sequence is 0 without anybody looking the sequence up.
#ifndef DH_PMASK_H
#define DH_PMASK_H

#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <vector>

#include "../../include/dentist_hip.h"

#if defined(__HIPCC__)
#define PM_HD __host__ __device__ __forceinline__
#else
#define PM_HD inline
#endif

#define PM_SHORT_WORDS 4   // a raw interval of up to that many bitmap words is painted by one lane, a longer one by its wavefront
#define PM_GROUP_WORDS 8   // the run counters are kept per group of that many words (a quarter of the bitmap's size for both)

namespace pm {

struct Rec {  // what is uploaded per record (40 bytes)
    int32_t abpos, aepos, bbpos, blen, aread, bread;
    uint32_t comp;
    int32_t ntp;   // trace tiles = tlen / 2
    int64_t toff;
};
struct Raw {  // one propagated interval before the union; b == e: empty
    int32_t rd, b, e;
};

PM_HD int32_t imax(int32_t x, int32_t y) { return x > y ? x : y; }
PM_HD int32_t imin(int32_t x, int32_t y) { return x < y ? x : y; }

// ---- plan: one lane per record.  lo = the first interval of the A sequence that ends after abpos, cnt = the intervals from
// there that begin before aepos (the mask of a sequence is sorted and disjoint: that is checked before the launch)
PM_HD void plan_lane(const Rec &r, const int64_t *mask_ptr, const int32_t *mask_iv, int64_t *lo_out, uint32_t *cnt_out)
{
    int64_t lo = mask_ptr[r.aread], hi = mask_ptr[r.aread + 1];
    const int64_t m1 = hi;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (mask_iv[2 * mid + 1] <= r.abpos)
            lo = mid + 1;
        else
            hi = mid;
    }
    const int64_t first = lo;
    hi = m1;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (mask_iv[2 * mid] < r.aepos)
            lo = mid + 1;
        else
            hi = mid;
    }
    *lo_out = first;
    *cnt_out = (uint32_t)(lo - first);
}

// ---- translate.  tracePointsUpTo!"contigA" (base.d:205-244) as dh_tracepoint.cpp restates it: the index of the trace point a
// position of A is assigned to, mode 0 = floor, 1 = ceil; clamped to [0, ntp]
PM_HD int32_t tp_index(const Rec &r, int32_t ts, int32_t apos, int32_t mode)
{
    const int32_t second = r.abpos / ts * ts + ts;
    int32_t idx;
    if (mode == 0)
        idx = apos < second ? 0 : (apos < r.aepos ? 1 + (apos - second) / ts : r.ntp);
    else {
        const int32_t second_from_last = (r.aepos - 1) / ts * ts;
        idx = apos == r.abpos ? 0 : (apos <= second ? 1 : (apos <= second_from_last ? 1 + (apos - second + ts - 1) / ts : r.ntp));
    }
    return imax(0, imin(idx, r.ntp));
}
// a mask interval cut to the record: the trace-point indices of its begin (floor) and of its end (ceil)
PM_HD void cut_indices(const Rec &r, int32_t ts, int32_t mb, int32_t me, int32_t *ib, int32_t *ie)
{
    *ib = tp_index(r, ts, imax(mb, r.abpos), 0);
    *ie = tp_index(r, ts, imin(me, r.aepos), 1);
}
// the b-bases before trace point idx are the inclusive prefix at tile idx - 1, which lies in this chunk of 64 tiles (idx 0
// needs no tile)
PM_HD int32_t chunk_of(int32_t idx) { return idx > 0 ? (idx - 1) >> 6 : 0; }
// the b-bases of a tile; tr = the record's trace values; tiles behind the record's last one count nothing
PM_HD int32_t tile_bases(const uint16_t *tr, int32_t ntp, int64_t tile) { return tile < ntp ? (int32_t)tr[2 * tile + 1] : 0; }
// pb / pe: b-bases before the two trace points.  false: a translated position lies outside [0, blen] (the record's trace
// runs past the read); the interval is written empty
PM_HD bool finish(const Rec &r, int64_t pb, int64_t pe, Raw *out)
{
    const int64_t b0 = (int64_t)r.bbpos + pb, b1 = (int64_t)r.bbpos + pe;
    if (r.bbpos < 0 || b0 > b1 || b1 > (int64_t)r.blen) {
        *out = Raw{r.bread, 0, 0};
        return false;
    }
    if (r.comp)
        *out = Raw{r.bread, (int32_t)((int64_t)r.blen - b1), (int32_t)((int64_t)r.blen - b0)};
    else
        *out = Raw{r.bread, (int32_t)b0, (int32_t)b1};
    return true;
}

// ---- paint.  The bits of word w that lie in [bit0, bit1)
PM_HD uint32_t word_mask(int64_t bit0, int64_t bit1, int64_t w)
{
    const int64_t w0 = w << 5;
    const int64_t lo = bit0 > w0 ? bit0 - w0 : 0, hi = bit1 < w0 + 32 ? bit1 - w0 : 32;
    if (hi <= lo) return 0u;
    const uint32_t upto = hi >= 32 ? 0xFFFFFFFFu : ((1u << (uint32_t)hi) - 1u);
    return upto & ~((1u << (uint32_t)lo) - 1u);
}
// may this raw interval be painted in a bitmap of the reads [r0, r1)?  (an interval that does not fit its read is never one
// of a successful call; the guard keeps every access inside the bitmap whatever the raw list holds)
PM_HD bool paintable(const Raw &x, const int64_t *boff, int32_t r0, int32_t r1)
{
    if (x.rd < r0 || x.rd >= r1 || x.b < 0 || x.b >= x.e) return false;
    return (int64_t)x.e < boff[x.rd + 1] - boff[x.rd];
}

// ---- runs
PM_HD uint32_t run_starts(uint32_t w, uint32_t carry) { return w & ~((w << 1) | carry); }
PM_HD uint32_t run_ends(uint32_t w, uint32_t carry) { return ~w & ((w << 1) | carry); }
PM_HD uint32_t popc(uint32_t x) { return (uint32_t)__builtin_popcount(x); }
// one lane per group of PM_GROUP_WORDS words (the bitmap is padded with zero words to whole groups)
PM_HD void runs_count_lane(const uint32_t *bm, int64_t g, uint32_t *cs, uint32_t *ce)
{
    const int64_t w0 = g * PM_GROUP_WORDS;
    uint32_t carry = w0 > 0 ? bm[w0 - 1] >> 31 : 0u, s = 0, e = 0;
    for (int k = 0; k < PM_GROUP_WORDS; k++) {
        const uint32_t w = bm[w0 + k];
        s += popc(run_starts(w, carry));
        e += popc(run_ends(w, carry));
        carry = w >> 31;
    }
    *cs = s;
    *ce = e;
}
// the read of [r0, r1) whose words hold this bit of the whole layout
PM_HD int32_t read_of_bit(const int64_t *boff, int32_t r0, int32_t r1, int64_t bit)
{
    int32_t lo = r0, hi = r1 - 1;
    while (lo < hi) {
        const int32_t mid = lo + (hi - lo + 1) / 2;
        if (boff[mid] <= bit)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}
// srank / erank: the starts / ends in front of the group (the exclusive scans of the counts); iv: the pairs of this range
PM_HD void runs_emit_lane(const uint32_t *bm, int64_t g, int64_t base_bit, const int64_t *boff, int32_t r0, int32_t r1, uint32_t srank,
                          uint32_t erank, int32_t *iv)
{
    const int64_t w0 = g * PM_GROUP_WORDS;
    uint32_t carry = w0 > 0 ? bm[w0 - 1] >> 31 : 0u;
    int32_t r = -1;
    for (int k = 0; k < PM_GROUP_WORDS; k++) {
        const uint32_t w = bm[w0 + k];
        uint32_t s = run_starts(w, carry), e = run_ends(w, carry);
        carry = w >> 31;
        if (!(s | e)) continue;
        const int64_t bit = base_bit + ((w0 + k) << 5);
        if (r < 0 || bit >= boff[r + 1]) r = read_of_bit(boff, r0, r1, bit);
        const int64_t origin = boff[r];
        while (s) {
            const int p = __builtin_ctz(s);
            s &= s - 1;
            iv[2 * (int64_t)srank++] = (int32_t)(bit + p - origin);
        }
        while (e) {
            const int p = __builtin_ctz(e);
            e &= e - 1;
            iv[2 * (int64_t)erank++ + 1] = (int32_t)(bit + p - origin);
        }
    }
}
// the start rank at the first word of read r: the group's rank plus the starts of the group's words in front of it
PM_HD uint32_t runs_ptr_lane(const uint32_t *bm, const uint32_t *soff, int64_t base_bit, const int64_t *boff, int32_t r)
{
    const int64_t word = (boff[r] - base_bit) >> 5, g = word / PM_GROUP_WORDS, w0 = g * PM_GROUP_WORDS;
    uint32_t carry = w0 > 0 ? bm[w0 - 1] >> 31 : 0u, rank = soff[g];
    for (int64_t w = w0; w < word; w++) {
        rank += popc(run_starts(bm[w], carry));
        carry = bm[w] >> 31;
    }
    return rank;
}

// ------------------------------------------------------------------------------------------------------------ host plan
struct Fault {
    int64_t record = -1;  // >= 0: the lowest offending record
    int32_t contig = -1;  // >= 0: the lowest contig with a malformed mask
    const char *what = "";
};
struct Plan {
    std::vector<Rec> recs;
    std::vector<int64_t> group_at;  // launch groups of records: group g is [group_at[g], group_at[g + 1])
    std::vector<int64_t> boff;      // nreads + 1 bit offsets
    std::vector<int32_t> range_at;  // destination ranges of reads: range p is [range_at[p], range_at[p + 1])
    int64_t max_range_bits = 0;
};
typedef std::function<void(int64_t, const std::function<void(int64_t, int64_t)> &)> ParallelFor;

inline int64_t roundup32(int64_t x) { return (x + 31) & ~(int64_t)31; }

// the mask per contig: sorted, 0 <= begin < end, begin >= the end before it
inline void check_mask(const int64_t *mask_ptr, const int32_t *mask_iv, int32_t ncontigs, Fault &f)
{
    for (int32_t c = 0; c < ncontigs; c++) {
        const int64_t m0 = mask_ptr[c], m1 = mask_ptr[c + 1];
        if (m0 < 0 || m1 < m0) {
            f.contig = c, f.what = "mask_ptr decreases";
            return;
        }
        int32_t prev = 0;
        for (int64_t j = m0; j < m1; j++) {
            const int32_t b = mask_iv[2 * j], e = mask_iv[2 * j + 1];
            if (b < 0 || b >= e || b < prev) {
                f.contig = c, f.what = b < 0 ? "a negative begin" : (b >= e ? "an empty interval" : "intervals that overlap or are not sorted");
                return;
            }
            prev = e;
        }
    }
}

inline const char *check_record(const dh_la &l, int64_t trace_len, int32_t ts, int32_t ncontigs, int32_t nreads)
{
    if (l.aread < 0 || l.aread >= ncontigs) return "aread out of range";
    if (l.bread < 0 || l.bread >= nreads) return "bread out of range";
    if (l.abpos < 0 || l.abpos > l.aepos) return "abpos < 0 or abpos > aepos";
    if (l.tlen < 0 || l.tlen % 2 || (int64_t)l.tlen != 2 * (((int64_t)l.aepos + ts - 1) / ts - l.abpos / ts))
        return "tlen does not fit the A interval";
    if (l.toff < 0 || l.toff > trace_len || (int64_t)l.tlen > trace_len - l.toff) return "toff + tlen lies behind the trace array";
    return nullptr;
}

// everything the host can check, the compact records, the launch groups (no group can have more than group_raw raw
// intervals: a record has at most min(intervals of its contig, aepos - abpos) of them, at least 1 is counted) and the
// destination layout.  cap_bits: the largest bitmap of one destination range (one sequence always fits)
inline void build_plan(const dh_la *las, int64_t n, int64_t trace_len, int32_t ts, const int64_t *mask_ptr, const int32_t *mask_iv,
                       int32_t ncontigs, const int64_t *read_off, int32_t nreads, int64_t group_raw, int64_t cap_bits,
                       const ParallelFor &pfor, Plan &pl, Fault &f)
{
    check_mask(mask_ptr, mask_iv, ncontigs, f);
    if (f.contig != -1) return;
    for (int32_t r = 0; r < nreads; r++)
        if (read_off[r + 1] < read_off[r] || read_off[r + 1] - read_off[r] > (int64_t)INT32_MAX - 64) {
            f.contig = -2, f.what = "read_off decreases or a read is longer than 2^31 - 65";  // (neither a record's nor a contig's)
            return;
        }
    std::atomic<int64_t> bad{INT64_MAX};
    pl.recs.resize((size_t)n);
    Rec *recs = pl.recs.data();
    pfor(n, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            const dh_la &l = las[i];
            if (check_record(l, trace_len, ts, ncontigs, nreads)) {
                int64_t cur = bad.load();
                while (i < cur && !bad.compare_exchange_weak(cur, i)) {
                }
                break;  // (records behind it in this chunk have higher indices)
            }
            recs[i] = Rec{l.abpos, l.aepos, l.bbpos, (int32_t)(read_off[l.bread + 1] - read_off[l.bread]), l.aread, l.bread,
                          l.flags & DH_FLAG_COMP, l.tlen / 2, l.toff};
        }
    });
    if (bad.load() != INT64_MAX) {
        f.record = bad.load();
        f.what = check_record(las[f.record], trace_len, ts, ncontigs, nreads);
        return;
    }
    pl.group_at.assign(1, 0);
    int64_t acc = 0;
    for (int64_t i = 0; i < n; i++) {
        const Rec &r = recs[i];
        const int64_t bound = std::max<int64_t>(1, std::min<int64_t>(mask_ptr[r.aread + 1] - mask_ptr[r.aread], (int64_t)r.aepos - r.abpos));
        if (acc + bound > group_raw && i > pl.group_at.back()) {
            pl.group_at.push_back(i);
            acc = 0;
        }
        acc += bound;
    }
    pl.group_at.push_back(n);
    pl.boff.resize((size_t)nreads + 1);
    pl.boff[0] = 0;
    for (int32_t r = 0; r < nreads; r++) pl.boff[(size_t)r + 1] = roundup32(pl.boff[(size_t)r] + (read_off[r + 1] - read_off[r]) + 1);
    pl.range_at.assign(1, 0);
    pl.max_range_bits = 0;
    for (int32_t r = 0; r < nreads; r++) {
        const int32_t r0 = pl.range_at.back();
        if (r > r0 && pl.boff[(size_t)r + 1] - pl.boff[(size_t)r0] > cap_bits) pl.range_at.push_back(r);
        pl.max_range_bits = std::max(pl.max_range_bits, pl.boff[(size_t)r + 1] - pl.boff[(size_t)pl.range_at.back()]);
    }
    if (nreads > 0) pl.range_at.push_back(nreads);
}
// the words of a range's bitmap, padded to whole groups
inline int64_t padded_words(int64_t bits) { return ((bits >> 5) + PM_GROUP_WORDS - 1) / PM_GROUP_WORDS * PM_GROUP_WORDS; }

}  // namespace pm

#endif
