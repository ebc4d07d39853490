// dh_pmask.hip -- the kernels of dh_la_propagate_mask (lane code and layouts: dh_pmask.h; driver: dh_pmask.cpp).  gfx950, wave64.
//
//   k_pm_plan         one lane per record: two binary searches in the mask of its A sequence -> lo, cnt, off (= cnt, scanned by
//                     the driver), has (= cnt > 0, scanned for the compaction).
//   k_pm_compact      the records with cnt > 0, in input order.
//   k_pm_translate    one wavefront per such record.  The trace is walked once in chunks of 64 tiles: lane l loads the b-bases of
//                     tile 64 c + l, a wave scan plus the carry of the chunks before gives the b-bases in front of every trace
//                     point of the chunk; the lanes hold 64 intervals per batch and read the prefix at their two indices across
//                     the lanes.  Both indices rise with the interval, so the next batch resumes at the chunk (and carry) of its
//                     first index.  One path for a record of one tile and for one of 20 000.  Writes (read, begin, end) at
//                     off[i] + j; a record whose b-bases run past its read is reported by atomicMin on its index.
//   k_pm_paint        one lane per raw interval of the destination range; an interval of more than PM_SHORT_WORDS words is handed
//                     to the whole wavefront, whose 64 lanes OR 64 consecutive words (256 contiguous bytes per atomic instruction).
//   k_pm_runs_count   \ starts and ends of the runs per group of PM_GROUP_WORDS words, and after the scans of both the pairs in
//   k_pm_runs_emit    / contract order: no atomics, the order is the bitmap's.
//   k_pm_runs_ptr     ptr[r] of the range's reads.
//
// No block leaves in front of a shuffle or a ballot other than as a whole.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dh_pmask.h"
#include "dh_scan.h"

using pm::Raw;
using pm::Rec;

__global__ void __launch_bounds__(256)
k_pm_plan(const Rec *__restrict__ recs, int64_t n, const int64_t *__restrict__ mask_ptr, const int32_t *__restrict__ mask_iv,
          int64_t *__restrict__ lo, uint32_t *__restrict__ cnt, uint32_t *__restrict__ off, uint32_t *__restrict__ has)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int64_t l;
    uint32_t c;
    pm::plan_lane(recs[i], mask_ptr, mask_iv, &l, &c);
    lo[i] = l;
    cnt[i] = c;
    off[i] = c;
    has[i] = c ? 1u : 0u;
}

// has: the exclusive scan of the flags within the launch group [i0, i0 + n)
__global__ void __launch_bounds__(256)
k_pm_compact(const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ has, int64_t i0, int64_t n, int64_t *__restrict__ list)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (cnt[i0 + i]) list[has[i0 + i]] = i0 + i;
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)((uint64_t)v >> 32), src, 64);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ void __launch_bounds__(64)
k_pm_translate(const Rec *__restrict__ recs, const int64_t *__restrict__ list, const int64_t *__restrict__ lo,
               const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ off, const uint16_t *__restrict__ trace, int32_t ts,
               const int32_t *__restrict__ mask_iv, Raw *__restrict__ raw, unsigned long long *bad, unsigned long long *nonempty)
{
    const int64_t i = list[blockIdx.x];
    const int32_t lane = (int32_t)threadIdx.x;
    const Rec r = recs[i];
    const uint32_t n_iv = cnt[i];
    const int64_t m0 = lo[i];
    Raw *out = raw + off[i];
    const uint16_t *tr = trace + r.toff;
    int32_t c = 0;      // the next chunk of tiles
    int64_t carry = 0;  // the b-bases of the chunks before it
    uint32_t filled = 0;
    for (uint32_t j0 = 0; j0 < n_iv; j0 += 64) {
        const int32_t nlive = (int32_t)min(64u, n_iv - j0);
        const bool live = lane < nlive;
        int32_t ib = 0, ie = 0;
        if (live) pm::cut_indices(r, ts, mask_iv[2 * (m0 + j0 + lane)], mask_iv[2 * (m0 + j0 + lane) + 1], &ib, &ie);
        // the last chunk this batch needs, and the chunk at which the next batch starts (its first begin index)
        const int32_t c_last = __builtin_amdgcn_readfirstlane(pm::chunk_of(__shfl(ie, nlive - 1, 64)));
        int32_t c_next = -1;
        if (j0 + 64 < n_iv) {
            int32_t nb, ne;
            pm::cut_indices(r, ts, mask_iv[2 * (m0 + j0 + 64)], mask_iv[2 * (m0 + j0 + 64) + 1], &nb, &ne);
            c_next = __builtin_amdgcn_readfirstlane(pm::chunk_of(nb));
        }
        const int32_t c_end = max(c_last, c_next);
        int32_t keep_c = c;
        int64_t keep_carry = carry, pb = 0, pe = 0;
        for (; c <= c_end; c++) {
            if (c == c_next) keep_c = c, keep_carry = carry;
            const int32_t incl = wave_incl_scan(pm::tile_bases(tr, r.ntp, (int64_t)c * 64 + lane), lane);
            const int32_t at_b = __shfl(incl, (ib - 1) & 63, 64), at_e = __shfl(incl, (ie - 1) & 63, 64);
            if (ib > 0 && pm::chunk_of(ib) == c) pb = carry + at_b;
            if (ie > 0 && pm::chunk_of(ie) == c) pe = carry + at_e;
            carry += __shfl(incl, 63, 64);
        }
        if (c_next >= 0) c = keep_c, carry = keep_carry;
        bool ok = true, full = false;
        if (live) {
            Raw x;
            ok = pm::finish(r, pb, pe, &x);
            out[j0 + lane] = x;
            full = x.b < x.e;
        }
        if (!ok) atomicMin(bad, (unsigned long long)i);
        filled += (uint32_t)__popcll(__ballot(full));
    }
    if (lane == 0 && filled) atomicAdd(nonempty, (unsigned long long)filled);
}

// raw intervals [at, at + n) of the list; the bitmap is the one of the reads [r0, r1), its bit 0 is bit base_bit of the layout
__global__ void __launch_bounds__(256)
k_pm_paint(const Raw *__restrict__ raw, int64_t n, const int64_t *__restrict__ boff, int32_t r0, int32_t r1, int64_t base_bit,
           uint32_t *bm)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    Raw x = Raw{-1, 0, 0};
    if (i < n) x = raw[i];
    const bool have = i < n && pm::paintable(x, boff, r0, r1);
    int64_t bit0 = 0, bit1 = 0;
    if (have) {
        bit0 = boff[x.rd] - base_bit + x.b;
        bit1 = boff[x.rd] - base_bit + x.e;
    }
    const bool wide = have && ((bit1 - 1) >> 5) - (bit0 >> 5) >= PM_SHORT_WORDS;
    if (have && !wide)
        for (int64_t w = bit0 >> 5; w <= (bit1 - 1) >> 5; w++) atomicOr(bm + w, pm::word_mask(bit0, bit1, w));
    uint64_t m = __ballot(wide);
    while (m) {
        const int src = (int)__ffsll((long long)m) - 1;
        m &= m - 1;
        const int64_t s0 = shfl64(bit0, src), s1 = shfl64(bit1, src);
        for (int64_t w = (s0 >> 5) + lane; w <= (s1 - 1) >> 5; w += 64) atomicOr(bm + w, pm::word_mask(s0, s1, w));
    }
}

__global__ void __launch_bounds__(256)
k_pm_runs_count(const uint32_t *__restrict__ bm, int64_t ngroups, uint32_t *__restrict__ cs, uint32_t *__restrict__ ce)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    pm::runs_count_lane(bm, g, cs + g, ce + g);
}

__global__ void __launch_bounds__(256)
k_pm_runs_emit(const uint32_t *__restrict__ bm, int64_t ngroups, int64_t base_bit, const int64_t *__restrict__ boff, int32_t r0, int32_t r1,
               const uint32_t *__restrict__ soff, const uint32_t *__restrict__ eoff, int32_t *__restrict__ iv)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups) return;
    pm::runs_emit_lane(bm, g, base_bit, boff, r0, r1, soff[g], eoff[g], iv);
}

__global__ void __launch_bounds__(256)
k_pm_runs_ptr(const uint32_t *__restrict__ bm, const uint32_t *__restrict__ soff, int64_t base_bit, const int64_t *__restrict__ boff,
              int32_t r0, int32_t r1, int64_t k0, int64_t *__restrict__ ptr)
{
    const int64_t r = (int64_t)r0 + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= r1) return;
    ptr[r] = k0 + pm::runs_ptr_lane(bm, soff, base_bit, boff, (int32_t)r);
}

// launches go out in slices: a grid stays below 2^31 blocks
static const int64_t PM_LAUNCH_BLOCKS = (int64_t)1 << 24;

extern "C" void dhk_pm_plan(hipStream_t st, const Rec *recs, int64_t n, const int64_t *mask_ptr, const int32_t *mask_iv, int64_t *lo,
                            uint32_t *cnt, uint32_t *off, uint32_t *has)
{
    for (int64_t at = 0; at < n; at += PM_LAUNCH_BLOCKS * 256) {
        const int64_t m = std::min<int64_t>(PM_LAUNCH_BLOCKS * 256, n - at);
        hipLaunchKernelGGL(k_pm_plan, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, recs + at, m, mask_ptr, mask_iv, lo + at, cnt + at,
                           off + at, has + at);
    }
}
extern "C" void dhk_pm_compact(hipStream_t st, const uint32_t *cnt, const uint32_t *has, int64_t i0, int64_t n, int64_t *list)
{
    for (int64_t at = 0; at < n; at += PM_LAUNCH_BLOCKS * 256) {
        const int64_t m = std::min<int64_t>(PM_LAUNCH_BLOCKS * 256, n - at);
        hipLaunchKernelGGL(k_pm_compact, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, cnt, has, i0 + at, m, list);
    }
}
extern "C" void dhk_pm_translate(hipStream_t st, const Rec *recs, const int64_t *list, int64_t nlist, const int64_t *lo, const uint32_t *cnt,
                                 const uint32_t *off, const uint16_t *trace, int32_t ts, const int32_t *mask_iv, Raw *raw,
                                 unsigned long long *bad, unsigned long long *nonempty)
{
    for (int64_t at = 0; at < nlist; at += PM_LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_pm_translate, dim3((unsigned)std::min<int64_t>(PM_LAUNCH_BLOCKS, nlist - at)), dim3(64), 0, st, recs, list + at, lo,
                           cnt, off, trace, ts, mask_iv, raw, bad, nonempty);
}
extern "C" void dhk_pm_paint(hipStream_t st, const Raw *raw, int64_t n, const int64_t *boff, int32_t r0, int32_t r1, int64_t base_bit,
                             uint32_t *bm)
{
    for (int64_t at = 0; at < n; at += PM_LAUNCH_BLOCKS * 256) {
        const int64_t m = std::min<int64_t>(PM_LAUNCH_BLOCKS * 256, n - at);
        hipLaunchKernelGGL(k_pm_paint, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, raw + at, m, boff, r0, r1, base_bit, bm);
    }
}
extern "C" void dhk_pm_runs_count(hipStream_t st, const uint32_t *bm, int64_t ngroups, uint32_t *cs, uint32_t *ce)
{
    if (ngroups <= 0) return;
    hipLaunchKernelGGL(k_pm_runs_count, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, st, bm, ngroups, cs, ce);
}
extern "C" void dhk_pm_runs_emit(hipStream_t st, const uint32_t *bm, int64_t ngroups, int64_t base_bit, const int64_t *boff, int32_t r0,
                                 int32_t r1, const uint32_t *soff, const uint32_t *eoff, int32_t *iv, int64_t k0, int64_t *ptr)
{
    if (ngroups <= 0) return;
    hipLaunchKernelGGL(k_pm_runs_emit, dim3((unsigned)((ngroups + 255) / 256)), dim3(256), 0, st, bm, ngroups, base_bit, boff, r0, r1, soff,
                       eoff, iv);
    hipLaunchKernelGGL(k_pm_runs_ptr, dim3((unsigned)((r1 - r0 + 255) / 256)), dim3(256), 0, st, bm, soff, base_bit, boff, r0, r1, k0, ptr);
}
