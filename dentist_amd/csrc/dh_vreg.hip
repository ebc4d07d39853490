// dh_vreg.hip -- the kernels of dh_la_validate_regions (lane code and layouts: dh_vreg.h; driver: dh_vreg.cpp).  gfx950, wave64.
//
//   k_vr_bind<false>    one lane per record: the candidate regions of its contig (two binary searches), every candidate tested;
//                       per region the pairs, the pairs that span a window start and the spanning records are counted (64-bit
//                       integer atomicAdd: the totals do not depend on the order).
//   k_vr_bind<true>     the same walk over the records of a launch group's contigs, restricted to the group's regions: (w0, w1e)
//                       of every pair with windows and the index of every spanning record go to a slot of the region's segment
//                       claimed by atomicAdd.  The order inside a segment reaches no result (see the next two kernels).
//   k_vr_span           one workgroup per region: every spanning record is placed at its rank among the region's record indices
//                       (ranked in LDS up to VR_SPAN_LDS records, in global memory beyond) and written as its bread.
//   k_vr_region<E, B>   one workgroup per region.  The pairs are added into the region's difference array (B = false: LDS,
//                       B = true: the region's part of the slab), which is then scanned in chunks of VR_BLOCK window starts with
//                       a carry: coverage, the last weak start in front, "opens an interval", the interval's rank.  E = false
//                       counts the intervals and their bases; E = true writes begin and end of every interval at its rank behind
//                       out_at, which the host has placed: no atomics, the order is the region's.
//
// No block leaves in front of a shuffle or a barrier other than as a whole.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dh_scan.h"
#include "dh_vreg.h"

using vr::Job;
using vr::Pair;
using vr::Rec;
using vr::Reg;

typedef unsigned long long u64;

// s0, s1: the regions of the plan that are bound; cnt: 3 per region of the plan.  EMIT: at / cur: 2 per region of [s0, s1), the
// first pair and the first spanning record of its segments and the slots claimed so far
template <bool EMIT>
__global__ void __launch_bounds__(256)
k_vr_bind(const Rec *__restrict__ recs, int64_t i0, int64_t n, const int64_t *__restrict__ rptr, const Reg *__restrict__ regs, int64_t s0,
          int64_t s1, u64 *cnt, const int64_t *__restrict__ at, u64 *cur, Pair *__restrict__ pairs, int64_t *__restrict__ span_idx)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const Rec r = recs[i0 + i];
    int64_t lo, hi;
    vr::candidates(r, rptr, regs, &lo, &hi);
    lo = lo > s0 ? lo : s0;
    hi = hi < s1 ? hi : s1;
    for (int64_t s = lo; s < hi; s++) {
        Pair p;
        const uint32_t what = vr::classify(r, regs[s], &p);
        if (!EMIT) {
            if (what & vr::PAIR) atomicAdd(cnt + 3 * s, (u64)1);
            if (what & vr::WINDOWS) atomicAdd(cnt + 3 * s + 1, (u64)1);
            if (what & vr::SPANS) atomicAdd(cnt + 3 * s + 2, (u64)1);
        } else {
            const int64_t k = s - s0;
            if (what & vr::WINDOWS) pairs[at[2 * k] + (int64_t)atomicAdd(cur + 2 * k, (u64)1)] = p;
            if (what & vr::SPANS) span_idx[at[2 * k + 1] + (int64_t)atomicAdd(cur + 2 * k + 1, (u64)1)] = i0 + i;
        }
    }
}

// at: as for k_vr_bind<true>; nspan[k]: the spanning records of region s0 + k (its count of the first pass)
__global__ void __launch_bounds__(VR_BLOCK)
k_vr_span(const Rec *__restrict__ recs, const int64_t *__restrict__ at, const u64 *__restrict__ cnt, int64_t s0,
          const int64_t *__restrict__ span_idx, int32_t *__restrict__ span_out)
{
    __shared__ int64_t staged[VR_SPAN_LDS];
    const int64_t k = blockIdx.x, m = (int64_t)cnt[3 * (s0 + k) + 2], first = at[2 * k + 1];
    const int64_t *idx = span_idx + first;
    if (m <= VR_SPAN_LDS) {  // (the same for the whole block)
        for (int64_t j = threadIdx.x; j < m; j += VR_BLOCK) staged[j] = idx[j];
        __syncthreads();
        idx = staged;
    }
    for (int64_t j = threadIdx.x; j < m; j += VR_BLOCK) {
        const int64_t x = idx[j];
        span_out[first + vr::rank_of(idx, m, x)] = recs[x].bread;
    }
}

// rcnt: 2 per job, the intervals of the region and their bases (EMIT: not written); iv: the group's intervals
template <bool EMIT, bool BIG>
__global__ void __launch_bounds__(VR_BLOCK)
k_vr_region(const Job *__restrict__ jobs, const Pair *__restrict__ pairs, int32_t *slab, int32_t min_cov, uint32_t *__restrict__ rcnt,
            int32_t *__restrict__ iv)
{
    extern __shared__ int32_t lds_diff[];
    __shared__ int32_t ws[VR_BLOCK / 64];
    __shared__ uint32_t bases;
    const Job j = jobs[blockIdx.x];
    const int32_t tid = (int32_t)threadIdx.x;
    if (j.nw <= 0) {  // (the whole block)
        if (!EMIT && tid == 0) rcnt[2 * blockIdx.x] = rcnt[2 * blockIdx.x + 1] = 0u;
        return;
    }
    int32_t *diff = BIG ? slab + j.slab_at : lds_diff;
    if (tid == 0) bases = 0u;
    for (int64_t k = tid; k <= (int64_t)j.nw; k += VR_BLOCK) diff[k] = 0;
    __syncthreads();
    for (int64_t k = tid; k < j.npairs; k += VR_BLOCK) {
        const Pair p = pairs[j.pair_at + k];
        if (p.w0 < 0 || p.w0 >= p.w1e || p.w1e > j.nw) continue;  // (never one of a pair list of k_vr_bind: no access outside the array)
        atomicAdd(diff + p.w0, 1);
        atomicSub(diff + p.w1e, 1);
    }
    __syncthreads();
    int32_t cov_carry = 0, last_carry = -1;
    uint32_t rank_carry = 0u, bp = 0u;  // (bp: modulo 2^32, the sum fits)
    int32_t *out = iv + 2 * j.out_at;
    for (int64_t base = 0; base < (int64_t)j.nw; base += VR_BLOCK) {
        const int64_t w = base + tid;
        const bool in = w < (int64_t)j.nw;
        // (the slab was written by atomics, which are served by the L2: read it there)
        const int32_t d = !in ? 0 : (BIG ? __hip_atomic_load(diff + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : diff[w]);
        int32_t excl, total;
        block_scan<VR_BLOCK, ScanSum, 0>(d, ws, &excl, &total);
        const int32_t cov = cov_carry + excl + d;
        cov_carry += total;
        const bool weak = in && cov < min_cov;
        block_scan<VR_BLOCK, ScanMax, -1>(weak ? (int32_t)w : -1, ws, &excl, &total);  // (the maxima are window starts or -1)
        const int32_t last = excl > last_carry ? excl : last_carry;
        last_carry = total > last_carry ? total : last_carry;
        const bool open = weak && vr::opens(w, last, j.wlen);
        block_scan<VR_BLOCK, ScanSum, 0>(open ? 1 : 0, ws, &excl, &total);
        const uint32_t rank = rank_carry + (uint32_t)excl;
        rank_carry += (uint32_t)total;
        if (open) {
            if (EMIT) {
                out[2 * (int64_t)rank] = j.cb + (int32_t)w;
                if (last >= 0) out[2 * (int64_t)rank - 1] = j.cb + last + j.wlen;
            } else
                bp += (last >= 0 ? (uint32_t)(last + j.wlen) : 0u) - (uint32_t)w;
        }
    }
    if (last_carry >= 0 && tid == 0) {  // the end of the last interval
        if (EMIT)
            out[2 * (int64_t)rank_carry - 1] = j.cb + last_carry + j.wlen;
        else
            bp += (uint32_t)(last_carry + j.wlen);
    }
    if (!EMIT) {
        if (bp) atomicAdd(&bases, bp);
        __syncthreads();
        if (tid == 0) {
            rcnt[2 * blockIdx.x] = rank_carry;
            rcnt[2 * blockIdx.x + 1] = bases;
        }
    }
}

// launches go out in slices: a grid stays below 2^31 blocks
static const int64_t VR_LAUNCH_BLOCKS = (int64_t)1 << 22;

extern "C" void dhk_vr_bind(hipStream_t st, int emit, const Rec *recs, int64_t i0, int64_t n, const int64_t *rptr, const Reg *regs, int64_t s0,
                            int64_t s1, u64 *cnt, const int64_t *at, u64 *cur, Pair *pairs, int64_t *span_idx)
{
    for (int64_t off = 0; off < n; off += VR_LAUNCH_BLOCKS * 256) {
        const int64_t m = std::min<int64_t>(VR_LAUNCH_BLOCKS * 256, n - off);
        const dim3 grid((unsigned)((m + 255) / 256));
        if (emit)
            hipLaunchKernelGGL(k_vr_bind<true>, grid, dim3(256), 0, st, recs, i0 + off, m, rptr, regs, s0, s1, cnt, at, cur, pairs, span_idx);
        else
            hipLaunchKernelGGL(k_vr_bind<false>, grid, dim3(256), 0, st, recs, i0 + off, m, rptr, regs, s0, s1, cnt, at, cur, pairs, span_idx);
    }
}
extern "C" void dhk_vr_span(hipStream_t st, const Rec *recs, const int64_t *at, const u64 *cnt, int64_t s0, int64_t nreg, const int64_t *span_idx,
                            int32_t *span_out)
{
    for (int64_t off = 0; off < nreg; off += VR_LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_vr_span, dim3((unsigned)std::min<int64_t>(VR_LAUNCH_BLOCKS, nreg - off)), dim3(VR_BLOCK), 0, st, recs, at + 2 * off,
                           cnt, s0 + off, span_idx, span_out);
}
// jobs [0, nsmall) keep their difference array in LDS (lds_entries: the largest of them), jobs [nsmall, njobs) in the slab
extern "C" void dhk_vr_region(hipStream_t st, int emit, const Job *jobs, int64_t nsmall, int64_t njobs, int64_t lds_entries, const Pair *pairs,
                              int32_t *slab, int32_t min_cov, uint32_t *rcnt, int32_t *iv)
{
    const size_t lds = sizeof(int32_t) * (size_t)lds_entries;
    for (int64_t off = 0; off < nsmall; off += VR_LAUNCH_BLOCKS) {
        const dim3 grid((unsigned)std::min<int64_t>(VR_LAUNCH_BLOCKS, nsmall - off));
        if (emit)
            hipLaunchKernelGGL((k_vr_region<true, false>), grid, dim3(VR_BLOCK), lds, st, jobs + off, pairs, slab, min_cov, rcnt + 2 * off, iv);
        else
            hipLaunchKernelGGL((k_vr_region<false, false>), grid, dim3(VR_BLOCK), lds, st, jobs + off, pairs, slab, min_cov, rcnt + 2 * off, iv);
    }
    for (int64_t off = nsmall; off < njobs; off += VR_LAUNCH_BLOCKS) {
        const dim3 grid((unsigned)std::min<int64_t>(VR_LAUNCH_BLOCKS, njobs - off));
        if (emit)
            hipLaunchKernelGGL((k_vr_region<true, true>), grid, dim3(VR_BLOCK), 0, st, jobs + off, pairs, slab, min_cov, rcnt + 2 * off, iv);
        else
            hipLaunchKernelGGL((k_vr_region<false, true>), grid, dim3(VR_BLOCK), 0, st, jobs + off, pairs, slab, min_cov, rcnt + 2 * off, iv);
    }
}
