// dh_rmask.hip -- the kernels of dh_la_repeat_mask (lane code and layouts: dh_rmask.h; driver: dh_rmask.cpp).  gfx950, wave64.
// All of them work on one launch group: m records of nc whole contigs.
//
//   (k_cf_start of dh_cfilt.hip and dhk_scan_total of dh_kernels.hip: the chain starts and their exclusive scan over m + 1 entries)
//   k_rm_events         one lane per record: the lane of a chain start walks its members and writes the unit's two keys at slots
//                       2u and 2u + 1; the improper units are counted per wavefront, one atomic each.
//   k_rm_classify       one lane per contig: its segment (twice the unit of its first record) and the list of its tier; a contig
//                       of the global tier claims its part of the slab.
//   k_rm_sort_wave      one wavefront per contig of up to 64 events: the keys in registers, ranked by rotation over the lanes and
//                       written to their places.
//   k_rm_sort_block     one workgroup per contig of up to the LDS cap: a bitonic network over its keys in LDS; the sorted keys go
//                       back to the segment.
//   k_rm_sort_big<MODE> the contigs above the cap: their keys into their parts of a slab of global memory, then one launch per
//                       step of the same network with one lane per comparator of every such contig, then the keys back.
//   k_rm_cover<PLACE>   one wavefront per contig: the walk over its sorted keys (rm::lane_edges), counting the runs of both
//                       assessors (PLACE = false) or writing them behind the scanned counts (PLACE = true).
//   k_rm_union<PLACE>   one lane per contig: rm::merge_union of its two lists, counted or written.
//
// No wavefront leaves in front of a shuffle, and no block in front of a barrier, other than as a whole.  Every index is bounded
// by the segment of its contig: seg[c] .. seg[c + 1] inside the 2 m keys, the lists by the number of contigs.
#include <hip/hip_runtime.h>

#include "dh_rmask.h"

using rm::Opts;
using rm::Rec;
using rm::u64;

__global__ void __launch_bounds__(RM_BLOCK)
k_rm_events(const Rec *__restrict__ recs, int64_t m, const int32_t *__restrict__ flag, const int32_t *__restrict__ uid,
            const int32_t *__restrict__ alen, const int32_t *__restrict__ blen, Opts o, u64 *__restrict__ ev, u64 *ctr)
{
    const int64_t i = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
    bool improper = false;
    if (i < m && flag[i]) {
        const int64_t u = uid[i];
        u64 kb, ke;
        improper = rm::unit_events(recs, i, m, alen, blen, o, &kb, &ke);
        ev[2 * u] = kb, ev[2 * u + 1] = ke;
    }
    const u64 b = __ballot(improper);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(ctr + rm::C_IMPROPER, (u64)__popcll(b));
}

// roff: the first record of every contig of the group, relative to the group's first (nc + 1 entries); uid: the scanned flags,
// m + 1 entries (the last: the number of units)
__global__ void __launch_bounds__(RM_BLOCK)
k_rm_classify(const int32_t *__restrict__ roff, const int32_t *__restrict__ uid, int32_t nc, int32_t lds_events, int32_t *__restrict__ seg,
              u64 *ctr, int32_t *__restrict__ l_wave, int32_t *__restrict__ l_lds, int32_t *__restrict__ l_glob, u64 *__restrict__ slab_at)
{
    const int64_t c = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
    if (c > nc) return;
    const int32_t s0 = 2 * uid[roff[c]];
    seg[c] = s0;
    if (c == nc) return;
    const int32_t events = 2 * uid[roff[c + 1]] - s0;
    const int tier = rm::tier_of(events, lds_events);
    if (tier == 0) atomicAdd(ctr + rm::C_ZERO, (u64)1);
    if (tier == 1) l_wave[atomicAdd(ctr + rm::C_WAVE, (u64)1)] = (int32_t)c;
    if (tier == 2) l_lds[atomicAdd(ctr + rm::C_LDS, (u64)1)] = (int32_t)c;
    if (tier == 3) {
        const u64 k = atomicAdd(ctr + rm::C_GLOBAL, (u64)1);
        l_glob[k] = (int32_t)c;
        slab_at[k] = atomicAdd(ctr + rm::C_SLAB, (u64)cf::pow2ceil(events));
    }
}

__device__ __forceinline__ u64 shfl_u64(u64 v, int src)
{
    const int32_t lo = __shfl((int32_t)(uint32_t)v, src, 64), hi = __shfl((int32_t)(uint32_t)(v >> 32), src, 64);
    return ((u64)(uint32_t)hi << 32) | (uint32_t)lo;
}

__global__ void __launch_bounds__(RM_BLOCK)
k_rm_sort_wave(u64 *ev, const int32_t *__restrict__ seg, const int32_t *__restrict__ list, int64_t nlist)
{
    const int64_t k = (int64_t)blockIdx.x * (RM_BLOCK / 64) + (threadIdx.x >> 6);
    if (k >= nlist) return;  // (a whole wavefront)
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    const int32_t c = list[k], s0 = seg[c], size = seg[c + 1] - s0;  // 1..64
    const bool in = lane < size;
    const u64 me = in ? ev[s0 + lane] : rm::PAD;
    int32_t rank = 0;
    for (int32_t z = 0; z < size; z++) rank += rm::ranks_before(shfl_u64(me, z), z, me, lane);
    if (in) ev[s0 + rank] = me;  // (every key is in a register: the ranks of the size keys are a permutation of 0 .. size - 1)
}

__global__ void __launch_bounds__(RM_BLOCK) k_rm_sort_block(u64 *ev, const int32_t *__restrict__ seg, const int32_t *__restrict__ list)
{
    extern __shared__ u64 key[];
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t c = list[blockIdx.x], s0 = seg[c], size = seg[c + 1] - s0, P = cf::pow2ceil(size);
    for (int32_t t = tid; t < P; t += RM_BLOCK) key[t] = t < size ? ev[s0 + t] : rm::PAD;
    __syncthreads();
    for (int32_t k = 2; k <= P; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t t = tid; t < P / 2; t += RM_BLOCK) rm::bt_compare(key, t, k, j);
            __syncthreads();
        }
    for (int32_t t = tid; t < size; t += RM_BLOCK) ev[s0 + t] = key[t];
}

// the global tier.  blockIdx.x: 256 places (or comparators) of a contig; blockIdx.y and its stride: the contigs of the list.
// MODE 0: the contig's keys into its part of the slab, PAD behind the last; 1: step (k, j) of the network (a contig whose padded
// size is below k is finished); 2: the sorted keys back to the segment.
template <int MODE>
__global__ void __launch_bounds__(RM_BLOCK)
k_rm_sort_big(u64 *ev, const int32_t *__restrict__ seg, const int32_t *__restrict__ list, int64_t nlist, const u64 *__restrict__ slab_at, u64 *slab,
              int32_t k, int32_t j)
{
    const int64_t t = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
    for (int64_t q = blockIdx.y; q < nlist; q += gridDim.y) {
        const int32_t c = list[q], s0 = seg[c], size = seg[c + 1] - s0, P = cf::pow2ceil(size);
        u64 *key = slab + slab_at[q];
        if (MODE == 0 && t < P) key[t] = t < size ? ev[s0 + t] : rm::PAD;
        if (MODE == 1 && t < P / 2 && k <= P) rm::bt_compare(key, (int32_t)t, k, j);
        if (MODE == 2 && t < size) ev[s0 + t] = key[t];
    }
}

__device__ __forceinline__ int32_t wave_inclusive(int32_t x, int32_t lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t t = __shfl_up(x, d, 64);
        if (lane >= d) x += t;
    }
    return x;
}

// one assessor's state over the walk of a contig
struct RmSide {
    int32_t lower, upper, carry, nstart, nend;
    bool prev;
    int64_t at;  // PLACE: the contig's first interval
    int32_t *iv;
};
template <bool PLACE>
__device__ __forceinline__ void rm_side_tile(RmSide &s, int32_t lane, u64 last, bool is_last, int32_t pos, int32_t len, int32_t incl)
{
    const u64 badb = __ballot(is_last && pos != len && rm::bad(s.carry + incl, s.lower, s.upper));
    bool st, en;
    rm::lane_edges(lane, last, badb, s.prev, &st, &en);
    const u64 sb = __ballot(st), eb = __ballot(en);
    if (PLACE) {
        if (st) s.iv[2 * (s.at + s.nstart + rm::lanes_below(sb, lane))] = pos;
        if (en) s.iv[2 * (s.at + s.nend + rm::lanes_below(eb, lane)) + 1] = pos;
    }
    s.nstart += (int32_t)__popcll(sb), s.nend += (int32_t)__popcll(eb);
    s.prev = rm::state_behind(last, badb, s.prev);
    s.carry += __shfl(incl, 63, 64);
}

// cnt_all / cnt_imp: nc + 1 entries; PLACE = false writes the runs of every contig, PLACE = true reads their exclusive scan
template <bool PLACE>
__global__ void __launch_bounds__(RM_BLOCK)
k_rm_cover(const u64 *__restrict__ ev, const int32_t *__restrict__ seg, int32_t nc, const int32_t *__restrict__ alen, Opts o,
           uint32_t *cnt_all, uint32_t *cnt_imp, int32_t *__restrict__ iv_all, int32_t *__restrict__ iv_imp)
{
    const int64_t c = (int64_t)blockIdx.x * (RM_BLOCK / 64) + (threadIdx.x >> 6);
    if (c >= nc) return;  // (a whole wavefront)
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    const int32_t s0 = seg[c], size = seg[c + 1] - s0, len = alen[c];
    RmSide side[2] = {{o.lower, o.upper, 0, 0, 0, false, PLACE ? (int64_t)cnt_all[c] : 0, iv_all},
                      {o.improper_lower, o.improper_upper, 0, 0, 0, false, PLACE && o.with_improper ? (int64_t)cnt_imp[c] : 0, iv_imp}};
    const int nsides = o.with_improper ? 2 : 1;
    // the zone in front of the first position (the whole contig without events): coverage 0, from base 0
    const bool head = len > 0 && (size == 0 || rm::key_pos(ev[s0]) > 0);
    for (int a = 0; a < nsides; a++) {
        RmSide &s = side[a];
        if (head && rm::bad(0, s.lower, s.upper)) {
            if (PLACE && lane == 0) s.iv[2 * s.at] = 0;
            s.nstart = 1, s.prev = true;
        }
    }
    for (int32_t base = 0; base < size; base += 64) {
        const int32_t idx = base + lane;
        const u64 k = idx < size ? ev[s0 + idx] : rm::PAD, nxt = idx + 1 < size ? ev[s0 + idx + 1] : rm::PAD;
        const bool is_last = idx < size && rm::key_pos(nxt) != rm::key_pos(k);
        const u64 last = __ballot(is_last);
        const int32_t pos = (int32_t)rm::key_pos(k);
        const int32_t incl_all = wave_inclusive(rm::delta_all(k), lane);
        rm_side_tile<PLACE>(side[0], lane, last, is_last, pos, len, incl_all);
        if (nsides == 2) {
            const int32_t incl_imp = wave_inclusive(rm::delta_improper(k), lane);
            rm_side_tile<PLACE>(side[1], lane, last, is_last, pos, len, incl_imp);
        }
    }
    for (int a = 0; a < nsides; a++) {
        RmSide &s = side[a];
        if (s.prev) {  // bad up to the contig's last base
            if (PLACE && lane == 0) s.iv[2 * (s.at + s.nend) + 1] = len;
            s.nend++;
        }
        if (!PLACE && lane == 0) (a == 0 ? cnt_all : cnt_imp)[c] = (uint32_t)s.nstart;
    }
}

// ptr_all / ptr_imp: the scanned counts (nc + 1); cnt: nc + 1 entries, written (PLACE = false) or read as their scan
template <bool PLACE>
__global__ void __launch_bounds__(RM_BLOCK)
k_rm_union(int32_t nc, const uint32_t *__restrict__ ptr_all, const int32_t *__restrict__ iv_all, const uint32_t *__restrict__ ptr_imp,
           const int32_t *__restrict__ iv_imp, uint32_t *cnt, int32_t *__restrict__ iv)
{
    const int64_t c = (int64_t)blockIdx.x * RM_BLOCK + threadIdx.x;
    if (c >= nc) return;
    const int32_t n = rm::merge_union(iv_all + 2 * (int64_t)ptr_all[c], (int32_t)(ptr_all[c + 1] - ptr_all[c]), iv_imp + 2 * (int64_t)ptr_imp[c],
                                      (int32_t)(ptr_imp[c + 1] - ptr_imp[c]), PLACE ? iv + 2 * (int64_t)cnt[c] : nullptr);
    if (!PLACE) cnt[c] = (uint32_t)n;
}

// m < 2^30 (the driver refuses more): every grid stays far below 2^31 blocks
static inline dim3 rm_grid(int64_t n, int64_t per_block) { return dim3((unsigned)((n + per_block - 1) / per_block)); }

extern "C" void dhk_rm_events(hipStream_t st, const Rec *recs, int64_t m, const int32_t *flag, const int32_t *uid, const int32_t *alen,
                              const int32_t *blen, Opts o, u64 *ev, u64 *ctr)
{
    if (m > 0) hipLaunchKernelGGL(k_rm_events, rm_grid(m, RM_BLOCK), dim3(RM_BLOCK), 0, st, recs, m, flag, uid, alen, blen, o, ev, ctr);
}
extern "C" void dhk_rm_classify(hipStream_t st, const int32_t *roff, const int32_t *uid, int32_t nc, int32_t lds_events, int32_t *seg, u64 *ctr,
                                int32_t *l_wave, int32_t *l_lds, int32_t *l_glob, u64 *slab_at)
{
    hipLaunchKernelGGL(k_rm_classify, rm_grid((int64_t)nc + 1, RM_BLOCK), dim3(RM_BLOCK), 0, st, roff, uid, nc, lds_events, seg, ctr, l_wave, l_lds,
                       l_glob, slab_at);
}
extern "C" void dhk_rm_sort(hipStream_t st, u64 *ev, const int32_t *seg, int64_t nwave, const int32_t *l_wave, int64_t nlds, const int32_t *l_lds,
                            int32_t lds_events, int64_t nglob, const int32_t *l_glob, const u64 *slab_at, u64 *slab, int64_t max_padded)
{
    if (nwave > 0) hipLaunchKernelGGL(k_rm_sort_wave, rm_grid(nwave, RM_BLOCK / 64), dim3(RM_BLOCK), 0, st, ev, seg, l_wave, nwave);
    const size_t lds = sizeof(u64) * (size_t)cf::pow2ceil(lds_events);
    if (nlds > 0) hipLaunchKernelGGL(k_rm_sort_block, dim3((unsigned)nlds), dim3(RM_BLOCK), lds, st, ev, seg, l_lds);
    if (nglob <= 0) return;
    // max_padded: a power of two that no contig's padded size exceeds.  One launch per step of the network, over all workgroups
    const dim3 all(rm_grid(max_padded, RM_BLOCK).x, (unsigned)std::min<int64_t>(nglob, 65535)), half(rm_grid(max_padded / 2, RM_BLOCK).x, all.y);
    hipLaunchKernelGGL(k_rm_sort_big<0>, all, dim3(RM_BLOCK), 0, st, ev, seg, l_glob, nglob, slab_at, slab, 0, 0);
    for (int64_t k = 2; k <= max_padded; k <<= 1)
        for (int64_t j = k >> 1; j > 0; j >>= 1)
            hipLaunchKernelGGL(k_rm_sort_big<1>, half, dim3(RM_BLOCK), 0, st, ev, seg, l_glob, nglob, slab_at, slab, (int32_t)k, (int32_t)j);
    hipLaunchKernelGGL(k_rm_sort_big<2>, all, dim3(RM_BLOCK), 0, st, ev, seg, l_glob, nglob, slab_at, slab, 0, 0);
}
extern "C" void dhk_rm_cover(hipStream_t st, int place, const u64 *ev, const int32_t *seg, int32_t nc, const int32_t *alen, Opts o,
                             uint32_t *cnt_all, uint32_t *cnt_imp, int32_t *iv_all, int32_t *iv_imp)
{
    if (nc <= 0) return;
    if (place)
        hipLaunchKernelGGL(k_rm_cover<true>, rm_grid(nc, RM_BLOCK / 64), dim3(RM_BLOCK), 0, st, ev, seg, nc, alen, o, cnt_all, cnt_imp, iv_all, iv_imp);
    else
        hipLaunchKernelGGL(k_rm_cover<false>, rm_grid(nc, RM_BLOCK / 64), dim3(RM_BLOCK), 0, st, ev, seg, nc, alen, o, cnt_all, cnt_imp, iv_all, iv_imp);
}
extern "C" void dhk_rm_union(hipStream_t st, int place, int32_t nc, const uint32_t *ptr_all, const int32_t *iv_all, const uint32_t *ptr_imp,
                             const int32_t *iv_imp, uint32_t *cnt, int32_t *iv)
{
    if (nc <= 0) return;
    if (place)
        hipLaunchKernelGGL(k_rm_union<true>, rm_grid(nc, RM_BLOCK), dim3(RM_BLOCK), 0, st, nc, ptr_all, iv_all, ptr_imp, iv_imp, cnt, iv);
    else
        hipLaunchKernelGGL(k_rm_union<false>, rm_grid(nc, RM_BLOCK), dim3(RM_BLOCK), 0, st, nc, ptr_all, iv_all, ptr_imp, iv_imp, cnt, iv);
}
