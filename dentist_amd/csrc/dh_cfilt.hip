// dh_cfilt.hip -- the kernels of dh_la_collect_filter (lane code and layouts: dh_cfilt.h; driver: dh_cfilt.cpp).  gfx950, wave64.
//
//   k_cf_start          one lane per record: 1 iff it starts a chain, written twice: the copy in uid is scanned in place.
//   (dhk_scan_total / dhk_scan of dh_kernels.hip: the exclusive scans of the flags, whose 64-bit total is the number of chains,
//   and of the per-read counts)
//   k_cf_first          one lane per record: its unit (the scanned flags), and for a chain's first record the unit's first record.
//   k_cf_unit           one lane per chain: cf::make_unit over its members, the stage of 1-3 it fails, +1 for its read.
//   k_cf_scatter        one lane per chain: a slot of its read's segment (atomicAdd; the order reaches no result).
//   k_cf_classify       one lane per read: a read of one unit is finished here, the others go on the list of their tier; a read of
//                       the global tier claims its part of the slab.
//   k_cf_wave           one wavefront per read of 2..64 units, the units in registers: ranked by rotation over the lanes and
//                       moved to their places; Contained as a loop over x with the lanes as y and a ballot for the end of the scan;
//                       Ambiguous as a rotation over the lanes; Redundant as a ballot.
//   k_cf_block<BIG>     one workgroup per read of more units: the order of its units in LDS (BIG = false) or in its part of the
//                       slab (BIG = true), sorted by a bitonic network; then cf::bt_contained and cf::bt_ambiguous per place.
//   k_cf_finish         one lane per record: its flag from its unit's; the six counts per wavefront, one atomic each.
//
// No block leaves in front of a shuffle or a barrier other than as a whole.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dh_cfilt.h"

using cf::Mask;
using cf::Opts;
using cf::Rec;
using cf::Unit;

typedef unsigned long long u64;

__global__ void __launch_bounds__(CF_BLOCK) k_cf_start(const Rec *__restrict__ recs, int64_t n, int32_t *__restrict__ flag, int32_t *__restrict__ uid)
{
    const int64_t i = (int64_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    if (i >= n) return;
    flag[i] = uid[i] = i == 0 || !cf::continues(recs[i - 1], recs[i]) ? 1 : 0;
}

// flag: 1 for a chain's first record; uid: in the exclusive scan of flag, out the unit of every record; nunits: the number of
// chains (the scan's total; below 2^30, as the records are)
__global__ void __launch_bounds__(CF_BLOCK)
k_cf_first(const int32_t *__restrict__ flag, int32_t *uid, int64_t n, const u64 *__restrict__ nunits, int32_t *__restrict__ first)
{
    const int64_t i = (int64_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    if (i >= n) return;
    const int32_t u = uid[i] + flag[i] - 1;
    uid[i] = u;
    if (flag[i]) first[u] = (int32_t)i;
    if (i == n - 1) first[*nunits] = (int32_t)n;
}

__global__ void __launch_bounds__(CF_BLOCK)
k_cf_unit(const Rec *__restrict__ recs, int64_t n, const u64 *__restrict__ nunits, const int32_t *__restrict__ first, Mask mask,
          const int32_t *__restrict__ alen, const int32_t *__restrict__ blen, Opts o, Unit *__restrict__ units, uint8_t *__restrict__ why,
          int32_t *cnt)
{
    const int64_t u = (int64_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    const int64_t nu = (int64_t)*nunits;
    if (u >= nu) return;
    Unit x;
    why[u] = cf::make_unit(recs, first[u], first[u + 1], nu == n, mask, alen, blen, o, &x);
    units[u] = x;
    atomicAdd(cnt + x.bread, 1);
}

// goff: the scanned counts (the first slot of every read); cur: the slots claimed so far
__global__ void __launch_bounds__(CF_BLOCK)
k_cf_scatter(const Unit *__restrict__ units, const u64 *__restrict__ nunits, const int32_t *__restrict__ goff, int32_t *cur,
             int32_t *__restrict__ gidx)
{
    const int64_t u = (int64_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    if (u >= (int64_t)*nunits) return;
    const int32_t r = units[u].bread;
    gidx[goff[r] + atomicAdd(cur + r, 1)] = (int32_t)u;
}

// lists: the reads of the wave tier, of the LDS tier and of the global tier (nreads entries each at most); slab_at[k]: the part
// of the slab of the k-th read of the global tier
__global__ void __launch_bounds__(CF_BLOCK)
k_cf_classify(const Unit *__restrict__ units, const int32_t *__restrict__ goff, const int32_t *__restrict__ gidx, int32_t nreads,
              int32_t lds_units, uint8_t *__restrict__ why, uint8_t *__restrict__ used, uint32_t *ctr, int32_t *__restrict__ l_wave,
              int32_t *__restrict__ l_lds, int32_t *__restrict__ l_glob, uint32_t *__restrict__ slab_at)
{
    const int64_t r = (int64_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    const int32_t size = r < nreads ? goff[r + 1] - goff[r] : 0;
    const int tier = cf::tier_of(size, lds_units);
    if (tier == 1) {
        const int32_t u = gidx[goff[r]];
        uint8_t w = why[u];
        if (cf::single(units[u], &w)) why[u] = w, used[r] = 0;
    }
    // the wave tier is the common one: one atomic per wavefront
    const u64 b = __ballot(tier == 2);
    if (b) {  // (the same for the whole wavefront)
        const int leader = (int)__ffsll((long long)b) - 1;
        uint32_t at = 0u;
        if (lane == leader) at = atomicAdd(ctr + cf::C_WAVE, (uint32_t)__popcll(b));
        at = (uint32_t)__shfl((int32_t)at, leader, 64);
        if (tier == 2) l_wave[at + (uint32_t)__popcll(b & (((u64)1 << lane) - 1))] = (int32_t)r;
    }
    if (tier == 3) l_lds[atomicAdd(ctr + cf::C_LDS, 1u)] = (int32_t)r;
    if (tier == 4) {
        const uint32_t k = atomicAdd(ctr + cf::C_GLOBAL, 1u);
        l_glob[k] = (int32_t)r;
        slab_at[k] = atomicAdd(ctr + cf::C_SLAB, (uint32_t)cf::pow2ceil(size));
    }
}

// ---- the wave tier
__device__ __forceinline__ Unit shfl_unit(const Unit &u, int src)
{
    Unit v;
    v.aread = __shfl(u.aread, src, 64), v.bread = u.bread, v.abpos = __shfl(u.abpos, src, 64), v.aepos = __shfl(u.aepos, src, 64);
    v.bbpos = __shfl(u.bbpos, src, 64), v.bepos = __shfl(u.bepos, src, 64), v.bfb = __shfl(u.bfb, src, 64), v.bfe = __shfl(u.bfe, src, 64);
    v.st = (uint32_t)__shfl((int32_t)u.st, src, 64), v.pad = 0;
    return v;
}
__global__ void __launch_bounds__(CF_BLOCK)
k_cf_wave(const Unit *__restrict__ units, const int32_t *__restrict__ goff, const int32_t *__restrict__ gidx, const int32_t *__restrict__ list,
          int64_t nlist, uint8_t *__restrict__ why, uint8_t *__restrict__ used)
{
    const int64_t k = (int64_t)blockIdx.x * (CF_BLOCK / 64) + (threadIdx.x >> 6);
    if (k >= nlist) return;  // (a whole wavefront)
    const int32_t lane = (int32_t)(threadIdx.x & 63);
    const int32_t r = list[k], g0 = goff[r], size = goff[r + 1] - g0;  // 2..64
    const bool in = lane < size;
    int32_t idx = in ? gidx[g0 + lane] : -1;
    Unit me = units[in ? idx : gidx[g0]];
    // the place of every unit in the order of Contained, then every unit to its place
    int32_t rank = 0;
    for (int32_t z = 0; z < size; z++) {
        const Unit uz = shfl_unit(me, z);
        const int32_t iz = __shfl(idx, z, 64);
        rank += in && cf::key_less(uz, iz, me, idx) ? 1 : 0;
    }
    int32_t src = 0;
    for (int32_t z = 0; z < size; z++)
        if (__shfl(rank, z, 64) == lane) src = z;
    if (!in) src = 0;
    me = shfl_unit(me, src);
    idx = __shfl(idx, src, 64);
    if (!in) idx = -1;
    // 4: contained, order-free: x as it left stage 3
    bool mark = false;
    for (int32_t x = 0; x + 1 < size; x++) {
        const Unit ux = shfl_unit(me, x);
        if (ux.st & cf::DIS) continue;  // (the same for the whole wavefront)
        const bool behind = in && lane > x;
        const u64 ends = __ballot(behind && !cf::scan_goes_on(ux, me));
        const int32_t reach = ends ? (int32_t)__ffsll((long long)ends) - 1 : size;
        if (behind && lane < reach && cf::drops(ux, me) && !(me.st & cf::DIS)) mark = true;
    }
    uint8_t w = in ? why[idx] : (uint8_t)cf::W_NONE;
    if (mark) w = cf::W_CONTAINED;
    const bool en = in && cf::enabled(me, w);
    // 5: ambiguous
    bool amb = false;
    for (int32_t z = 0; z < size; z++) {
        const Unit uz = shfl_unit(me, z);
        const int32_t zen = __shfl(en ? 1 : 0, z, 64);
        if (en && zen && z != lane && cf::intersect(me, uz)) amb = true;
    }
    const bool any_amb = __ballot(amb) != 0;
    // 6: redundant
    const bool any_red = !any_amb && __ballot(en && (me.st & cf::RED)) != 0;
    if (en && (any_amb || any_red)) w = any_amb ? cf::W_AMBIGUOUS : cf::W_REDUNDANT;
    if (in && w != cf::W_NONE) why[idx] = w;
    if (lane == 0 && (any_amb || any_red)) used[r] = 0;
}

// ---- the workgroup tiers
template <bool BIG>
__global__ void __launch_bounds__(CF_BLOCK)
k_cf_block(const Unit *__restrict__ units, const int32_t *__restrict__ goff, const int32_t *__restrict__ gidx, const int32_t *__restrict__ list,
           const uint32_t *__restrict__ slab_at, int32_t *slab, uint8_t *why, uint8_t *__restrict__ used)
{
    extern __shared__ int32_t lds_ord[];
    __shared__ int32_t hit;
    const int32_t tid = (int32_t)threadIdx.x;
    const int32_t r = list[blockIdx.x], g0 = goff[r], size = goff[r + 1] - g0, P = cf::pow2ceil(size);
    int32_t *ord = BIG ? slab + slab_at[blockIdx.x] : lds_ord;
    for (int32_t t = tid; t < P; t += CF_BLOCK) ord[t] = t < size ? gidx[g0 + t] : -1;
    if (tid == 0) hit = 0;
    __syncthreads();
    for (int32_t k = 2; k <= P; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1) {
            for (int32_t t = tid; t < P / 2; t += CF_BLOCK) cf::bt_compare(ord, units, t, k, j);
            __syncthreads();
        }
    for (int32_t x = tid; x + 1 < size; x += CF_BLOCK) cf::bt_contained(ord, size, units, why, x);
    __syncthreads();
    for (int32_t x = tid; x + 1 < size; x += CF_BLOCK)
        if (cf::bt_ambiguous(ord, size, units, why, x)) hit = 1;
    __syncthreads();
    const bool any_amb = hit != 0;
    __syncthreads();
    if (!any_amb) {  // (the whole block)
        for (int32_t x = tid; x < size; x += CF_BLOCK)
            if (cf::enabled(units[ord[x]], why[ord[x]]) && (units[ord[x]].st & cf::RED)) hit = 1;
        __syncthreads();
    }
    if (!hit) return;  // (the whole block, behind the last barrier)
    for (int32_t x = tid; x < size; x += CF_BLOCK)
        if (cf::enabled(units[ord[x]], why[ord[x]])) why[ord[x]] = any_amb ? cf::W_AMBIGUOUS : cf::W_REDUNDANT;
    if (tid == 0) used[r] = 0;
}

__global__ void __launch_bounds__(CF_BLOCK)
k_cf_finish(const int32_t *__restrict__ flag, const int32_t *__restrict__ uid, int64_t n, const Unit *__restrict__ units,
            const uint8_t *__restrict__ why, uint8_t *__restrict__ out, u64 *cnt6)
{
    const int64_t i = (int64_t)blockIdx.x * CF_BLOCK + threadIdx.x;
    uint8_t w = cf::W_NONE;
    if (i < n) {
        const int32_t u = uid[i];
        const uint8_t wu = why[u];
        out[i] = ((units[u].st & cf::DIS) || wu != cf::W_NONE) ? 1 : 0;
        if (flag[i]) w = wu;  // a chain counts once
    }
    for (int s = 1; s <= 6; s++) {
        const u64 b = __ballot(w == s);
        if (b && (threadIdx.x & 63) == 0) atomicAdd(cnt6 + (s - 1), (u64)__popcll(b));
    }
}

// n < 2^30 (the driver refuses more): every grid stays far below 2^31 blocks
static inline dim3 cf_grid(int64_t m, int64_t per_block) { return dim3((unsigned)((m + per_block - 1) / per_block)); }

extern "C" void dhk_cf_start(hipStream_t st, const Rec *recs, int64_t n, int32_t *flag, int32_t *uid)
{
    if (n > 0) hipLaunchKernelGGL(k_cf_start, cf_grid(n, CF_BLOCK), dim3(CF_BLOCK), 0, st, recs, n, flag, uid);
}
extern "C" void dhk_cf_units(hipStream_t st, const Rec *recs, int64_t n, const int32_t *flag, int32_t *uid, const u64 *nunits, int32_t *first,
                             Mask mask, const int32_t *alen, const int32_t *blen, Opts o, Unit *units, uint8_t *why, int32_t *cnt)
{
    hipLaunchKernelGGL(k_cf_first, cf_grid(n, CF_BLOCK), dim3(CF_BLOCK), 0, st, flag, uid, n, nunits, first);
    hipLaunchKernelGGL(k_cf_unit, cf_grid(n, CF_BLOCK), dim3(CF_BLOCK), 0, st, recs, n, nunits, (const int32_t *)first, mask, alen, blen, o, units,
                       why, cnt);
}
extern "C" void dhk_cf_group(hipStream_t st, const Unit *units, int64_t n, int32_t nreads, int32_t lds_units, const int32_t *goff, int32_t *cur,
                             int32_t *gidx, uint8_t *why, uint8_t *used, const u64 *nunits, uint32_t *ctr, int32_t *l_wave, int32_t *l_lds,
                             int32_t *l_glob, uint32_t *slab_at)
{
    hipLaunchKernelGGL(k_cf_scatter, cf_grid(n, CF_BLOCK), dim3(CF_BLOCK), 0, st, units, nunits, goff, cur, gidx);
    hipLaunchKernelGGL(k_cf_classify, cf_grid(nreads, CF_BLOCK), dim3(CF_BLOCK), 0, st, units, goff, (const int32_t *)gidx, nreads, lds_units, why,
                       used, ctr, l_wave, l_lds, l_glob, slab_at);
}
extern "C" void dhk_cf_tiers(hipStream_t st, const Unit *units, const int32_t *goff, const int32_t *gidx, int64_t nwave, const int32_t *l_wave,
                             int64_t nlds, const int32_t *l_lds, int32_t lds_units, int64_t nglob, const int32_t *l_glob,
                             const uint32_t *slab_at, int32_t *slab, uint8_t *why, uint8_t *used)
{
    if (nwave > 0) hipLaunchKernelGGL(k_cf_wave, cf_grid(nwave, CF_BLOCK / 64), dim3(CF_BLOCK), 0, st, units, goff, gidx, l_wave, nwave, why, used);
    const size_t lds = sizeof(int32_t) * (size_t)cf::pow2ceil(lds_units);
    if (nlds > 0)
        hipLaunchKernelGGL(k_cf_block<false>, dim3((unsigned)nlds), dim3(CF_BLOCK), lds, st, units, goff, gidx, l_lds, slab_at, slab, why, used);
    if (nglob > 0)
        hipLaunchKernelGGL(k_cf_block<true>, dim3((unsigned)nglob), dim3(CF_BLOCK), 0, st, units, goff, gidx, l_glob, slab_at, slab, why, used);
}
extern "C" void dhk_cf_finish(hipStream_t st, const int32_t *flag, const int32_t *uid, int64_t n, const Unit *units, const uint8_t *why, uint8_t *out,
                              u64 *cnt6)
{
    if (n > 0) hipLaunchKernelGGL(k_cf_finish, cf_grid(n, CF_BLOCK), dim3(CF_BLOCK), 0, st, flag, uid, n, units, why, out, cnt6);
}
