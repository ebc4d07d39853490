// dh_chain.hip -- the kernels of dh_la_chain (lane code and layouts: dh_chain.h; driver: dh_chain.cpp).  gfx950, wave64.
//
//   k_chain_single       pairs with one enabled record: a flat kernel, one lane per pair.
//   k_chain_wave         2..64 nodes: one wavefront per pair, lane v owns node v, everything in registers.  Rank sort by
//                        counting; the relaxation broadcasts node u with its final distance and lane v > u relaxes its own
//                        node; the components come from a 64-bit adjacency mask per lane (Warshall over the lanes); the
//                        selection walks with wave-uniform masks of the taken, end and alternate nodes.
//   k_chain_lds          65..cap nodes: the arr_* phases of dh_chain.h with the node arrays in LDS.
//   k_chain_global       more: the same phases with the arrays in a slab of global memory (a barrier orders a step's
//                        stores before the next step's loads; the workgroup is one wavefront).
//   k_chain_emit_single  \ after the scan of the pairs' record and chain counts: src_index, flags, off and score in the
//   k_chain_emit         / order of the contract (one lane, one wavefront per pair).
//
// Every block is one wavefront.  No block leaves in front of a barrier or a ballot other than as a whole.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "dh_chain.h"

using chn::Arrays;
using chn::Key;
using chn::Node;
using chn::Opts;
using chn::State;

struct DevMem {
    static __device__ __forceinline__ int32_t load(const int32_t *p)
    {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    static __device__ __forceinline__ int32_t atomic_min(int32_t *p, int32_t v) { return atomicMin(p, v); }
};

__device__ __forceinline__ int32_t wave_max(int32_t v)
{
    for (int s = 32; s > 0; s >>= 1) v = max(v, __shfl_xor(v, s, 64));
    return v;
}
__device__ __forceinline__ uint64_t wave_sum(uint64_t v)
{
    for (int s = 32; s > 0; s >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s, 64);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src, 64), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

__global__ void __launch_bounds__(256)
k_chain_single(const Node *__restrict__ nodes, const int64_t *__restrict__ pair_off, const int32_t *__restrict__ list, int64_t npairs,
               Opts o, State *__restrict__ state, uint32_t *__restrict__ cnt_rec, uint32_t *__restrict__ cnt_ch)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int32_t p = list[i];
    const int64_t at = pair_off[p];
    const State s = chn::single_state(nodes[at], o);
    state[at] = s;
    cnt_rec[p] = cnt_ch[p] = (s.depth & CH_END) ? 1u : 0u;
}

__global__ void __launch_bounds__(64)
k_chain_wave(const Node *__restrict__ nodes, const int64_t *__restrict__ pair_off, const int32_t *__restrict__ list, Opts o,
             State *__restrict__ state, uint32_t *__restrict__ cnt_rec, uint32_t *__restrict__ cnt_ch)
{
    const int32_t p = list[blockIdx.x];
    const int64_t node0 = pair_off[p];
    const int32_t n = (int32_t)(pair_off[p + 1] - node0);  // 2..64
    const int32_t lane = (int32_t)threadIdx.x;
    const bool live = lane < n;
    Node x = Node{0, 0, 0, 0, 0u};
    if (live) x = nodes[node0 + lane];
    // the node order: every lane counts the nodes that precede its own, then fetches the node of its own rank
    int32_t rank = 0;
    for (int32_t w = 0; w < n; w++) {
        const int32_t wab = __shfl(x.abpos, w, 64), wbb = __shfl(x.bbpos, w, 64);
        rank += chn::precedes(wab, wbb, w, x.abpos, x.bbpos, lane) ? 1 : 0;
    }
    int32_t from = lane;
    for (int32_t w = 0; w < n; w++)
        if (__shfl(rank, w, 64) == lane && live) from = w;
    const int32_t ab = __shfl(x.abpos, from, 64), ae = __shfl(x.aepos, from, 64), bb = __shfl(x.bbpos, from, 64),
                  be = __shfl(x.bepos, from, 64);
    const uint32_t comp = (uint32_t)__shfl((int)x.flags, from, 64) & CH_FLAG_COMP;
    int32_t dist = -chn::score(ab, ae, bb, be), pred = -1;
    uint32_t depth = 1u;
    uint64_t nbr = 0;
    // the relaxation: u ascending, node u is final when its turn comes
    for (int32_t u = 0; u < n; u++) {
        const int32_t uab = __shfl(ab, u, 64), uae = __shfl(ae, u, 64), ubb = __shfl(bb, u, 64), ube = __shfl(be, u, 64);
        const uint32_t ucomp = (uint32_t)__shfl((int)comp, u, 64), udepth = (uint32_t)__shfl((int)depth, u, 64);
        const int32_t ud = __shfl(dist, u, 64);
        bool edge = false;
        if (live && lane > u) edge = chn::relax_edge(uab, uae, ubb, ube, ucomp, ud, udepth, u, ab, ae, bb, be, comp, o, dist, pred, depth);
        const uint64_t m = __ballot(edge);
        if (edge) nbr |= 1ull << u;
        if (lane == u) nbr |= m;
    }
    // components: the transitive closure of the adjacency rows; the label is the smallest position reached
    uint64_t reach = nbr | (1ull << lane);
    for (int32_t w = 0; w < n; w++) {
        const uint64_t rw = shfl64(reach, w);
        if ((reach >> w) & 1ull) reach |= rw;
    }
    const int32_t label = (int32_t)__ffsll((long long)reach) - 1;
    // selection order: (component, dist, position)
    int32_t srank = 0;
    for (int32_t w = 0; w < n; w++) {
        const int32_t lw = __shfl(label, w, 64), dw = __shfl(dist, w, 64);
        srank += (lw != label ? lw < label : (dw != dist ? dw < dist : w < lane)) ? 1 : 0;
    }
    uint64_t taken = 0, ends = 0, alts = 0;  // wave-uniform
    int32_t cur = -1, cthr = 0;
    for (int32_t k = 0; k < n; k++) {
        const int32_t e = (int32_t)__ffsll((long long)__ballot(live && srank == k)) - 1;
        const int32_t le = __shfl(label, e, 64), de = __shfl(dist, e, 64);
        if (le != cur) {
            cur = le;
            cthr = chn::threshold(o.min_score, o.min_rel_score, -de);
        }
        if (((taken >> e) & 1ull) || -de < cthr) continue;
        bool alt = false;
        int32_t v = e;
        while (v >= 0) {
            if ((taken >> v) & 1ull) {
                alt = true;
                break;
            }
            taken |= 1ull << v;
            v = __shfl(pred, v, 64);
        }
        ends |= 1ull << e;
        if (alt) alts |= 1ull << e;
    }
    const int32_t best = wave_max(live ? -dist : INT32_MIN);
    const int32_t thr = chn::threshold(o.min_score, o.min_rel_score, best);
    const bool acc = live && ((ends >> lane) & 1ull) && -dist >= thr;
    if (live)
        state[node0 + lane] = State{(int32_t)((uint32_t)from | (comp << 31)), pred,
                                    depth | (acc ? CH_END | (((alts >> lane) & 1ull) ? CH_ALT : 0u) : 0u), dist};
    const uint64_t nrec = wave_sum(acc ? (uint64_t)depth : 0ull);
    const uint64_t macc = __ballot(acc);
    if (lane == 0) {
        cnt_rec[p] = (uint32_t)nrec;
        cnt_ch[p] = (uint32_t)__popcll(macc);
    }
}

// the phases of dh_chain.h, a barrier between them
__device__ __forceinline__ void chain_arrays(const Node *nodes, int32_t n, const Arrays &a, const Opts &o, State *state, uint32_t *cnt_rec,
                                             uint32_t *cnt_ch)
{
    const int32_t lane = (int32_t)threadIdx.x;
    chn::arr_load(nodes, n, a, lane);
    __syncthreads();
    for (int32_t u = 0; u < n; u++) {
        chn::arr_relax<DevMem>(a, n, u, o, lane);
        __syncthreads();
    }
    chn::arr_label<DevMem>(a, n, lane);
    __syncthreads();
    chn::arr_rank(a, n, lane);
    __syncthreads();
    chn::arr_select(a, n, o, lane);
    __syncthreads();
    const int32_t best = wave_max(chn::arr_best(a, n, lane));
    const int32_t thr = chn::threshold(o.min_score, o.min_rel_score, best);
    uint64_t nrec = 0;
    uint32_t nch = 0;
    chn::arr_finish(a, n, thr, state, lane, nrec, nch);
    nrec = wave_sum(nrec);
    const uint64_t nchs = wave_sum((uint64_t)nch);
    if (lane == 0) {
        *cnt_rec = chn::clamp_records(nrec);
        *cnt_ch = (uint32_t)nchs;
    }
}

__global__ void __launch_bounds__(64)
k_chain_lds(const Node *nodes, const int64_t *__restrict__ pair_off, const int32_t *__restrict__ list, Opts o, State *state,
            uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    __shared__ int32_t s_arr[CH_ARRAYS * CH_LDS_NODES];
    const int32_t p = list[blockIdx.x];
    const int64_t node0 = pair_off[p];
    const int32_t n = (int32_t)(pair_off[p + 1] - node0);
    if (n > CH_LDS_NODES) return;  // (the driver never sends one; the whole block leaves)
    chain_arrays(nodes + node0, n, chn::carve(s_arr, n), o, state + node0, cnt_rec + p, cnt_ch + p);
}

__global__ void __launch_bounds__(64)
k_chain_global(const Node *nodes, const int64_t *__restrict__ pair_off, const int32_t *__restrict__ list,
               const int64_t *__restrict__ woff, int32_t *slab, Opts o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    const int32_t p = list[blockIdx.x];
    const int64_t node0 = pair_off[p];
    const int32_t n = (int32_t)(pair_off[p + 1] - node0);
    chain_arrays(nodes + node0, n, chn::carve(slab + woff[blockIdx.x], n), o, state + node0, cnt_rec + p, cnt_ch + p);
}

__global__ void __launch_bounds__(256)
k_chain_emit_single(const Node *__restrict__ nodes, const State *__restrict__ state, const int64_t *__restrict__ pair_off,
                    const int32_t *__restrict__ list, int64_t npairs, const uint32_t *__restrict__ rec_at,
                    const uint32_t *__restrict__ ch_at, int64_t *__restrict__ off, int32_t *__restrict__ sc, int64_t *__restrict__ src,
                    uint32_t *__restrict__ flags)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const int32_t p = list[i];
    if (ch_at[p + 1] == ch_at[p]) return;
    const int64_t at = pair_off[p];
    const uint32_t r = rec_at[p], c = ch_at[p];
    off[c] = r;
    sc[c] = -state[at].dist;
    src[r] = at;
    flags[r] = nodes[at].flags | CH_FLAG_START | CH_FLAG_BEST;
}

__global__ void __launch_bounds__(64)
k_chain_emit(const Node *__restrict__ nodes, const State *__restrict__ state, const int64_t *__restrict__ pair_off,
             const int32_t *__restrict__ list, const uint32_t *__restrict__ rec_at, const uint32_t *__restrict__ ch_at, Key *key,
             int64_t *__restrict__ off, int32_t *__restrict__ sc, int64_t *__restrict__ src, uint32_t *__restrict__ flags)
{
    const int32_t p = list[blockIdx.x];
    if (ch_at[p + 1] == ch_at[p]) return;  // no accepted chain: the whole block leaves
    const int64_t node0 = pair_off[p];
    const int32_t n = (int32_t)(pair_off[p + 1] - node0);
    const int32_t lane = (int32_t)threadIdx.x;
    chn::emit_keys(nodes + node0, state + node0, n, key + node0, lane);
    __syncthreads();
    chn::emit_write(nodes + node0, state + node0, n, key + node0, node0, (int64_t)rec_at[p], (int64_t)ch_at[p], off, sc, src, flags, lane);
}

static inline Opts opts_of(const void *o) { return *(const Opts *)o; }
// wavefront-per-pair launches go out in slices: a grid stays below 2^32 threads
static const int64_t CH_LAUNCH_BLOCKS = (int64_t)1 << 24;

extern "C" void dhk_chain_single(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, int64_t npairs,
                                 const void *o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    if (npairs <= 0) return;
    hipLaunchKernelGGL(k_chain_single, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, st, nodes, pair_off, list, npairs, opts_of(o),
                       state, cnt_rec, cnt_ch);
}
extern "C" void dhk_chain_wave(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, int64_t npairs,
                               const void *o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    for (int64_t at = 0; at < npairs; at += CH_LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_chain_wave, dim3((unsigned)std::min<int64_t>(CH_LAUNCH_BLOCKS, npairs - at)), dim3(64), 0, st, nodes, pair_off,
                           list + at, opts_of(o), state, cnt_rec, cnt_ch);
}
extern "C" void dhk_chain_lds(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, int64_t npairs, const void *o,
                              State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    for (int64_t at = 0; at < npairs; at += CH_LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_chain_lds, dim3((unsigned)std::min<int64_t>(CH_LAUNCH_BLOCKS, npairs - at)), dim3(64), 0, st, nodes, pair_off,
                           list + at, opts_of(o), state, cnt_rec, cnt_ch);
}
extern "C" void dhk_chain_global(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, const int64_t *woff,
                                 int64_t npairs, int32_t *slab, const void *o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    for (int64_t at = 0; at < npairs; at += CH_LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_chain_global, dim3((unsigned)std::min<int64_t>(CH_LAUNCH_BLOCKS, npairs - at)), dim3(64), 0, st, nodes, pair_off,
                           list + at, woff + at, slab, opts_of(o), state, cnt_rec, cnt_ch);
}
extern "C" void dhk_chain_emit(hipStream_t st, const Node *nodes, const State *state, const int64_t *pair_off, const int32_t *list,
                               int64_t nsingle, int64_t nmulti, const uint32_t *rec_at, const uint32_t *ch_at, Key *key, int64_t *off,
                               int32_t *sc, int64_t *src, uint32_t *flags)
{
    if (nsingle > 0)
        hipLaunchKernelGGL(k_chain_emit_single, dim3((unsigned)((nsingle + 255) / 256)), dim3(256), 0, st, nodes, state, pair_off, list, nsingle,
                           rec_at, ch_at, off, sc, src, flags);
    for (int64_t at = 0; at < nmulti; at += CH_LAUNCH_BLOCKS)
        hipLaunchKernelGGL(k_chain_emit, dim3((unsigned)std::min<int64_t>(CH_LAUNCH_BLOCKS, nmulti - at)), dim3(64), 0, st, nodes, state, pair_off,
                           list + nsingle + at, rec_at, ch_at, key, off, sc, src, flags);
}
