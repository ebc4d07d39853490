// dh_tjoin.hip -- gfx950 kernels of the per-group k-mer table join that seeds a grouped call A != B (design: dh_tjoin.h).
// Replaces, for the consensus re-alignment (templates against the reads of their pile-ups), the directory lookups of the
// seed filter (k_seed, dh_seed.hip): the hits a read gets are the same multiset.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "dh_kmer.h"
#include "dh_tjoin.h"

#define LANES 64
#define HIT_QBITS 24

#ifdef DH_TJ_PROF
__device__ unsigned long long g_tj_prof[4];
#define TP(i) if (tid == 0) { const unsigned long long t_ = wall_clock64(); atomicAdd(&g_tj_prof[i], t_ - tp_); tp_ = t_; }
#define TP_BEGIN unsigned long long tp_ = wall_clock64();
extern "C" void dhk_tj_prof_dump()
{
    unsigned long long h[4];
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_tj_prof), sizeof(h));
    if (h[3])
        fprintf(stderr, "[tj prof] k_tjoin, %llu units: table build %.1f roll + probe %.1f write %.1f us per unit and block\n", h[3],
                h[0] / 100.0 / h[3], h[1] / 100.0 / h[3], h[2] / 100.0 / h[3]);
    unsigned long long z[4] = {0};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_tj_prof), z, sizeof(z));
}
#else
#define TP(i)
#define TP_BEGIN
#endif

__global__ void __launch_bounds__(256)
k_tj_group_offsets(const uint32_t *__restrict__ dir, int32_t ngroups, int32_t k, int32_t shift, int64_t nb, uint32_t *__restrict__ gent)
{
    const int32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > ngroups) return;
    int64_t b = (int64_t)(((uint64_t)g << (2 * k)) >> shift);
    b = b < nb ? b : nb;
    gent[g] = dir[b - 1];  // (dir[-1] == 0)
}

// 8 base codes (one per byte, the first base in the lowest byte) as 16 bits, the first base on top
static __device__ __forceinline__ uint32_t tj_pack8(uint64_t w)
{
    uint64_t x = __builtin_bswap64(w) & 0x0303030303030303ull;
    x = (x | (x >> 6)) & 0x000F000F000F000Full;
    x = (x | (x >> 12)) & 0x000000FF000000FFull;
    return (uint32_t)((x | (x >> 24)) & 0xFFFFull);
}

// One read by one wavefront, 512 consecutive k-mer starts per step: lane l takes the eight that start at 8 l .. 8 l + 7
// of the step.  Its 23 bases are three 8-byte loads (8 bytes apart from lane to lane: the wavefront reads consecutive
// lines; the DB buffers are padded), packed ONCE into 48 bits with the first base on top; their reverse complement is
// one bit reversal of that word.  k-mer j is then a shift and a mask of either word (k <= 16) -- no rolling, no k - 1
// bases of warm-up.  What seed_item decides while rolling is decided here from the same bases: a base outside a, c, g, t
// among the k (valid >= k there), the canonical choice, kmer_sampled, mask_touch on B (one load of mask bits per lane
// and step).  The next step's loads are on their way while a step is worked on.
// (Two earlier forms, LABNOTES 24: a stretch of the read per lane rolled as seed_item does -- loads 40 bytes apart
// from lane to lane, a third of the steps warm-up; and a k-mer per lane packed from 16 bases of its own -- 130 vector
// instructions per k-mer, the kernel bound by them.)
// WRITE = false: the hits of the lane are counted; WRITE = true: they are written to out[0, limit) at the positions
// the wavefront's LDS cursor hands out (the order inside a segment is free: the back end sorts).
template <bool WRITE>
static __device__ uint32_t tj_read(const DbView &B, const IndexView &ix, const DhOpts &o, const KmerSampler &smp, const uint64_t *tab,
                                   int32_t r, int lane, uint32_t g0, uint64_t *__restrict__ out, uint32_t limit, uint32_t *cur)
{
    constexpr int PER = 8, STEP = LANES * PER;
    constexpr uint64_t BAD = 0xFCFCFCFCFCFCFCFCull;
    const int64_t bo = B.off[r];
    const int32_t blen = (int32_t)(B.off[r + 1] - bo);
    const uint8_t *b = B.bases + bo;
    const int k = o.k;
    const int32_t npos = blen - k + 1;
    const uint32_t kmask = k >= 16 ? 0xFFFFFFFFu : ((1u << (2 * k)) - 1u);
    const uint32_t kbits = (1u << k) - 1u;
    uint32_t cnt = 0;
    uint64_t n0 = 0, n1 = 0, n2 = 0, nm = 0;
    auto fetch = [&](int32_t q0) {
        if (q0 < npos) {
            n0 = load8(b + q0);
            n1 = load8(b + q0 + 8);
            n2 = load8(b + q0 + 16);
            if (B.mask_bits) nm = load8(B.mask_bits + ((bo + q0) >> 3)) >> ((bo + q0) & 7);  // as mask_touch (dh_kmer.h)
        }
    };
    fetch(lane * PER);
    for (int32_t base = 0; base < npos; base += STEP) {
        const int32_t q0 = base + lane * PER;
        const uint64_t w0 = n0, w1 = n1, w2 = n2;
        const uint32_t mbits = (uint32_t)nm;
        fetch(q0 + STEP);
        if (q0 >= npos) continue;
        // bit i: base i of the lane's 23 is outside a, c, g, t (rare: the bitmap is made only then)
        uint32_t nbits = 0;
        if ((w0 | w1 | w2) & BAD) {
            for (int i = 0; i < 8; i++) {
                nbits |= (((w0 >> (8 * i)) & 0xFC) ? 1u : 0u) << i;
                nbits |= (((w1 >> (8 * i)) & 0xFC) ? 1u : 0u) << (8 + i);
                nbits |= (((w2 >> (8 * i)) & 0xFC) ? 1u : 0u) << (16 + i);
            }
        }
        const uint64_t P = ((uint64_t)tj_pack8(w0) << 32) | ((uint64_t)tj_pack8(w1) << 16) | (uint64_t)tj_pack8(w2);
        // complement of base i at bits 2 i: the 2-bit groups of ~P reversed inside 48 bits
        uint64_t R = __brevll(~P);
        R = (((R >> 1) & 0x5555555555555555ull) | ((R & 0x5555555555555555ull) << 1)) >> 16;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const int32_t q = q0 + j;
            const uint32_t km = (uint32_t)(P >> (48 - 2 * k - 2 * j)) & kmask;
            const uint32_t rc = (uint32_t)(R >> (2 * j)) & kmask;
            const uint32_t canon = km < rc ? km : rc;
            const bool em = q < npos && !(((nbits | mbits) >> j) & kbits) && kmer_sampled((uint64_t)canon, smp);
            if (!em) continue;
            const uint32_t bori = km != canon ? 1u : 0u;
            const bool pal = km == rc;
            const TjMatch m = tj_match(tab, canon, bori, pal, o.tcap, o.strands);
            if (!WRITE)
                cnt += (uint32_t)(m.fwd + m.rev);
            else if (m.emit) {
                tj_walk(tab, canon, [&](uint32_t lo) {
                    const bool same = (lo >> 31) == bori;
                    const int64_t gv = (int64_t)(ix.ent[g0 + (lo & 0x7FFFFFFFu)].y & ((1ull << 40) - 1));
                    for (int32_t strand = 0; strand < 2; strand++) {
                        if (!(m.emit & (1u << strand)) || !(strand ? (!same || pal) : (same || pal))) continue;
                        const int32_t qs = strand ? blen - k - q : q;  // position on the oriented read
                        const int64_t D = gv + ix.sepv - qs;
                        const uint32_t slot = atomicAdd(cur, 1u);
                        if (slot < limit) out[slot] = ((uint64_t)strand << 63) | ((uint64_t)D << HIT_QBITS) | (uint32_t)qs;
                        cnt++;
                    }
                });
            }
        }
    }
    return cnt;
}

// Persistent blocks, one per CU (the table takes 128 of its 160 KB of LDS); a unit = (group, up to TJ_RUN consecutive
// reads of it), a wavefront per read.  Units of one group follow each other in the list and a block takes TJ_QBATCH of
// them per atomic on the queue, so most units find their group's table built.
__global__ void __launch_bounds__(TJ_THREADS, 1)
k_tjoin(DbView B, IndexView ix, DhOpts o, TjView t)
{
    __shared__ uint64_t tab[TJ_SLOTS];
    __shared__ uint32_t s_cnt[TJ_RUN], s_cur[TJ_RUN];
    __shared__ unsigned long long s_base;
    __shared__ int32_t s_work, s_ok;
    const int tid = threadIdx.x, lane = tid & (LANES - 1), wv = tid / LANES;
    const KmerSampler smp = kmer_sampler(o.kmer_mod, o.k);
    const uint64_t kmask = (1ull << (2 * o.k)) - 1;
    int32_t have = -1;  // the group whose table is built
    uint32_t g0 = 0;
    TP_BEGIN
    for (;;) {
        __syncthreads();
        if (tid == 0) s_work = (int32_t)atomicAdd(t.queue, (uint32_t)TJ_QBATCH);
        __syncthreads();
        const int32_t u0 = s_work;
        if (u0 >= t.nunits) break;
#pragma unroll 1
        for (int32_t u = u0; u < min(u0 + TJ_QBATCH, t.nunits); u++) {
            const int4 un = t.units[u];
            if (un.x != have) {
                have = un.x;
                uint32_t g1 = 0;
                g0 = 0;
                if ((uint32_t)un.x < (uint32_t)t.ngroups) {
                    g0 = t.gent[un.x];
                    g1 = t.gent[un.x + 1];
                }
                if (g1 - g0 > (uint32_t)TJ_CAP || g1 > (uint32_t)ix.n || g1 < g0) {  // (the host plans no such call)
                    if (tid == 0) atomicOr(t.status, DH_ST_TJ_OVERFLOW);
                    g1 = g0;
                }
                for (int32_t i = tid; i < TJ_SLOTS; i += TJ_THREADS) tab[i] = TJ_EMPTY;
                __syncthreads();
                for (uint32_t e = g0 + tid; e < g1; e += TJ_THREADS) {
                    const uint64_t x = ix.ent[e].x;
                    tj_insert(tab, tj_slot((uint32_t)(x & kmask), (uint32_t)(x >> 63), e - g0), [](uint64_t *p, uint64_t v) {
                        return atomicCAS((unsigned long long *)p, (unsigned long long)TJ_EMPTY, (unsigned long long)v) == TJ_EMPTY;
                    });
                }
                __syncthreads();
                TP(0)
            }
            const int32_t r = un.y + wv;
            const bool mine = r < un.z;
            uint32_t c = mine ? tj_read<false>(B, ix, o, smp, tab, r, lane, g0, nullptr, 0u, nullptr) : 0u;
            for (int off = LANES / 2; off > 0; off >>= 1) c += __shfl_xor(c, off, LANES);
            if (lane == 0) {
                s_cnt[wv] = c;
                s_cur[wv] = 0;
            }
            __syncthreads();
            if (tid == 0) {
                unsigned long long total = 0;
                for (int i = 0; i < TJ_RUN; i++) total += s_cnt[i];
                const unsigned long long base = total ? atomicAdd(t.cursor, total) : 0ull;
                const bool ok = base + total <= (unsigned long long)t.hits_cap;
                if (!ok) atomicOr(t.status, DH_ST_TJ_HITCAP);
                s_base = base;
                s_ok = ok ? 1 : 0;
            }
            __syncthreads();
            TP(1)
            if (mine && s_ok) {
                unsigned long long first = s_base;
                for (int i = 0; i < wv; i++) first += s_cnt[i];
                if (c >= (1u << 24) || first >= (1ull << 40)) {
                    if (lane == 0) atomicOr(t.status, DH_ST_TJ_OVERFLOW);
                } else {
                    if (c) tj_read<true>(B, ix, o, smp, tab, r, lane, g0, t.hits + first, c, &s_cur[wv]);
                    if (lane == 0) t.segtab[r - t.read0] = (first << 24) | c;
                }
            }
            __syncthreads();  // the unit's counters and (a new group) the table are done with
            TP(2)
#ifdef DH_TJ_PROF
            if (tid == 0) atomicAdd(&g_tj_prof[3], 1ull);
#endif
        }
    }
}

extern "C" void dhk_tj_group_offsets(hipStream_t st, const uint32_t *dir, int32_t ngroups, int32_t k, int32_t shift, int64_t nb,
                                     uint32_t *gent)
{
    hipLaunchKernelGGL(k_tj_group_offsets, dim3((unsigned)((ngroups + 1 + 255) / 256)), dim3(256), 0, st, dir, ngroups, k, shift, nb, gent);
}

extern "C" void dhk_tjoin(hipStream_t st, DbView B, IndexView ix, DhOpts o, TjView t, int32_t ncu)
{
    if (t.nunits <= 0) return;
    const int32_t batches = (t.nunits + TJ_QBATCH - 1) / TJ_QBATCH;
    hipLaunchKernelGGL(k_tjoin, dim3((unsigned)std::min(batches, std::max(1, ncu))), dim3(TJ_THREADS), 0, st, B, ix, o, t);
#ifdef DH_TJ_PROF
    if (getenv("DH_TRACE")) {
        (void)hipStreamSynchronize(st);
        dhk_tj_prof_dump();
    }
#endif
}
