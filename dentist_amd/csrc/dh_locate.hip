// dh_locate.hip -- the kernels of dh_exact_locate (lane code and layouts: dh_locate.h; driver: dh_locate.cpp).  gfx950, wave64.
//
//   k_locate_scan<BM>  streams the packed text.  A thread owns the 32 positions of one word: it holds the word and its
//                      successor and rolls the 64-bit window across them, probing the anchor table for every window
//                      (BM: behind a pre-filter bitmap in LDS).  On a hit it walks the group: record test, the next
//                      LOC_INLINE_BASES bases, then the candidate.  The walk is a wave-uniform loop (`any lane has a member
//                      left`), so that the candidates of a step are appended with ONE atomic add per wavefront.
//   k_locate_verify    one wavefront per (candidate, segment): a lane compares one pattern word per step of 64 words, the
//                      wavefront ballots after every step and leaves on the first mismatch, clearing the candidate's flag
//                      with a plain store of 0.
//   k_locate_short     patterns of 1..31 bases: one thread per text position, one masked compare per pattern (cost:
//                      positions x short patterns; contigs are never short).
//
// No kernel returns early in a way that splits a wavefront in front of a ballot: threads without work stay as `live ==
// false` lanes.  All counters and flags are written with vector instructions.
#include <hip/hip_runtime.h>

#include "dh_locate.h"

// the candidates of one step of a wavefront: one atomic add by the first emitting lane, slots by prefix count.  The counter
// keeps counting past the capacity (the host needs the true number); only the stores are bounded.
__device__ __forceinline__ void loc_append(bool emit, int64_t pos, uint32_t pat, LocCand *__restrict__ cands, int64_t cap,
                                           unsigned long long *__restrict__ counter)
{
    const uint64_t m = __ballot(emit);
    if (m == 0) return;  // wave-uniform
    const uint32_t lane = threadIdx.x & 63u, leader = (uint32_t)__ffsll((long long)m) - 1u;
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(m));
    base = __shfl(base, (int)leader, 64);
    if (emit) {
        const int64_t at = (int64_t)base + __popcll(m & ((1ull << lane) - 1ull));
        if (at < cap) cands[at] = LocCand{pos, pat, 1u};
    }
}

template <bool BM>
__global__ void __launch_bounds__(256)
k_locate_scan(const uint64_t *__restrict__ text, int64_t nbases, int64_t w0, int64_t w1, const LocSlot *__restrict__ table,
              int32_t tbits, const uint32_t *__restrict__ bitmap, const uint32_t *__restrict__ memb, const LocPat *__restrict__ pats,
              const uint64_t *__restrict__ pw, const int64_t *__restrict__ starts, int64_t nref, LocCand *__restrict__ cands,
              int64_t cap, unsigned long long *__restrict__ counter)
{
    __shared__ uint32_t s_bm[BM ? LOC_BITMAP_BITS / 32 : 1];
    if (BM) {
        for (int i = threadIdx.x; i < LOC_BITMAP_BITS / 32; i += 256) s_bm[i] = bitmap[i];
        __syncthreads();
    }
    const int64_t ntiles = (w1 - w0 + 255) >> 8;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t t = w0 + (tile << 8) + threadIdx.x;
        const bool live = t < w1;
        uint64_t lo = 0, hi = 0;
        if (live) {
            lo = text[t];
            hi = text[t + 1];
        }
        for (uint32_t j = 0; j < 32; j++) {
            const int64_t pos = (t << 5) + j;
            uint32_t first = 0, count = 0;
            if (live && pos + 32 <= nbases) {
                const uint64_t key = loc::funnel(lo, hi, 2u * j);
                if (BM)
                    loc::probe(table, tbits, (const uint32_t *)s_bm, key, first, count);
                else
                    loc::probe(table, tbits, (const uint32_t *)nullptr, key, first, count);
            }
            for (uint32_t k = 0; __any(k < count); k++) {
                bool emit = false;
                uint32_t e = 0;
                if (k < count) {
                    e = memb[first + k];
                    emit = loc::scan_member(text, nbases, starts, nref, pw, pats[e], pos);
                }
                loc_append(emit, pos, e, cands, cap, counter);
            }
        }
    }
}

__global__ void __launch_bounds__(256)
k_locate_short(const uint64_t *__restrict__ text, int64_t nbases, int64_t p0, int64_t p1, const LocShort *__restrict__ shorts,
               int64_t nshort, const int64_t *__restrict__ starts, int64_t nref, LocCand *__restrict__ cands, int64_t cap,
               unsigned long long *__restrict__ counter)
{
    const int64_t ntiles = (p1 - p0 + 255) >> 8;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t pos = p0 + (tile << 8) + threadIdx.x;
        const bool live = pos < p1 && pos < nbases;
        const uint64_t win = live ? loc::window(text, pos) : 0;
        int64_t rec_end = -1;  // end of the record of pos, found on the first match
        for (int64_t s = 0; s < nshort; s++) {
            const LocShort sp = shorts[s];
            bool emit = live && pos + (int64_t)sp.len <= nbases && loc::short_match(win, sp);
            if (emit) {
                if (rec_end < 0) rec_end = starts[loc::record_of(starts, nref, pos) + 1];
                emit = pos + (int64_t)sp.len <= rec_end;
            }
            loc_append(emit, pos, sp.pat, cands, cap, counter);
        }
    }
}

__global__ void __launch_bounds__(256)
k_locate_verify(const uint64_t *__restrict__ text, int64_t nbases, const uint64_t *__restrict__ pw, const LocPat *__restrict__ pats,
                LocCand *cands, int64_t ncands, const LocUnit *__restrict__ units, int64_t nunits, int64_t seg)
{
    const int64_t u = ((int64_t)blockIdx.x << 2) + (threadIdx.x >> 6);
    if (u >= nunits) return;  // a whole wavefront
    const uint32_t lane = threadIdx.x & 63u;
    const LocUnit un = units[u];
    if ((int64_t)un.cand >= ncands) return;
    const int64_t pos = cands[un.cand].pos;
    const LocPat p = pats[cands[un.cand].pat];
    const int64_t base0 = (int64_t)un.seg * seg;
    // (the host built the units from these very numbers: the test keeps a wrong plan from becoming a wild load)
    if (base0 >= p.len || pos < 0 || pos + p.len > nbases) return;
    const int64_t nb = p.len - base0 < seg ? p.len - base0 : seg, nw = (nb + 31) >> 5;
    for (int64_t wb = 0; wb < nw; wb += 64) {  // 64 x 32 bases a step
        const int64_t w = wb + lane;
        const uint64_t diff = w < nw ? loc::verify_word(text, pw, p, pos, base0, nb, w) : 0;
        if (__any(diff != 0)) {
            if (lane == 0) cands[un.cand].ok = 0u;
            return;
        }
    }
}

extern "C" void dhk_locate_scan(hipStream_t st, int use_bitmap, const uint64_t *text, int64_t nbases, int64_t w0, int64_t w1,
                                const LocSlot *table, int32_t tbits, const uint32_t *bitmap, const uint32_t *memb, const LocPat *pats,
                                const uint64_t *pw, const int64_t *starts, int64_t nref, LocCand *cands, int64_t cap,
                                unsigned long long *counter)
{
    if (w1 <= w0) return;
    const int64_t ntiles = (w1 - w0 + 255) >> 8;
    // a persistent grid: the bitmap is copied to LDS once per block, not once per tile
    const dim3 grid((uint32_t)(ntiles < 2048 ? ntiles : 2048)), block(256);
    if (use_bitmap)
        hipLaunchKernelGGL(k_locate_scan<true>, grid, block, 0, st, text, nbases, w0, w1, table, tbits, bitmap, memb, pats, pw, starts,
                           nref, cands, cap, counter);
    else
        hipLaunchKernelGGL(k_locate_scan<false>, grid, block, 0, st, text, nbases, w0, w1, table, tbits, bitmap, memb, pats, pw, starts,
                           nref, cands, cap, counter);
}

extern "C" void dhk_locate_short(hipStream_t st, const uint64_t *text, int64_t nbases, int64_t p0, int64_t p1, const LocShort *shorts,
                                 int64_t nshort, const int64_t *starts, int64_t nref, LocCand *cands, int64_t cap,
                                 unsigned long long *counter)
{
    if (p1 <= p0 || nshort <= 0) return;
    const int64_t ntiles = (p1 - p0 + 255) >> 8;
    hipLaunchKernelGGL(k_locate_short, dim3((uint32_t)(ntiles < 8192 ? ntiles : 8192)), dim3(256), 0, st, text, nbases, p0, p1, shorts,
                       nshort, starts, nref, cands, cap, counter);
}

extern "C" void dhk_locate_verify(hipStream_t st, const uint64_t *text, int64_t nbases, const uint64_t *pw, const LocPat *pats,
                                  LocCand *cands, int64_t ncands, const LocUnit *units, int64_t nunits, int64_t seg)
{
    if (nunits <= 0) return;
    hipLaunchKernelGGL(k_locate_verify, dim3((uint32_t)((nunits + 3) >> 2)), dim3(256), 0, st, text, nbases, pw, pats, cands, ncands,
                       units, nunits, seg);
}
