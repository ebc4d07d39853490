// dh_nwa.hip -- global alignment of whole sequence pairs with affine gap costs (Gotoh; what EMBOSS stretcher computes for
// `dentist check-results`).  gfx950, wave64.
//
//   k_nwa<CPL, NS>  one wavefront per pair: the diagonals [lo, hi] of the matrix, a matrix row per step, CPL band cells per
//                   lane and strip, NS strips (dh_nwa.h has the recurrence, the decisions and the exactness argument).
//                   Rows i - 1 of H and F stay in registers; a lane takes H and F of the first cell of the lane to its right
//                   and G of the last cell of the lane to its left by shuffles, the prefix minimum by DPP (nw_scan_min of
//                   dh_nw.h), the carries between strips by readlane.  No LDS.  Lane 0 walks the decisions back and leaves
//                   the ops as the back-to-front words k_edit_compact (dh_editpath.hip) consumes.
//
// The decision words (4 bits per cell, [row][word]) live in global memory, as k_nw's do; the host bounds the footprint by
// the pairs it hands to a launch (DH_NW_CHUNK_KB).
#include <hip/hip_runtime.h>

#include "dh_nwa.h"

template <int CPL, int NS>
__global__ void __launch_bounds__(64)
k_nwa(const NwPair *__restrict__ pairs, int32_t n, const uint8_t *__restrict__ refs, const uint8_t *__restrict__ qrys, NwaCost c,
      uint64_t *__restrict__ dmat, int64_t dm_words, uint64_t *__restrict__ owords, int64_t ow_words, EpResult *__restrict__ res)
{
    constexpr int STRIP = 64 * CPL;
    const int32_t g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    const NwPair p = pairs[g];
    const int32_t rl = p.rl, ql = p.ql, lo = p.lo, W = p.hi - p.lo + 1;
    const int64_t stride = nwa::row_words(W);
    // (the host planned the buffers from these very numbers: the test keeps a wrong plan from becoming a wild store)
    if (rl < 1 || ql < 1 || rl > NWA_MAX_LEN || ql > NWA_MAX_LEN || W < 1 || W > NS * STRIP || lo < -rl || p.hi > ql ||
        ql - rl < lo || ql - rl > p.hi || p.dm_off < 0 || p.dm_off + (int64_t)rl * stride > dm_words || p.ow_off < 0 ||
        p.ow_off + (((int64_t)rl + ql + 7) >> 3) > ow_words) {
        if (lane == 0) res[g] = EpResult{EP_REJECTED, 0u};
        return;
    }
    const uint8_t *ref = refs + p.roff, *qry = qrys + p.qoff;
    uint64_t *dm = dmat + p.dm_off;
    int32_t H[NS][CPL], F[NS][CPL];
    uint32_t qn[NS][CPL / 4];  // the query window of the next row
#pragma unroll
    for (int s = 0; s < NS; s++) {
        const int32_t R0 = s * STRIP + lane * CPL;
        nwa::row0<CPL>(H[s], F[s], lo + R0, nw::valid_limit(lo + R0, R0, W, ql), c);
        nw::load_window<CPL>(qry, lo + R0, ql, qn[s]);
    }
    uint64_t refw = 0;
    for (int32_t i = 1; i <= rl; i++) {
        const int32_t o = (i - 1) & 7;
        if (o == 0) memcpy(&refw, ref + (i - 1), 8);
        const uint32_t rc = (uint32_t)(refw >> (8 * o)) & 0xFFu;
        const int32_t border = c.co + c.ce * i;
        // rows i - 1 of the cell behind a lane's cells: the first cell of the lane to the right, for lane 63 the first cell
        // of lane 0 of the next strip.  All of them before any strip overwrites its rows.
        int32_t nh[NS], nf[NS];
        uint32_t qc[NS][CPL / 4];
#pragma unroll
        for (int s = 0; s < NS; s++) {
            nh[s] = __shfl_down(H[s][0], 1, 64);
            nf[s] = __shfl_down(F[s][0], 1, 64);
            const int32_t wh = s + 1 < NS ? __builtin_amdgcn_readlane(H[s + 1 < NS ? s + 1 : s][0], 0) : NW_INF;
            const int32_t wf = s + 1 < NS ? __builtin_amdgcn_readlane(F[s + 1 < NS ? s + 1 : s][0], 0) : NW_INF;
            if (lane == 63) {
                nh[s] = wh;
                nf[s] = wf;
            }
#pragma unroll
            for (int k = 0; k < CPL / 4; k++) qc[s][k] = qn[s][k];
            nw::load_window<CPL>(qry, i + lo + s * STRIP + lane * CPL, ql, qn[s]);  // row i + 1: j - 1 = i + lo + R
        }
        int32_t carry = NW_INF;   // min of (G - ce R) over the strips in front: wave-uniform
        int32_t gcarry = NW_INF;  // G of the last cell of the strip in front: wave-uniform
        uint64_t *row = dm + (int64_t)(i - 1) * stride;
#pragma unroll
        for (int s = 0; s < NS; s++) {
            const int32_t R0 = s * STRIP + lane * CPL, j0 = i + lo + R0;
            const uint32_t ulim = nw::valid_limit(j0, R0, W, ql);
            int32_t loc[CPL], glast;
            uint32_t mmbits;
            const int32_t m = nwa::row_min<CPL>(H[s], F[s], nh[s], nf[s], rc, qc[s], j0, R0, ulim, border, c, loc, mmbits, glast);
            const int32_t incl = nw_scan_min(m);
            int32_t excl = __shfl_up(incl, 1, 64), gleft = __shfl_up(glast, 1, 64);
            excl = lane == 0 ? NW_INF : excl;
            excl = excl < carry ? excl : carry;
            gleft = lane == 0 ? gcarry : gleft;
            const uint64_t bits = nwa::row_finish<CPL>(H[s], F[s], nh[s], loc, mmbits, excl, gleft, j0, R0, ulim, border, c);
            if (R0 < W) nwa::store_decisions<CPL>(row, R0, bits);
            if (s + 1 < NS) {
                const int32_t last = __builtin_amdgcn_readlane(incl, 63);
                carry = carry < last ? carry : last;
                gcarry = __builtin_amdgcn_readlane(glast, 63);
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    if (lane != 0) return;
    res[g] = nwa::traceback(rl, ql, lo, W, c, dm, owords + p.ow_off);
}

extern "C" void dhk_nwa(hipStream_t st, int cpl, int ns, const NwPair *pairs, int32_t n, const uint8_t *refs, const uint8_t *qrys,
                        NwaCost c, uint64_t *dm, int64_t dm_words, uint64_t *ow, int64_t ow_words, EpResult *res)
{
    if (n <= 0) return;
    const dim3 grid((uint32_t)n), block(64);
#define NWA_LAUNCH(C, S) \
    hipLaunchKernelGGL((k_nwa<C, S>), grid, block, 0, st, pairs, n, refs, qrys, c, dm, dm_words, ow, ow_words, res)
    if (cpl == 4 && ns == 1)
        NWA_LAUNCH(4, 1);
    else if (cpl == 8 && ns == 1)
        NWA_LAUNCH(8, 1);
    else if (cpl == 16 && ns == 1)
        NWA_LAUNCH(16, 1);
    else if (cpl == 16 && ns == 2)
        NWA_LAUNCH(16, 2);
#undef NWA_LAUNCH
}
