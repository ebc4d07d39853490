// dh_editpath.hip -- base-level alignments from trace points (getExactAlignment's per-trace-point part,
// dazzler.d:2405-2426): the edit path of every trace tile of a local alignment.  gfx950, wave64.
//
//   k_edit_fast<NW>   one tile per lane: bit-parallel banded fill + traceback (dh_editpath.h), band = trace diffs + 1 at
//                     most 31 (NW = 1) or 63 (NW = 2).  The result carries EP_REJECTED unless the cost of the path proves
//                     the band wide enough; the host sends such tiles to
//   k_edit_general    one wavefront per tile, full matrix: a matrix row per step, 16 columns per lane, the dependency on the
//                     left neighbour resolved by a prefix minimum over the wavefront.  Any rl <= 250, ql <= 1000.
//   k_edit_compact    the op words of a chunk's tiles (back to front, eight per word) to their place in the chunk's output,
//                     front to back, one byte per op.
//
// Where the decision words live: three planes of 64 NW bits per matrix row are up to 6 (NW = 1) / 12 KB (NW = 2) per tile
// at tspace = 250.  In LDS that is 384 / 768 KB per wavefront of 64 tiles against 160 KB per CU -- even at tspace = 100 a
// CU would hold one wavefront (154 KB) or none, and the fill is VALU-bound with nothing but other wavefronts to hide
// its store and load latencies behind.  They therefore live in global memory, interleaved over the launch
// ([row][plane][word][tile]): a wavefront's store of one word is one contiguous 512-byte piece, the kernel uses no LDS
// at all and its occupancy is set by registers alone.  The traceback reads the words of 8 / 4 rows at once, since one at a
// time the walk is a chain of dependent misses (measured on k_seg_vote_bp, round 6).  The footprint is bounded by the
// chunk of tiles the host hands to a launch (DH_EDIT_CHUNK), not by the call.
#include <hip/hip_runtime.h>

#include "dh_editpath.h"

template <int NW>
__global__ void __launch_bounds__(64)
k_edit_fast(const EpTile *__restrict__ tiles, int32_t n, const uint8_t *__restrict__ abases,
            const uint8_t *__restrict__ bfwd, const uint8_t *__restrict__ brc, int32_t rows, int32_t owords,
            uint64_t *__restrict__ dm, uint64_t *__restrict__ ow, EpResult *__restrict__ res)
{
    const int32_t t = blockIdx.x * 64 + threadIdx.x;
    if (t >= n) return;
    const EpTile tl = tiles[t];
    const int32_t d = tl.rl > tl.ql ? tl.rl - tl.ql : tl.ql - tl.rl;
    // (the host planned the buffers from these very numbers: the test keeps a wrong plan from becoming a wild store)
    if (tl.rl < 0 || tl.ql < 0 || tl.rl > rows || d >= 32 * NW || ((tl.rl + tl.ql + 7) >> 3) > owords) {
        res[t] = EpResult{EP_REJECTED, 0u};
        return;
    }
    const uint8_t *ref = abases + tl.aoff;
    const uint8_t *qry = (tl.comp ? brc : bfwd) + tl.boff;
    ep::fill<NW>(ref, tl.rl, qry, tl.ql, dm + t, (int64_t)n);
    EpResult r = ep::traceback<NW>(tl.rl, tl.ql, dm + t, (int64_t)n, ow + t, (int64_t)n);
    if ((int64_t)r.score > (int64_t)tl.diffs) r.nops |= EP_REJECTED;
    res[t] = r;
}

#define EP_GEN_W (64 * EP_GEN_COLS)

__global__ void __launch_bounds__(64)
k_edit_general(const EpTile *__restrict__ tiles, int32_t n, const uint8_t *__restrict__ abases,
               const uint8_t *__restrict__ bfwd, const uint8_t *__restrict__ brc, int32_t rows,
               uint32_t *__restrict__ dmat, const int64_t *__restrict__ ow_off, uint64_t *__restrict__ ow,
               EpResult *__restrict__ res)
{
    __shared__ int32_t s_row[2][EP_GEN_W + 1];
    __shared__ uint8_t s_q[EP_GEN_W];
    const int32_t g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    const EpTile tl = tiles[g];
    const int32_t rl = tl.rl, ql = tl.ql;
    if (rl < 0 || ql < 0 || rl > rows || ql > EP_GEN_W) {
        if (lane == 0) res[g] = EpResult{EP_REJECTED, 0u};
        return;
    }
    const uint8_t *ref = abases + tl.aoff;
    const uint8_t *qry = (tl.comp ? brc : bfwd) + tl.boff;
    for (int32_t j = lane; j < EP_GEN_W; j += 64) s_q[j] = j < ql ? qry[j] : (uint8_t)0xFF;
    for (int32_t j = lane; j <= EP_GEN_W; j += 64) s_row[0][j] = j;  // F[0][j] = j
    __syncthreads();
    // decisions: 2 bits per cell (0 diagonal, 2 insertion, 1 deletion), the 16 cells of a lane in one word, [row][lane]
    uint32_t *dm = dmat + (int64_t)g * rows * 64;
    const int32_t j0 = 1 + lane * EP_GEN_COLS;
    const bool active = j0 <= ql;
    for (int32_t i = 1; i <= rl; i++) {
        const int32_t *prev = s_row[(i - 1) & 1];
        int32_t *cur = s_row[i & 1];
        const uint32_t rc = ref[i - 1];
        // F[i][j] = min(G[j], F[i][j-1] + 1) with G[j] = min(F[i-1][j-1] + mismatch, F[i-1][j] + 1), G[0] = i, unrolled:
        // F[i][j] = j + min over k <= j of (G[k] - k) -- a running minimum inside the lane, a prefix minimum across lanes
        int32_t loc[EP_GEN_COLS], dg[EP_GEN_COLS], up[EP_GEN_COLS];
        int32_t m = 0x3fffffff;
        if (active) {
            int32_t pd = prev[j0 - 1];
#pragma unroll
            for (int u = 0; u < EP_GEN_COLS; u++) {
                const int32_t j = j0 + u;
                const int32_t a = prev[j];
                const int32_t x = pd + (rc == (uint32_t)s_q[j - 1] ? 0 : 1);
                const int32_t gv = x < a + 1 ? x : a + 1;
                m = m < gv - j ? m : gv - j;
                loc[u] = m;
                dg[u] = pd;
                up[u] = a;
                pd = a;
            }
        }
        int32_t incl = m;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) {
            const int32_t o = __shfl_up(incl, s, 64);
            if (lane >= s) incl = incl < o ? incl : o;
        }
        int32_t excl = __shfl_up(incl, 1, 64);
        excl = (lane == 0 || excl > i) ? i : excl;  // G[0] - 0 = i
        if (active) {
            int32_t left = excl + (j0 - 1);  // F[i][j0 - 1]
            uint32_t acc = 0;
#pragma unroll
            for (int u = 0; u < EP_GEN_COLS; u++) {
                const int32_t j = j0 + u;
                const int32_t f = (excl < loc[u] ? excl : loc[u]) + j;
                const uint32_t op = (dg[u] <= left && dg[u] <= up[u]) ? 0u : (left <= up[u] ? 2u : 1u);
                acc |= op << (2 * u);
                cur[j] = f;
                left = f;
            }
            dm[(int64_t)(i - 1) * 64 + lane] = acc;
        }
        if (lane == 0) cur[0] = i;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    if (lane != 0) return;
    ep::OpWriter w(ow + ow_off[g], 1);
    int32_t i = rl, j = ql;
    uint32_t cost = 0;
    while (i > 0 && j > 0) {
        const uint32_t word = dm[(int64_t)(i - 1) * 64 + ((j - 1) >> 4)];
        const uint32_t op = (word >> (2 * ((j - 1) & 15))) & 3u;
        if (op == 0) {
            const uint32_t mm = (uint32_t)ref[i - 1] == (uint32_t)s_q[j - 1] ? 0u : 1u;
            w.put(mm ? EP_OP_MISMATCH : EP_OP_MATCH);
            cost += mm;
            --i;
            --j;
        } else if (op == 2) {
            w.put(EP_OP_INS);
            cost++;
            --j;
        } else {
            w.put(EP_OP_DEL);
            cost++;
            --i;
        }
    }
    while (i > 0) {
        w.put(EP_OP_DEL);
        cost++;
        --i;
    }
    while (j > 0) {
        w.put(EP_OP_INS);
        cost++;
        --j;
    }
    w.flush();
    res[g] = EpResult{w.nops, cost};
}

__global__ void __launch_bounds__(64)
k_edit_compact(const EpCopy *__restrict__ cp, int32_t n, const uint64_t *__restrict__ ow_fast,
               const uint64_t *__restrict__ ow_general, uint8_t *__restrict__ out)
{
    const int32_t g = blockIdx.x;
    if (g >= n) return;
    const EpCopy c = cp[g];
    const uint64_t *ow = c.general ? ow_general : ow_fast;
    for (int32_t p = threadIdx.x; p < c.nops; p += 64) {
        const int32_t q = c.nops - 1 - p;  // op number counted from the end of the path
        const uint64_t wv = ow[c.wbase + (int64_t)(q >> 3) * c.wstride];
        out[c.out + p] = (uint8_t)(wv >> (8 * (q & 7)));
    }
}

extern "C" void dhk_edit_fast(hipStream_t st, int nw, const EpTile *tiles, int32_t n, const uint8_t *abases,
                              const uint8_t *bfwd, const uint8_t *brc, int32_t rows, int32_t owords, uint64_t *dm,
                              uint64_t *ow, EpResult *res)
{
    if (n <= 0) return;
    const dim3 grid((uint32_t)((n + 63) / 64)), block(64);
    if (nw == 1)
        hipLaunchKernelGGL(k_edit_fast<1>, grid, block, 0, st, tiles, n, abases, bfwd, brc, rows, owords, dm, ow, res);
    else
        hipLaunchKernelGGL(k_edit_fast<2>, grid, block, 0, st, tiles, n, abases, bfwd, brc, rows, owords, dm, ow, res);
}

extern "C" void dhk_edit_general(hipStream_t st, const EpTile *tiles, int32_t n, const uint8_t *abases, const uint8_t *bfwd,
                                 const uint8_t *brc, int32_t rows, uint32_t *dmat, const int64_t *ow_off, uint64_t *ow,
                                 EpResult *res)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_edit_general, dim3((uint32_t)n), dim3(64), 0, st, tiles, n, abases, bfwd, brc, rows, dmat, ow_off, ow,
                       res);
}

extern "C" void dhk_edit_compact(hipStream_t st, const EpCopy *cp, int32_t n, const uint64_t *ow_fast, const uint64_t *ow_general,
                                 uint8_t *out)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_edit_compact, dim3((uint32_t)n), dim3(64), 0, st, cp, n, ow_fast, ow_general, out);
}
