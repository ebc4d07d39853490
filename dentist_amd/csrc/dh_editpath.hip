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
//   k_trace_transpose one wavefront per record: from those ops, the running (diffs, bases) at every trace point of the
//                     TRANSPOSED record, whose grid lies on the B read (dh_la_transpose); k_trace_pairs turns them into the
//                     trace pairs.  The ops never leave the device.
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

// inclusive sum over the 64 lanes: row_shr 1, 2, 4, 8 inside the rows of 16, then row_bcast:15 / row_bcast:31 (the
// sequence dh_mjoin.hip's scans use)
template <int CTRL, int ROWMASK>
__device__ __forceinline__ uint32_t ep_dpp0(uint32_t v)
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, ROWMASK, 0xF, false);
}
__device__ __forceinline__ uint32_t ep_scan_add(uint32_t v)
{
    v += ep_dpp0<0x111, 0xF>(v);
    v += ep_dpp0<0x112, 0xF>(v);
    v += ep_dpp0<0x114, 0xF>(v);
    v += ep_dpp0<0x118, 0xF>(v);
    v += ep_dpp0<0x142, 0xA>(v);
    v += ep_dpp0<0x143, 0xC>(v);
    return v;
}

// One wavefront per record, passes of 64 lanes x 64 ops of the transposed path (dh_editpath.h: tr_word).  A lane counts
// what its 64 ops advance, a scan over the wavefront and the wave-uniform carry of the passes before give the position at
// the start of its slice, and the lane walks its ops only when a grid point of A' lies inside: at the op that reaches
// grid point m it stores the running (diffs, B' bases) to bound[m - 1], i.e. the END of tile m - 1.  The op that reaches
// a grid point is unique, so every slot has one writer; the last slot takes the totals.  status: 2 when the ops do not
// advance A' by a1 - a0 (the host planned the tiles from that interval).
__global__ void __launch_bounds__(64)
k_trace_transpose(const EpTrRec *__restrict__ recs, int32_t n, const uint8_t *__restrict__ ops, int32_t ts,
                  uint2 *__restrict__ bound, int32_t *__restrict__ status)
{
    const int32_t g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    const EpTrRec r = recs[g];
    const uint8_t *o = ops + r.op0;
    const int32_t ntiles = ep::tr_tiles(r.a0, r.a1, ts), g0 = r.a0 / ts;
    uint2 *bd = bound + r.slot0;
    uint32_t ca = 0, cb = 0, cd = 0;  // what the passes before advanced: wave-uniform
    for (int32_t p0 = 0; p0 < r.nops; p0 += EP_TR_PASS_OPS) {
        const int32_t k0 = p0 + lane * EP_TR_LANE_OPS;
        uint64_t w[8];
        uint32_t sa = 0, sb = 0, sd = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            w[j] = k0 + 8 * j < r.nops ? ep::tr_word(o, r.nops, r.comp, k0 + 8 * j) : 0x0404040404040404ull;
            ep::tr_count(w[j], sa, sb, sd);
        }
        const uint32_t iab = ep_scan_add(sa | (sb << 16));  // (a pass advances either sequence by 4096 at most)
        const uint32_t id = ep_scan_add(sd);
        const int32_t pos = r.a0 + (int32_t)(ca + (iab & 0xFFFFu) - sa), next = (pos / ts + 1) * ts;
        if (next <= pos + (int32_t)sa && next < r.a1)
            ep::tr_walk(w, pos, ts, cb + (iab >> 16) - sb, cd + id - sd, [&](int32_t gp, uint32_t d, uint32_t b) {
                const int32_t m = gp / ts - g0 - 1;
                if (gp < r.a1 && m >= 0 && m < ntiles - 1) bd[m] = make_uint2(d, b);
            });
        const uint32_t tab = (uint32_t)__builtin_amdgcn_readlane((int)iab, 63);
        ca += tab & 0xFFFFu;
        cb += tab >> 16;
        cd += (uint32_t)__builtin_amdgcn_readlane((int)id, 63);
    }
    if (lane == 0) {
        if (ntiles > 0) bd[ntiles - 1] = make_uint2(cd, cb);
        status[g] = (int64_t)ca == (int64_t)r.a1 - r.a0 ? 0 : 2;
    }
}

// pair m of a record = bound[m] - bound[m - 1], (diffs, B' bases) as two u16 in one 32-bit store: consecutive lanes write
// consecutive words.  status |= 1 when a value does not fit.
__global__ void __launch_bounds__(64)
k_trace_pairs(const EpTrRec *__restrict__ recs, int32_t n, int32_t ts, const uint2 *__restrict__ bound,
              uint32_t *__restrict__ pairs, int32_t *__restrict__ status)
{
    const int32_t g = blockIdx.x, lane = threadIdx.x;
    if (g >= n) return;
    const EpTrRec r = recs[g];
    const int32_t ntiles = ep::tr_tiles(r.a0, r.a1, ts);
    const uint2 *bd = bound + r.slot0;
    bool over = false;
    for (int32_t m = lane; m < ntiles; m += 64) {
        const uint2 e = bd[m], s = m ? bd[m - 1] : make_uint2(0u, 0u);
        const uint32_t d = e.x - s.x, b = e.y - s.y;
        over |= d > 0xFFFFu || b > 0xFFFFu;
        pairs[r.slot0 + m] = (d & 0xFFFFu) | (b << 16);
    }
    const bool any = __any(over);
    if (lane == 0 && any) status[g] |= 1;
}

extern "C" void dhk_trace_transpose(hipStream_t st, const EpTrRec *recs, int32_t n, const uint8_t *ops, int32_t ts, uint2 *bound,
                                    uint32_t *pairs, int32_t *status)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_trace_transpose, dim3((uint32_t)n), dim3(64), 0, st, recs, n, ops, ts, bound, status);
    hipLaunchKernelGGL(k_trace_pairs, dim3((uint32_t)n), dim3(64), 0, st, recs, n, ts, bound, pairs, status);
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
