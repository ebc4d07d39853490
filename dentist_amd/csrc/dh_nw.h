// dh_nw.h -- lane code of the global-alignment kernel (dh_nw.hip): Needleman-Wunsch of two whole sequences with unit
// mismatch, indel 1, optional free shift and the traceback rule of findAlignment / tracebackScoringMatrix
// (util/string.d:478-520, 775-831; oracle/nw.c).  One wavefront per pair.  Compiles for the host as well
// (tests/native/nw_host.cpp), so that the CPU tests run the very expressions the kernel runs.
//
// Coordinates.  Matrix cell (i, j), i = reference bases consumed, j = query bases consumed, lies on diagonal j - i.  The
// kernel fills the diagonals [lo, hi] only: band column R of matrix row i is j = i + lo + R, W = hi - lo + 1 columns.  In
// these coordinates the three neighbours of a cell are
//     diagonal (i - 1, j - 1) = column R     of row i - 1
//     up       (i - 1, j)     = column R + 1 of row i - 1
//     left     (i,     j - 1) = column R - 1 of row i
// A lane owns CPL consecutive columns of a strip of 64 * CPL, NS strips side by side, row i - 1 of its cells in registers.
// Of the row above it needs its own cells and ONE more, the first cell of the lane to its right: one lane-crossing value
// per lane, strip and row.  The left neighbour is resolved the way k_edit_general resolves it:
//     F[i][j] = min(G[j], F[i][j - 1] + 1),  G[j] = min(F[i-1][j-1] + mismatch, F[i-1][j] + 1),  G[0] = F[i][0]
//            = R + min over R' <= R of (G(R') - R')
// a running minimum inside the lane (row_min), an inclusive prefix minimum across the wavefront, a wave-uniform carry from
// strip to strip, and a second pass (row_finish) that forms F and the decisions.  Cells outside the matrix (j < 0, j > ql)
// or the band (R >= W) are NW_INF and never win a minimum.
//
// Decisions.  Two bits per cell, and they ARE the op code: 0 match / 3 mismatch (diagonal), 2 insertion (left), 1 deletion
// (up), chosen by the reference's rule -- the neighbour with the smallest score, diagonal before insertion before
// deletion.  The CPL cells of a lane make one 32-bit word; the words of a row are contiguous ([row][word]), so a
// wavefront's store is one contiguous piece.  The traceback is one lane's walk from (rl, ql); it fetches the words of
// PB rows at once (a step stays in its row or moves up one, and R moves by one at most).  At a border the rest is padded
// with deletions, then insertions.  The cost of the walk's ops (without the padding when free_shift) equals F[rl][ql] of
// the banded matrix: moving to the smallest neighbour m costs exactly F - m (if the diagonal is smallest, F = m +
// mismatch; if left or up is strictly smaller than the diagonal, F = m + 1), so the costs telescope down to the border.
//
// When is a banded result the full matrix's result?  Write F for the full matrix, B >= F for the banded one, c for the
// cost of the traced path = B[rl][ql].  Neighbouring cells of F differ by at most 1.
//
//   free_shift == 0: band [min(0, d) - w, max(0, d) + w], d = ql - rl.  Accepted when c + 1 <= w.
//     F[i][j] >= |i - j|, and an optimal path to a cell of score s never leaves |i - j| <= s (every step off a diagonal
//     costs 1, and the path starts on diagonal 0).  So every cell with F <= w lies in the band with all its optimal paths,
//     and by induction along them B = F there.  The corner has F <= B = c < w, hence B = F = c.  Scores do not increase
//     along the walk, so every cell of the path has F <= B <= c and is exact.  A neighbour the tie rule inspects has
//     F <= c + 1 <= w: it lies in the band and is exact as well.  With the same three numbers and the same rule the walk
//     is the reference's walk.
//
//   free_shift != 0: band [d - w, d + w] (a path may start on any diagonal, so the band is centred on the END diagonal d).
//     Border cells inside the band are 0, as in the full matrix.  A cell of score s on diagonal e has an optimal path that
//     starts on the border and stays within e +- s; if those diagonals are in the band, B = F there.  A cell of the walk
//     with score f has been reached with c - f of cost, so it lies within c - f of d; a neighbour lies within c - f + 1 and
//     has F <= f + 1.  Everything the walk inspects is therefore determined by diagonals within (c - f + 1) + (f + 1) = c + 2
//     of d.  The acceptance used is the stricter w >= 2 (c + 1) (cells within c + 1 of the end diagonal with score <= c + 1),
//     which the host replay of tests/test_nw_host.py checks against the full matrix.
//
//   Either mode: the band is clipped to the diagonals of the rectangle, [-rl, ql].  A band that holds all of them is the
//   full matrix and is accepted whatever c is.
//
// The kernel never decides on its own result: it reports (ops, c) and the host applies nw::accepted, doubles w for the
// pairs that fail, and gives up (DH_NW_BAND_EXCEEDED) when the band would be wider than NW_MAX_W columns.
#ifndef DH_NW_H
#define DH_NW_H

#include <stdint.h>
#include <string.h>

#include "dh_editpath.h"

#define NW_INF 0x3fffffff
#define NW_MAX_W 4096      /* widest band: 16 cells per lane, 4 strips */
#define NW_MAX_LEN 65536   /* longest sequence of a pair (include/dentist_hip.h: DH_NW_MAX_LEN) */
#define NW_SEQ_PAD 64      /* bytes in front of and behind the sequences of a launch: the window loads reach CPL bytes past
                              either end of a query, the reference loads 7 bytes past its end */

struct NwPair {             // one pair of a launch
    int64_t roff, qoff;     // first base in the launch's reference / query bytes
    int64_t dm_off, ow_off; // first decision word (32 bits) / first op word (64 bits) of the pair
    int32_t rl, ql;
    int32_t lo, hi;         // the band of diagonals j - i
};

namespace nw {

struct Band {
    int32_t lo, hi;
    bool full;  // every diagonal of the rectangle
};

// the band of half-width w, clipped to the rectangle
EP_HD Band band(int32_t rl, int32_t ql, int64_t w, int32_t free_shift)
{
    const int64_t d = (int64_t)ql - rl;
    int64_t lo = (free_shift ? d : (d < 0 ? d : 0)) - w, hi = (free_shift ? d : (d > 0 ? d : 0)) + w;
    if (lo < -(int64_t)rl) lo = -(int64_t)rl;
    if (hi > ql) hi = ql;
    Band b;
    b.lo = (int32_t)lo;
    b.hi = (int32_t)hi;
    b.full = lo == -(int64_t)rl && hi == ql;
    return b;
}

// the exactness argument above as a predicate: c = cost of the traced path in a band of half-width w
EP_HD bool accepted(int64_t c, int64_t w, int32_t free_shift, bool full)
{
    return full || (free_shift ? 2 * (c + 1) <= w : c + 1 <= w);
}

// which kernel serves a band of W columns: cells per lane and strips; false when none does
EP_HD bool band_class(int32_t W, int32_t &cpl, int32_t &ns)
{
    if (W < 1 || W > NW_MAX_W) return false;
    cpl = W <= 256 ? 4 : (W <= 512 ? 8 : 16);
    ns = W <= 1024 ? 1 : (W <= 2048 ? 2 : 4);
    return true;
}

EP_HD int32_t band_width(int32_t rl, int32_t ql, int64_t w, int32_t free_shift)
{
    const Band b = band(rl, ql, w, free_shift);
    return b.hi - b.lo + 1;
}

// the half-width of the attempt after one at w_prev (0: the first, at w0): twice as much, or the largest whose band the
// widest kernel (max_w columns) still serves; -1 when that is no wider than w_prev
inline int64_t next_w(int32_t rl, int32_t ql, int32_t free_shift, int64_t w_prev, int64_t w0, int32_t max_w = NW_MAX_W)
{
    const int64_t w = w_prev ? 2 * w_prev : w0;
    if (band_width(rl, ql, w, free_shift) <= max_w) return w;
    int64_t a = w_prev, b = w;  // the band of b does not fit
    while (b - a > 1) {
        const int64_t m = (a + b) / 2;
        if (band_width(rl, ql, m, free_shift) <= max_w)
            a = m;
        else
            b = m;
    }
    return a == w_prev ? -1 : a;
}

// query bytes qbase .. qbase + CPL - 1 (0-based) of a lane's cells; windows without a base of the query are not loaded
template <int CPL>
EP_HD void load_window(const uint8_t *qry, int32_t qbase, int32_t ql, uint32_t (&qw)[CPL / 4])
{
    if (qbase > -CPL && qbase < ql) {
        memcpy(qw, qry + qbase, CPL);
    } else {
        for (int k = 0; k < CPL / 4; k++) qw[k] = 0;
    }
}

// which of a lane's cells exist: cell u (column R0 + u, j = j0 + u) iff 0 <= j <= ql and R0 + u < W, as (uint32_t)(j0 + u) <
// the returned limit
EP_HD uint32_t valid_limit(int32_t j0, int32_t R0, int32_t W, int32_t ql)
{
    const int32_t byband = j0 + (W - 1 - R0);
    const int32_t jlim = byband < ql ? byband : ql;
    return jlim < 0 ? 0u : (uint32_t)jlim + 1u;
}

// row 0 of a lane's cells: F[0][j] = j, or 0 with free shift
template <int CPL>
EP_HD void row0(int32_t (&prev)[CPL], int32_t j0, uint32_t ulim, int32_t free_shift)
{
    for (int u = 0; u < CPL; u++) prev[u] = (uint32_t)(j0 + u) < ulim ? (free_shift ? 0 : j0 + u) : NW_INF;
}

// First pass over a lane's cells of row i: loc[u] = min over the lane's cells u' <= u of (G - R), the mismatch bits, and the
// lane's minimum as the return value.  prev: row i - 1 of the lane's cells, nxt: of the cell behind them; rc: reference
// base of the row; qw: load_window of the row; border: F[i][0].
template <int CPL>
EP_HD int32_t row_min(const int32_t (&prev)[CPL], int32_t nxt, uint32_t rc, const uint32_t (&qw)[CPL / 4], int32_t j0, int32_t R0,
                      uint32_t ulim, int32_t border, int32_t (&loc)[CPL], uint32_t &mmbits)
{
    int32_t m = NW_INF;
    uint32_t mb = 0;
#pragma unroll
    for (int u = 0; u < CPL; u++) {
        const int32_t up = u + 1 < CPL ? prev[u + 1] : nxt;
        const uint32_t mm = ((qw[u >> 2] >> (8 * (u & 3))) & 0xFFu) != rc ? 1u : 0u;
        const int32_t x = prev[u] + (int32_t)mm, y = up + 1;
        int32_t g = x < y ? x : y;
        g = j0 + u == 0 ? border : g;
        g = (uint32_t)(j0 + u) < ulim ? g : NW_INF;
        const int32_t t = g - (R0 + u);
        m = m < t ? m : t;
        loc[u] = m;
        mb |= mm << u;
    }
    mmbits = mb;
    return m;
}

// Second pass: F of the lane's cells into prev, the decision word as the return value.  excl: the minimum of (G - R) over
// every cell of the row in front of the lane's (NW_INF when there is none).
template <int CPL>
EP_HD uint32_t row_finish(int32_t (&prev)[CPL], int32_t nxt, const int32_t (&loc)[CPL], uint32_t mmbits, int32_t excl, int32_t j0,
                          int32_t R0, uint32_t ulim)
{
    int32_t left = excl + (R0 - 1);
    left = left < NW_INF ? left : NW_INF;
    uint32_t acc = 0;
#pragma unroll
    for (int u = 0; u < CPL; u++) {
        const int32_t dg = prev[u], up = u + 1 < CPL ? prev[u + 1] : nxt;
        int32_t f = (excl < loc[u] ? excl : loc[u]) + (R0 + u);
        f = f < NW_INF ? f : NW_INF;
        f = (uint32_t)(j0 + u) < ulim ? f : NW_INF;
        const uint32_t sub = ((mmbits >> u) & 1u) ? (uint32_t)EP_OP_MISMATCH : (uint32_t)EP_OP_MATCH;
        const uint32_t op = (dg <= left && dg <= up) ? sub : (left <= up ? (uint32_t)EP_OP_INS : (uint32_t)EP_OP_DEL);
        acc |= op << (2 * u);
        prev[u] = f;
        left = f;
    }
    return acc;
}

// decision words of a row are contiguous; a pair's rows follow each other
template <int CPL>
EP_HD int32_t row_words(int32_t W) { return (W + CPL - 1) / CPL; }

// Traceback over the decision words of a pair: from (rl, ql) along the stored ops to a border, then deletions, then
// insertions.  Ops go out back to front, eight per 64-bit word (ep::OpWriter, stride 1).  Returns the number of ops and the
// cost of the path (without the padding when free_shift); EP_REJECTED is set when the walk left the band.
template <int CPL>
EP_HD EpResult traceback(int32_t rl, int32_t ql, int32_t lo, int32_t W, int32_t free_shift, const uint32_t *dm, uint64_t *ow)
{
    constexpr int PB = CPL >= 8 ? 8 : 4;  // rows fetched together; R grows by PB - 1 < CPL at most on the way up
    const int64_t stride = row_words<CPL>(W);
    ep::OpWriter w(ow, 1);
    int32_t i = rl, j = ql;
    uint32_t cost = 0, bad = 0;
    while (i > 0 && j > 0 && !bad) {
        const int32_t i0 = i, Rs = j - i - lo;
        if ((uint32_t)Rs >= (uint32_t)W) {
            bad = 1;
            break;
        }
        const int32_t kc = Rs / CPL;
        uint32_t w0[PB], w1[PB];
#pragma unroll
        for (int u = 0; u < PB; u++) {
            const bool in = i0 - u > 0;
            const int64_t base = (int64_t)(i0 - u - 1) * stride;
            w0[u] = in ? dm[base + kc] : 0u;
            w1[u] = (in && kc + 1 < stride) ? dm[base + kc + 1] : 0u;
        }
#pragma unroll
        for (int u = 0; u < PB; u++) {
            while (i == i0 - u && i > 0 && j > 0) {
                const int32_t R = j - i - lo;
                if ((uint32_t)R >= (uint32_t)W) {
                    bad = 1;
                    i = -1;  // leaves every loop
                    break;
                }
                const int32_t k = R / CPL;
                const uint32_t word = k == kc ? w0[u] : (k == kc + 1 ? w1[u] : dm[(int64_t)(i - 1) * stride + k]);
                const uint32_t op = (word >> (2 * (R % CPL))) & 3u;
                w.put(op);
                if (op == EP_OP_MATCH || op == EP_OP_MISMATCH) {
                    cost += op == EP_OP_MISMATCH;
                    --i;
                    --j;
                } else if (op == EP_OP_INS) {
                    cost++;
                    --j;
                } else {
                    cost++;
                    --i;
                }
            }
        }
    }
    const uint32_t pad = free_shift ? 0u : 1u;
    while (i > 0) {
        w.put(EP_OP_DEL);
        cost += pad;
        --i;
    }
    while (j > 0 && !bad) {
        w.put(EP_OP_INS);
        cost += pad;
        --j;
    }
    w.flush();
    EpResult r;
    r.nops = w.nops | (bad ? EP_REJECTED : 0u);
    r.score = cost;
    return r;
}

}  // namespace nw

#if defined(__HIPCC__)
// inclusive prefix minimum over the 64 lanes: row_shr 1, 2, 4, 8 inside the rows of 16, then row_bcast:15 / row_bcast:31
// (the sequence of ep_scan_add); a lane without a source keeps its own value.  Shared by k_nw and k_nwa.
template <int CTRL, int ROWMASK>
__device__ __forceinline__ int32_t nw_dpp_min(int32_t v)
{
    const int32_t o = __builtin_amdgcn_update_dpp(v, v, CTRL, ROWMASK, 0xF, false);
    return v < o ? v : o;
}
__device__ __forceinline__ int32_t nw_scan_min(int32_t v)
{
    v = nw_dpp_min<0x111, 0xF>(v);
    v = nw_dpp_min<0x112, 0xF>(v);
    v = nw_dpp_min<0x114, 0xF>(v);
    v = nw_dpp_min<0x118, 0xF>(v);
    v = nw_dpp_min<0x142, 0xA>(v);
    v = nw_dpp_min<0x143, 0xC>(v);
    return v;
}
#endif

#endif
