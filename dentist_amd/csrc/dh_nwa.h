// dh_nwa.h -- lane code of the affine-gap global-alignment kernel (dh_nwa.hip): Gotoh's three-state recurrence on the
// diagonal band of dh_nw.h, one wavefront per pair.  Compiles for the host as well (tests/native/nwa_host.cpp), so that the
// CPU tests run the very expressions the kernel runs.
//
// Costs.  A scoring {match, mismatch, gap_open, gap_extend} (a gap of k bases scores -(gap_open + k gap_extend), end gaps
// included) is minimised as
//     cm = 2 (match - mismatch)   an unequal pair          ce = 2 gap_extend + match   every base of a gap
//     co = 2 gap_open             once per gap             0                           an equal pair
// An alignment with x equal pairs, y unequal pairs and gaps g_1 .. g_n has rl + ql = 2 (x + y) + sum g, hence
//     2 score = match (rl + ql) - cost,
// and the alignment of smallest cost is the one of largest score.  nwa::costs refuses cm < 0, ce <= 0, co < 0 and values
// with which any number the kernel forms could reach NW_INF / 2.
//
// Recurrence, in the coordinates of dh_nw.h (band column R of row i is j = i + lo + R; diagonal = column R of row i - 1, up =
// column R + 1 of row i - 1, left = column R - 1 of row i).  Three states per cell: E ends in an insertion, F in a deletion,
//     F[i][R] = min(H[i-1][R+1] + co + ce, F[i-1][R+1] + ce)
//     G[R]    = min(H[i-1][R] + sub, F[R])
//     E[R]    = ce R + co + min over R' < R of (G[R'] - ce R')
//     H[R]    = min(G[R], E[R])
// with H[0][j] = co + ce j, H[i][0] = F[i][0] = co + ce i, H[0][0] = 0.  E[j] = min over j' < j of H[j'] + co + ce (j - j'); a
// term whose H[j'] is E[j'] itself is never smaller than the term that extends the same gap (co >= 0), so G stands in for
// H.  A lane keeps rows i - 1 of H and of F of its CPL cells in registers and needs TWO values of the lane to its right
// (H and F of its first cell).  The running minimum in the lane (row_min), the inclusive prefix minimum over the wavefront,
// the wave-uniform carry between strips and the second pass (row_finish) are those of k_nw; the minimum is exclusive here
// (R' < R).  Cells outside the matrix or the band are NW_INF.  Every valid cell is finite: its diagonal reaches a border
// cell inside the band.
//
// Decisions.  Four bits per cell: bits 0-1 the source of H, which IS the op code (0 match / 3 mismatch: diagonal; 2: E;
// 1: F), chosen among the sources that attain H in the reference's order -- diagonal, then E, then F -- with one clause
// more: where the diagonal ties with a gap state it is taken only if sub >= ce.  findAlignment moves to the neighbour of
// the smallest SCORE (diagonal, insertion, deletion on equal scores), not to the first source that attains the cell's
// value: for a / aa its last op is the insertion, because F[1][1] = 0 < F[0][1] = 1, although the diagonal attains
// F[1][2] = 1 as well.  The predecessor of the diagonal has value H - sub, the state before the last base of a gap that
// attains H has H - ce, so "the smaller predecessor, the diagonal on a tie" is "sub >= ce"; with {0, -1, 0, 1} (cm = ce = 2,
// co = 0) this is findAlignment's rule op for op, which plain "diagonal first" is not.  Bit 2: E of
// the cell extends E of its left neighbour (clear: the gap opens there, H[i][j-1] + co + ce == E[i][j]; opening wins a
// tie); bit 3: the same for F and the cell above.  Bit 2 needs G of the cell to the left, a third lane-crossing value:
//     H[j-1] + co + ce == E[j]   <=>   co == 0  or  G[j-1] + co + ce == E[j]
// (if E[j-1] < G[j-1], H[j-1] + co + ce = E[j-1] + co + ce equals E[j] = E[j-1] + ce only for co = 0, and G[j-1] + co + ce
// is larger than E[j]).  Sixteen cells make one 64-bit word, the words of a row are contiguous ([row][word]).
//
// Traceback: one lane's walk from (rl, ql) in state H.  In H a diagonal op is emitted and the walk moves to (i-1, j-1); ops 2
// and 1 switch to state E / F at the same cell.  In E an insertion is emitted, the walk moves to (i, j-1) and returns to H
// unless bit 2 of the cell it left is set; F likewise, one row up, with bit 3.  At a border the rest is padded with
// deletions, then insertions.  The cost of the walk (cm per mismatch, ce per gap base, co per gap, co + ce k for a padding
// of k) telescopes to H[rl][ql] of the banded matrix.
//
// When is a banded result the full matrix's result?  The band is [min(0, d) - w, max(0, d) + w], d = ql - rl, clipped to the
// rectangle; it holds every diagonal of |j - i| <= w.  Write T for the true value of a state (H, E or F of a cell), B >= T
// for the banded one, c for the cost of the traced path = B(H[rl][ql]).  Accepted when c <= ce w (or the band is full).
//   * A path that touches diagonal e holds |e| gap bases at least, ce each.  So every optimal path of a state with
//     T <= ce w stays within |j - i| <= w, inside the band, and so do its prefixes, which are optimal paths of their states
//     with no larger T.  By induction along them B = T for every state with T <= ce w.
//   * The corner has T <= B = c <= ce w, so B = T.  Values do not increase along the walk backwards, so every state the
//     walk is in has T <= B <= c and is exact.
//   * In a state of value v the rule asks which candidates (diagonal + sub, E, F; H + co + ce of the neighbour) equal v.  A
//     candidate whose banded value is v has a true value <= v, and v is the minimum of the true values: it is v.  A candidate
//     whose true value is v <= ce w is exact in the band (its state has T <= v) and has banded value v; a candidate outside
//     the band cannot have true value v.  The banded walk therefore answers every question as the full matrix does.
// No stricter predicate is needed; the host replay of tests/test_nwa_host.py checks this one against the full matrix.
//
// The kernel never decides on its own result: it reports (ops, c), the host applies nwa::accepted, doubles w for the pairs
// that fail and gives up (DH_NW_BAND_EXCEEDED) when the band would be wider than NWA_MAX_W columns.
#ifndef DH_NWA_H
#define DH_NWA_H

#include "dh_nw.h"

#define NWA_MAX_W 2048     /* widest band: 16 cells per lane, 2 strips (include/dentist_hip.h: DH_NWA_MAX_BAND) */
#define NWA_MAX_LEN 65536  /* longest sequence of a pair (DH_NWA_MAX_LEN) */
#define NWA_EXT_E 4u       /* decision bit 2 */
#define NWA_EXT_F 8u       /* decision bit 3 */

struct NwaCost {
    int32_t cm, ce, co;  // mismatch, gap base, gap open
    int32_t match;
};

namespace nwa {

// the cost form of a scoring; false when the host has to refuse it
inline bool costs(int32_t match, int32_t mismatch, int32_t gap_open, int32_t gap_extend, NwaCost &c)
{
    const int64_t cm = 2 * ((int64_t)match - mismatch), ce = 2 * (int64_t)gap_extend + match, co = 2 * (int64_t)gap_open;
    if (cm < 0 || ce <= 0 || co < 0) return false;
    // the largest number formed: a border or worst path (2 co + ce (rl + ql)) plus one step (co + ce, cm), and ce R
    const int64_t worst = 4 * co + ce * (2 * (int64_t)NWA_MAX_LEN + NWA_MAX_W + 2) + cm;
    const int64_t am = match < 0 ? -(int64_t)match : match;
    if (worst >= NW_INF / 2 || am * 2 * NWA_MAX_LEN >= NW_INF / 2) return false;
    c.cm = (int32_t)cm;
    c.ce = (int32_t)ce;
    c.co = (int32_t)co;
    c.match = match;
    return true;
}

// the alignment score of a path of cost `cost`
inline int32_t score_of(const NwaCost &c, int64_t rl, int64_t ql, int64_t cost)
{
    return (int32_t)(((int64_t)c.match * (rl + ql) - cost) / 2);
}

// cost of a pair with an empty side: one gap
inline int64_t gap_cost(const NwaCost &c, int64_t k) { return k > 0 ? (int64_t)c.co + (int64_t)c.ce * k : 0; }

// the exactness argument above as a predicate
EP_HD bool accepted(int64_t c, int64_t w, int32_t ce, bool full) { return full || c <= (int64_t)ce * w; }

// which kernel serves a band of W columns
EP_HD bool band_class(int32_t W, int32_t &cpl, int32_t &ns)
{
    if (W < 1 || W > NWA_MAX_W) return false;
    cpl = W <= 256 ? 4 : (W <= 512 ? 8 : 16);
    ns = W <= 1024 ? 1 : 2;
    return true;
}

inline int64_t next_w(int32_t rl, int32_t ql, int64_t w_prev, int64_t w0) { return nw::next_w(rl, ql, 0, w_prev, w0, NWA_MAX_W); }

// 64-bit decision words of a row: sixteen cells each
EP_HD int32_t row_words(int32_t W) { return (W + 15) / 16; }

// row 0 of a lane's cells: H[0][j] = co + ce j, H[0][0] = 0; F has no value there
template <int CPL>
EP_HD void row0(int32_t (&h)[CPL], int32_t (&f)[CPL], int32_t j0, uint32_t ulim, const NwaCost &c)
{
    for (int u = 0; u < CPL; u++) {
        const int32_t j = j0 + u;
        h[u] = (uint32_t)j < ulim ? (j == 0 ? 0 : c.co + c.ce * j) : NW_INF;
        f[u] = NW_INF;
    }
}

// First pass over a lane's cells of row i: F of the row into f, loc[u] = min over the lane's cells u' <= u of (G - ce R),
// the mismatch bits; returns the lane's minimum.  h, f: rows i - 1 of the lane's cells; nh, nf: of the cell behind them;
// border: H[i][0]; glast: G of the lane's last cell (NW_INF when it does not exist).
template <int CPL>
EP_HD int32_t row_min(const int32_t (&h)[CPL], int32_t (&f)[CPL], int32_t nh, int32_t nf, uint32_t rc, const uint32_t (&qw)[CPL / 4],
                      int32_t j0, int32_t R0, uint32_t ulim, int32_t border, const NwaCost &c, int32_t (&loc)[CPL], uint32_t &mmbits,
                      int32_t &glast)
{
    int32_t m = NW_INF, g = NW_INF;
    uint32_t mb = 0;
#pragma unroll
    for (int u = 0; u < CPL; u++) {
        const int32_t hup = u + 1 < CPL ? h[u + 1] : nh, fup = u + 1 < CPL ? f[u + 1] : nf;
        const uint32_t mm = ((qw[u >> 2] >> (8 * (u & 3))) & 0xFFu) != rc ? 1u : 0u;
        const int32_t x = hup + c.co + c.ce, y = fup + c.ce;
        int32_t fn = x < y ? x : y;
        fn = fn < NW_INF ? fn : NW_INF;
        const int32_t sub = h[u] + (mm ? c.cm : 0);
        g = sub < fn ? sub : fn;
        g = g < NW_INF ? g : NW_INF;
        const bool valid = (uint32_t)(j0 + u) < ulim;
        if (j0 + u == 0) g = fn = border;
        if (!valid) g = fn = NW_INF;
        const int32_t t = valid ? g - c.ce * (R0 + u) : NW_INF;
        m = m < t ? m : t;
        loc[u] = m;
        f[u] = fn;
        mb |= mm << u;
    }
    mmbits = mb;
    glast = g;
    return m;
}

// Second pass: H of the lane's cells into h, the decisions (four bits per cell) as the return value.  f: F of the row
// (row_min); excl: the minimum of (G - ce R) over every cell of the row in front of the lane's (NW_INF: none); gleft: G of the
// cell in front of the lane's first.
template <int CPL>
EP_HD uint64_t row_finish(int32_t (&h)[CPL], const int32_t (&f)[CPL], int32_t nh, const int32_t (&loc)[CPL], uint32_t mmbits,
                          int32_t excl, int32_t gleft, int32_t j0, int32_t R0, uint32_t ulim, int32_t border, const NwaCost &c)
{
    uint64_t acc = 0;
    const int32_t open = c.co + c.ce;
#pragma unroll
    for (int u = 0; u < CPL; u++) {
        const int32_t hup = u + 1 < CPL ? h[u + 1] : nh;
        const uint32_t mm = (mmbits >> u) & 1u;
        const int32_t sub = h[u] + (mm ? c.cm : 0), fn = f[u];
        int32_t g = sub < fn ? sub : fn;
        g = g < NW_INF ? g : NW_INF;
        const int32_t pm = u == 0 ? excl : (excl < loc[u - 1] ? excl : loc[u - 1]);
        int32_t e = pm + c.ce * (R0 + u) + c.co;
        e = (pm < NW_INF && e < NW_INF) ? e : NW_INF;
        int32_t hn = g < e ? g : e;
        const bool valid = (uint32_t)(j0 + u) < ulim;
        if (j0 + u == 0) hn = g = border;
        if (!valid) hn = g = NW_INF;
        const uint32_t dgop = mm ? (uint32_t)EP_OP_MISMATCH : (uint32_t)EP_OP_MATCH;
        const bool dg = (sub < e && sub < fn) || (sub <= e && sub <= fn && mm && c.cm >= c.ce);
        uint32_t d = dg ? dgop : (e <= fn ? (uint32_t)EP_OP_INS : (uint32_t)EP_OP_DEL);
        d |= (c.co == 0 || gleft + open == e) ? 0u : NWA_EXT_E;
        d |= (hup + open == fn) ? 0u : NWA_EXT_F;
        acc |= (uint64_t)d << (4 * u);
        h[u] = hn;
        gleft = g;
    }
    return acc;
}

// the CPL / 2 bytes of a lane's decisions into the row's words (row: the first 64-bit word of the row)
template <int CPL>
EP_HD void store_decisions(uint64_t *row, int32_t R0, uint64_t bits)
{
    if (CPL == 16) {
        row[R0 / 16] = bits;
    } else if (CPL == 8) {
        const uint32_t v = (uint32_t)bits;
        memcpy(__builtin_assume_aligned((uint8_t *)row + R0 / 2, 4), &v, 4);
    } else {
        const uint16_t v = (uint16_t)bits;
        memcpy(__builtin_assume_aligned((uint8_t *)row + R0 / 2, 2), &v, 2);
    }
}

// Traceback over the decision words of a pair (see above).  Ops go out back to front, eight per 64-bit word (ep::OpWriter,
// stride 1).  Returns the number of ops and the cost of the path; EP_REJECTED is set when the walk left the band.
EP_HD EpResult traceback(int32_t rl, int32_t ql, int32_t lo, int32_t W, const NwaCost &c, const uint64_t *dm, uint64_t *ow)
{
    constexpr int PB = 8;  // rows fetched together; R grows by PB - 1 < 16 at most on the way up
    const int64_t stride = row_words(W);
    ep::OpWriter w(ow, 1);
    int32_t i = rl, j = ql;
    uint32_t cost = 0, bad = 0, state = 0;  // 0: H, EP_OP_INS: E, EP_OP_DEL: F
    while (i > 0 && j > 0 && !bad) {
        const int32_t i0 = i, Rs = j - i - lo;
        if ((uint32_t)Rs >= (uint32_t)W) {
            bad = 1;
            break;
        }
        const int32_t kc = Rs / 16;
        uint64_t w0[PB], w1[PB];
#pragma unroll
        for (int u = 0; u < PB; u++) {
            const bool in = i0 - u > 0;
            const int64_t base = (int64_t)(i0 - u - 1) * stride;
            w0[u] = in ? dm[base + kc] : 0ull;
            w1[u] = (in && kc + 1 < stride) ? dm[base + kc + 1] : 0ull;
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
                const int32_t k = R / 16;
                const uint64_t word = k == kc ? w0[u] : (k == kc + 1 ? w1[u] : dm[(int64_t)(i - 1) * stride + k]);
                const uint32_t d = (uint32_t)(word >> (4 * (R % 16))) & 15u;
                if (state == 0) {
                    const uint32_t op = d & 3u;
                    if (op == EP_OP_MATCH || op == EP_OP_MISMATCH) {
                        w.put(op);
                        cost += op == EP_OP_MISMATCH ? (uint32_t)c.cm : 0u;
                        --i;
                        --j;
                        continue;
                    }
                    state = op;
                }
                if (state == EP_OP_INS) {
                    w.put(EP_OP_INS);
                    cost += (uint32_t)c.ce;
                    --j;
                    if (!(d & NWA_EXT_E)) {
                        cost += (uint32_t)c.co;
                        state = 0;
                    }
                } else {
                    w.put(EP_OP_DEL);
                    cost += (uint32_t)c.ce;
                    --i;
                    if (!(d & NWA_EXT_F)) {
                        cost += (uint32_t)c.co;
                        state = 0;
                    }
                }
            }
        }
    }
    if (i > 0) cost += (uint32_t)c.co + (uint32_t)c.ce * (uint32_t)i;
    while (i > 0) {
        w.put(EP_OP_DEL);
        --i;
    }
    if (j > 0 && !bad) cost += (uint32_t)c.co + (uint32_t)c.ce * (uint32_t)j;
    while (j > 0 && !bad) {
        w.put(EP_OP_INS);
        --j;
    }
    w.flush();
    EpResult r;
    r.nops = w.nops | (bad ? EP_REJECTED : 0u);
    r.score = cost;
    return r;
}

}  // namespace nwa

#endif
