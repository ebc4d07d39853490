// dh_editpath.h -- lane code of the edit-path kernels (dh_editpath.hip): one trace tile per lane, Needleman-Wunsch with
// unit mismatch, indel 1, no free shift and the traceback rule of findAlignment / tracebackScoringMatrix
// (util/string.d:478-520, 775-831; oracle/nw.c).  Compiles for the host as well (tests/native/editpath_host.cpp), so that
// the CPU tests run the very expressions the kernel runs.
//
// The banded fill is the recurrence spelled out above k_seg_vote_bp (dh_consensus.hip): Hyyro's diagonal-band form of Myers'
// bit-vector step, band row R of matrix row i = query index j = i - HALF + R, D[0][j] = |j|, rows j <= 0 never match.  Here
// it runs on H = 2 NW words of 32 bits, every three-input function one dhbv::b3 (v_bitop3_b32), the way dh_tile.h's column
// step does.  Differences to k_seg_vote_bp:
//   * no LDS: the query window (three bit planes of the base codes) is built from the first HALF query bases and fed one
//     base per matrix row from an 8-byte word that is reloaded every 8 rows, as the template bases are.  Bases past the end
//     of the query enter as whatever the word holds (the DBs are padded): information only ever moves from a band row to
//     rows of larger j, so rows j > ql cannot reach a cell the traceback visits;
//   * a third decision plane E (the match bits): op0 & E is a match, op0 & ~E a mismatch, so the traceback tells the
//     two substitution codes apart without loading a base;
//   * the traceback checks that it stays inside the band and counts the cost of its path.  A path of cost c <= diffs < band
//     proves that the optimum is <= diffs, which is what makes the banded fill exact (a cell of true score <= w is exact
//     inside |i - j| <= w): the caller accepts a tile on that condition and sends every other one to the full-matrix kernel.
#ifndef DH_EDITPATH_H
#define DH_EDITPATH_H

#include <stdint.h>
#include <string.h>

#include "dh_bitvec.h"

#if defined(__HIPCC__)
#define EP_HD __host__ __device__ __forceinline__
#else
#define EP_HD inline
#endif

#define EP_OP_MATCH 0
#define EP_OP_DEL 1 /* A base without B base */
#define EP_OP_INS 2 /* B base without A base */
#define EP_OP_MISMATCH 3

#define EP_TSPACE_MAX 250                /* longest A side of a tile */
#define EP_QL_FACTOR 4                   /* B side of a tile <= EP_QL_FACTOR * tspace */
#define EP_GEN_COLS 16                   /* columns per lane of the full-matrix kernel: 64 * 16 >= 4 * 250 */
#define EP_REJECTED 0x80000000u          /* in EpResult::nops: the banded result is not proven exact */

struct EpTile {          // one trace tile
    int64_t aoff, boff;  // first base of the tile in the A bases / in the B bases (forward or reverse-complement copy)
    int32_t rl, ql;      // A bases, B bases
    int32_t diffs;       // of the trace
    int32_t comp;        // B is read from the reverse-complement copy
};
struct EpResult {
    uint32_t nops;   // | EP_REJECTED
    uint32_t score;  // cost of the path
};

struct EpCopy {               // k_edit_compact: where a tile's op words are and where its ops go
    int64_t wbase, wstride;   // op word t (eight ops, counted from the END of the path) at wbase + t * wstride
    int64_t out;              // first op of the tile in the chunk's output
    int32_t nops, general;    // general: the words are in the full-matrix kernel's buffer
};

struct EpTrRec {        // one record of a launch of k_trace_transpose
    int64_t op0;        // its first op in the chunk's ops
    int64_t slot0;      // its first tile among the tiles of the launch (boundary scratch and output pairs)
    int32_t nops, comp;
    int32_t a0, a1;     // abpos', aepos': the interval on the B read's forward strand
};

namespace ep {
using namespace dhbv;

template <int H>
EP_HD void shl1(const uint32_t (&a)[H], uint32_t (&r)[H])
{
    for (int k = H - 1; k > 0; k--) r[k] = funnel32(a[k], a[k - 1], 31);
    r[0] = a[0] << 1;
}
template <int H>
EP_HD void shr1(const uint32_t (&a)[H], uint32_t top, uint32_t (&r)[H])  // logical; `top` (0 / 1) enters at the highest bit
{
    for (int k = 0; k < H - 1; k++) r[k] = funnel32(a[k + 1], a[k], 1);
    r[H - 1] = (a[H - 1] >> 1) | (top << 31);
}

// decision words of matrix row i (1-based), plane p (0: op0, 1: L, 2: E), 64-bit word k of the band: interleaved over the
// tiles of a launch, so that the 64 lanes of a wavefront store one contiguous 512-byte piece
template <int NW>
EP_HD int64_t dm_index(int32_t i, int p, int k, int64_t stride)
{
    return ((int64_t)(i - 1) * (3 * NW) + p * NW + k) * stride;
}

// Banded fill of one tile: writes the three decision planes of rows 1 .. rl.  Needs rl, ql >= 0 only; `ref` and `qry` are
// read in 8-byte words that may reach 7 bytes past rl / ql.
template <int NW>
EP_HD void fill(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, uint64_t *dm, int64_t stride)
{
    constexpr int H = 2 * NW, HALF = 32 * NW;
    // window of row 1: bit R <-> j = 1 - HALF + R, i.e. query bases 1 .. HALF in the upper half of the words
    uint32_t p0[H], p1[H], p2[H];
    for (int h = 0; h < H; h++) p0[h] = p1[h] = p2[h] = 0;
    for (int g = 0; g < HALF / 8; g++) {
        uint64_t qw = 0;
        if (g * 8 < ql) memcpy(&qw, qry + g * 8, 8);
        uint32_t b0 = 0, b1 = 0, b2 = 0;
        for (int u = 0; u < 8; u++) {
            const uint32_t c = (uint32_t)(qw >> (8 * u));
            b0 |= (c & 1u) << u;
            b1 |= ((c >> 1) & 1u) << u;
            b2 |= ((c >> 2) & 1u) << u;
        }
        const int h = H / 2 + g / 4, sh = 8 * (g & 3);
        p0[h] |= b0 << sh;
        p1[h] |= b1 << sh;
        p2[h] |= b2 << sh;
    }
    // column 0: vertical deltas aligned for row 1 (+1 for j >= 1, -1 above), rows j >= 1 of row 0
    uint32_t Pv[H], Mv[H], lv[H];
    for (int h = 0; h < H; h++) {
        Pv[h] = h >= H / 2 ? ~0u : 0u;
        Mv[h] = ~Pv[h];
        lv[h] = h > H / 2 ? ~0u : (h == H / 2 ? ~1u : 0u);
    }
    uint64_t refw = 0, qfw = 0;
    for (int32_t i = 1; i <= rl; i++) {
        const int32_t o = (i - 1) & 7;
        if (o == 0) {
            memcpy(&refw, ref + (i - 1), 8);
            qfw = 0;
            if (HALF + i - 1 < ql) memcpy(&qfw, qry + HALF + i - 1, 8);
        }
        const uint32_t rc = (uint32_t)(refw >> (8 * o));
        // the COMPLEMENTED bits of the template base as masks: p ^ n = the bits that agree
        const uint32_t n0 = ~bitmask(rc, 0), n1 = ~bitmask(rc, 1), n2 = ~bitmask(rc, 2);
        {
            uint32_t t[H];
            shr1<H>(lv, lv[H - 1] >> 31, t);  // arithmetic: one more row has j >= 1
            for (int h = 0; h < H; h++) lv[h] = t[h];
        }
        uint32_t Eq[H], S[H], EM[H], sum[H];
        for (int h = 0; h < H; h++) {
            const uint32_t a = b3<(BA ^ BB) & BC>(p0[h], n0, lv[h]);
            const uint32_t e = b3<BA & (BB ^ BC)>(a, p1[h], n1);
            Eq[h] = b3<BA & (BB ^ BC)>(e, p2[h], n2);
            S[h] = Eq[h] & Pv[h];
            EM[h] = Eq[h] | Mv[h];
        }
        {
            uint64_t carry = 0;
            for (int k = 0; k < NW; k++) {  // the carry crosses the words
                const uint64_t x = ((uint64_t)S[2 * k + 1] << 32) | S[2 * k], y = ((uint64_t)Pv[2 * k + 1] << 32) | Pv[2 * k];
                const uint64_t s1 = x + y, s2 = s1 + carry;
                carry = (uint64_t)(s1 < x) | (uint64_t)(s2 < s1);
                sum[2 * k] = (uint32_t)s2;
                sum[2 * k + 1] = (uint32_t)(s2 >> 32);
            }
        }
        uint32_t D0[H], HP[H], HN[H], HPs[H], HNs[H], Xv[H];
        for (int h = 0; h < H; h++) {
            D0[h] = b3<(BA ^ BB) | BC>(sum[h], Pv[h], EM[h]);
            HP[h] = b3<BA | ~(BB | BC)>(Mv[h], D0[h], Pv[h]);
            HN[h] = Pv[h] & D0[h];
        }
        shl1<H>(HP, HPs);
        shl1<H>(HN, HNs);
        // decisions (dh_consensus.hip, above k_seg_vote_bp): op0 = ~HN' & ~(D0 & HP); L = [h(R - 1) + h(R) <= 1 - D0], false
        // iff both deltas are +1, or exactly one is +1, the other 0, and D0 is set.  The top row of the band has no left
        // neighbour: HN' has bit 0 clear, L gets it cleared.
        uint32_t Z[H], L[H];
        for (int h = 0; h < H; h++) {
            Z[h] = b3<~BA & ~(BB & BC)>(HNs[h], D0[h], HP[h]);
            const uint32_t u = b3<BA & ~BB & ~BC>(HPs[h], HP[h], HN[h]);   // h(R - 1) = +1, h(R) = 0
            const uint32_t v = b3<~BA & ~BB & BC>(HPs[h], HNs[h], HP[h]);  // h(R - 1) = 0, h(R) = +1
            const uint32_t t1 = b3<(BA | BB) & BC>(u, v, D0[h]);
            L[h] = b3<~(BA & BB) & ~BC>(HPs[h], HP[h], t1);
        }
        L[0] &= ~1u;
        for (int k = 0; k < NW; k++) {
            dm[dm_index<NW>(i, 0, k, stride)] = ((uint64_t)Z[2 * k + 1] << 32) | Z[2 * k];
            dm[dm_index<NW>(i, 1, k, stride)] = ((uint64_t)L[2 * k + 1] << 32) | L[2 * k];
            dm[dm_index<NW>(i, 2, k, stride)] = ((uint64_t)Eq[2 * k + 1] << 32) | Eq[2 * k];
        }
        // next row: vertical deltas one band row further down, the window one base further
        shr1<H>(D0, 0u, Xv);
        for (int h = 0; h < H; h++) {
            Pv[h] = b3<BA | ~(BB | BC)>(HN[h], Xv[h], HP[h]);
            Mv[h] = HP[h] & Xv[h];
        }
        const uint32_t qc = (uint32_t)(qfw >> (8 * o));
        uint32_t t[H];
        shr1<H>(p0, qc & 1u, t);
        for (int h = 0; h < H; h++) p0[h] = t[h];
        shr1<H>(p1, (qc >> 1) & 1u, t);
        for (int h = 0; h < H; h++) p1[h] = t[h];
        shr1<H>(p2, (qc >> 2) & 1u, t);
        for (int h = 0; h < H; h++) p2[h] = t[h];
    }
}

// ops back to front, eight per word; word t of a tile at ow[t * ostride]
struct OpWriter {
    uint64_t *ow;
    int64_t ostride;
    uint64_t acc = 0;
    uint32_t nops = 0;
    EP_HD OpWriter(uint64_t *ow_, int64_t ostride_) : ow(ow_), ostride(ostride_) {}
    EP_HD void put(uint32_t op)
    {
        acc |= (uint64_t)op << (8 * (nops & 7));
        nops++;
        if ((nops & 7) == 0) {
            ow[(int64_t)((nops >> 3) - 1) * ostride] = acc;
            acc = 0;
        }
    }
    EP_HD void flush()
    {
        if (nops & 7) ow[(int64_t)(nops >> 3) * ostride] = acc;
    }
};

// Traceback over the decision planes of fill<NW>: from (rl, ql) to the smallest neighbour, diagonal > insertion >
// deletion; leftover rows are deletions, leftover columns insertions.  Needs |ql - rl| < HALF.  Returns the number of ops
// and the cost of the path; EP_REJECTED is set when the path left the band.
template <int NW>
EP_HD EpResult traceback(int32_t rl, int32_t ql, const uint64_t *dm, int64_t stride, uint64_t *ow, int64_t ostride)
{
    constexpr int HALF = 32 * NW;
    constexpr int PB = NW == 1 ? 8 : 4;  // rows whose words are fetched together: a step stays in its row or moves up one
    OpWriter w(ow, ostride);
    int32_t i = rl, j = ql;
    uint32_t cost = 0, bad = 0;
    while (i > 0 && j > 0 && !bad) {
        uint64_t zr[PB][NW], lr[PB][NW], er[PB][NW];
        const int32_t i0 = i;
        for (int u = 0; u < PB; u++)
            for (int k = 0; k < NW; k++) {
                const bool in = i0 - u > 0;
                zr[u][k] = in ? dm[dm_index<NW>(i0 - u, 0, k, stride)] : 0ull;
                lr[u][k] = in ? dm[dm_index<NW>(i0 - u, 1, k, stride)] : 0ull;
                er[u][k] = in ? dm[dm_index<NW>(i0 - u, 2, k, stride)] : 0ull;
            }
        for (int u = 0; u < PB; u++) {
            while (i == i0 - u && i > 0 && j > 0) {
                const int32_t R = j - i + HALF;
                if ((uint32_t)R >= (uint32_t)(2 * HALF)) {
                    bad = 1;
                    i = -1;  // leaves every loop
                    break;
                }
                uint64_t z = zr[u][0], l = lr[u][0], e = er[u][0];
                if (NW > 1 && (R >> 6)) {
                    z = zr[u][NW - 1];
                    l = lr[u][NW - 1];
                    e = er[u][NW - 1];
                }
                const uint32_t sh = (uint32_t)R & 63u;
                if ((z >> sh) & 1ull) {
                    const uint32_t m = (uint32_t)(e >> sh) & 1u;
                    w.put(m ? EP_OP_MATCH : EP_OP_MISMATCH);
                    cost += 1u - m;
                    --i;
                    --j;
                } else if ((l >> sh) & 1ull) {
                    w.put(EP_OP_INS);
                    cost++;
                    --j;
                } else {
                    w.put(EP_OP_DEL);
                    cost++;
                    --i;
                }
            }
        }
    }
    while (i > 0) {
        w.put(EP_OP_DEL);
        cost++;
        --i;
    }
    while (j > 0 && !bad) {
        w.put(EP_OP_INS);
        cost++;
        --j;
    }
    w.flush();
    EpResult r;
    r.nops = w.nops | (bad ? EP_REJECTED : 0u);
    r.score = cost;
    return r;
}

// which fast class a tile may try: 1 (band <= 31), 2 (band <= 63), 0 = full-matrix kernel at once
inline int tile_class(int32_t rl, int32_t ql, int32_t diffs)
{
    const int64_t band = (int64_t)diffs + 1;
    const int32_t d = rl > ql ? rl - ql : ql - rl;
    if (diffs < 0 || band > 63 || d >= band) return 0;
    return band <= 31 ? 1 : 2;
}

// ---- transposition of a record's path (k_trace_transpose): the ops of the transposed record are the record's own with
// codes 1 and 2 exchanged, for a COMP record in reverse order.  Nothing is rewritten: the words below hold the codes as
// k_edit_compact left them, in the order of the transposed path, and the counts read them with the roles exchanged.

#define EP_TR_NONE 4u                          /* a byte behind the end of the path */
#define EP_TR_LANE_OPS 64                      /* ops per lane and pass */
#define EP_TR_PASS_OPS (64 * EP_TR_LANE_OPS)   /* ops per pass of a wavefront */

// ops k .. k + 7 of the transposed path (k a multiple of 8), op k in the lowest byte
EP_HD uint64_t tr_word(const uint8_t *ops, int32_t nops, int32_t comp, int32_t k)
{
    const int32_t lo = comp ? nops - 8 - k : k;  // the first of the eight in the record's own order
    uint64_t w = 0;
    if (lo >= 0 && lo + 8 <= nops) {
        memcpy(&w, ops + lo, 8);
    } else {
        for (int u = 0; u < 8; u++) {
            const int32_t x = lo + u;
            w |= (uint64_t)((x >= 0 && x < nops) ? (uint32_t)ops[x] : EP_TR_NONE) << (8 * u);
        }
    }
    return comp ? __builtin_bswap64(w) : w;
}

// adds what the ops of a word advance: a = bases of A' (every op but the record's code 1), b = bases of B' (every op but its
// code 2), d = non-zero ops
EP_HD void tr_count(uint64_t w, uint32_t &a, uint32_t &b, uint32_t &d)
{
    const uint64_t M = 0x0101010101010101ull;
    const uint64_t lo = w & M, hi = (w >> 1) & M, valid = ~(w >> 2) & M;
    a += (uint32_t)__builtin_popcountll(valid & ~(lo & ~hi));
    b += (uint32_t)__builtin_popcountll(valid & ~(hi & ~lo));
    d += (uint32_t)__builtin_popcountll(valid & (lo | hi));
}

// walk of the 64 ops of a lane's slice from position `pos` of A' with the running (b, d) at its start: at_grid(g, d, b)
// right after every op that brings A' to a multiple g of ts
template <typename F>
EP_HD void tr_walk(const uint64_t (&w)[8], int32_t pos, int32_t ts, uint32_t b, uint32_t d, F &&at_grid)
{
    int32_t next = (pos / ts + 1) * ts;
    for (int j = 0; j < 8; j++)
        for (int u = 0; u < 8; u++) {
            const uint32_t c = (uint32_t)(w[j] >> (8 * u)) & 0xFFu;
            if (c & EP_TR_NONE) continue;
            b += c != EP_OP_INS;
            d += c != EP_OP_MATCH;
            if (c == EP_OP_DEL || ++pos != next) continue;
            at_grid(next, d, b);
            next += ts;
        }
}

// tiles of the transposed record: the grid points strictly inside (a0, a1), plus one (a1 > a0)
EP_HD int32_t tr_tiles(int32_t a0, int32_t a1, int32_t ts) { return (a1 + ts - 1) / ts - a0 / ts; }

}  // namespace ep

#endif
