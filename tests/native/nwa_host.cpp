// The lane code of k_nwa (dentist_amd/csrc/dh_nwa.h: costs, row0, row_min, row_finish, store_decisions, traceback,
// accepted, next_w) compiled for the CPU.  A wavefront is played lane by lane the way the kernel uses these functions: per
// row the values that cross lanes are taken first (H and F of the first cell of the lane to the right, of the next strip
// for lane 63), then per strip the first pass of every lane, an inclusive prefix minimum over the 64 lanes with the carry of
// the strips in front, G of the last cell of the lane to the left, the second pass of every lane and the store of the
// decisions; lane 0 walks them back.  The attempts at growing half-widths are the host's loop of dh_nwa.cpp.
// tests/test_nwa_host.py compares with tests/nwa_ref.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../dentist_amd/csrc/dh_nwa.h"

namespace {

struct Attempt {
    EpResult res;
    int32_t corner;  // H[rl][ql] of the banded fill
    std::vector<uint8_t> ops;
};

template <int CPL, int NS>
Attempt play(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, nw::Band b, const NwaCost &c)
{
    constexpr int STRIP = 64 * CPL;
    const int32_t lo = b.lo, W = b.hi - b.lo + 1;
    const int64_t stride = nwa::row_words(W);
    std::vector<uint64_t> dm((size_t)(rl * stride), 0xAAAAAAAAAAAAAAAAull);
    std::vector<uint8_t> written((size_t)(rl * stride * 8), 0);  // per byte of the decisions
    static int32_t H[64][NS][CPL], F[64][NS][CPL];
    static uint32_t qn[64][NS][CPL / 4], qc[64][NS][CPL / 4];
    for (int lane = 0; lane < 64; lane++)
        for (int s = 0; s < NS; s++) {
            const int32_t R0 = s * STRIP + lane * CPL;
            nwa::row0<CPL>(H[lane][s], F[lane][s], lo + R0, nw::valid_limit(lo + R0, R0, W, ql), c);
            nw::load_window<CPL>(qry, lo + R0, ql, qn[lane][s]);
        }
    uint64_t refw = 0;
    for (int32_t i = 1; i <= rl; i++) {
        const int32_t o = (i - 1) & 7;
        if (o == 0) memcpy(&refw, ref + (i - 1), 8);
        const uint32_t rc = (uint32_t)(refw >> (8 * o)) & 0xFFu;
        const int32_t border = c.co + c.ce * i;
        int32_t nh[64][NS], nf[64][NS];
        for (int lane = 0; lane < 64; lane++)
            for (int s = 0; s < NS; s++) {
                nh[lane][s] = lane < 63 ? H[lane + 1][s][0] : (s + 1 < NS ? H[0][s + 1][0] : NW_INF);
                nf[lane][s] = lane < 63 ? F[lane + 1][s][0] : (s + 1 < NS ? F[0][s + 1][0] : NW_INF);
                memcpy(qc[lane][s], qn[lane][s], sizeof(qc[lane][s]));
                nw::load_window<CPL>(qry, i + lo + s * STRIP + lane * CPL, ql, qn[lane][s]);
            }
        int32_t carry = NW_INF, gcarry = NW_INF;
        uint64_t *row = dm.data() + (int64_t)(i - 1) * stride;
        for (int s = 0; s < NS; s++) {
            int32_t loc[64][CPL], incl[64], glast[64];
            uint32_t mmbits[64];
            int32_t run = NW_INF;
            for (int lane = 0; lane < 64; lane++) {
                const int32_t R0 = s * STRIP + lane * CPL, j0 = i + lo + R0;
                const int32_t m = nwa::row_min<CPL>(H[lane][s], F[lane][s], nh[lane][s], nf[lane][s], rc, qc[lane][s], j0, R0,
                                                    nw::valid_limit(j0, R0, W, ql), border, c, loc[lane], mmbits[lane], glast[lane]);
                run = run < m ? run : m;
                incl[lane] = run;
            }
            for (int lane = 0; lane < 64; lane++) {
                const int32_t R0 = s * STRIP + lane * CPL, j0 = i + lo + R0;
                int32_t excl = lane == 0 ? NW_INF : incl[lane - 1];
                excl = excl < carry ? excl : carry;
                const int32_t gleft = lane == 0 ? gcarry : glast[lane - 1];
                const uint64_t bits = nwa::row_finish<CPL>(H[lane][s], F[lane][s], nh[lane][s], loc[lane], mmbits[lane], excl, gleft, j0, R0,
                                                           nw::valid_limit(j0, R0, W, ql), border, c);
                if (R0 < W) {
                    nwa::store_decisions<CPL>(row, R0, bits);
                    for (int k = 0; k < CPL / 2; k++) written[(size_t)(((int64_t)(i - 1) * stride) * 8 + R0 / 2 + k)]++;
                }
            }
            carry = carry < incl[63] ? carry : incl[63];
            gcarry = glast[63];
        }
    }
    Attempt a;
    {
        const int32_t R = ql - rl - lo;  // the corner's column in the last row
        a.corner = H[(R % STRIP) / CPL][R / STRIP][R % CPL];
    }
    for (int32_t i = 0; i < rl; i++)  // every byte that holds a cell of the band stored exactly once, no byte twice
        for (int64_t k = 0; k < stride * 8; k++) {
            const uint8_t n = written[(size_t)(i * stride * 8 + k)];
            if (n > 1 || (n == 0 && 2 * k < W)) a.corner = -1;
        }
    std::vector<uint64_t> ow((size_t)((rl + ql + 7) >> 3) + 1, 0);
    a.res = nwa::traceback(rl, ql, lo, W, c, dm.data(), ow.data());
    const int32_t nops = (int32_t)(a.res.nops & ~EP_REJECTED);
    a.ops.resize((size_t)nops);
    for (int32_t p = 0; p < nops; p++) {  // k_edit_compact
        const int32_t q = nops - 1 - p;
        a.ops[(size_t)p] = (uint8_t)(ow[(size_t)(q >> 3)] >> (8 * (q & 7)));
    }
    return a;
}

bool attempt(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, nw::Band b, const NwaCost &c, Attempt &a)
{
    int32_t cpl, ns;
    if (!nwa::band_class(b.hi - b.lo + 1, cpl, ns)) return false;
    if (cpl == 4)
        a = play<4, 1>(ref, rl, qry, ql, b, c);
    else if (cpl == 8)
        a = play<8, 1>(ref, rl, qry, ql, b, c);
    else if (ns == 1)
        a = play<16, 1>(ref, rl, qry, ql, b, c);
    else
        a = play<16, 2>(ref, rl, qry, ql, b, c);
    return true;
}

// the sequences with the padding the device buffers have (dh_nwa.cpp): the bytes around them are never compared
struct Padded {
    std::vector<uint8_t> r, q;
    Padded(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql) : r((size_t)rl + 2 * NW_SEQ_PAD, 0x5A), q((size_t)ql + 2 * NW_SEQ_PAD, 0xA5)
    {
        if (rl) memcpy(r.data() + NW_SEQ_PAD, ref, (size_t)rl);
        if (ql) memcpy(q.data() + NW_SEQ_PAD, qry, (size_t)ql);
    }
};

}  // namespace

// limits[0] = NWA_MAX_W, [1] = NWA_MAX_LEN
extern "C" void nwa_host_limits(int32_t *limits)
{
    limits[0] = NWA_MAX_W;
    limits[1] = NWA_MAX_LEN;
}

// nwa::costs: cost[0..2] = cm, ce, co; returns 0 when the scoring is refused
extern "C" int32_t nwa_host_costs(const int32_t *sc, int32_t *cost)
{
    NwaCost c;
    if (!nwa::costs(sc[0], sc[1], sc[2], sc[3], c)) return 0;
    cost[0] = c.cm;
    cost[1] = c.ce;
    cost[2] = c.co;
    return 1;
}

// One attempt at half-width w.  info[0] = cost of the walk, [1] = nwa::accepted, [2] = the walk left the band, [3] = band lo,
// [4] = band hi, [5] = H[rl][ql] of the banded fill (-1: a decision byte stored twice or never), [6] = cells per lane,
// [7] = strips.  Returns the number of ops (written when cap suffices), -1 when no kernel class serves the band, -4 for a
// refused scoring.
extern "C" int32_t nwa_host_attempt(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, const int32_t *sc, int32_t w,
                                    uint8_t *ops, int32_t cap, int32_t *info)
{
    if (rl < 1 || ql < 1) return -2;
    NwaCost c;
    if (!nwa::costs(sc[0], sc[1], sc[2], sc[3], c)) return -4;
    const Padded p(ref, rl, qry, ql);
    const nw::Band b = nw::band(rl, ql, w, 0);
    Attempt a;
    if (!attempt(p.r.data() + NW_SEQ_PAD, rl, p.q.data() + NW_SEQ_PAD, ql, b, c, a)) return -1;
    const bool left = (a.res.nops & EP_REJECTED) != 0;
    info[0] = (int32_t)a.res.score;
    info[1] = !left && nwa::accepted((int64_t)a.res.score, w, c.ce, b.full) ? 1 : 0;
    info[2] = left ? 1 : 0;
    info[3] = b.lo;
    info[4] = b.hi;
    info[5] = a.corner;
    nwa::band_class(b.hi - b.lo + 1, info[6], info[7]);
    if ((int32_t)a.ops.size() <= cap && !a.ops.empty()) memcpy(ops, a.ops.data(), a.ops.size());
    return (int32_t)a.ops.size();
}

// The whole policy of dh_nwa.cpp for one pair with both sides non-empty: attempts at w0, 2 w0, ... until nwa::accepted.
// out[0] = status (0, or 1 = band exceeded), [1] = cost, [2] = attempts, [3] = half-width of the last attempt, [4] = the
// alignment score.  Returns the number of ops.
extern "C" int32_t nwa_host_align(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, const int32_t *sc, int32_t w0,
                                  uint8_t *ops, int32_t cap, int32_t *out)
{
    if (rl < 1 || ql < 1) return -2;
    NwaCost c;
    if (!nwa::costs(sc[0], sc[1], sc[2], sc[3], c)) return -4;
    const Padded p(ref, rl, qry, ql);
    int64_t w = 0;
    out[0] = 1;
    out[1] = -1;
    out[2] = 0;
    out[3] = 0;
    out[4] = -1;
    for (;;) {
        w = nwa::next_w(rl, ql, w, w0);
        if (w < 0) return 0;
        const nw::Band b = nw::band(rl, ql, w, 0);
        Attempt a;
        if (!attempt(p.r.data() + NW_SEQ_PAD, rl, p.q.data() + NW_SEQ_PAD, ql, b, c, a)) return -1;
        out[2]++;
        out[3] = (int32_t)w;
        if ((a.res.nops & EP_REJECTED) || !nwa::accepted((int64_t)a.res.score, w, c.ce, b.full)) continue;
        if (a.corner != (int32_t)a.res.score) return -3;  // the walk's cost is H[rl][ql] of the banded matrix
        out[0] = 0;
        out[1] = (int32_t)a.res.score;
        out[4] = nwa::score_of(c, rl, ql, (int64_t)a.res.score);
        if ((int32_t)a.ops.size() <= cap && !a.ops.empty()) memcpy(ops, a.ops.data(), a.ops.size());
        return (int32_t)a.ops.size();
    }
}
