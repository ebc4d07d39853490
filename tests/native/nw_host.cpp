// The lane code of k_nw (dentist_amd/csrc/dh_nw.h: band, row0, load_window, row_min, row_finish, traceback, accepted,
// next_w) compiled for the CPU.  A wavefront is played lane by lane the way the kernel uses these functions: per row the
// values that cross lanes are taken first (the first cell of the lane to the right, of the next strip for lane 63), then
// per strip the first pass of every lane, an inclusive prefix minimum over the 64 lanes with the carry of the strips in
// front, the second pass of every lane and the store of the decision words; lane 0 walks them back.  The attempts at
// growing half-widths are the host's loop of dh_nw.cpp.  tests/test_nw_host.py compares with oracle/nw.c.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../dentist_amd/csrc/dh_nw.h"

namespace {

struct Attempt {
    EpResult res;
    int32_t corner;  // F[rl][ql] of the banded fill
    std::vector<uint8_t> ops;
};

template <int CPL, int NS>
Attempt play(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, nw::Band b, int32_t fs)
{
    constexpr int STRIP = 64 * CPL;
    const int32_t lo = b.lo, W = b.hi - b.lo + 1;
    const int64_t stride = nw::row_words<CPL>(W);
    std::vector<uint32_t> dm((size_t)(rl * stride), 0xAAAAAAAAu);
    std::vector<int32_t> written((size_t)(rl * stride), 0);
    static int32_t prev[64][NS][CPL];
    static uint32_t qn[64][NS][CPL / 4], qc[64][NS][CPL / 4];
    for (int lane = 0; lane < 64; lane++)
        for (int s = 0; s < NS; s++) {
            const int32_t R0 = s * STRIP + lane * CPL;
            nw::row0<CPL>(prev[lane][s], lo + R0, nw::valid_limit(lo + R0, R0, W, ql), fs);
            nw::load_window<CPL>(qry, lo + R0, ql, qn[lane][s]);
        }
    uint64_t refw = 0;
    for (int32_t i = 1; i <= rl; i++) {
        const int32_t o = (i - 1) & 7;
        if (o == 0) memcpy(&refw, ref + (i - 1), 8);
        const uint32_t rc = (uint32_t)(refw >> (8 * o)) & 0xFFu;
        const int32_t border = fs ? 0 : i;
        int32_t nxt[64][NS];
        for (int lane = 0; lane < 64; lane++)
            for (int s = 0; s < NS; s++) {
                nxt[lane][s] = lane < 63 ? prev[lane + 1][s][0] : (s + 1 < NS ? prev[0][s + 1][0] : NW_INF);
                memcpy(qc[lane][s], qn[lane][s], sizeof(qc[lane][s]));
                nw::load_window<CPL>(qry, i + lo + s * STRIP + lane * CPL, ql, qn[lane][s]);
            }
        int32_t carry = NW_INF;
        for (int s = 0; s < NS; s++) {
            int32_t loc[64][CPL], incl[64];
            uint32_t mmbits[64];
            int32_t run = NW_INF;
            for (int lane = 0; lane < 64; lane++) {
                const int32_t R0 = s * STRIP + lane * CPL, j0 = i + lo + R0;
                const int32_t m = nw::row_min<CPL>(prev[lane][s], nxt[lane][s], rc, qc[lane][s], j0, R0, nw::valid_limit(j0, R0, W, ql),
                                                   border, loc[lane], mmbits[lane]);
                run = run < m ? run : m;
                incl[lane] = run;
            }
            for (int lane = 0; lane < 64; lane++) {
                const int32_t R0 = s * STRIP + lane * CPL, j0 = i + lo + R0;
                int32_t excl = lane == 0 ? NW_INF : incl[lane - 1];
                excl = excl < carry ? excl : carry;
                const uint32_t word = nw::row_finish<CPL>(prev[lane][s], nxt[lane][s], loc[lane], mmbits[lane], excl, j0, R0,
                                                          nw::valid_limit(j0, R0, W, ql));
                if (R0 < W) {
                    const size_t at = (size_t)((int64_t)(i - 1) * stride + R0 / CPL);
                    dm[at] = word;
                    written[at]++;
                }
            }
            carry = carry < incl[63] ? carry : incl[63];
        }
    }
    Attempt a;
    a.corner = NW_INF;
    {
        const int32_t R = ql - rl - lo;  // the corner's column in the last row
        a.corner = prev[(R % STRIP) / CPL][R / STRIP][R % CPL];
    }
    for (int32_t w : written)
        if (w != 1) a.corner = -1;  // a decision word stored twice or never
    std::vector<uint64_t> ow((size_t)((rl + ql + 7) >> 3) + 1, 0);
    a.res = nw::traceback<CPL>(rl, ql, lo, W, fs, dm.data(), ow.data());
    const int32_t nops = (int32_t)(a.res.nops & ~EP_REJECTED);
    a.ops.resize((size_t)nops);
    for (int32_t p = 0; p < nops; p++) {  // k_edit_compact
        const int32_t q = nops - 1 - p;
        a.ops[(size_t)p] = (uint8_t)(ow[(size_t)(q >> 3)] >> (8 * (q & 7)));
    }
    return a;
}

bool attempt(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, nw::Band b, int32_t fs, Attempt &a)
{
    int32_t cpl, ns;
    if (!nw::band_class(b.hi - b.lo + 1, cpl, ns)) return false;
    if (cpl == 4)
        a = play<4, 1>(ref, rl, qry, ql, b, fs);
    else if (cpl == 8)
        a = play<8, 1>(ref, rl, qry, ql, b, fs);
    else if (ns == 1)
        a = play<16, 1>(ref, rl, qry, ql, b, fs);
    else if (ns == 2)
        a = play<16, 2>(ref, rl, qry, ql, b, fs);
    else
        a = play<16, 4>(ref, rl, qry, ql, b, fs);
    return true;
}

// the sequences with the padding the device buffers have (dh_nw.cpp): the bytes around them are never compared
struct Padded {
    std::vector<uint8_t> r, q;
    Padded(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql) : r((size_t)rl + 2 * NW_SEQ_PAD, 0x5A), q((size_t)ql + 2 * NW_SEQ_PAD, 0xA5)
    {
        if (rl) memcpy(r.data() + NW_SEQ_PAD, ref, (size_t)rl);
        if (ql) memcpy(q.data() + NW_SEQ_PAD, qry, (size_t)ql);
    }
};

}  // namespace

// One attempt at half-width w.  info[0] = cost of the walk, [1] = nw::accepted, [2] = the walk left the band, [3] = band lo,
// [4] = band hi, [5] = F[rl][ql] of the banded fill (-1: a decision word stored twice or never), [6] = cells per lane,
// [7] = strips.  Returns the number of ops (written when cap suffices), -1 when no kernel class serves the band.
extern "C" int32_t nw_host_attempt(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, int32_t fs, int32_t w, uint8_t *ops,
                                   int32_t cap, int32_t *info)
{
    if (rl < 1 || ql < 1) return -2;
    const Padded p(ref, rl, qry, ql);
    const nw::Band b = nw::band(rl, ql, w, fs);
    Attempt a;
    if (!attempt(p.r.data() + NW_SEQ_PAD, rl, p.q.data() + NW_SEQ_PAD, ql, b, fs, a)) return -1;
    const bool left = (a.res.nops & EP_REJECTED) != 0;
    info[0] = (int32_t)a.res.score;
    info[1] = !left && nw::accepted((int64_t)a.res.score, w, fs, b.full) ? 1 : 0;
    info[2] = left ? 1 : 0;
    info[3] = b.lo;
    info[4] = b.hi;
    info[5] = a.corner;
    nw::band_class(b.hi - b.lo + 1, info[6], info[7]);
    if ((int32_t)a.ops.size() <= cap && !a.ops.empty()) memcpy(ops, a.ops.data(), a.ops.size());
    return (int32_t)a.ops.size();
}

// The whole policy of dh_nw.cpp for one pair with both sides non-empty: attempts at w0, 2 w0, ... until nw::accepted.
// out[0] = status (0, or 1 = band exceeded), [1] = score, [2] = attempts, [3] = half-width of the last attempt.  Returns
// the number of ops.
extern "C" int32_t nw_host_align(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, int32_t fs, int32_t w0, uint8_t *ops,
                                 int32_t cap, int32_t *out)
{
    if (rl < 1 || ql < 1) return -2;
    const Padded p(ref, rl, qry, ql);
    int64_t w = 0;
    out[0] = 1;
    out[1] = -1;
    out[2] = 0;
    out[3] = 0;
    for (;;) {
        w = nw::next_w(rl, ql, fs, w, w0);
        if (w < 0) return 0;
        const nw::Band b = nw::band(rl, ql, w, fs);
        Attempt a;
        if (!attempt(p.r.data() + NW_SEQ_PAD, rl, p.q.data() + NW_SEQ_PAD, ql, b, fs, a)) return -1;
        out[2]++;
        out[3] = (int32_t)w;
        if ((a.res.nops & EP_REJECTED) || !nw::accepted((int64_t)a.res.score, w, fs, b.full)) continue;
        if (a.corner != (int32_t)a.res.score) return -3;  // the walk's cost is F[rl][ql] of the banded matrix
        out[0] = 0;
        out[1] = (int32_t)a.res.score;
        if ((int32_t)a.ops.size() <= cap && !a.ops.empty()) memcpy(ops, a.ops.data(), a.ops.size());
        return (int32_t)a.ops.size();
    }
}
