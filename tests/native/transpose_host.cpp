// The lane code of k_trace_transpose (dentist_amd/csrc/dh_editpath.h: tr_word, tr_count, tr_walk, tr_tiles) compiled for
// the CPU.  A wavefront is played lane by lane the way the kernel uses these functions: slice counts, an inclusive sum
// over the 64 lanes, the carry of the passes before, a walk only where a grid point lies in the slice, one slot per trace
// point; then the pairs as k_trace_pairs forms them.  tests/test_transpose_host.py compares with tests/transpose_ref.py.
#include <stdint.h>

#include <vector>

#include "../../dentist_amd/csrc/dh_editpath.h"

// returns the number of tiles, or -1 (a slot written twice or never), -2 (the ops do not advance A' by a1 - a0),
// -3 (cap too small); pairs[m] = diffs | bases << 16
extern "C" int32_t tr_host_record(const uint8_t *ops, int32_t nops, int32_t comp, int32_t a0, int32_t a1, int32_t ts,
                                  uint32_t *pairs, int32_t cap)
{
    const int32_t ntiles = ep::tr_tiles(a0, a1, ts), g0 = a0 / ts;
    if (ntiles > cap) return -3;
    std::vector<uint32_t> bd_d((size_t)ntiles, 0), bd_b((size_t)ntiles, 0);
    std::vector<int32_t> writes((size_t)ntiles, 0);
    uint32_t ca = 0, cb = 0, cd = 0;
    for (int32_t p0 = 0; p0 < nops; p0 += EP_TR_PASS_OPS) {
        uint64_t w[64][8];
        uint32_t sa[64], sb[64], sd[64], iab[64], id[64];
        uint32_t run_ab = 0, run_d = 0;
        for (int lane = 0; lane < 64; lane++) {
            const int32_t k0 = p0 + lane * EP_TR_LANE_OPS;
            sa[lane] = sb[lane] = sd[lane] = 0;
            for (int j = 0; j < 8; j++) {
                w[lane][j] = k0 + 8 * j < nops ? ep::tr_word(ops, nops, comp, k0 + 8 * j) : 0x0404040404040404ull;
                ep::tr_count(w[lane][j], sa[lane], sb[lane], sd[lane]);
            }
            run_ab += sa[lane] | (sb[lane] << 16);
            run_d += sd[lane];
            iab[lane] = run_ab;
            id[lane] = run_d;
        }
        for (int lane = 0; lane < 64; lane++) {
            const int32_t pos = a0 + (int32_t)(ca + (iab[lane] & 0xFFFFu) - sa[lane]), next = (pos / ts + 1) * ts;
            if (next <= pos + (int32_t)sa[lane] && next < a1)
                ep::tr_walk(w[lane], pos, ts, cb + (iab[lane] >> 16) - sb[lane], cd + id[lane] - sd[lane],
                            [&](int32_t gp, uint32_t d, uint32_t b) {
                                const int32_t m = gp / ts - g0 - 1;
                                if (gp < a1 && m >= 0 && m < ntiles - 1) {
                                    bd_d[(size_t)m] = d;
                                    bd_b[(size_t)m] = b;
                                    writes[(size_t)m]++;
                                }
                            });
        }
        ca += iab[63] & 0xFFFFu;
        cb += iab[63] >> 16;
        cd += id[63];
    }
    if ((int64_t)ca != (int64_t)a1 - a0) return -2;
    bd_d[(size_t)ntiles - 1] = cd;
    bd_b[(size_t)ntiles - 1] = cb;
    writes[(size_t)ntiles - 1]++;
    for (int32_t m = 0; m < ntiles; m++) {
        if (writes[(size_t)m] != 1) return -1;
        const uint32_t d = bd_d[(size_t)m] - (m ? bd_d[(size_t)m - 1] : 0u), b = bd_b[(size_t)m] - (m ? bd_b[(size_t)m - 1] : 0u);
        pairs[m] = (d & 0xFFFFu) | (b << 16);
    }
    return ntiles;
}
