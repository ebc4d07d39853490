// The plan lane code of the chain padder (dentist_amd/csrc/dh_chainpad.h) played on the CPU: the segments and the status of one
// chain, as rows of six values -- (0, record, first tile, end tile, 0, 0) for a tile run, (1, record p, a0, a1, b0, b1) for a
// filler -- the way k_cp_plan's two runs see them.  Test infrastructure (tests/test_chainpad_host.py, chainpad_host_main.cpp).
#include <stdint.h>

#include "../../dentist_amd/csrc/dh_chainpad.h"

namespace {
struct RowOut {
    int32_t *rows;
    int64_t cap, n;
    void put(int32_t a, int32_t b, int32_t c, int32_t d, int32_t e, int32_t f)
    {
        if (n < cap) {
            int32_t *r = rows + 6 * n;
            r[0] = a, r[1] = b, r[2] = c, r[3] = d, r[4] = e, r[5] = f;
        }
        n++;
    }
    void tiles(int64_t k, int32_t t0, int32_t t1) { put(CP_SEG_TILES, (int32_t)k, t0, t1, 0, 0); }
    void filler(int64_t k, int32_t a0, int32_t a1, int32_t b0, int32_t b1) { put(CP_SEG_FILLER, (int32_t)k, a0, a1, b0, b1); }
};
}  // namespace

// returns the status; *nrows = segments emitted (rows holds the first `cap` of them)
extern "C" int32_t chainpad_host_plan(const CpRec *recs, int64_t nrec, const uint16_t *tr, int32_t ts, int32_t *rows, int64_t cap,
                                      int64_t *nrows)
{
    RowOut o{rows, cap, 0};
    const int32_t st = cp::walk_chain(recs, tr, ts, 0, nrec, o);
    *nrows = st == CP_OK ? o.n : 0;
    return st;
}

extern "C" int32_t chainpad_host_point_a(const CpRec *r, int32_t ts, int32_t i) { return cp::point_a(*r, ts, i); }

extern "C" int32_t chainpad_host_generated_op(const uint8_t *a, const uint8_t *b, int32_t la, int32_t lb, int32_t p)
{
    return cp::generated_op(a, b, la, lb, p);
}
