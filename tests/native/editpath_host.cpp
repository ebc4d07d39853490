// editpath_host.cpp -- the lane code of the edit-path kernel (dentist_amd/csrc/dh_editpath.h: ep::fill / ep::traceback,
// three-input functions through dh_bitvec.h: b3) compiled for the CPU.
//
// TEST INFRASTRUCTURE: one lane's view of k_edit_fast -- the banded bit-parallel fill of one tile into its three decision
// planes, the traceback over them and the acceptance rule -- so that the CPU tests compare the very expressions the kernel
// runs with oracle/nw.c.
// Build: g++ -O2 -shared -fPIC -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ (Makefile target tests/native/libdh_editpath_host.so)
#include <cstdint>
#include <vector>

#include "../../dentist_amd/csrc/dh_editpath.h"

// One tile as lane `lane` of a launch of `stride` tiles would run it (the other lanes' words stay untouched: checked).
// ref / qry must be readable 8 bytes past their ends.  Returns 0 = accepted, 1 = rejected (path left the band or costs
// more than diffs), 2 = not eligible for class nw, 3 = a word outside the lane's own was written.
extern "C" int ep_host_tile(const uint8_t *ref, int32_t rl, const uint8_t *qry, int32_t ql, int32_t diffs, int32_t nw,
                            int32_t stride, int32_t lane, uint8_t *ops, int32_t *nops, int32_t *score)
{
    const int cls = ep::tile_class(rl, ql, diffs);
    if (cls == 0 || cls > nw) return 2;
    const uint64_t MAGIC = 0x5a5a5a5a5a5a5a5aull;
    const int64_t owords = (rl + ql + 7) / 8 + 1;
    std::vector<uint64_t> dm((size_t)(rl + 1) * 3 * nw * stride, MAGIC), ow((size_t)owords * stride, MAGIC);
    if (nw == 1)
        ep::fill<1>(ref, rl, qry, ql, dm.data() + lane, stride);
    else
        ep::fill<2>(ref, rl, qry, ql, dm.data() + lane, stride);
    const EpResult r = nw == 1 ? ep::traceback<1>(rl, ql, dm.data() + lane, stride, ow.data() + lane, stride)
                               : ep::traceback<2>(rl, ql, dm.data() + lane, stride, ow.data() + lane, stride);
    for (size_t k = 0; k < dm.size(); k++)
        if ((int64_t)(k % stride) != lane && dm[k] != MAGIC) return 3;
    for (size_t k = 0; k < ow.size(); k++)
        if ((int64_t)(k % stride) != lane && ow[k] != MAGIC) return 3;
    const int32_t n = (int32_t)(r.nops & ~EP_REJECTED);
    *nops = n;
    *score = (int32_t)r.score;
    for (int32_t p = 0; p < n; p++) {
        const int32_t q = n - 1 - p;
        ops[p] = (uint8_t)(ow[(size_t)(q >> 3) * stride + lane] >> (8 * (q & 7)));
    }
    return ((r.nops & EP_REJECTED) || (int64_t)r.score > diffs) ? 1 : 0;
}
