// dh_bpsload.hip -- the 2-bit packed bytes of a chunk of reads unpacked into a DB's bases on the device: one lane per 16
// consecutive output bytes, one aligned 16-byte store per lane whose window lies in one read (lane code: dh_bpsload.h).  No
// atomics, no LDS, no dependence between lanes; neighbouring chunks share at most their ragged edge windows, whose bytes
// each of them writes singly and only its own.
#include <hip/hip_runtime.h>

#include "dh_bpsload.h"

// out: the bases of the whole DB (16-byte aligned); w0: the chunk's first window
__global__ __launch_bounds__(BL_BLOCK) void k_bps_unpack(bl::Chunk c, int64_t w0, int64_t nwin, uint8_t *out)
{
    const int64_t lane = (int64_t)blockIdx.x * BL_BLOCK + threadIdx.x;
    if (lane >= nwin) return;
    const int64_t w = w0 + lane;
    uint32_t v[4];
    if (bl::lane16(c, w, out, v)) ((uint4 *)out)[w] = make_uint4(v[0], v[1], v[2], v[3]);
}

// c's pointers are device pointers; out_off[0] and out_off[nreads] are passed by the host, which knows them
extern "C" void dhk_bps_unpack(hipStream_t st, const bl::Chunk *c, int64_t d0, int64_t d1, uint8_t *out)
{
    const int64_t w0 = d0 / BL_LANE_BYTES, nwin = (d1 + BL_LANE_BYTES - 1) / BL_LANE_BYTES - w0;
    if (c->nreads <= 0 || nwin <= 0) return;
    hipLaunchKernelGGL(k_bps_unpack, dim3((unsigned)((nwin + BL_BLOCK - 1) / BL_BLOCK)), dim3(BL_BLOCK), 0, st, *c, w0, nwin, out);
}
