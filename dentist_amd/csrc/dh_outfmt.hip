// dh_outfmt.hip -- the FASTA text of dh_output_db formatted on the device: one lane per 16 consecutive bytes of a chunk of the
// file, one aligned 16-byte store per lane (lane code: dh_outfmt.h).  No atomics, no LDS, no dependence between lanes.
#include <hip/hip_runtime.h>

#include "dh_outfmt.h"

// bytes [q0, q1) of the file into out[0 .. q1 - q0); out is 16-byte aligned and holds a multiple of 16 bytes (the bytes of
// the last lane behind q1 are written as zero)
__global__ __launch_bounds__(OF_BLOCK) void k_outfmt(of::Plan p, int64_t q0, int64_t q1, uint4 *out)
{
    const int64_t lane = (int64_t)blockIdx.x * OF_BLOCK + threadIdx.x;
    const int64_t q = q0 + lane * OF_LANE_BYTES;
    if (q >= q1) return;
    uint32_t w[4];
    of::lane16(p, q, q1, w);
    out[lane] = make_uint4(w[0], w[1], w[2], w[3]);
}

extern "C" void dhk_outfmt(hipStream_t st, const of::Plan *p, int64_t q0, int64_t q1, void *out)
{
    const int64_t lanes = (q1 - q0 + OF_LANE_BYTES - 1) / OF_LANE_BYTES;
    if (lanes <= 0) return;
    hipLaunchKernelGGL(k_outfmt, dim3((unsigned)((lanes + OF_BLOCK - 1) / OF_BLOCK)), dim3(OF_BLOCK), 0, st, *p, q0, q1, (uint4 *)out);
}
