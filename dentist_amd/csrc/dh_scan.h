// dh_scan.h -- the scans of one value per lane over a wavefront and over a workgroup.  Device code (shuffles): only .hip files
// include it, never dh_device.h, which the CPU harnesses compile.  gfx950, wave64.
// (mj_block_scan of dh_mjoin.hip is a copy of its own: the mapping join is on the benchmark's path and stays as it is.)
#ifndef DH_SCAN_H
#define DH_SCAN_H

#include <hip/hip_runtime.h>
#include <stdint.h>

struct ScanSum {
    static __device__ __forceinline__ int32_t op(int32_t x, int32_t y) { return x + y; }
};
struct ScanMax {
    static __device__ __forceinline__ int32_t op(int32_t x, int32_t y) { return x > y ? x : y; }
};

// lane l gets op over the values of lanes 0..l; the whole wavefront calls
template <class Op = ScanSum>
__device__ __forceinline__ int32_t wave_incl_scan(int32_t v, int32_t lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v = Op::op(v, t);
    }
    return v;
}

// One value per thread over a block of BLOCK threads, all of which call: *excl = op over the values in front of the thread's
// (IDENT for thread 0), *total = op over all of them.  IDENT is the operation's identity on the values passed: 0 for a sum, -1
// for a maximum of values >= -1.  ws: BLOCK / 64 words of LDS, free again when the call returns (it ends with a barrier).
template <int BLOCK, class Op, int32_t IDENT>
__device__ __forceinline__ void block_scan(int32_t v, int32_t *ws, int32_t *excl, int32_t *total)
{
    const int32_t lane = (int32_t)(threadIdx.x & 63), wave = (int32_t)(threadIdx.x >> 6);
    v = wave_incl_scan<Op>(v, lane);
    int32_t before = __shfl_up(v, 1, 64);
    if (lane == 0) before = IDENT;
    if (lane == 63) ws[wave] = v;
    __syncthreads();
    int32_t pre = IDENT, tot = IDENT;
    for (int w = 0; w < BLOCK / 64; w++) {
        const int32_t x = ws[w];
        if (w < wave) pre = Op::op(pre, x);
        tot = Op::op(tot, x);
    }
    __syncthreads();  // (ws is written again by the next scan)
    *excl = Op::op(pre, before);
    *total = tot;
}

#endif
