// dh_bitvec.h -- three-input bit logic on 32-bit words for the bit-vector kernels (k_tile, k_seg_vote_bp).
//
// gfx950 evaluates any Boolean function of three 32-bit operands in one VALU instruction (v_bitop3_b32, the function
// given as an 8-bit truth table).  The compiler forms it on its own only from 32-bit operations: a 64-bit and / or / xor
// is split into halves after the combine has run, so code on 64-bit bit vectors gets none.  The kernels therefore work
// on 32-bit halves and name the function explicitly: b3<LUT>(a, b, c), the table composed from the three operand
// columns BA / BB / BC, e.g. b3<BA & (BB ^ BC)>(x, y, z) = x & (y ^ z).  The host evaluates the same table bit by bit,
// so that the CPU tests run the very expressions the kernels run.
#ifndef DH_BITVEC_H
#define DH_BITVEC_H

#include <stdint.h>

#if defined(__HIPCC__)
#define DH_BV __host__ __device__ __forceinline__
#else
#define DH_BV inline
#endif

namespace dhbv {

// truth-table columns of the operands: bit m of a table is the result for a = m >> 2 & 1, b = m >> 1 & 1, c = m & 1
constexpr uint32_t BA = 0xF0, BB = 0xCC, BC = 0xAA;

// (the table is taken mod 256, so that a complement in its formula needs no mask: b3<BA | ~(BB | BC)>)
template <uint32_t LUT>
DH_BV uint32_t b3(uint32_t a, uint32_t b, uint32_t c)
{
    constexpr uint32_t T = LUT & 0xFFu;
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, T);
#else
    uint32_t r = 0;
    for (uint32_t m = 0; m < 8; m++)
        if (T >> m & 1u) r |= ((m & 4u) ? a : ~a) & ((m & 2u) ? b : ~b) & ((m & 1u) ? c : ~c);
    return r;
#endif
}

// bit `pos` of w (pos in [0, 31]) as a mask: 0 or ~0 (one v_bfe_i32)
DH_BV uint32_t bitmask(uint32_t w, uint32_t pos)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)__builtin_amdgcn_sbfe((int32_t)w, pos, 1u);
#else
    return (uint32_t)(((int32_t)(w << (31u - pos))) >> 31);
#endif
}

// ({hi, lo} >> sh)[31:0], sh in [0, 31] (one v_alignbit_b32)
DH_BV uint32_t funnel32(uint32_t hi, uint32_t lo, uint32_t sh)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_alignbit(hi, lo, sh);
#else
    return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u));
#endif
}

}  // namespace dhbv

#endif
