// dh_bpsload.h -- the lane code of the sparse packed read loader (dh_dazz_load_reads): 16 consecutive bytes of a DB's bases
// from the 2-bit packed bytes of a .bps.  Shared by the kernel of dh_bpsload.hip and the CPU harness of
// tests/native/bpsload_host.cpp.  Driver: dh_bpsload.cpp.
//
//   chunk     reads [0, nreads) of one upload: pk holds their packed runs, pk_off[r] is the byte of pk where read r starts,
//             out_off[r .. r + 1] its bases in the output (offsets into the whole DB's bases, ascending; out_off has
//             nreads + 1 entries).  A read of rlen bases has (rlen + 3) / 4 packed bytes; base x of it is
//             (byte[x >> 2] >> (6 - 2 * (x & 3))) & 3, and the low bits of its last byte behind rlen are not data.
//   window    the 16 output bytes [16 w, 16 w + 16).  The output's base is 16-byte aligned, so a window that lies inside one
//             read and inside the chunk is one aligned 16-byte store; the others (a window that straddles reads, the ragged
//             first and last window of a chunk) are written byte by byte, and only their bytes inside the chunk.
#ifndef DH_BPSLOAD_H
#define DH_BPSLOAD_H

#include <stdint.h>

#if defined(__HIPCC__)
#define BL_HD __host__ __device__ __forceinline__
#else
#define BL_HD inline
#endif

#define BL_BLOCK 256     // threads of a workgroup
#define BL_LANE_BYTES 16 // bytes a lane unpacks and stores at once

namespace bl {
struct Chunk {
    const uint8_t *pk;       // packed bytes of the chunk
    const int64_t *pk_off;   // nreads
    const int64_t *out_off;  // nreads + 1
    int64_t nreads;
};

// the last i in [lo, hi) with v[i] <= x (v[lo] <= x is given)
BL_HD int64_t last_le(const int64_t *v, int64_t lo, int64_t hi, int64_t x)
{
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] <= x)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// windows of a chunk: [first_window, end_window)
BL_HD int64_t first_window(const Chunk &c) { return c.out_off[0] / BL_LANE_BYTES; }
BL_HD int64_t end_window(const Chunk &c) { return (c.out_off[c.nreads] + BL_LANE_BYTES - 1) / BL_LANE_BYTES; }

BL_HD uint8_t base_at(const Chunk &c, int64_t r, int64_t x)
{
    return (uint8_t)((c.pk[c.pk_off[r] + (x >> 2)] >> (6 - 2 * (int)(x & 3))) & 3);
}

// the four bases of one packed byte as the four bytes of a little-endian word
BL_HD uint32_t spread4(uint32_t b)
{
    return ((b >> 6) & 3u) | (((b >> 4) & 3u) << 8) | (((b >> 2) & 3u) << 16) | ((b & 3u) << 24);
}

// Window w of the chunk.  Returns true with the 16 bytes in v[0..3] (little-endian words) when the whole window lies in one
// read of the chunk: the caller stores them at out + 16 w.  Otherwise writes the window's bytes inside the chunk itself.
BL_HD bool lane16(const Chunk &c, int64_t w, uint8_t *out, uint32_t v[4])
{
    const int64_t q = w * BL_LANE_BYTES;
    const int64_t d0 = c.out_off[0], d1 = c.out_off[c.nreads];
    const int64_t lo = q > d0 ? q : d0, hi = q + BL_LANE_BYTES < d1 ? q + BL_LANE_BYTES : d1;
    if (lo >= hi) return false;
    int64_t r = last_le(c.out_off, 0, c.nreads, lo);
    if (lo == q && hi == q + BL_LANE_BYTES && c.out_off[r + 1] >= hi) {
        // bases x .. x + 15 of read r: packed bytes x >> 2 .. (x + 15) >> 2, four of them or five, all inside the read's run
        const int64_t x = q - c.out_off[r];
        const uint8_t *s = c.pk + c.pk_off[r] + (x >> 2);
        const int sh = 2 * (int)(x & 3);
        uint64_t bits = ((uint64_t)s[0] << 32) | ((uint64_t)s[1] << 24) | ((uint64_t)s[2] << 16) | ((uint64_t)s[3] << 8);
        if (sh) bits |= s[4];
        const uint32_t b32 = (uint32_t)(bits >> (8 - sh));  // base i of the window in bits 31 - 2 i, 30 - 2 i
        for (int j = 0; j < 4; j++) v[j] = spread4((b32 >> (24 - 8 * j)) & 0xffu);
        return true;
    }
    for (int64_t g = lo; g < hi; g++) {
        while (c.out_off[r + 1] <= g) r++;  // (g < d1: a read that holds g exists)
        out[g] = base_at(c, r, g - c.out_off[r]);
    }
    return false;
}
}  // namespace bl

#endif
