// The lane code of the sparse packed read loader (dentist_amd/csrc/dh_bpsload.h) compiled for the CPU: the selected reads go
// through chunks as dh_dazz_load_reads makes them, every chunk's windows are played as wavefronts of 64 lanes, a lane whose
// window lies in one read storing its 16 bytes at once -- what k_bps_unpack (dh_bpsload.hip) does on the device.  Test
// infrastructure (tests/test_bpsload_host.py, tests/native/bpsload_host_main.cpp).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../dentist_amd/csrc/dh_bpsload.h"

// Reads 0 .. n - 1 with rlen[r] bases whose packed bytes start at bps[boff[r]]; chunk c holds the reads
// [chunk_first[c], chunk_first[c + 1]) (nchunks + 1 ascending entries from 0 to n).  out has out_len bytes, the sum of the
// lengths, and is 16-byte aligned.  Every chunk gets a packed buffer of exactly its own bytes, so a lane that reads past a
// read's run at a chunk's end is seen by a sanitizer.  Returns the number of aligned 16-byte stores, or -1 for bad chunks,
// -2 when the lengths do not sum to out_len.
extern "C" int64_t bl_host_unpack(const uint8_t *bps, const int64_t *boff, const int32_t *rlen, int64_t n, const int64_t *chunk_first,
                                  int64_t nchunks, uint8_t *out, int64_t out_len)
{
    if (nchunks < 1 || chunk_first[0] != 0 || chunk_first[nchunks] != n) return -1;
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; r++) off[(size_t)r + 1] = off[(size_t)r] + rlen[r];
    if (off[(size_t)n] != out_len) return -2;
    int64_t stores = 0;
    for (int64_t c = 0; c < nchunks; c++) {
        const int64_t r0 = chunk_first[c], r1 = chunk_first[c + 1];
        if (r1 < r0) return -1;
        if (r1 == r0) continue;
        std::vector<int64_t> pk_off((size_t)(r1 - r0));
        int64_t bytes = 0;
        for (int64_t r = r0; r < r1; r++) {
            pk_off[(size_t)(r - r0)] = bytes;
            bytes += ((int64_t)rlen[r] + 3) / 4;
        }
        uint8_t *pk = new uint8_t[(size_t)bytes];  // exact size, no slack
        for (int64_t r = r0; r < r1; r++) memcpy(pk + pk_off[(size_t)(r - r0)], bps + boff[r], (size_t)(((int64_t)rlen[r] + 3) / 4));
        const bl::Chunk ck{pk, pk_off.data(), off.data() + r0, r1 - r0};
        const int64_t w0 = bl::first_window(ck), w1 = bl::end_window(ck);
        for (int64_t wave = w0; wave < w1; wave += 64)
            for (int64_t w = wave; w < std::min(w1, wave + 64); w++) {
                uint32_t v[4];
                if (bl::lane16(ck, w, out, v)) {
                    memcpy(out + w * BL_LANE_BYTES, v, BL_LANE_BYTES);
                    stores++;
                }
            }
        delete[] pk;
    }
    return stores;
}
