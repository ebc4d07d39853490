// The lane code of dh_output_db's FASTA formatter (dentist_amd/csrc/dh_outfmt.h) compiled for the CPU: a chunk [q0, q1) of the
// file is played as wavefronts of 64 lanes, each lane formatting 16 bytes into a 16-byte aligned chunk buffer -- what
// k_outfmt (dh_outfmt.hip) does on the device.  Test infrastructure (tests/test_outfmt_host.py).
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../dentist_amd/csrc/dh_outfmt.h"

// the whole file through chunks of `chunk` bytes (a multiple of 16, at least 64) into out[0 .. total); returns total, or -1
// for a bad chunk size, -2 when a lane wrote a non-zero byte behind the end of its chunk
extern "C" int64_t of_host_format(const int64_t *rec_off, const int64_t *hdr_off, const int64_t *seg_first, const int64_t *seg_base,
                                  const int64_t *seg_src, const uint32_t *seg_flags, const uint8_t *hdr, const uint8_t *contig,
                                  const uint8_t *cons, int64_t nrec, int64_t nseg, int32_t width, int64_t chunk, uint8_t *out)
{
    if (chunk < 64 || chunk % 16) return -1;
    of::Plan p;
    memset(&p, 0, sizeof(p));
    p.rec_off = rec_off;
    p.hdr_off = hdr_off;
    p.seg_first = seg_first;
    p.seg_base = seg_base;
    p.seg_src = seg_src;
    p.seg_flags = seg_flags;
    p.hdr = hdr;
    p.contig = contig;
    p.cons = cons;
    p.nrec = nrec;
    p.nseg = nseg;
    p.width = width;
    const int64_t total = nrec > 0 ? rec_off[nrec] : 0;
    std::vector<uint32_t> buf;
    for (int64_t q0 = 0; q0 < total; q0 += chunk) {
        const int64_t q1 = std::min(total, q0 + chunk);
        const int64_t lanes = (q1 - q0 + OF_LANE_BYTES - 1) / OF_LANE_BYTES;
        buf.assign((size_t)lanes * 4, 0xffffffffu);
        for (int64_t wave = 0; wave * 64 < lanes; wave++)
            for (int64_t lane = wave * 64; lane < std::min(lanes, wave * 64 + 64); lane++)
                of::lane16(p, q0 + lane * OF_LANE_BYTES, q1, buf.data() + 4 * lane);
        const uint8_t *b = (const uint8_t *)buf.data();
        for (int64_t x = q1 - q0; x < lanes * OF_LANE_BYTES; x++)
            if (b[x] != 0) return -2;
        memcpy(out + q0, b, (size_t)(q1 - q0));
    }
    return total;
}
