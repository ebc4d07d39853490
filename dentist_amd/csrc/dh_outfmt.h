// dh_outfmt.h -- the FASTA text of `dentist output` as a function of the byte position (dh_output_db): the plan a walk of the
// assembly graph leaves behind, and the lane code that formats 16 consecutive bytes of the file from it.  Shared by the kernel
// of dh_outfmt.hip and the CPU harness of tests/native/outfmt_host.cpp.  Driver: dh_outfmt.cpp; the walk: dh_output.cpp.
//
//   record    one FASTA record: its header bytes, literally (hdr[hdr_off[r] .. hdr_off[r + 1])), then its body.  rec_off[r] is
//             the record's first byte in the file, rec_off[nrec] the file's length.
//   body      the bases of the record's segments seg_first[r] .. seg_first[r + 1], wrapped like LineWriter wraps them
//             (dh_output.cpp): with width W > 0 a '\n' behind every W bases and one at the end unless the body ended on a full
//             line (an empty body has no byte at all); with W <= 0 one line and its '\n'.  So the last byte of a body is always
//             '\n', and of the others byte p is '\n' when p % (W + 1) == W, else base p - p / (W + 1).
//   segment   seg_base[s] = number of bases in front of segment s, counted over all records (seg_base[nseg] = all bases; no
//             segment is empty); seg_src[s] = where its FIRST OUTPUT base lies in the buffer of its kind; seg_flags[s] = kind |
//             OF_REV (walk the buffer downwards and complement codes below 4) | OF_UPPER.
#ifndef DH_OUTFMT_H
#define DH_OUTFMT_H

#include <stdint.h>

#if defined(__HIPCC__)
#define OF_HD __host__ __device__ __forceinline__
#else
#define OF_HD inline
#endif

#define OF_BLOCK 256     // threads of a workgroup
#define OF_LANE_BYTES 16 // bytes a lane formats and stores at once

namespace of {
enum : uint32_t { OF_CONTIG = 0, OF_NRUN = 1, OF_CONS = 2, OF_KIND = 3, OF_REV = 4, OF_UPPER = 8 };

struct Plan {
    const int64_t *rec_off;    // nrec + 1
    const int64_t *hdr_off;    // nrec + 1
    const int64_t *seg_first;  // nrec + 1
    const int64_t *seg_base;   // nseg + 1
    const int64_t *seg_src;    // nseg
    const uint32_t *seg_flags; // nseg
    const uint8_t *hdr;        // header bytes of all records
    const uint8_t *contig;     // base codes of the contigs (dh_db::d_bases)
    const uint8_t *cons;       // base codes of the consensus sequences
    int64_t nrec, nseg;
    int32_t width;
};

// bytes a body of nb bases takes in the file
OF_HD int64_t body_bytes(int64_t nb, int32_t width)
{
    if (width <= 0) return nb + 1;
    return nb == 0 ? 0 : nb + (nb + width - 1) / width;
}

// the last i in [lo, hi) with v[i] <= x (v[lo] <= x is given)
OF_HD int64_t last_le(const int64_t *v, int64_t lo, int64_t hi, int64_t x)
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

OF_HD uint8_t letter(uint32_t code, bool upper)
{
    // a c g t n: 0x61 0x63 0x67 0x74 0x6e, one byte each of a 40-bit constant (no table in memory)
    const uint64_t lower = 0x6e74676361ull;
    const uint32_t c = (uint32_t)(lower >> (8 * (code < 4 ? code : 4))) & 0xffu;
    return (uint8_t)(upper ? c - 32 : c);
}

// where a lane stands in the file: the record, the byte inside it, and inside a body the column and the next base
struct Cursor {
    int64_t r, rel, hlen, blen;  // record, byte inside it, bytes of its header and of its body
    int64_t g, s, s_end;         // next base (over all records), its segment, the first base behind that segment
    int32_t col;                 // bases of the current line so far (width > 0)
};

OF_HD void enter_record(const Plan &p, Cursor &c, int64_t r, int64_t rel)
{
    c.r = r;
    c.rel = rel;
    c.hlen = p.hdr_off[r + 1] - p.hdr_off[r];
    const int64_t s0 = p.seg_first[r], s1 = p.seg_first[r + 1];
    const int64_t nb = p.seg_base[s1] - p.seg_base[s0];
    c.blen = body_bytes(nb, p.width);
    c.g = p.seg_base[s0];
    c.s = s0;
    c.col = 0;
    if (rel > c.hlen) {  // inside the body: bases and column of body byte rel - hlen
        const int64_t q = rel - c.hlen;
        if (p.width > 0) {
            const int64_t lines = q / (p.width + 1);
            c.col = (int32_t)(q - lines * (p.width + 1));
            c.g += q - lines;
        } else
            c.g += q;
        if (c.g < p.seg_base[s1]) c.s = last_le(p.seg_base, s0, s1, c.g);
    }
    c.s_end = c.s < p.nseg ? p.seg_base[c.s + 1] : c.g;
}

OF_HD void seek(const Plan &p, Cursor &c, int64_t q)
{
    const int64_t r = last_le(p.rec_off, 0, p.nrec, q);
    enter_record(p, c, r, q - p.rec_off[r]);
}

// the byte under the cursor; the cursor moves one byte on
OF_HD uint8_t next_byte(const Plan &p, Cursor &c)
{
    if (c.rel >= c.hlen + c.blen) enter_record(p, c, c.r + 1, 0);  // (a record has a header: it is never empty)
    const int64_t rel = c.rel++;
    if (rel < c.hlen) return p.hdr[p.hdr_off[c.r] + rel];
    if (rel == c.hlen + c.blen - 1) return (uint8_t)'\n';
    if (p.width > 0 && c.col == p.width) {
        c.col = 0;
        return (uint8_t)'\n';
    }
    c.col++;
    while (c.g >= c.s_end) {  // the linear step: neighbouring bytes share segments
        c.s++;
        c.s_end = p.seg_base[c.s + 1];
    }
    const uint32_t fl = p.seg_flags[c.s];
    const int64_t k = c.g - p.seg_base[c.s];
    c.g++;
    const uint32_t kind = fl & OF_KIND;
    uint32_t code = 4;
    if (kind != OF_NRUN) {
        const uint8_t *buf = kind == OF_CONTIG ? p.contig : p.cons;
        const int64_t at = p.seg_src[c.s] + ((fl & OF_REV) ? -k : k);
        code = buf[at];
        if ((fl & OF_REV) && code < 4) code = 3 - code;
    }
    return letter(code, (fl & OF_UPPER) != 0);
}

// the 16 bytes [q, q + 16) of the file as four little-endian words; bytes at and behind `end` stay zero
OF_HD void lane16(const Plan &p, int64_t q, int64_t end, uint32_t w[4])
{
    Cursor c;
    seek(p, c, q);
    for (int i = 0; i < 4; i++) {
        uint32_t v = 0;
        for (int j = 0; j < 4; j++)
            if (q + 4 * i + j < end) v |= (uint32_t)next_byte(p, c) << (8 * j);
        w[i] = v;
    }
}
}  // namespace of

#endif
