// dh_dazzfmt.h -- what dazzdb.cpp (dh_dazz_open) and dh_bpsload.cpp (dh_dazz_load_reads) share about a DAZZ_DB on disk: the
// images of its .idx, the stub and .idx of a path read into a view, and the rule that decides which reads the trimmed view
// shows.  Host only.
#ifndef DH_DAZZFMT_H
#define DH_DAZZFMT_H

#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#define DB_QV 0x03ff
#define DB_CCS 0x0400
#define DB_BEST 0x0800
#define DB_ALL 0x1

#pragma pack(push, 1)
struct DazzHeader {  // image of struct DAZZ_DB as fwrite()n by fasta2DB/fasta2DAM, 112 bytes
    int32_t ureads, treads, cutoff, allarr;
    float freq[4];
    int32_t maxlen, pad0;
    int64_t totlen;
    int32_t nreads, trimmed, part, ufirst, tfirst, pad1;
    int64_t path;
    int32_t loaded, pad2;
    int64_t bases, reads, tracks;
};
struct DazzRead {  // struct DAZZ_READ, 40 bytes
    int32_t origin, rlen, fpulse, pad0;
    int64_t boff, coff;
    int32_t flags, pad1;
};
#pragma pack(pop)
static_assert(sizeof(DazzHeader) == 112, "DAZZ_DB image");
static_assert(sizeof(DazzRead) == 40, "DAZZ_READ image");

// the stub and the .idx of a DB or of one block of it ("name.3"); no byte of the .bps is touched
struct DazzView {
    std::string stub, root, bps_path, hdr_path;
    bool is_dam = false;
    DazzHeader h;
    std::vector<DazzRead> reads;                        // all h.ureads of them
    std::vector<std::pair<int, std::string>> prologs;  // (cumulative read count, prolog) per input file
    int ulo = 0, uhi = 0;                               // untrimmed ids of the path's block (the whole DB without one)
    int tfirst = 0;                                     // trimmed id of the view's first read
    // the trim rule: reads shorter than the cutoff and, for a .db split without -a, reads that are not the best of their
    // well are invisible
    bool keep(const DazzRead &r) const { return r.rlen >= h.cutoff && (is_dam || (h.allarr & DB_ALL) || (r.flags & DB_BEST)); }
};
int dh_dazz_view_open(const char *path, DazzView &v);

#endif
