// dh_chainpad.h -- lane code of the chain padder's plan (k_cp_plan, dh_chainpad.hip): AlignmentPadder (dazzler.d:2249-2607)
// restated over a whole chain.  One lane walks the records of one chain and emits its segments in order: runs of whole trace
// tiles of a record, and fillers (an A range against a B range) between a record p and the next record q.  The plan reads
// records and trace values only, never bases or ops.  Compiles for the host as well (tests/native/chainpad_host.cpp), so that
// the CPU tests run the very expressions the kernel runs.
//
// Trace points.  Record r with nt tiles has the points 0 .. nt: point 0 = (abpos, bbpos), point i = (min((abpos / ts + i) ts,
// aepos), bbpos + the B bases of tiles 0 .. i - 1), point nt = (aepos, bepos).  translate(pos, floor) is the last point whose
// coordinate is <= pos, translate(pos, ceil) the first whose coordinate is >= pos, on either sequence; a position in front of
// the record gives point 0, one behind it point nt.
//
// Junction of p (whose tile run starts at point s) and q:
//   gap      p.aepos <= q.abpos and p.bepos <= q.bbpos: p keeps tiles [s, nt), the filler is A [p.aepos, q.abpos) x B [p.bepos,
//            q.bbpos), q starts at its point 0.
//   overlap  anything else (getNonOverlappingCoordinates, :2512-2560): on every sequence X that overlaps, begin_X =
//            p.translate_X(q.Xbpos, floor) and end_X = q.translate_X(p.Xepos, ceil); of two, begin is the one with the smaller A
//            and end the one with the larger A (the A resolution on a tie).  p keeps tiles [s, begin), the filler is A [begin.A,
//            end.A) x B [begin.B, end.B), q starts at point end.
//   A filler without bases and a run without tiles are no segments.
// DH_CP_NESTED: begin < s, end.A < begin.A or end.B < begin.B -- the reference's cleanUpLocalAlignments / path cropping would
// cut into earlier material there; the walk stops and the chain has no segments.
#ifndef DH_CHAINPAD_H
#define DH_CHAINPAD_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CP_HD __host__ __device__ __forceinline__
#else
#define CP_HD inline
#endif

#define CP_OK 0
#define CP_FAKED 1
#define CP_NESTED 2

#define CP_SEG_TILES 0
#define CP_SEG_FILLER 1

struct CpRec {           // one record of a launch group
    int64_t aoff, boff;  // first base of its A read in the A bases / of its B read in the B bases (either copy)
    int64_t toff;        // its first trace value (diffs, B bases per tile) in the group's trace values
    int32_t abpos, aepos, bbpos, bepos;
    int32_t nt, comp;
};

struct CpFill {          // one filler
    int64_t aoff, boff;  // first base in the A bases / in the B bases (forward or reverse-complement copy)
    int32_t la, lb;
    int32_t comp, chain;  // chain: of the launch group
};

struct CpSeg {  // one segment of a chain, in path order
    int32_t kind;
    int32_t first;  // CP_SEG_TILES: first tile among the group's tiles; CP_SEG_FILLER: the filler among the group's fillers
    int32_t count;  // tiles (1 for a filler)
};

namespace cp {

struct Point {
    int32_t idx, a, b;
};

CP_HD int32_t point_a(const CpRec &r, int32_t ts, int32_t i)
{
    if (i <= 0) return r.abpos;
    const int64_t a = ((int64_t)(r.abpos / ts) + i) * ts;
    return i >= r.nt || a > r.aepos ? r.aepos : (int32_t)a;
}

// the trace point `i` of a record: its B coordinate is a walk over the trace
CP_HD Point point_at(const CpRec &r, const uint16_t *tr, int32_t ts, int32_t i)
{
    int32_t b = r.bbpos;
    for (int32_t t = 0; t < i; t++) b += tr[r.toff + 2 * t + 1];
    return Point{i, point_a(r, ts, i), b};
}

// onb: the position is one of B.  mode 0 = floor, 1 = ceil
CP_HD Point translate(const CpRec &r, const uint16_t *tr, int32_t ts, int32_t pos, int onb, int mode)
{
    Point cur{0, r.abpos, r.bbpos}, best = cur;
    bool found = false;
    for (int32_t i = 0;; i++) {
        const int32_t c = onb ? cur.b : cur.a;
        if (mode == 0) {
            if (c <= pos) best = cur;  // (the last one wins)
        } else if (!found && c >= pos) {
            best = cur;
            found = true;
        }
        if (i == r.nt) break;
        cur.b += tr[r.toff + 2 * i + 1];
        cur.idx = i + 1;
        cur.a = point_a(r, ts, i + 1);
    }
    if (mode == 1 && !found) best = cur;  // behind the record: its last point
    return best;
}

struct Junction {
    int32_t status;      // CP_OK or CP_NESTED
    int32_t p_end;       // p keeps tiles [s, p_end)
    int32_t q_start;     // q starts at this point
    int32_t a0, a1, b0, b1;  // the filler
};

CP_HD Junction junction(const CpRec &p, const CpRec &q, const uint16_t *tr, int32_t ts, int32_t s)
{
    Junction j;
    j.status = CP_OK;
    if (p.aepos <= q.abpos && p.bepos <= q.bbpos) {
        j.p_end = p.nt;
        j.q_start = 0;
        j.a0 = p.aepos;
        j.a1 = q.abpos;
        j.b0 = p.bepos;
        j.b1 = q.bbpos;
        return j;
    }
    const bool ova = p.aepos > q.abpos, ovb = p.bepos > q.bbpos;
    Point begin{0, 0, 0}, end{0, 0, 0};
    if (ova) {
        begin = translate(p, tr, ts, q.abpos, 0, 0);
        end = translate(q, tr, ts, p.aepos, 0, 1);
    }
    if (ovb) {
        const Point bb = translate(p, tr, ts, q.bbpos, 1, 0), eb = translate(q, tr, ts, p.bepos, 1, 1);
        if (!ova || bb.a < begin.a) begin = bb;
        if (!ova || eb.a > end.a) end = eb;
    }
    j.p_end = begin.idx;
    j.q_start = end.idx;
    j.a0 = begin.a;
    j.a1 = end.a;
    j.b0 = begin.b;
    j.b1 = end.b;
    if (begin.idx < s || end.a < begin.a || end.b < begin.b) j.status = CP_NESTED;
    return j;
}

// The segments of the chain of records [r0, r1), in path order: out.tiles(record, first tile, end tile) and out.filler(record
// p, a0, a1, b0, b1).  Returns CP_OK or CP_NESTED; after CP_NESTED whatever was emitted is void.
template <class Out>
CP_HD int32_t walk_chain(const CpRec *recs, const uint16_t *tr, int32_t ts, int64_t r0, int64_t r1, Out &out)
{
    int32_t s = 0;
    for (int64_t k = r0; k < r1; k++) {
        const CpRec &p = recs[k];
        if (k + 1 == r1) {
            if (p.nt > s) out.tiles(k, s, p.nt);
            break;
        }
        const Junction j = junction(p, recs[k + 1], tr, ts, s);
        if (j.status != CP_OK) return j.status;
        if (j.p_end > s) out.tiles(k, s, j.p_end);
        if (j.a1 > j.a0 || j.b1 > j.b0) out.filler(k, j.a0, j.a1, j.b0, j.b1);
        s = j.q_start;
    }
    return CP_OK;
}

// what a generated filler is: |la - lb| indels (insertions when A is the shorter side), then min(la, lb) columns by
// comparing the bases ("faking too long alignment gap", dazzler.d:2450-2474); a filler with an empty side is all indels
CP_HD uint8_t generated_op(const uint8_t *a, const uint8_t *b, int32_t la, int32_t lb, int32_t p)
{
    const int32_t nind = la > lb ? la - lb : lb - la;
    if (p < nind) return la < lb ? 2 : 1;
    const int32_t i = p - nind;
    const uint8_t x = a[(la > lb ? nind : 0) + i], y = b[(lb > la ? nind : 0) + i];
    return x == y ? 0 : 3;
}

}  // namespace cp

#endif
