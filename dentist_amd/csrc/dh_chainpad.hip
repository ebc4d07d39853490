// dh_chainpad.hip -- the chain padder (AlignmentPadder, dazzler.d:2249-2607): the base-level alignment of whole chains from
// the ops of their trace tiles (k_edit_fast / k_edit_general) and of the fillers between their records (k_nw, free shift).
// gfx950, wave64.
//
//   k_cp_plan    one lane per chain, run twice over the lane code of dh_chainpad.h.  The first run counts the chain's segments,
//                tiles and fillers and decides its status; dhk_scan_total turns the counts into offsets; the second run writes
//                the segments, an EpTile per tile of a run (what cut_record makes of the record, dh_editpath.cpp) and a CpFill
//                per filler.  A lane's work is a walk over the trace values of its records: latency, no arithmetic.
//   k_cp_stitch  one wavefront per chain, run twice.  The op lengths of 64 segments at a time are scanned across the lanes, with
//                a wave-uniform carry from chunk to chunk; then the wavefront copies segment after segment into the chain's slot,
//                lane l the bytes l, l + 64, ...: every load and store of the wavefront is one contiguous run of bytes.  A filler
//                the global-alignment kernel gave up on, and one with an empty side, is generated in place (cp::generated_op).
//                The first run only leaves the chain's length; the second copies and counts the non-zero ops into `score`.
#include <hip/hip_runtime.h>

#include "dh_chainpad.h"
#include "dh_editpath.h"
#include "dh_scan.h"

namespace {

struct CountOut {
    uint32_t nseg = 0, ntile = 0, nfill = 0;
    __device__ void tiles(int64_t, int32_t t0, int32_t t1)
    {
        nseg++;
        ntile += (uint32_t)(t1 - t0);
    }
    __device__ void filler(int64_t, int32_t, int32_t, int32_t, int32_t)
    {
        nseg++;
        nfill++;
    }
};

struct WriteOut {
    const CpRec *recs;
    const uint16_t *tr;
    int32_t ts, chain;
    CpSeg *seg;     // the chain's first segment
    EpTile *tile;   // the group's tiles
    CpFill *fill;   // the group's fillers
    uint32_t at_tile, at_fill;
    __device__ void tiles(int64_t k, int32_t t0, int32_t t1)
    {
        const CpRec &r = recs[k];
        *seg++ = CpSeg{CP_SEG_TILES, (int32_t)at_tile, t1 - t0};
        cp::Point p = cp::point_at(r, tr, ts, t0);
        for (int32_t t = t0; t < t1; t++) {
            const int32_t a1 = cp::point_a(r, ts, t + 1), b1 = p.b + tr[r.toff + 2 * t + 1];
            EpTile tl;
            tl.aoff = r.aoff + p.a;
            tl.boff = r.boff + p.b;
            tl.rl = a1 - p.a;
            tl.ql = b1 - p.b;
            tl.diffs = tr[r.toff + 2 * t];
            tl.comp = r.comp;
            tile[at_tile++] = tl;
            p.a = a1;
            p.b = b1;
        }
    }
    __device__ void filler(int64_t k, int32_t a0, int32_t a1, int32_t b0, int32_t b1)
    {
        const CpRec &r = recs[k];
        *seg++ = CpSeg{CP_SEG_FILLER, (int32_t)at_fill, 1};
        fill[at_fill++] = CpFill{r.aoff + a0, r.boff + b0, a1 - a0, b1 - b0, r.comp, chain};
    }
};

}  // namespace

// write == 0: cnt_* [c] = the chain's counts, status[c]; write != 0: cnt_* hold the exclusive scans of those counts
__global__ void __launch_bounds__(64)
k_cp_plan(const CpRec *__restrict__ recs, const uint16_t *__restrict__ tr, int32_t ts, const int32_t *__restrict__ chain_off,
          int32_t nchains, int32_t write, uint32_t *__restrict__ cnt_seg, uint32_t *__restrict__ cnt_tile,
          uint32_t *__restrict__ cnt_fill, int32_t *__restrict__ status, CpSeg *__restrict__ segs, EpTile *__restrict__ tiles,
          CpFill *__restrict__ fills)
{
    const int32_t c = blockIdx.x * 64 + threadIdx.x;
    if (c >= nchains) return;
    const int64_t r0 = chain_off[c], r1 = chain_off[c + 1];
    if (!write) {
        CountOut o;
        const int32_t s = cp::walk_chain(recs, tr, ts, r0, r1, o);
        const bool ok = s == CP_OK;
        cnt_seg[c] = ok ? o.nseg : 0u;
        cnt_tile[c] = ok ? o.ntile : 0u;
        cnt_fill[c] = ok ? o.nfill : 0u;
        status[c] = s;
        return;
    }
    if (status[c] != CP_OK) return;
    WriteOut o{recs, tr, ts, c, segs + cnt_seg[c], tiles, fills, cnt_tile[c], cnt_fill[c]};
    cp::walk_chain(recs, tr, ts, r0, r1, o);
}

// seg_off: nchains + 1 (exclusive scan of the segment counts); tile_op: first op of every tile of the group in tile_ops (ntiles + 1);
// fill_src[f]: first op of filler f in fill_ops, or -1 for a generated one; fill_nops[f] its length.
// copy == 0: len[c] = ops of the chain.  copy != 0: len holds the exclusive scan of the lengths, the ops go to out, score[c] =
// the non-zero ones.
__global__ void __launch_bounds__(64)
k_cp_stitch(const CpSeg *__restrict__ segs, const uint32_t *__restrict__ seg_off, int32_t nchains,
            const int64_t *__restrict__ tile_op, const uint8_t *__restrict__ tile_ops, const CpFill *__restrict__ fills,
            const int64_t *__restrict__ fill_src, const int32_t *__restrict__ fill_nops, const uint8_t *__restrict__ fill_ops,
            const uint8_t *__restrict__ abases, const uint8_t *__restrict__ bfwd, const uint8_t *__restrict__ brc, int32_t copy,
            uint32_t *__restrict__ len, uint8_t *__restrict__ out, int32_t *__restrict__ score)
{
    const int32_t c = blockIdx.x, lane = threadIdx.x;
    if (c >= nchains) return;
    const uint32_t s0 = seg_off[c], s1 = seg_off[c + 1];
    uint8_t *dst = copy ? out + len[c] : nullptr;
    int32_t carry = 0, nz = 0;  // carry: ops of the chunks in front, wave-uniform
    for (uint32_t sb = s0; sb < s1; sb += 64) {
        const bool have = sb + lane < s1;
        const CpSeg sg = have ? segs[sb + lane] : CpSeg{CP_SEG_TILES, 0, 0};
        int32_t n = 0;
        int64_t src = -1;  // in tile_ops / fill_ops
        if (have && sg.kind == CP_SEG_TILES) {
            src = tile_op[sg.first];
            n = (int32_t)(tile_op[sg.first + sg.count] - src);
        } else if (have) {
            src = fill_src[sg.first];
            n = fill_nops[sg.first];
        }
        const int32_t incl = wave_incl_scan<ScanSum>(n, lane);
        if (copy) {
            const int32_t cnt = (int32_t)min(64u, s1 - sb);
            for (int32_t k = 0; k < cnt; k++) {  // segment after segment, the whole wavefront on each
                const int32_t kn = __shfl(n, k, 64), kat = carry + __shfl(incl, k, 64) - kn;
                const int64_t ksrc = (int64_t)__shfl((long long)src, k, 64);
                const int32_t kkind = __shfl(sg.kind, k, 64), kfirst = __shfl(sg.first, k, 64);
                if (kkind == CP_SEG_TILES || ksrc >= 0) {
                    const uint8_t *from = (kkind == CP_SEG_TILES ? tile_ops : fill_ops) + ksrc;
                    for (int32_t p = lane; p < kn; p += 64) {
                        const uint8_t op = from[p];
                        dst[kat + p] = op;
                        nz += op != 0;
                    }
                } else {
                    const CpFill f = fills[kfirst];
                    const uint8_t *a = abases + f.aoff, *b = (f.comp ? brc : bfwd) + f.boff;
                    for (int32_t p = lane; p < kn; p += 64) {
                        const uint8_t op = cp::generated_op(a, b, f.la, f.lb, p);
                        dst[kat + p] = op;
                        nz += op != 0;
                    }
                }
            }
        }
        carry += __shfl(incl, 63, 64);
    }
    if (!copy) {
        if (lane == 0) len[c] = (uint32_t)carry;
        return;
    }
    const int32_t total = wave_incl_scan<ScanSum>(nz, lane);
    if (lane == 63) score[c] = total;
}

extern "C" void dhk_cp_plan(hipStream_t st, const CpRec *recs, const uint16_t *tr, int32_t ts, const int32_t *chain_off, int32_t nchains,
                            int32_t write, uint32_t *cnt_seg, uint32_t *cnt_tile, uint32_t *cnt_fill, int32_t *status, CpSeg *segs,
                            EpTile *tiles, CpFill *fills)
{
    if (nchains <= 0) return;
    hipLaunchKernelGGL(k_cp_plan, dim3((uint32_t)((nchains + 63) / 64)), dim3(64), 0, st, recs, tr, ts, chain_off, nchains, write, cnt_seg,
                       cnt_tile, cnt_fill, status, segs, tiles, fills);
}

extern "C" void dhk_cp_stitch(hipStream_t st, const CpSeg *segs, const uint32_t *seg_off, int32_t nchains, const int64_t *tile_op,
                              const uint8_t *tile_ops, const CpFill *fills, const int64_t *fill_src, const int32_t *fill_nops,
                              const uint8_t *fill_ops, const uint8_t *abases, const uint8_t *bfwd, const uint8_t *brc, int32_t copy,
                              uint32_t *len, uint8_t *out, int32_t *score)
{
    if (nchains <= 0) return;
    hipLaunchKernelGGL(k_cp_stitch, dim3((uint32_t)nchains), dim3(64), 0, st, segs, seg_off, nchains, tile_op, tile_ops, fills, fill_src,
                       fill_nops, fill_ops, abases, bfwd, brc, copy, len, out, score);
}
