// dh_chainpad.cpp -- host side of the chain padder (dh_la_chain_paths, dh_la_set_chain_paths): the base-level alignment of
// whole chains (AlignmentPadder, dazzler.d:2249-2607).  The kernels are in dh_chainpad.hip, the plan's lane code in
// dh_chainpad.h.
//
// A call validates every record and every chain on the host, then runs the chains in launch groups of whole chains whose
// records have DH_EDIT_CHUNK tiles at most (a larger chain on its own).  Per group: k_cp_plan counts and, behind the device
// scan, writes segments, tiles and fillers; the tiles go through the edit-path kernels (dh_ep_run_tiles: their ops stay on the
// device), the fillers with two non-empty sides through the global-alignment kernel under dh_nw.cpp's widening protocol
// (dh_nw_run_pairs, straight from the DBs' bases, launch groups bounded by DH_NW_CHUNK_KB); k_cp_stitch puts the ops of every
// chain in path order and counts its score.  The result does not depend on either knob.
//
// Deviation from the reference: cleanUpLocalAlignments (findTilings) is not restated.  dh_la_chain's max_relative_overlap
// keeps nested records out of its chains; a junction that would cut into earlier material is reported as DH_CP_NESTED, not
// guessed.
#include "dh_host.h"

#include <stdio.h>
#include <string.h>

#include "dh_chainpad.h"
#include "dh_nw.h"

extern "C" void dhk_cp_plan(hipStream_t st, const CpRec *recs, const uint16_t *tr, int32_t ts, const int32_t *chain_off, int32_t nchains,
                            int32_t write, uint32_t *cnt_seg, uint32_t *cnt_tile, uint32_t *cnt_fill, int32_t *status, CpSeg *segs,
                            EpTile *tiles, CpFill *fills);
extern "C" void dhk_cp_stitch(hipStream_t st, const CpSeg *segs, const uint32_t *seg_off, int32_t nchains, const int64_t *tile_op,
                              const uint8_t *tile_ops, const CpFill *fills, const int64_t *fill_src, const int32_t *fill_nops,
                              const uint8_t *fill_ops, const uint8_t *abases, const uint8_t *bfwd, const uint8_t *brc, int32_t copy,
                              uint32_t *len, uint8_t *out, int32_t *score);

static_assert(DB_PAD >= NW_SEQ_PAD, "k_nw reads the fillers where they lie in the DBs' bases: its padding must be there");
static_assert(CP_OK == DH_CP_OK && CP_FAKED == DH_CP_FAKED && CP_NESTED == DH_CP_NESTED, "the header states the plan's codes");

namespace {

struct CpCall {
    dh_ctx *ctx;
    dh_db *A, *B;
    const dh_la *las;
    const uint16_t *trace;
    int32_t ts;
    const std::vector<int64_t> *off;  // nchains + 1
    dh_edit_paths *out;
    std::vector<int32_t> *status;
};

// chains [c0, c1) as one launch group
int run_group(const CpCall &c, int64_t c0, int64_t c1)
{
    dh_ctx *ctx = c.ctx;
    hipStream_t st = ctx->stream;
    const std::vector<int64_t> &off = *c.off;
    const int64_t r0 = off[(size_t)c0], r1 = off[(size_t)c1];
    const size_t nrec = (size_t)(r1 - r0), nch = (size_t)(c1 - c0);
    // ---- the group's records, trace values and record ranges
    std::vector<CpRec> recs(nrec);
    std::vector<uint16_t> tr;
    for (size_t i = 0; i < nrec; i++) {
        const dh_la &la = c.las[r0 + (int64_t)i];
        CpRec &r = recs[i];
        r.aoff = c.A->h_off[(size_t)la.aread];
        r.boff = c.B->h_off[(size_t)la.bread];
        r.toff = (int64_t)tr.size();
        r.abpos = la.abpos;
        r.aepos = la.aepos;
        r.bbpos = la.bbpos;
        r.bepos = la.bepos;
        r.nt = la.tlen / 2;
        r.comp = (la.flags & DH_FLAG_COMP) ? 1 : 0;
        tr.insert(tr.end(), c.trace + la.toff, c.trace + la.toff + la.tlen);
    }
    std::vector<int32_t> coff(nch + 1);
    for (size_t k = 0; k <= nch; k++) coff[k] = (int32_t)(off[(size_t)c0 + k] - r0);
    CpRec *d_recs;
    uint16_t *d_tr;
    int32_t *d_coff, *d_status;
    uint32_t *d_nseg, *d_ntile, *d_nfill, *d_sums, *d_len;
    unsigned long long *d_total;
    if (int rc = dh_upload(ctx, SLOT_CP_RECS, recs, &d_recs)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CP_TRACE, tr, &d_tr)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CP_CHAIN_OFF, coff, &d_coff)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_NSEG, nch + 1, &d_nseg)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_NTILE, nch + 1, &d_ntile)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_NFILL, nch + 1, &d_nfill)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_LEN, nch + 1, &d_len)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_STATUS, nch, &d_status)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_SUMS, (nch + 1 + 2047) / 2048, &d_sums)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_TOTAL, 4, &d_total)) return rc;
    HIPCHK(hipMemsetAsync(d_nseg + nch, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(d_ntile + nch, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(d_nfill + nch, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(d_len + nch, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(d_total, 0, 4 * sizeof(unsigned long long), st));
    // ---- the plan: counts, their scans, then segments, tiles and fillers
    dhk_cp_plan(st, d_recs, d_tr, c.ts, d_coff, (int32_t)nch, 0, d_nseg, d_ntile, d_nfill, d_status, nullptr, nullptr, nullptr);
    dhk_scan_total(st, d_nseg, (int64_t)nch + 1, d_sums, d_total);
    dhk_scan_total(st, d_ntile, (int64_t)nch + 1, d_sums, d_total + 1);
    dhk_scan_total(st, d_nfill, (int64_t)nch + 1, d_sums, d_total + 2);
    HIPCHK(hipGetLastError());
    unsigned long long total[3];
    std::vector<int32_t> status(nch);
    HIPCHK(hipMemcpyAsync(total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status.data(), d_status, sizeof(int32_t) * nch, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int k = 0; k < 3; k++)
        if (total[k] > (unsigned long long)INT32_MAX) return dh_fail(DH_EOVERFLOW, "dh_la_chain_paths: more than 2^31 - 1 segments in a launch group");
    const size_t nseg = (size_t)total[0], ntile = (size_t)total[1], nfill = (size_t)total[2];
    CpSeg *d_segs;
    EpTile *d_tiles;
    CpFill *d_fills;
    if (int rc = dh_scr(ctx, SLOT_CP_SEGS, nseg, &d_segs)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_TILES, ntile, &d_tiles)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_FILLS, nfill, &d_fills)) return rc;
    dhk_cp_plan(st, d_recs, d_tr, c.ts, d_coff, (int32_t)nch, 1, d_nseg, d_ntile, d_nfill, d_status, d_segs, d_tiles, d_fills);
    HIPCHK(hipGetLastError());
    std::vector<EpTile> tiles(ntile);
    std::vector<CpFill> fills(nfill);
    if (ntile) HIPCHK(hipMemcpyAsync(tiles.data(), d_tiles, sizeof(EpTile) * ntile, hipMemcpyDeviceToHost, st));
    if (nfill) HIPCHK(hipMemcpyAsync(fills.data(), d_fills, sizeof(CpFill) * nfill, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    // ---- the tiles: their ops stay on the device, tile after tile
    std::vector<int64_t> tile_op(ntile + 1, 0);
    const uint8_t *d_tile_ops = nullptr;
    if (ntile) {
        std::vector<EpResult> res(ntile);
        if (int rc = dh_ep_run_tiles(ctx, c.A, c.B, c.ts, tiles, 0, ntile, res, c.out, &d_tile_ops)) return rc;
        for (size_t t = 0; t < ntile; t++) tile_op[t + 1] = tile_op[t] + res[t].nops;
    }
    // ---- the fillers: forward and COMP ones apart (one query buffer per launch); what the kernel gives up on, what exceeds its
    // length limit and what has an empty side is generated by the stitch
    std::vector<DhNwSeq> seq(nfill);
    std::vector<DhNwPairOut> po(nfill);
    std::vector<uint8_t> stage;
    std::vector<int64_t> todo[2];
    for (size_t f = 0; f < nfill; f++) {
        const CpFill &fl = fills[f];
        seq[f] = DhNwSeq{fl.aoff, fl.boff, fl.la, fl.lb};
        if (fl.la > 0 && fl.lb > 0 && fl.la <= NW_MAX_LEN && fl.lb <= NW_MAX_LEN) todo[fl.comp ? 1 : 0].push_back((int64_t)f);
    }
    for (int k = 0; k < 2; k++)
        if (!todo[k].empty())
            if (int rc = dh_nw_run_pairs(ctx, c.A->d_bases, k ? c.B->d_rc : c.B->d_bases, seq.data(), todo[k], 1, po, stage)) return rc;
    std::vector<int64_t> fill_src(nfill);
    std::vector<int32_t> fill_nops(nfill);
    for (size_t f = 0; f < nfill; f++) {
        const CpFill &fl = fills[f];
        const bool empty_side = fl.la == 0 || fl.lb == 0;
        const bool aligned = !empty_side && fl.la <= NW_MAX_LEN && fl.lb <= NW_MAX_LEN && po[f].status == DH_NW_OK;
        fill_src[f] = aligned ? po[f].at : -1;
        fill_nops[f] = aligned ? po[f].nops : (empty_side ? fl.la + fl.lb : std::max(fl.la, fl.lb));
        if (aligned) {
            c.out->fillers++;
            c.out->entry_fillers[(size_t)c0 + (size_t)fl.chain]++;
        } else if (!empty_side)
            status[(size_t)fl.chain] = CP_FAKED;
    }
    // ---- the stitch: lengths, their scan, then the ops and scores
    int64_t *d_tile_op, *d_fill_src;
    int32_t *d_fill_nops, *d_score;
    uint8_t *d_fill_ops, *d_out;
    if (int rc = dh_upload(ctx, SLOT_CP_TILE_OP, tile_op, &d_tile_op)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CP_FILL_SRC, fill_src, &d_fill_src)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CP_FILL_NOPS, fill_nops, &d_fill_nops)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CP_FILL_OPS, stage, &d_fill_ops)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CP_SCORE, nch, &d_score)) return rc;
    const uint8_t *ab = c.A->d_bases, *bf = c.B->d_bases, *brc = c.B->d_rc;
    dhk_cp_stitch(st, d_segs, d_nseg, (int32_t)nch, d_tile_op, d_tile_ops, d_fills, d_fill_src, d_fill_nops, d_fill_ops, ab, bf, brc, 0,
                  d_len, nullptr, nullptr);
    dhk_scan_total(st, d_len, (int64_t)nch + 1, d_sums, d_total + 3);
    HIPCHK(hipGetLastError());
    unsigned long long nops = 0;
    std::vector<uint32_t> len(nch + 1);
    HIPCHK(hipMemcpyAsync(&nops, d_total + 3, sizeof(nops), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(len.data(), d_len, sizeof(uint32_t) * (nch + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (nops > (unsigned long long)UINT32_MAX) return dh_fail(DH_EOVERFLOW, "dh_la_chain_paths: more than 2^32 - 1 ops in a launch group");
    if (int rc = dh_scr(ctx, SLOT_CP_OUT, (size_t)nops, &d_out)) return rc;
    dhk_cp_stitch(st, d_segs, d_nseg, (int32_t)nch, d_tile_op, d_tile_ops, d_fills, d_fill_src, d_fill_nops, d_fill_ops, ab, bf, brc, 1,
                  d_len, d_out, d_score);
    HIPCHK(hipGetLastError());
    dh_edit_paths *p = c.out;
    const size_t at = p->ops.size();
    p->ops.resize(at + (size_t)nops);
    if (nops) HIPCHK(hipMemcpyAsync(p->ops.data() + at, d_out, (size_t)nops, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(p->score.data() + c0, d_score, sizeof(int32_t) * nch, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < nch; k++) {
        const size_t ci = (size_t)c0 + k;
        p->op_off[ci + 1] = p->op_off[ci] + (int64_t)(len[k + 1] - len[k]);
        if (status[k] == CP_NESTED) p->score[ci] = -1;
        (*c.status)[ci] = status[k];
    }
    return DH_OK;
}

int chain_paths_impl(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace, int64_t trace_len, int32_t ts,
                     const int64_t *chain_off, int64_t nchains, dh_edit_paths **out, int32_t *status)
{
    if (!ctx || !A || !B || !out || n < 0 || (n > 0 && (!las || !trace)) || (chain_off && nchains < 0))
        return dh_fail(DH_EINVAL, "dh_la_chain_paths: bad argument");
    if (ts < 1 || ts > EP_TSPACE_MAX) return dh_fail(DH_EINVAL, "dh_la_chain_paths: tspace must be in [1, 250]");
    *out = nullptr;
    char msg[256];
    // ---- the chains as record ranges
    std::vector<int64_t> off;
    if (chain_off) {
        off.assign(chain_off, chain_off + nchains + 1);
        if (off[0] != 0) return dh_fail(DH_EINVAL, "dh_la_chain_paths: chain_off does not start at 0");
        for (int64_t i = 0; i < nchains; i++)
            if (off[(size_t)i + 1] <= off[(size_t)i]) {
                snprintf(msg, sizeof(msg), "dh_la_chain_paths: chain %lld is empty or its offsets decrease", (long long)i);
                return dh_fail(DH_EINVAL, msg);
            }
        if (off[(size_t)nchains] > n) return dh_fail(DH_EINVAL, "dh_la_chain_paths: chain_off ends past the records");
    } else {
        for (int64_t i = 0; i < n; i++)
            if (i == 0 || !(las[i].flags & DH_FLAG_NEXT)) off.push_back(i);
        off.push_back(n);
        nchains = (int64_t)off.size() - 1;
    }
    // ---- validation on the host, before anything is launched: every record as dh_la_edit_paths validates it, every chain
    std::vector<int64_t> tiles_to((size_t)nchains + 1, 0);  // tiles of the records of the chains in front
    {
        std::vector<EpTile> scratch;
        for (int64_t ci = 0; ci < nchains; ci++) {
            for (int64_t i = off[(size_t)ci]; i < off[(size_t)ci + 1]; i++) {
                scratch.clear();
                if (int rc = dh_ep_check_record(A, B, las[i], i, trace, trace_len, ts, scratch)) return rc;
                if (i == off[(size_t)ci]) continue;
                const dh_la &f = las[off[(size_t)ci]], &p = las[i - 1], &q = las[i];
                if (q.aread != f.aread || q.bread != f.bread || ((q.flags ^ f.flags) & DH_FLAG_COMP)) {
                    snprintf(msg, sizeof(msg), "dh_la_chain_paths: LA %lld: not the reads or the strand of its chain's first record", (long long)i);
                    return dh_fail(DH_EINVAL, msg);
                }
                if (q.abpos < p.abpos) {
                    snprintf(msg, sizeof(msg), "dh_la_chain_paths: LA %lld: abpos %d decreases within its chain", (long long)i, q.abpos);
                    return dh_fail(DH_EINVAL, msg);
                }
            }
            int64_t nt = 0;
            for (int64_t i = off[(size_t)ci]; i < off[(size_t)ci + 1]; i++) nt += las[i].tlen / 2;
            tiles_to[(size_t)ci + 1] = tiles_to[(size_t)ci] + nt;
        }
    }
    std::unique_ptr<dh_edit_paths> p(new dh_edit_paths);
    p->score.assign((size_t)nchains, 0);
    p->op_off.assign((size_t)nchains + 1, 0);
    p->tile_off.assign((size_t)nchains + 1, 0);
    p->entry_fillers.assign((size_t)nchains, 0);
    std::vector<int32_t> st((size_t)nchains, CP_OK);
    if (nchains > 0) {
        HIPCHK(hipSetDevice(ctx->device));
        if (int rc = dh_ensure_rc(B)) return rc;
        const int64_t chunk = (int64_t)dh_ep_chunk_tiles();
        const CpCall c{ctx, A, B, las, trace, ts, &off, p.get(), &st};
        for (int64_t c0 = 0, c1; c0 < nchains; c0 = c1) {
            c1 = c0 + 1;
            while (c1 < nchains && tiles_to[(size_t)c1 + 1] - tiles_to[(size_t)c0] <= chunk && off[(size_t)c1 + 1] - off[(size_t)c0] < INT32_MAX) c1++;
            if (int rc = run_group(c, c0, c1)) return rc;
        }
    }
    if (status)
        for (int64_t i = 0; i < nchains; i++) status[i] = st[(size_t)i];
    *out = p.release();
    return DH_OK;
}

}  // namespace

extern "C" int dh_la_chain_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace, int32_t tspace,
                                 const int64_t *chain_off, int64_t nchains, dh_edit_paths **out, int32_t *status)
{
    return chain_paths_impl(ctx, A, B, las, n, trace, -1, tspace, chain_off, nchains, out, status);
}

extern "C" int dh_la_set_chain_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la_set *set, dh_edit_paths **out, int32_t *status)
{
    const dh_la *las;
    int64_t n;
    if (int rc = dh_set_host_records("dh_la_set_chain_paths", ctx && A && B && out, set, &las, &n)) return rc;
    if (int rc = dh_la_set_ensure_host_trace(const_cast<dh_la_set *>(set))) return rc;
    return chain_paths_impl(ctx, A, B, las, n, set->trace.data(), (int64_t)set->trace.size(), set->tspace, nullptr, 0, out, status);
}
