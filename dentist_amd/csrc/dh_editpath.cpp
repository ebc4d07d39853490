// dh_editpath.cpp -- host side of the edit-path API (dh_la_edit_paths, dh_la_set_edit_paths, dh_edit_paths_*) and the
// host-only formatters dh_format_cigar / dh_format_alignment.  The kernels are in dh_editpath.hip.
//
// A call validates every record against the two DBs, cuts the records into trace tiles and runs them chunk by chunk
// (DH_EDIT_CHUNK tiles, a development knob): the tiles whose band fits a class go through k_edit_fast, the ones it does not
// prove exact and the ones no class fits through k_edit_general, k_edit_compact puts the ops of the chunk in alignment
// order, and the host appends them to the result.  Device scratch (the SLOT_EP_* group) is bounded by the chunk.
//
// dh_la_transpose / dh_la_set_transpose run the same chunks cut between records, leave the ops of a chunk on the device
// and let k_trace_transpose put the trace points of every record's transposed path on the grid of the B read (the
// SLOT_TR_* group); the host adds the coordinates, the chain flags and LAsort order.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dh_editpath.h"

extern "C" void dhk_edit_fast(hipStream_t st, int nw, const EpTile *tiles, int32_t n, const uint8_t *abases,
                              const uint8_t *bfwd, const uint8_t *brc, int32_t rows, int32_t owords, uint64_t *dm,
                              uint64_t *ow, EpResult *res);
extern "C" void dhk_edit_general(hipStream_t st, const EpTile *tiles, int32_t n, const uint8_t *abases, const uint8_t *bfwd,
                                 const uint8_t *brc, int32_t rows, uint32_t *dmat, const int64_t *ow_off, uint64_t *ow,
                                 EpResult *res);
extern "C" void dhk_edit_compact(hipStream_t st, const EpCopy *cp, int32_t n, const uint64_t *ow_fast, const uint64_t *ow_general,
                                 uint8_t *out);
extern "C" void dhk_trace_transpose(hipStream_t st, const EpTrRec *recs, int32_t n, const uint8_t *ops, int32_t ts, uint2 *bound,
                                    uint32_t *pairs, int32_t *status);

extern "C" void dh_edit_paths_destroy(dh_edit_paths *p) { delete p; }
extern "C" int64_t dh_edit_paths_count(const dh_edit_paths *p) { return p ? (int64_t)p->score.size() : 0; }
extern "C" const int64_t *dh_edit_paths_op_off(const dh_edit_paths *p) { return p ? p->op_off.data() : nullptr; }
extern "C" const uint8_t *dh_edit_paths_ops(const dh_edit_paths *p) { return p ? p->ops.data() : nullptr; }
extern "C" const int32_t *dh_edit_paths_score(const dh_edit_paths *p) { return p ? p->score.data() : nullptr; }
extern "C" const int64_t *dh_edit_paths_tile_off(const dh_edit_paths *p) { return p ? p->tile_off.data() : nullptr; }
extern "C" const uint16_t *dh_edit_paths_tile_score(const dh_edit_paths *p) { return p ? p->tile_score.data() : nullptr; }
extern "C" int64_t dh_edit_paths_general_tiles(const dh_edit_paths *p) { return p ? p->general_tiles : 0; }
extern "C" int64_t dh_edit_paths_fillers(const dh_edit_paths *p) { return p ? p->fillers : 0; }
extern "C" const int32_t *dh_edit_paths_entry_fillers(const dh_edit_paths *p)
{
    return p && !p->entry_fillers.empty() ? p->entry_fillers.data() : nullptr;
}

namespace {

#define EP_GENERAL_BATCH 2048 /* tiles per launch of the full-matrix kernel: 64 KB of decisions each at tspace = 250 */

// the tiles of record `idx` (dazzler.d:2405-2426: A from abpos to the next multiple of tspace, then in steps of tspace, the
// last one ending at aepos; B the running sum of the trace's bbases), validated: nothing the kernels read lies outside
// the sequences
int cut_record(const dh_db *A, const dh_db *B, const dh_la &la, int64_t idx, const uint16_t *trace, int64_t trace_len,
               int32_t ts, std::vector<EpTile> &tiles)
{
    char msg[256];
#define EP_BAD(...)                                  \
    do {                                             \
        snprintf(msg, sizeof(msg), __VA_ARGS__);     \
        return dh_fail(DH_EINVAL, msg);              \
    } while (0)
    if (la.aread < 0 || la.aread >= A->n || la.bread < 0 || la.bread >= B->n)
        EP_BAD("dh_la_edit_paths: LA %lld: read numbers (%d, %d) outside the DBs", (long long)idx, la.aread, la.bread);
    const int64_t alen = A->h_off[(size_t)la.aread + 1] - A->h_off[(size_t)la.aread];
    const int64_t blen = B->h_off[(size_t)la.bread + 1] - B->h_off[(size_t)la.bread];
    if (la.abpos < 0 || la.aepos < la.abpos || la.aepos > alen || la.bbpos < 0 || la.bepos < la.bbpos || la.bepos > blen)
        EP_BAD("dh_la_edit_paths: LA %lld: coordinates [%d, %d) x [%d, %d) outside the sequences (%lld, %lld bases)",
               (long long)idx, la.abpos, la.aepos, la.bbpos, la.bepos, (long long)alen, (long long)blen);
    if (la.tlen < 0 || (la.tlen & 1)) EP_BAD("dh_la_edit_paths: LA %lld: tlen %d is odd or negative", (long long)idx, la.tlen);
    if (la.toff < 0 || (trace_len >= 0 && la.toff + la.tlen > trace_len))
        EP_BAD("dh_la_edit_paths: LA %lld: trace values [%lld, +%d) outside the trace", (long long)idx, (long long)la.toff, la.tlen);
    const int32_t nt = la.tlen / 2;
    const int32_t want = la.aepos > la.abpos ? (la.aepos + ts - 1) / ts - la.abpos / ts : nt;
    if (nt != want || (la.aepos == la.abpos && nt > 1))
        EP_BAD("dh_la_edit_paths: LA %lld: %d trace points for A [%d, %d) at tspace %d (%d expected)", (long long)idx, nt, la.abpos,
               la.aepos, ts, want);
    const uint16_t *tr = trace + la.toff;
    int64_t bsum = 0;
    for (int32_t t = 0; t < nt; t++) bsum += tr[2 * t + 1];
    if (bsum != (int64_t)la.bepos - la.bbpos)
        EP_BAD("dh_la_edit_paths: LA %lld: the trace's B bases sum to %lld, the record spans %d", (long long)idx, (long long)bsum,
               la.bepos - la.bbpos);
    const bool comp = (la.flags & DH_FLAG_COMP) != 0;
    int32_t a = la.abpos, b = la.bbpos;
    for (int32_t t = 0; t < nt; t++) {
        const int32_t a1 = std::min<int32_t>((a / ts + 1) * ts, la.aepos), b1 = b + tr[2 * t + 1];
        EpTile tl;
        tl.aoff = A->h_off[(size_t)la.aread] + a;
        tl.boff = B->h_off[(size_t)la.bread] + b;
        tl.rl = a1 - a;
        tl.ql = b1 - b;
        tl.diffs = tr[2 * t];
        tl.comp = comp ? 1 : 0;
        if (tl.ql > EP_QL_FACTOR * ts)
            EP_BAD("dh_la_edit_paths: LA %lld tile %d: %d B bases against %d A bases exceed the cap of %d x tspace", (long long)idx, t,
                   tl.ql, tl.rl, EP_QL_FACTOR);
        tiles.push_back(tl);
        a = a1;
        b = b1;
    }
    return DH_OK;
#undef EP_BAD
}

size_t edit_chunk()  // tiles per launch
{
    return (size_t)dh_env_knob("DH_EDIT_CHUNK", 131072, 1, INT32_MAX);  // development
}

struct ChunkRun {
    dh_ctx *ctx;
    dh_db *A, *B;
    int32_t ts;
};

// tiles [t0, t1) of `tiles` (alignment order): nops / score per tile into res[], the ops appended to out->ops -- or, with
// keep_ops, left on the device (SLOT_EP_OPS, tile after tile: a tile's first op is the sum of the nops before it) for a kernel
// queued behind this call; *keep_ops is NULL when the chunk has no op
int run_chunk(const ChunkRun &r, const std::vector<EpTile> &tiles, size_t t0, size_t t1, std::vector<EpResult> &res,
              dh_edit_paths *out, const uint8_t **keep_ops = nullptr)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = ctx->stream;
    const size_t n = t1 - t0;
    const uint8_t *ab = r.A->d_bases, *bf = r.B->d_bases, *brc = r.B->d_rc;
    // ---- fast path: class 1, then class 2, each its own launch
    std::vector<int32_t> idx[3];
    for (size_t t = 0; t < n; t++) idx[ep::tile_class(tiles[t0 + t].rl, tiles[t0 + t].ql, tiles[t0 + t].diffs)].push_back((int32_t)t);
    std::vector<EpCopy> cp(n);
    std::vector<EpTile> stage;
    std::vector<EpResult> fres;
    const size_t nfast = idx[1].size() + idx[2].size();
    size_t wbase[3] = {0, 0, 0};
    uint64_t *d_ow = nullptr;
    if (nfast) {
        int32_t rows[3] = {0, 0, 0}, owords[3] = {0, 0, 0};
        stage.reserve(nfast);
        for (int c = 1; c <= 2; c++)
            for (int32_t t : idx[c]) {
                const EpTile &tl = tiles[t0 + (size_t)t];
                rows[c] = std::max(rows[c], tl.rl);
                owords[c] = std::max(owords[c], (tl.rl + tl.ql + 7) >> 3);
                stage.push_back(tl);
            }
        const size_t n1 = idx[1].size(), n2 = idx[2].size();
        const size_t dm1 = n1 * (size_t)rows[1] * 3, dm2 = n2 * (size_t)rows[2] * 6;
        wbase[1] = 0;
        wbase[2] = n1 * (size_t)owords[1];
        EpTile *d_tiles;
        uint64_t *d_dm;
        EpResult *d_res;
        if (int rc = dh_scr(ctx, SLOT_EP_TILES, nfast, &d_tiles)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_DM, dm1 + dm2, &d_dm)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_OW, wbase[2] + n2 * (size_t)owords[2], &d_ow)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_RES, nfast, &d_res)) return rc;
        HIPCHK(hipMemcpyAsync(d_tiles, stage.data(), sizeof(EpTile) * nfast, hipMemcpyHostToDevice, st));
        dhk_edit_fast(st, 1, d_tiles, (int32_t)n1, ab, bf, brc, rows[1], owords[1], d_dm, d_ow, d_res);
        dhk_edit_fast(st, 2, d_tiles + n1, (int32_t)n2, ab, bf, brc, rows[2], owords[2], d_dm + dm1, d_ow + wbase[2], d_res + n1);
        HIPCHK(hipGetLastError());
        fres.resize(nfast);
        HIPCHK(hipMemcpyAsync(fres.data(), d_res, sizeof(EpResult) * nfast, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        size_t k = 0;
        for (int c = 1; c <= 2; c++) {
            const size_t nc = idx[c].size();
            for (size_t p = 0; p < nc; p++, k++) {
                const int32_t t = idx[c][p];
                if (fres[k].nops & EP_REJECTED) {
                    idx[0].push_back(t);
                    continue;
                }
                res[t0 + (size_t)t] = fres[k];
                cp[(size_t)t] = EpCopy{(int64_t)(wbase[c] + p), (int64_t)nc, 0, (int32_t)fres[k].nops, 0};
            }
        }
    }
    // ---- general path: what no class fits and what the fast path could not prove exact
    uint64_t *d_gow = nullptr;
    if (!idx[0].empty()) {
        const size_t ng = idx[0].size();
        out->general_tiles += (int64_t)ng;
        std::vector<int64_t> goff(ng + 1, 0);
        stage.clear();
        int32_t rows = 1;
        for (size_t p = 0; p < ng; p++) {
            const EpTile &tl = tiles[t0 + (size_t)idx[0][p]];
            stage.push_back(tl);
            rows = std::max(rows, tl.rl);
            goff[p + 1] = goff[p] + ((tl.rl + tl.ql + 7) >> 3);
        }
        const size_t gb = std::min<size_t>(ng, EP_GENERAL_BATCH);
        EpTile *d_tiles;
        int64_t *d_goff;
        uint32_t *d_dm;
        EpResult *d_res;
        if (int rc = dh_scr(ctx, SLOT_EP_GEN_TILES, ng, &d_tiles)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_GEN_DM, gb * (size_t)rows * 64, &d_dm)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_GEN_OW, (size_t)goff[ng], &d_gow)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_GEN_OFF, ng + 1, &d_goff)) return rc;
        if (int rc = dh_scr(ctx, SLOT_EP_GEN_RES, ng, &d_res)) return rc;
        HIPCHK(hipMemcpyAsync(d_tiles, stage.data(), sizeof(EpTile) * ng, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_goff, goff.data(), sizeof(int64_t) * (ng + 1), hipMemcpyHostToDevice, st));
        for (size_t g0 = 0; g0 < ng; g0 += gb)  // (one stream: a batch starts when the one before it is done with d_dm)
            dhk_edit_general(st, d_tiles + g0, (int32_t)std::min(gb, ng - g0), ab, bf, brc, rows, d_dm, d_goff + g0, d_gow, d_res + g0);
        HIPCHK(hipGetLastError());
        fres.resize(ng);
        HIPCHK(hipMemcpyAsync(fres.data(), d_res, sizeof(EpResult) * ng, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t p = 0; p < ng; p++) {
            const int32_t t = idx[0][p];
            if (fres[p].nops & EP_REJECTED) return dh_fail(DH_EINVAL, "dh_la_edit_paths: a tile exceeds the full-matrix kernel's caps");
            res[t0 + (size_t)t] = fres[p];
            cp[(size_t)t] = EpCopy{goff[p], 1, 0, (int32_t)fres[p].nops, 1};
        }
    }
    // ---- the ops of the chunk in alignment order
    int64_t total = 0;
    for (size_t t = 0; t < n; t++) {
        cp[t].out = total;
        total += cp[t].nops;
    }
    if (keep_ops) *keep_ops = nullptr;
    if (total == 0) return DH_OK;
    EpCopy *d_cp;
    uint8_t *d_out;
    if (int rc = dh_scr(ctx, SLOT_EP_COPY, n, &d_cp)) return rc;
    if (int rc = dh_scr(ctx, SLOT_EP_OPS, (size_t)total, &d_out)) return rc;
    HIPCHK(hipMemcpyAsync(d_cp, cp.data(), sizeof(EpCopy) * n, hipMemcpyHostToDevice, st));
    dhk_edit_compact(st, d_cp, (int32_t)n, d_ow, d_gow, d_out);
    HIPCHK(hipGetLastError());
    if (keep_ops) {
        *keep_ops = d_out;
        return DH_OK;
    }
    const size_t at = out->ops.size();
    out->ops.resize(at + (size_t)total);
    HIPCHK(hipMemcpyAsync(out->ops.data() + at, d_out, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}

int edit_paths_impl(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace, int64_t trace_len,
                    int32_t ts, int64_t first, int64_t count, dh_edit_paths **out)
{
    if (!ctx || !A || !B || !out || n < 0 || first < 0 || count < 0 || first + count > n || (count > 0 && (!las || !trace)))
        return dh_fail(DH_EINVAL, "dh_la_edit_paths: bad argument");
    if (ts < 1 || ts > EP_TSPACE_MAX) return dh_fail(DH_EINVAL, "dh_la_edit_paths: tspace must be in [1, 250]");
    *out = nullptr;
    // ---- validation and tiling on the host, before anything is launched
    std::unique_ptr<dh_edit_paths> p(new dh_edit_paths);
    std::vector<EpTile> tiles;
    p->score.assign((size_t)count, 0);
    p->op_off.assign((size_t)count + 1, 0);
    p->tile_off.assign((size_t)count + 1, 0);
    for (int64_t i = 0; i < count; i++) {
        if (int rc = cut_record(A, B, las[first + i], first + i, trace, trace_len, ts, tiles)) return rc;
        p->tile_off[(size_t)i + 1] = (int64_t)tiles.size();
    }
    p->tile_score.assign(tiles.size(), 0);
    if (!tiles.empty()) {
        HIPCHK(hipSetDevice(ctx->device));
        if (int rc = dh_ensure_rc(B)) return rc;
        const size_t chunk = edit_chunk();
        std::vector<EpResult> res(tiles.size());
        const ChunkRun r{ctx, A, B, ts};
        for (size_t t0 = 0; t0 < tiles.size(); t0 += chunk)
            if (int rc = run_chunk(r, tiles, t0, std::min(tiles.size(), t0 + chunk), res, p.get())) return rc;
        for (int64_t i = 0; i < count; i++) {
            int64_t nops = 0, score = 0;
            for (int64_t t = p->tile_off[(size_t)i]; t < p->tile_off[(size_t)i + 1]; t++) {
                nops += res[(size_t)t].nops;
                score += res[(size_t)t].score;
                p->tile_score[(size_t)t] = (uint16_t)res[(size_t)t].score;
            }
            p->op_off[(size_t)i + 1] = p->op_off[(size_t)i] + nops;
            p->score[(size_t)i] = (int32_t)score;
        }
    }
    *out = p.release();
    return DH_OK;
}

// the records of [r0, r1) -- whole records, tiles [tile_off[r0], tile_off[r1]) -- through the edit-path kernels and
// k_trace_transpose: their transposed trace pairs into set->trace, their diffs into set->la
int transpose_chunk(const ChunkRun &r, const std::vector<EpTile> &tiles, const std::vector<int64_t> &tile_off,
                    const std::vector<int64_t> &slot_off, int64_t r0, int64_t r1, std::vector<EpResult> &res, dh_edit_paths *tmp,
                    dh_la_set *set)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = ctx->stream;
    const uint8_t *d_ops = nullptr;
    if (int rc = run_chunk(r, tiles, (size_t)tile_off[(size_t)r0], (size_t)tile_off[(size_t)r1], res, tmp, &d_ops)) return rc;
    const size_t nrec = (size_t)(r1 - r0), nslots = (size_t)(slot_off[(size_t)r1] - slot_off[(size_t)r0]);
    std::vector<EpTrRec> recs(nrec);
    int64_t op = 0;
    for (int64_t i = r0; i < r1; i++) {
        dh_la &t = set->la[(size_t)i];
        int64_t nops = 0, score = 0;
        for (int64_t k = tile_off[(size_t)i]; k < tile_off[(size_t)i + 1]; k++) {
            nops += res[(size_t)k].nops;
            score += res[(size_t)k].score;
        }
        if (nops > INT32_MAX) return dh_fail(DH_EINVAL, "dh_la_transpose: a path of more than 2^31 ops");
        t.diffs = (int32_t)score;
        recs[(size_t)(i - r0)] = EpTrRec{op, slot_off[(size_t)i] - slot_off[(size_t)r0], (int32_t)nops,
                                         (t.flags & DH_FLAG_COMP) ? 1 : 0, t.abpos, t.aepos};
        op += nops;
    }
    if (!d_ops) return dh_fail(DH_EHIP, "dh_la_transpose: the chunk left no ops");  // (every record has B bases, hence ops)
    EpTrRec *d_recs;
    uint2 *d_bound;
    uint32_t *d_pairs;
    int32_t *d_status;
    if (int rc = dh_scr(ctx, SLOT_TR_RECS, nrec, &d_recs)) return rc;
    if (int rc = dh_scr(ctx, SLOT_TR_BOUND, nslots, &d_bound)) return rc;
    if (int rc = dh_scr(ctx, SLOT_TR_PAIRS, nslots, &d_pairs)) return rc;
    if (int rc = dh_scr(ctx, SLOT_TR_STATUS, nrec, &d_status)) return rc;
    HIPCHK(hipMemcpyAsync(d_recs, recs.data(), sizeof(EpTrRec) * nrec, hipMemcpyHostToDevice, st));
    dhk_trace_transpose(st, d_recs, (int32_t)nrec, d_ops, r.ts, d_bound, d_pairs, d_status);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> status(nrec);
    HIPCHK(hipMemcpyAsync(set->trace.data() + 2 * slot_off[(size_t)r0], d_pairs, sizeof(uint32_t) * nslots, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(status.data(), d_status, sizeof(int32_t) * nrec, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t k = 0; k < nrec; k++) {
        char msg[160];
        if (status[k] & 2) {
            snprintf(msg, sizeof(msg), "dh_la_transpose: LA %lld: the ops of its path do not span its B interval", (long long)(r0 + (int64_t)k));
            return dh_fail(DH_EHIP, msg);
        }
        if (status[k] & 1) {
            snprintf(msg, sizeof(msg), "dh_la_transpose: LA %lld: a tile of the transposed trace does not fit 16 bits", (long long)(r0 + (int64_t)k));
            return dh_fail(DH_EOVERFLOW, msg);
        }
    }
    return DH_OK;
}

int transpose_impl(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace, int64_t trace_len,
                   int32_t ts, int32_t want_best, dh_la_set **out, int64_t *src_index)
{
    if (!ctx || !A || !B || !out || n < 0 || (n > 0 && (!las || !trace))) return dh_fail(DH_EINVAL, "dh_la_transpose: bad argument");
    if (ts < 1 || ts > EP_TSPACE_MAX) return dh_fail(DH_EINVAL, "dh_la_transpose: tspace must be in [1, 250]");
    *out = nullptr;
    // ---- validation, tiling and the transposed coordinates on the host, before anything is launched
    std::unique_ptr<dh_la_set> set(new dh_la_set);
    set->tspace = ts;
    set->device = ctx->device;
    set->la.resize((size_t)n);
    std::vector<EpTile> tiles;
    std::vector<int64_t> tile_off((size_t)n + 1, 0), slot_off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        const dh_la &l = las[i];
        if (int rc = cut_record(A, B, l, i, trace, trace_len, ts, tiles)) return rc;
        tile_off[(size_t)i + 1] = (int64_t)tiles.size();
        if (l.bepos == l.bbpos) {
            char msg[128];
            snprintf(msg, sizeof(msg), "dh_la_transpose: LA %lld: no B bases, the transposed record has no A interval", (long long)i);
            return dh_fail(DH_EINVAL, msg);
        }
        const int32_t alen = (int32_t)(A->h_off[(size_t)l.aread + 1] - A->h_off[(size_t)l.aread]);
        const int32_t blen = (int32_t)(B->h_off[(size_t)l.bread + 1] - B->h_off[(size_t)l.bread]);
        const bool comp = (l.flags & DH_FLAG_COMP) != 0;
        dh_la t;
        memset(&t, 0, sizeof(t));
        t.aread = l.bread;
        t.bread = l.aread;
        t.abpos = comp ? blen - l.bepos : l.bbpos;
        t.aepos = comp ? blen - l.bbpos : l.bepos;
        t.bbpos = comp ? alen - l.aepos : l.abpos;
        t.bepos = comp ? alen - l.abpos : l.aepos;
        t.flags = l.flags & ~(DH_FLAG_START | DH_FLAG_NEXT | DH_FLAG_BEST | DH_FLAG_DISABLED);
        const int32_t nt = ep::tr_tiles(t.abpos, t.aepos, ts);
        t.tlen = 2 * nt;
        t.toff = 2 * slot_off[(size_t)i];
        slot_off[(size_t)i + 1] = slot_off[(size_t)i] + nt;
        set->la[(size_t)i] = t;
    }
    set->trace.resize((size_t)(2 * slot_off[(size_t)n]));
    if (n > 0) {
        HIPCHK(hipSetDevice(ctx->device));
        if (int rc = dh_ensure_rc(B)) return rc;
        // ---- chunks of whole records: DH_EDIT_CHUNK tiles at most, a larger record on its own
        const int64_t chunk = (int64_t)edit_chunk();
        std::vector<EpResult> res(tiles.size());
        dh_edit_paths tmp;
        const ChunkRun r{ctx, A, B, ts};
        for (int64_t r0 = 0, r1; r0 < n; r0 = r1) {
            r1 = r0 + 1;
            while (r1 < n && tile_off[(size_t)r1 + 1] - tile_off[(size_t)r0] <= chunk) r1++;
            if (int rc = transpose_chunk(r, tiles, tile_off, slot_off, r0, r1, res, &tmp, set.get())) return rc;
        }
    }
    // ---- chain flags and LAsort order; records equal in every key of the order keep the order of their sources (toff
    // ascends with the source index)
    std::stable_sort(set->la.begin(), set->la.end(), dh_la_less);  // groups the records by aread
    dh_finish_transposed_set(set.get(), want_best != 0, dh_ctx_near_best_ppm(ctx));
    for (size_t i = 0, j; i < set->la.size(); i = j) {
        for (j = i + 1; j < set->la.size() && !dh_la_less(set->la[i], set->la[j]); j++) {}
        if (j - i > 1) std::sort(set->la.begin() + (int64_t)i, set->la.begin() + (int64_t)j, [](const dh_la &p, const dh_la &q) { return p.toff < q.toff; });
    }
    if (src_index)
        for (size_t i = 0; i < set->la.size(); i++)
            src_index[i] = (std::upper_bound(slot_off.begin(), slot_off.end(), set->la[i].toff / 2) - slot_off.begin()) - 1;
    *out = set.release();
    return DH_OK;
}

}  // namespace

int dh_ep_check_record(const dh_db *A, const dh_db *B, const dh_la &la, int64_t idx, const uint16_t *trace, int64_t trace_len,
                       int32_t ts, std::vector<EpTile> &tiles)
{
    return cut_record(A, B, la, idx, trace, trace_len, ts, tiles);
}

size_t dh_ep_chunk_tiles() { return edit_chunk(); }

int dh_ep_run_tiles(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t ts, const std::vector<EpTile> &tiles, size_t t0, size_t t1,
                    std::vector<EpResult> &res, dh_edit_paths *out, const uint8_t **d_ops)
{
    return run_chunk(ChunkRun{ctx, A, B, ts}, tiles, t0, t1, res, out, d_ops);
}

extern "C" int dh_la_transpose(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace,
                               int32_t tspace, int32_t want_best, dh_la_set **out, int64_t *src_index)
{
    return transpose_impl(ctx, A, B, las, n, trace, -1, tspace, want_best, out, src_index);
}

extern "C" int dh_la_set_transpose(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la_set *set, int32_t want_best, dh_la_set **out,
                                   int64_t *src_index)
{
    if (!set) return dh_fail(DH_EINVAL, "dh_la_set_transpose: set is NULL");
    if (set->la.empty() && set->d_la_n > 0)
        return dh_fail(DH_EINVAL, "dh_la_set_transpose: the records of this set were left on the device");
    if (int rc = dh_la_set_ensure_host_trace(const_cast<dh_la_set *>(set))) return rc;
    return transpose_impl(ctx, A, B, set->la.data(), (int64_t)set->la.size(), set->trace.data(), (int64_t)set->trace.size(),
                          set->tspace, want_best, out, src_index);
}

extern "C" int dh_la_edit_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace,
                                int32_t tspace, int64_t first, int64_t count, dh_edit_paths **out)
{
    return edit_paths_impl(ctx, A, B, las, n, trace, -1, tspace, first, count, out);
}

extern "C" int dh_la_set_edit_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la_set *set, int64_t first, int64_t count,
                                    dh_edit_paths **out)
{
    if (!set) return dh_fail(DH_EINVAL, "dh_la_set_edit_paths: set is NULL");
    if (set->la.empty() && set->d_la_n > 0)
        return dh_fail(DH_EINVAL, "dh_la_set_edit_paths: the records of this set were left on the device");
    if (int rc = dh_la_set_ensure_host_trace(const_cast<dh_la_set *>(set))) return rc;
    return edit_paths_impl(ctx, A, B, set->la.data(), (int64_t)set->la.size(), set->trace.data(), (int64_t)set->trace.size(),
                           set->tspace, first, count, out);
}

// ------------------------------------------------------------------------------------ formatters (host only)

extern "C" int64_t dh_format_cigar(const uint8_t *ops, int64_t nops, int32_t extended, char *out, int64_t cap)
{
    if (nops < 0 || (nops > 0 && !ops)) return dh_fail(DH_EINVAL, "dh_format_cigar: bad argument");
    std::string s;
    for (int64_t i = 0; i < nops;) {
        if (ops[i] > EP_OP_MISMATCH) return dh_fail(DH_EINVAL, "dh_format_cigar: op code above 3");
        auto sym = [&](uint8_t op) {
            return op == EP_OP_DEL ? 'D' : (op == EP_OP_INS ? 'I' : (!extended ? 'M' : (op == EP_OP_MATCH ? '=' : 'X')));
        };
        const char c = sym(ops[i]);
        int64_t j = i + 1;
        while (j < nops && ops[j] <= EP_OP_MISMATCH && sym(ops[j]) == c) j++;
        s += std::to_string(j - i);
        s += c;
        i = j;
    }
    if (out && cap > (int64_t)s.size()) memcpy(out, s.c_str(), s.size() + 1);
    return (int64_t)s.size();
}

extern "C" int64_t dh_format_alignment(const uint8_t *a, const uint8_t *b, const uint8_t *ops, int64_t nops, int32_t width,
                                       char *out, int64_t cap)
{
    if (nops < 0 || width < 0 || (nops > 0 && (!ops || !a || !b))) return dh_fail(DH_EINVAL, "dh_format_alignment: bad argument");
    // SequenceAlignment.toString (util/string.d:365-426): reference line, compare line, query line; blocks of `width`
    // columns separated by an empty line, no newline at the end.  Base codes 0..4 print as acgtn, other bytes as they are.
    auto chr = [](uint8_t x) { return x < 5 ? "acgtn"[x] : (char)x; };
    std::string l[3];
    for (int k = 0; k < 3; k++) l[k].reserve((size_t)nops);
    int64_t i = 0, j = 0;
    for (int64_t k = 0; k < nops; k++) switch (ops[k]) {
            case EP_OP_MATCH:
            case EP_OP_MISMATCH:
                l[0] += chr(a[i++]);
                l[1] += ops[k] == EP_OP_MATCH ? '|' : '*';
                l[2] += chr(b[j++]);
                break;
            case EP_OP_DEL:
                l[0] += chr(a[i++]);
                l[1] += ' ';
                l[2] += '-';
                break;
            case EP_OP_INS:
                l[0] += '-';
                l[1] += ' ';
                l[2] += chr(b[j++]);
                break;
            default:
                return dh_fail(DH_EINVAL, "dh_format_alignment: op code above 3");
        }
    std::string s;
    if (width == 0) {
        s = l[0] + "\n" + l[1] + "\n" + l[2];
    } else {
        for (int64_t c0 = 0; c0 < nops; c0 += width) {
            if (c0) s += "\n\n";
            for (int k = 0; k < 3; k++) {
                if (k) s += "\n";
                s += l[k].substr((size_t)c0, (size_t)width);
            }
        }
    }
    if (out && cap > (int64_t)s.size()) memcpy(out, s.c_str(), s.size() + 1);
    return (int64_t)s.size();
}
