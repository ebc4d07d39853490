// dh_nw.cpp -- host side of dh_nw_batch: global alignment of arbitrary sequence pairs (the kernel is in dh_nw.hip, the
// lane code and the exactness argument in dh_nw.h).
//
// A call validates the offsets, answers the pairs with an empty side itself and cuts the rest into chunks of consecutive
// pairs whose decision words fit DH_NW_CHUNK_KB (a development knob, like DH_EDIT_CHUNK).  The sequences of a chunk go to
// the device once.  Every pair starts at half-width DH_NW_W0 (default 64); k_nw fills the band and walks it back, the host
// applies nw::accepted to the cost it reports, and the pairs that fail run again, together, at twice the half-width -- in
// launch groups bounded by the same knob, one launch per kernel class -- until the band would exceed NW_MAX_W columns:
// those get DH_NW_BAND_EXCEEDED.  k_edit_compact (dh_editpath.hip) puts the ops of a group in path order.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dh_nw.h"

extern "C" void dhk_nw(hipStream_t st, int cpl, int ns, const NwPair *pairs, int32_t n, const uint8_t *refs, const uint8_t *qrys,
                       int32_t free_shift, uint32_t *dm, int64_t dm_words, uint64_t *ow, int64_t ow_words, EpResult *res);
extern "C" void dhk_edit_compact(hipStream_t st, const EpCopy *cp, int32_t n, const uint64_t *ow_fast, const uint64_t *ow_general,
                                 uint8_t *out);

namespace {

static_assert(NW_MAX_LEN == DH_NW_MAX_LEN && NW_MAX_W == DH_NW_MAX_BAND, "the header states the kernel's limits");

int64_t nw_budget_words()  // decision words (32 bits) per launch group
{
    return dh_env_knob("DH_NW_CHUNK_KB", 1 << 20, 1, INT64_MAX) * 256;  // development; no upper bound
}

int64_t nw_first_w()
{
    return dh_env_knob("DH_NW_W0", 64, 1, NW_MAX_W);  // development
}

struct Job {
    int64_t pair;  // index in the call
    int64_t w;
    nw::Band b;
    int32_t cpl, ns;
    int64_t words;  // decision words
};

using PairOut = DhNwPairOut;

struct NwRun {
    dh_ctx *ctx;
    const DhNwSeq *seq;  // by pair of the call: where its sequences are in the device buffers
    const uint8_t *d_ref, *d_qry;
    int32_t fs;
    std::vector<PairOut> *out;
    std::vector<uint8_t> *stage;
};

// jobs [j0, j1) (sorted by class) as one launch group; the rejected ones are appended to `again`
int run_launch(const NwRun &r, const std::vector<Job> &jobs, size_t j0, size_t j1, std::vector<Job> &again)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = ctx->stream;
    const size_t n = j1 - j0;
    std::vector<NwPair> pairs(n);
    int64_t dm_words = 0, ow_words = 0;
    for (size_t k = 0; k < n; k++) {
        const Job &jb = jobs[j0 + k];
        const DhNwSeq &sq = r.seq[jb.pair];
        NwPair &p = pairs[k];
        p.roff = sq.roff;
        p.qoff = sq.qoff;
        p.rl = sq.rl;
        p.ql = sq.ql;
        p.lo = jb.b.lo;
        p.hi = jb.b.hi;
        p.dm_off = dm_words;
        p.ow_off = ow_words;
        dm_words += jb.words;
        ow_words += ((int64_t)p.rl + p.ql + 7) >> 3;
    }
    NwPair *d_pairs;
    uint32_t *d_dm;
    uint64_t *d_ow;
    EpResult *d_res;
    if (int rc = dh_scr(ctx, SLOT_NW_PAIRS, n, &d_pairs)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NW_DM, (size_t)dm_words, &d_dm)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NW_OW, (size_t)ow_words, &d_ow)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NW_RES, n, &d_res)) return rc;
    HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(NwPair) * n, hipMemcpyHostToDevice, st));
    for (size_t a = 0, b; a < n; a = b) {  // one launch per class
        for (b = a + 1; b < n && jobs[j0 + b].cpl == jobs[j0 + a].cpl && jobs[j0 + b].ns == jobs[j0 + a].ns; b++) {}
        dhk_nw(st, jobs[j0 + a].cpl, jobs[j0 + a].ns, d_pairs + a, (int32_t)(b - a), r.d_ref, r.d_qry, r.fs, d_dm, dm_words, d_ow,
               ow_words, d_res + a);
    }
    HIPCHK(hipGetLastError());
    std::vector<EpResult> res(n);
    HIPCHK(hipMemcpyAsync(res.data(), d_res, sizeof(EpResult) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<EpCopy> cp;
    int64_t total = 0;
    for (size_t k = 0; k < n; k++) {
        const Job &jb = jobs[j0 + k];
        const bool walked = !(res[k].nops & EP_REJECTED);
        if (!walked && jb.b.full) return dh_fail(DH_EHIP, "dh_nw_batch: the kernel refused a pair the host planned");
        if (!walked || !nw::accepted((int64_t)res[k].score, jb.w, r.fs, jb.b.full)) {
            again.push_back(jb);
            continue;
        }
        cp.push_back(EpCopy{pairs[k].ow_off, 1, total, (int32_t)res[k].nops, 1});
        PairOut &o = (*r.out)[(size_t)jb.pair];
        o.at = (int64_t)r.stage->size() + total;
        o.nops = (int32_t)res[k].nops;
        o.score = (int32_t)res[k].score;
        total += res[k].nops;
    }
    if (total == 0) return DH_OK;
    EpCopy *d_cp;
    uint8_t *d_out;
    if (int rc = dh_scr(ctx, SLOT_NW_COPY, cp.size(), &d_cp)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NW_OPS, (size_t)total, &d_out)) return rc;
    HIPCHK(hipMemcpyAsync(d_cp, cp.data(), sizeof(EpCopy) * cp.size(), hipMemcpyHostToDevice, st));
    dhk_edit_compact(st, d_cp, (int32_t)cp.size(), nullptr, d_ow, d_out);
    HIPCHK(hipGetLastError());
    const size_t at = r.stage->size();
    r.stage->resize(at + (size_t)total);
    HIPCHK(hipMemcpyAsync(r.stage->data() + at, d_out, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}

// the pairs `todo` of the chunk [p0, p1) of a call on host sequences: their bases go to the device once
int run_chunk(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry, const int64_t *qry_off, int64_t p0,
              int64_t p1, const std::vector<int64_t> &todo, int32_t fs, std::vector<DhNwSeq> &seq, std::vector<PairOut> &out,
              std::vector<uint8_t> &stage)
{
    hipStream_t st = ctx->stream;
    const int64_t rbytes = ref_off[p1] - ref_off[p0], qbytes = qry_off[p1] - qry_off[p0];
    uint8_t *d_ref, *d_qry;
    if (int rc = dh_scr(ctx, SLOT_NW_REF, (size_t)rbytes + 2 * NW_SEQ_PAD, &d_ref)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NW_QRY, (size_t)qbytes + 2 * NW_SEQ_PAD, &d_qry)) return rc;
    if (rbytes) HIPCHK(hipMemcpyAsync(d_ref + NW_SEQ_PAD, ref + ref_off[p0], (size_t)rbytes, hipMemcpyHostToDevice, st));
    if (qbytes) HIPCHK(hipMemcpyAsync(d_qry + NW_SEQ_PAD, qry + qry_off[p0], (size_t)qbytes, hipMemcpyHostToDevice, st));
    for (int64_t p : todo)
        seq[(size_t)p] = DhNwSeq{NW_SEQ_PAD + ref_off[p] - ref_off[p0], NW_SEQ_PAD + qry_off[p] - qry_off[p0],
                                 (int32_t)(ref_off[p + 1] - ref_off[p]), (int32_t)(qry_off[p + 1] - qry_off[p])};
    return dh_nw_run_pairs(ctx, d_ref, d_qry, seq.data(), todo, fs, out, stage);
}

}  // namespace

// The widening protocol, shared by dh_nw_batch and the chain padder's fillers (dh_chainpad.cpp): attempts at growing
// half-widths until every pair of `todo` is accepted or given up.  The sequences are on the device already, NW_SEQ_PAD
// readable bytes on either side of each; seq is indexed by pair, as out is.
int dh_nw_run_pairs(dh_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_qry, const DhNwSeq *seq, const std::vector<int64_t> &todo,
                    int32_t fs, std::vector<DhNwPairOut> &out, std::vector<uint8_t> &stage)
{
    const NwRun r{ctx, seq, d_ref, d_qry, fs, &out, &stage};
    const int64_t budget = nw_budget_words(), w0 = nw_first_w();
    std::vector<Job> jobs, again;
    for (int64_t p : todo) {
        Job jb;
        jb.pair = p;
        jb.w = 0;
        again.push_back(jb);
    }
    while (!again.empty()) {
        jobs.clear();
        for (Job jb : again) {
            const int32_t rl = seq[jb.pair].rl, ql = seq[jb.pair].ql;
            jb.w = nw::next_w(rl, ql, fs, jb.w, w0);
            if (jb.w < 0) {
                PairOut &o = out[(size_t)jb.pair];
                o.status = DH_NW_BAND_EXCEEDED;
                o.score = -1;
                o.nops = 0;
                continue;
            }
            jb.b = nw::band(rl, ql, jb.w, fs);
            const int32_t W = jb.b.hi - jb.b.lo + 1;
            if (!nw::band_class(W, jb.cpl, jb.ns)) return dh_fail(DH_EHIP, "dh_nw_batch: no kernel class for a planned band");
            jb.words = (int64_t)rl * ((W + jb.cpl - 1) / jb.cpl);
            jobs.push_back(jb);
        }
        again.clear();
        std::stable_sort(jobs.begin(), jobs.end(), [](const Job &a, const Job &b) { return a.cpl != b.cpl ? a.cpl < b.cpl : a.ns < b.ns; });
        for (size_t j0 = 0, j1; j0 < jobs.size(); j0 = j1) {
            int64_t words = jobs[j0].words;
            for (j1 = j0 + 1; j1 < jobs.size() && words + jobs[j1].words <= budget; j1++) words += jobs[j1].words;
            if (int rc = run_launch(r, jobs, j0, j1, again)) return rc;
        }
    }
    return DH_OK;
}

extern "C" int dh_nw_batch(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry, const int64_t *qry_off,
                           int64_t n, int32_t free_shift, dh_edit_paths **out, int32_t *status)
{
    if (!ctx || !out || n < 0 || n > INT32_MAX || (n > 0 && (!ref_off || !qry_off))) return dh_fail(DH_EINVAL, "dh_nw_batch: bad argument");
    *out = nullptr;
    const int32_t fs = free_shift ? 1 : 0;
    // ---- validation on the host, before anything is launched
    if (n > 0 && (ref_off[0] < 0 || qry_off[0] < 0)) return dh_fail(DH_EINVAL, "dh_nw_batch: negative first offset");
    for (int64_t i = 0; i < n; i++) {
        const int64_t rl = ref_off[i + 1] - ref_off[i], ql = qry_off[i + 1] - qry_off[i];
        char msg[160];
        if (rl < 0 || ql < 0) {
            snprintf(msg, sizeof(msg), "dh_nw_batch: pair %lld: offsets decrease", (long long)i);
            return dh_fail(DH_EINVAL, msg);
        }
        if (rl > NW_MAX_LEN || ql > NW_MAX_LEN) {
            snprintf(msg, sizeof(msg), "dh_nw_batch: pair %lld: %lld x %lld bases exceed the limit of %d per sequence", (long long)i,
                     (long long)rl, (long long)ql, NW_MAX_LEN);
            return dh_fail(DH_EINVAL, msg);
        }
    }
    if (n > 0 && ((ref_off[n] > ref_off[0] && !ref) || (qry_off[n] > qry_off[0] && !qry)))
        return dh_fail(DH_EINVAL, "dh_nw_batch: sequences are NULL");
    std::vector<PairOut> po((size_t)n);
    std::vector<DhNwSeq> seq((size_t)n);
    std::vector<uint8_t> stage;
    // ---- chunks of consecutive pairs: the decision words of the first attempts within the budget, 256 MB of bases at most
    const int64_t budget = nw_budget_words(), w0 = nw_first_w();
    bool device_set = false;
    for (int64_t p0 = 0, p1; p0 < n; p0 = p1) {
        std::vector<int64_t> todo;
        int64_t words = 0, bases = 0;
        for (p1 = p0; p1 < n; p1++) {
            const int32_t rl = (int32_t)(ref_off[p1 + 1] - ref_off[p1]), ql = (int32_t)(qry_off[p1 + 1] - qry_off[p1]);
            if (rl == 0 || ql == 0) continue;  // answered below
            const int64_t w = nw::next_w(rl, ql, fs, 0, w0);
            int32_t cpl = 4, ns = 1;
            int64_t need = 0;
            if (w >= 0) {
                const int32_t W = nw::band_width(rl, ql, w, fs);
                nw::band_class(W, cpl, ns);
                need = (int64_t)rl * ((W + cpl - 1) / cpl);
            }
            if (!todo.empty() && (words + need > budget || bases + rl + ql > ((int64_t)1 << 28))) break;
            words += need;
            bases += (int64_t)rl + ql;
            todo.push_back(p1);
        }
        if (todo.empty()) continue;
        if (!device_set) {
            HIPCHK(hipSetDevice(ctx->device));
            device_set = true;
        }
        if (int rc = run_chunk(ctx, ref, ref_off, qry, qry_off, p0, p1, todo, fs, seq, po, stage)) return rc;
    }
    // ---- the result in pair order; a pair with an empty side is all insertions or all deletions (oracle/nw.c)
    std::unique_ptr<dh_edit_paths> p(new dh_edit_paths);
    p->score.assign((size_t)n, 0);
    p->op_off.assign((size_t)n + 1, 0);
    p->tile_off.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        const int64_t rl = ref_off[i + 1] - ref_off[i], ql = qry_off[i + 1] - qry_off[i];
        const PairOut &o = po[(size_t)i];
        const int64_t nops = (rl == 0 || ql == 0) ? rl + ql : o.nops;
        p->op_off[(size_t)i + 1] = p->op_off[(size_t)i] + nops;
    }
    p->ops.resize((size_t)p->op_off[(size_t)n]);
    for (int64_t i = 0; i < n; i++) {
        const int64_t rl = ref_off[i + 1] - ref_off[i], ql = qry_off[i + 1] - qry_off[i];
        const PairOut &o = po[(size_t)i];
        uint8_t *dst = p->ops.data() + p->op_off[(size_t)i];
        if (rl == 0 || ql == 0) {
            memset(dst, rl ? EP_OP_DEL : EP_OP_INS, (size_t)(rl + ql));
            p->score[(size_t)i] = fs ? 0 : (int32_t)(rl + ql);
        } else {
            if (o.nops) memcpy(dst, stage.data() + o.at, (size_t)o.nops);
            p->score[(size_t)i] = o.score;
        }
        if (status) status[i] = o.status;
    }
    *out = p.release();
    return DH_OK;
}
