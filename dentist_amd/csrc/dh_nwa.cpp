// dh_nwa.cpp -- host side of dh_nw_affine_batch: global alignment of arbitrary sequence pairs with affine gap costs (the
// kernel is in dh_nwa.hip, the lane code, the cost form and the exactness argument in dh_nwa.h), and dh_format_pair, the
// EMBOSS `pair` text `dentist check-results` reads from stretcher (commands/checkResults.d:2113-2162).
//
// The call is dh_nw_batch's (dh_nw.cpp): the offsets and the scoring are validated before anything is launched, pairs with
// an empty side are answered here, the rest is cut into chunks of consecutive pairs whose decision words fit
// DH_NW_CHUNK_KB.  Every pair starts at half-width DH_NWA_W0 (default 64); k_nwa fills the band and walks it back, the host
// applies nwa::accepted to the cost it reports, and the pairs that fail run again, together, at twice the half-width -- in
// launch groups bounded by the same knob, one launch per kernel class -- until the band would exceed NWA_MAX_W columns:
// those get DH_NW_BAND_EXCEEDED.  k_edit_compact (dh_editpath.hip) puts the ops of a group in path order.
// dh_nwa_run_pairs is the same protocol for a caller whose pairs are on the device already (dh_check_gaps, dh_checkgaps.cpp).
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dh_nwa.h"

extern "C" void dhk_nwa(hipStream_t st, int cpl, int ns, const NwPair *pairs, int32_t n, const uint8_t *refs, const uint8_t *qrys,
                        NwaCost c, uint64_t *dm, int64_t dm_words, uint64_t *ow, int64_t ow_words, EpResult *res);
extern "C" void dhk_edit_compact(hipStream_t st, const EpCopy *cp, int32_t n, const uint64_t *ow_fast, const uint64_t *ow_general,
                                 uint8_t *out);

namespace {

static_assert(NWA_MAX_LEN == DH_NWA_MAX_LEN && NWA_MAX_W == DH_NWA_MAX_BAND, "the header states the kernel's limits");

const dh_nw_scoring kDefaultScoring = {5, -4, 16, 4};  // EDNAFULL, gapopen 16, gapextend 4: nucleotide stretcher

int64_t nwa_budget_words()  // decision words (64 bits) per launch group
{
    return dh_env_knob("DH_NW_CHUNK_KB", 1 << 20, 1, INT64_MAX) * 128;  // development; no upper bound
}

int64_t nwa_first_w()
{
    return dh_env_knob("DH_NWA_W0", 64, 1, NWA_MAX_W);  // development
}

struct Job {
    int64_t pair;  // index in the call
    int64_t w;
    nw::Band b;
    int32_t cpl, ns;
    int64_t words;  // decision words
};

using PairOut = DhNwPairOut;

struct NwaRun {
    dh_ctx *ctx;
    const DhNwSeq *seq;  // by pair: where its sequences start in the device buffers, and their lengths
    const uint8_t *d_ref, *d_qry;
    NwaCost cost;
    std::vector<PairOut> *out;
    std::vector<uint8_t> *stage;
    int64_t *groups;  // launch groups run (NULL: not counted)
};

// jobs [j0, j1) (sorted by class) as one launch group; the rejected ones are appended to `again`
int run_launch(const NwaRun &r, const std::vector<Job> &jobs, size_t j0, size_t j1, std::vector<Job> &again)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = ctx->stream;
    const size_t n = j1 - j0;
    if (r.groups) ++*r.groups;
    std::vector<NwPair> pairs(n);
    int64_t dm_words = 0, ow_words = 0;
    for (size_t k = 0; k < n; k++) {
        const Job &jb = jobs[j0 + k];
        NwPair &p = pairs[k];
        p.roff = r.seq[jb.pair].roff;
        p.qoff = r.seq[jb.pair].qoff;
        p.rl = r.seq[jb.pair].rl;
        p.ql = r.seq[jb.pair].ql;
        p.lo = jb.b.lo;
        p.hi = jb.b.hi;
        p.dm_off = dm_words;
        p.ow_off = ow_words;
        dm_words += jb.words;
        ow_words += ((int64_t)p.rl + p.ql + 7) >> 3;
    }
    NwPair *d_pairs;
    uint64_t *d_dm, *d_ow;
    EpResult *d_res;
    if (int rc = dh_scr(ctx, SLOT_NWA_PAIRS, n, &d_pairs)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NWA_DM, (size_t)dm_words, &d_dm)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NWA_OW, (size_t)ow_words, &d_ow)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NWA_RES, n, &d_res)) return rc;
    HIPCHK(hipMemcpyAsync(d_pairs, pairs.data(), sizeof(NwPair) * n, hipMemcpyHostToDevice, st));
    for (size_t a = 0, b; a < n; a = b) {  // one launch per class
        for (b = a + 1; b < n && jobs[j0 + b].cpl == jobs[j0 + a].cpl && jobs[j0 + b].ns == jobs[j0 + a].ns; b++) {}
        dhk_nwa(st, jobs[j0 + a].cpl, jobs[j0 + a].ns, d_pairs + a, (int32_t)(b - a), r.d_ref, r.d_qry, r.cost, d_dm, dm_words, d_ow,
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
        if (!walked && jb.b.full) return dh_fail(DH_EHIP, "dh_nw_affine_batch: the kernel refused a pair the host planned");
        if (!walked || !nwa::accepted((int64_t)res[k].score, jb.w, r.cost.ce, jb.b.full)) {
            again.push_back(jb);
            continue;
        }
        cp.push_back(EpCopy{pairs[k].ow_off, 1, total, (int32_t)res[k].nops, 1});
        PairOut &o = (*r.out)[(size_t)jb.pair];
        o.at = (int64_t)r.stage->size() + total;
        o.nops = (int32_t)res[k].nops;
        o.score = nwa::score_of(r.cost, pairs[k].rl, pairs[k].ql, (int64_t)res[k].score);
        total += res[k].nops;
    }
    if (total == 0) return DH_OK;
    EpCopy *d_cp;
    uint8_t *d_out;
    if (int rc = dh_scr(ctx, SLOT_NWA_COPY, cp.size(), &d_cp)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NWA_OPS, (size_t)total, &d_out)) return rc;
    HIPCHK(hipMemcpyAsync(d_cp, cp.data(), sizeof(EpCopy) * cp.size(), hipMemcpyHostToDevice, st));
    dhk_edit_compact(st, d_cp, (int32_t)cp.size(), nullptr, d_ow, d_out);
    HIPCHK(hipGetLastError());
    const size_t at = r.stage->size();
    r.stage->resize(at + (size_t)total);
    HIPCHK(hipMemcpyAsync(r.stage->data() + at, d_out, (size_t)total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}

// decision words of a pair at half-width w (w >= 0), and its class
bool plan(int32_t rl, int32_t ql, int64_t w, Job &jb)
{
    jb.w = w;
    jb.b = nw::band(rl, ql, w, 0);
    const int32_t W = jb.b.hi - jb.b.lo + 1;
    if (!nwa::band_class(W, jb.cpl, jb.ns)) return false;
    jb.words = (int64_t)rl * nwa::row_words(W);
    return true;
}

// the pairs `todo` whose sequences are on the device: attempts at growing half-widths until every pair is accepted or given up
int run_pairs(const NwaRun &r, const std::vector<int64_t> &todo)
{
    const DhNwSeq *seq = r.seq;
    std::vector<PairOut> &out = *r.out;
    const int64_t budget = nwa_budget_words(), w0 = nwa_first_w();
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
            const int64_t w = nwa::next_w(rl, ql, jb.w, w0);
            if (w < 0) {
                PairOut &o = out[(size_t)jb.pair];
                o.status = DH_NW_BAND_EXCEEDED;
                o.score = -1;
                o.nops = 0;
                continue;
            }
            if (!plan(rl, ql, w, jb)) return dh_fail(DH_EHIP, "dh_nw_affine_batch: no kernel class for a planned band");
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

// the device pairs `todo` of chunk [p0, p1): their bases go up as one range, `seq` (one entry per pair of the call) gets theirs
int run_chunk(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry, const int64_t *qry_off, int64_t p0,
              int64_t p1, const std::vector<int64_t> &todo, const NwaCost &cost, std::vector<DhNwSeq> &seq, std::vector<PairOut> &out,
              std::vector<uint8_t> &stage)
{
    hipStream_t st = ctx->stream;
    const int64_t rbytes = ref_off[p1] - ref_off[p0], qbytes = qry_off[p1] - qry_off[p0];
    uint8_t *d_ref, *d_qry;
    if (int rc = dh_scr(ctx, SLOT_NWA_REF, (size_t)rbytes + 2 * NW_SEQ_PAD, &d_ref)) return rc;
    if (int rc = dh_scr(ctx, SLOT_NWA_QRY, (size_t)qbytes + 2 * NW_SEQ_PAD, &d_qry)) return rc;
    if (rbytes) HIPCHK(hipMemcpyAsync(d_ref + NW_SEQ_PAD, ref + ref_off[p0], (size_t)rbytes, hipMemcpyHostToDevice, st));
    if (qbytes) HIPCHK(hipMemcpyAsync(d_qry + NW_SEQ_PAD, qry + qry_off[p0], (size_t)qbytes, hipMemcpyHostToDevice, st));
    for (int64_t p = p0; p < p1; p++)
        seq[(size_t)p] = DhNwSeq{NW_SEQ_PAD + ref_off[p] - ref_off[p0], NW_SEQ_PAD + qry_off[p] - qry_off[p0], (int32_t)(ref_off[p + 1] - ref_off[p]),
                                 (int32_t)(qry_off[p + 1] - qry_off[p])};
    return run_pairs(NwaRun{ctx, seq.data(), d_ref, d_qry, cost, &out, &stage, nullptr}, todo);
}

}  // namespace

// The same protocol on pairs whose sequences the caller left on the device (dh_check_gaps): d_ref / d_qry carry NW_SEQ_PAD bytes in
// front of the first and behind the last sequence, seq[p] says where pair p lies; sc is a scoring dh_nw_affine_batch accepts and
// no sequence is empty or longer than DH_NWA_MAX_LEN (DH_EINVAL otherwise).  The ops of the accepted pairs are appended to `stage`.
int dh_nwa_run_pairs(dh_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_qry, const DhNwSeq *seq, const std::vector<int64_t> &todo,
                     const dh_nw_scoring *sc, std::vector<DhNwPairOut> &out, std::vector<uint8_t> &stage, int64_t *groups)
{
    NwaCost cost;
    if (!sc) sc = &kDefaultScoring;
    if (!nwa::costs(sc->match, sc->mismatch, sc->gap_open, sc->gap_extend, cost)) return dh_fail(DH_EINVAL, "dh_nwa_run_pairs: scoring refused");
    for (int64_t p : todo)
        if (seq[p].rl < 1 || seq[p].ql < 1 || seq[p].rl > NWA_MAX_LEN || seq[p].ql > NWA_MAX_LEN)
            return dh_fail(DH_EINVAL, "dh_nwa_run_pairs: a pair is empty or too long");
    return run_pairs(NwaRun{ctx, seq, d_ref, d_qry, cost, &out, &stage, groups}, todo);
}

extern "C" int dh_nw_affine_batch(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off, const uint8_t *qry, const int64_t *qry_off,
                                  int64_t n, const dh_nw_scoring *sc, dh_edit_paths **out, int32_t *status)
{
    if (!ctx || !out || n < 0 || n > INT32_MAX || (n > 0 && (!ref_off || !qry_off)))
        return dh_fail(DH_EINVAL, "dh_nw_affine_batch: bad argument");
    *out = nullptr;
    if (!sc) sc = &kDefaultScoring;
    // ---- validation on the host, before anything is launched
    NwaCost cost;
    if (!nwa::costs(sc->match, sc->mismatch, sc->gap_open, sc->gap_extend, cost))
        return dh_fail(DH_EINVAL, "dh_nw_affine_batch: scoring refused (needs match >= mismatch, 2 gap_extend + match > 0, gap_open >= 0, "
                                  "and costs that cannot overflow on two sequences of DH_NWA_MAX_LEN)");
    if (n > 0 && (ref_off[0] < 0 || qry_off[0] < 0)) return dh_fail(DH_EINVAL, "dh_nw_affine_batch: negative first offset");
    for (int64_t i = 0; i < n; i++) {
        const int64_t rl = ref_off[i + 1] - ref_off[i], ql = qry_off[i + 1] - qry_off[i];
        char msg[160];
        if (rl < 0 || ql < 0) {
            snprintf(msg, sizeof(msg), "dh_nw_affine_batch: pair %lld: offsets decrease", (long long)i);
            return dh_fail(DH_EINVAL, msg);
        }
        if (rl > NWA_MAX_LEN || ql > NWA_MAX_LEN) {
            snprintf(msg, sizeof(msg), "dh_nw_affine_batch: pair %lld: %lld x %lld bases exceed the limit of %d per sequence",
                     (long long)i, (long long)rl, (long long)ql, NWA_MAX_LEN);
            return dh_fail(DH_EINVAL, msg);
        }
    }
    if (n > 0 && ((ref_off[n] > ref_off[0] && !ref) || (qry_off[n] > qry_off[0] && !qry)))
        return dh_fail(DH_EINVAL, "dh_nw_affine_batch: sequences are NULL");
    std::vector<PairOut> po((size_t)n);
    std::vector<DhNwSeq> seq((size_t)n);
    std::vector<uint8_t> stage;
    // ---- chunks of consecutive pairs: the decision words of the first attempts within the budget, 256 MB of bases at most (those of
    // pairs with an empty side included: a chunk's bases are uploaded as one range)
    const int64_t budget = nwa_budget_words(), w0 = nwa_first_w();
    bool device_set = false;
    for (int64_t p0 = 0, p1; p0 < n; p0 = p1) {
        std::vector<int64_t> todo;
        int64_t words = 0, bases = 0;
        for (p1 = p0; p1 < n; p1++) {
            const int32_t rl = (int32_t)(ref_off[p1 + 1] - ref_off[p1]), ql = (int32_t)(qry_off[p1 + 1] - qry_off[p1]);
            const bool device = rl > 0 && ql > 0;  // else answered below; its bases are uploaded with the chunk all the same
            const int64_t w = device ? nwa::next_w(rl, ql, 0, w0) : -1;
            Job jb;
            const int64_t need = (w >= 0 && plan(rl, ql, w, jb)) ? jb.words : 0;
            if ((!todo.empty() && words + need > budget) || (bases > 0 && bases + rl + ql > ((int64_t)1 << 28))) break;
            words += need;
            bases += (int64_t)rl + ql;
            if (device) todo.push_back(p1);
        }
        if (todo.empty()) continue;
        if (!device_set) {
            HIPCHK(hipSetDevice(ctx->device));
            device_set = true;
        }
        if (int rc = run_chunk(ctx, ref, ref_off, qry, qry_off, p0, p1, todo, cost, seq, po, stage)) return rc;
    }
    // ---- the result in pair order; a pair with an empty side is one gap
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
            if (rl + ql) memset(dst, rl ? EP_OP_DEL : EP_OP_INS, (size_t)(rl + ql));
            p->score[(size_t)i] = nwa::score_of(cost, rl, ql, nwa::gap_cost(cost, rl + ql));
        } else {
            if (o.nops) memcpy(dst, stage.data() + o.at, (size_t)o.nops);
            p->score[(size_t)i] = o.score;
        }
        if (status) status[i] = o.status;
    }
    *out = p.release();
    return DH_OK;
}

// EMBOSS `pair` text of one alignment.  What check-results parses (checkResults.d:2113-2162): a comment line
// "# Identity: n/m", and exactly three lines that are neither empty nor comments when width >= nops -- sequence, markup,
// sequence, the markup starting in the column the sequences start in.  The other header lines follow EMBOSS's documented
// layout and are not pinned by anything here.
extern "C" int64_t dh_format_pair(const char *name_a, const uint8_t *a, int64_t la, const char *name_b, const uint8_t *b, int64_t lb,
                                  const uint8_t *ops, int64_t nops, int32_t score, const dh_nw_scoring *sc, int64_t width, char *out,
                                  int64_t cap)
{
    if (!name_a || !name_b || la < 0 || lb < 0 || nops < 0 || width < 0 || (nops > 0 && !ops) || (la > 0 && !a) || (lb > 0 && !b))
        return dh_fail(DH_EINVAL, "dh_format_pair: bad argument");
    if (!sc) sc = &kDefaultScoring;
    auto chr = [](uint8_t x) -> char {
        if (x < 5) return "ACGTN"[x];
        const char u = (char)(x >= 'a' && x <= 'z' ? x - 32 : x);
        return (u == 'A' || u == 'C' || u == 'G' || u == 'T') ? u : 'N';
    };
    std::string l[3];
    for (int k = 0; k < 3; k++) l[k].reserve((size_t)nops);
    int64_t i = 0, j = 0, ident = 0, gaps = 0;
    for (int64_t k = 0; k < nops; k++) {
        const uint8_t op = ops[k];
        if (op > 3) return dh_fail(DH_EINVAL, "dh_format_pair: op code above 3");
        if ((op != EP_OP_INS && i >= la) || (op != EP_OP_DEL && j >= lb))
            return dh_fail(DH_EINVAL, "dh_format_pair: the ops consume more bases than the sequences have");
        l[0] += op == EP_OP_INS ? '-' : chr(a[i++]);
        l[2] += op == EP_OP_DEL ? '-' : chr(b[j++]);
        l[1] += op == EP_OP_MATCH ? '|' : (op == EP_OP_MISMATCH ? '.' : ' ');
        ident += op == EP_OP_MATCH;
        gaps += op == EP_OP_INS || op == EP_OP_DEL;
    }
    char line[512];
    std::string s = "########################################\n# Program: stretcher\n# Align_format: pair\n# Report_file: stdout\n"
                    "########################################\n\n#=======================================\n#\n# Aligned_sequences: 2\n";
    s += std::string("# 1: ") + name_a + "\n# 2: " + name_b + "\n";
    if (sc->match == 5 && sc->mismatch == -4)
        s += "# Matrix: EDNAFULL\n";
    else {
        snprintf(line, sizeof(line), "# Matrix: match %d mismatch %d\n", sc->match, sc->mismatch);
        s += line;
    }
    const double pct = nops ? 100.0 / (double)nops : 0.0;
    snprintf(line, sizeof(line),
             "# Gap_penalty: %d\n# Extend_penalty: %d\n#\n# Length: %lld\n# Identity:   %7lld/%lld (%4.1f%%)\n"
             "# Similarity: %7lld/%lld (%4.1f%%)\n# Gaps:       %7lld/%lld (%4.1f%%)\n# Score: %d\n#\n#\n"
             "#=======================================\n\n",
             sc->gap_open, sc->gap_extend, (long long)nops, (long long)ident, (long long)nops, pct * (double)ident, (long long)ident,
             (long long)nops, pct * (double)ident, (long long)gaps, (long long)nops, pct * (double)gaps, score);
    s += line;
    const int64_t step = (width == 0 || width > nops) ? std::max<int64_t>(nops, 1) : width;
    int64_t pa = 0, pb = 0;  // bases of a / b in front of the block
    for (int64_t c0 = 0; c0 < nops; c0 += step) {
        const std::string ta = l[0].substr((size_t)c0, (size_t)step), tm = l[1].substr((size_t)c0, (size_t)step),
                          tb = l[2].substr((size_t)c0, (size_t)step);
        const int64_t na = (int64_t)ta.size() - (int64_t)std::count(ta.begin(), ta.end(), '-');
        const int64_t nb = (int64_t)tb.size() - (int64_t)std::count(tb.begin(), tb.end(), '-');
        snprintf(line, sizeof(line), "%-13.13s %6lld ", name_a, (long long)(na ? pa + 1 : pa));
        s += line + ta;
        snprintf(line, sizeof(line), " %6lld\n", (long long)(pa + na));
        s += line + std::string(21, ' ') + tm + "\n";
        snprintf(line, sizeof(line), "%-13.13s %6lld ", name_b, (long long)(nb ? pb + 1 : pb));
        s += line + tb;
        snprintf(line, sizeof(line), " %6lld\n\n", (long long)(pb + nb));
        s += line;
        pa += na;
        pb += nb;
    }
    s += "\n#---------------------------------------\n#---------------------------------------\n";
    if (out && cap > (int64_t)s.size()) memcpy(out, s.c_str(), s.size() + 1);
    return (int64_t)s.size();
}
