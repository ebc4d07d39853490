// dh_checkgaps.cpp -- host side of dh_check_gaps: the gap analysis of `dentist check-results` on the device.  Kernels:
// dh_checkgaps.hip; lane code and the checks: dh_checkgaps.h.
//
// The call: everything is checked on the host; the mappings are sorted by input contig (stable: the caller's order decides among
// equals) and go up with the mapped intervals, the N-runs and the dust mask as one block.  k_cg_bind classifies every gap and writes
// the lengths of its pair; they come back once, because the aligner plans its bands and launch groups on the host (and their sum
// is checked in 64 bits).  Two scans (dhk_scan) turn the lengths into offsets, k_cg_gather writes the pairs from the DBs' device
// copies into the aligner's padded layout and says which queries are all n: those are not aligned.  dh_nwa_run_pairs runs the
// widening protocol, bounded by DH_NW_CHUNK_KB, and leaves the ops of every launch group in the staging vector.  The ops in gap
// order go up again with their offsets (the aligner's op buffer is rewritten by every launch group), k_cg_stats crops and counts,
// and its nine numbers per aligned gap are merged into the summaries.  DH_TRACE prints a line per call.
#include "dh_host.h"

#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>

#include "dh_checkgaps.h"
#include "dh_nw.h"

extern "C" void dhk_cg_bind(hipStream_t st, CgEnv e, int32_t count, CgSummary *sum, uint32_t *rlen, uint32_t *qlen);
extern "C" void dhk_cg_gather(hipStream_t st, const CgSummary *sum, int32_t count, const uint32_t *roff, const uint32_t *qoff,
                              const uint8_t *true_bases, const int64_t *true_off, const uint8_t *res_bases, const uint8_t *res_rc,
                              const int64_t *res_off, const int32_t *result_gap, uint8_t *ref, uint8_t *qry, uint32_t *has_base);
extern "C" void dhk_cg_stats(hipStream_t st, const CgSummary *sum, int32_t count, const uint32_t *roff, const uint32_t *qoff, const uint8_t *refs,
                             const uint8_t *qrys, const int64_t *op_off, const uint8_t *ops, const int64_t *dust_ptr, const int32_t *dust_iv,
                             int32_t crop, void *out);

static_assert(sizeof(CgSummary) == sizeof(dh_gap_summary) && sizeof(CgMap) == sizeof(dh_contig_mapping) && sizeof(dh_contig_mapping) == 32,
              "dh_checkgaps.h states the layouts");
static_assert(CG_UNKOWN == DH_GAP_UNKOWN && CG_BROKEN == DH_GAP_BROKEN && CG_UNCLOSED == DH_GAP_UNCLOSED && CG_PARTIAL == DH_GAP_PARTIALLY_CLOSED &&
                  CG_CLOSED == DH_GAP_CLOSED && CG_IGNORED == DH_GAP_IGNORED && CG_ST_NONE == DH_CG_NONE && CG_ST_OK == DH_CG_OK &&
                  CG_ST_EMPTY == DH_CG_EMPTY && CG_ST_BAND == DH_CG_BAND_EXCEEDED && CG_ST_LONG == DH_CG_TOO_LONG && CG_MAX_LEN == DH_NWA_MAX_LEN,
              "dh_checkgaps.h states the public values");
static_assert(CG_OP_MATCH == EP_OP_MATCH && CG_OP_DEL == EP_OP_DEL && CG_OP_INS == EP_OP_INS && CG_OP_MISMATCH == EP_OP_MISMATCH, "the ops are the edit paths'");

struct dh_gap_report {
    std::vector<dh_gap_summary> sum;
    dh_edit_paths paths;
    int64_t aligned = 0, groups = 0;
};

extern "C" int dh_check_gaps(dh_ctx *ctx, dh_db *true_db, dh_db *result_db, const int32_t *mapped, int32_t n_input, const dh_contig_mapping *maps,
                             int32_t nmaps, const int32_t *result_gap, const int64_t *dust_ptr, const int32_t *dust_iv, int32_t crop,
                             const dh_nw_scoring *scoring, int32_t first_contig, int32_t count, dh_gap_report **out)
{
    const std::string name("dh_check_gaps");
    if (!ctx || !true_db || !result_db || !out || n_input < 0 || nmaps < 0 || count < 0 || crop < 0 || (n_input > 0 && !mapped) ||
        (nmaps > 0 && !maps) || (result_db->n > 0 && !result_gap) || (dust_ptr == nullptr) != (dust_iv == nullptr))
        return dh_fail(DH_EINVAL, name + ": bad argument");
    *out = nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    if (scoring && (scoring->match < scoring->mismatch || 2 * (int64_t)scoring->gap_extend + scoring->match <= 0 || scoring->gap_open < 0))
        return dh_fail(DH_EINVAL, name + ": scoring refused (needs match >= mismatch, 2 gap_extend + match > 0, gap_open >= 0)");
    // ---- the mappings by input contig, then the checks
    std::vector<CgMap> sm((size_t)nmaps);
    for (int32_t k = 0; k < nmaps; k++)
        sm[(size_t)k] = CgMap{maps[k].ref_contig, maps[k].ref_begin, maps[k].ref_end, maps[k].ref_contig_length, maps[k].query_contig,
                              maps[k].duplicate != 0, maps[k].complement != 0, k};
    std::stable_sort(sm.begin(), sm.end(), [](const CgMap &a, const CgMap &b) { return a.query < b.query; });
    const int32_t n_true = true_db->n, n_res = result_db->n;
    char msg[200];
    {
        // (the lowest offender in the caller's order)
        std::vector<CgMap> by_index(sm);
        std::sort(by_index.begin(), by_index.end(), [](const CgMap &a, const CgMap &b) { return a.index < b.index; });
        if (cg::check(mapped, n_input, by_index.data(), nmaps, true_db->h_off.data(), n_true, result_db->h_off.data(), n_res, dust_ptr, dust_iv, crop,
                      first_contig, count, msg, sizeof(msg)))
            return dh_fail(DH_EINVAL, name + ": " + msg);
    }
    std::unique_ptr<dh_gap_report> rep(new dh_gap_report);
    rep->sum.resize((size_t)count);
    rep->paths.score.assign((size_t)count, 0);
    rep->paths.op_off.assign((size_t)count + 1, 0);
    rep->paths.tile_off.assign((size_t)count + 1, 0);
    if (count == 0) {
        *out = rep.release();
        return DH_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = dh_ensure_rc(result_db)) return rc;
    // ---- one block of input
    const int64_t ndust = dust_ptr ? dust_ptr[n_true] : 0;
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_mapped = take(sizeof(int32_t) * 3 * (size_t)n_input), o_maps = take(sizeof(CgMap) * (size_t)nmaps),
                 o_gap = take(sizeof(int32_t) * (size_t)n_res), o_dptr = take(dust_ptr ? sizeof(int64_t) * ((size_t)n_true + 1) : 0),
                 o_div = take(sizeof(int32_t) * 2 * (size_t)ndust);
    std::vector<char, PinnedAlloc<char>> h_in(at);
    memcpy(h_in.data() + o_mapped, mapped, sizeof(int32_t) * 3 * (size_t)n_input);
    if (nmaps) memcpy(h_in.data() + o_maps, sm.data(), sizeof(CgMap) * (size_t)nmaps);
    if (n_res) memcpy(h_in.data() + o_gap, result_gap, sizeof(int32_t) * (size_t)n_res);
    if (dust_ptr) memcpy(h_in.data() + o_dptr, dust_ptr, sizeof(int64_t) * ((size_t)n_true + 1));
    if (ndust) memcpy(h_in.data() + o_div, dust_iv, sizeof(int32_t) * 2 * (size_t)ndust);
    char *d_in;
    if (int rc = dh_upload(ctx, SLOT_CG_IN, h_in.data(), h_in.size(), &d_in)) return rc;
    const int32_t *d_gap = (const int32_t *)(d_in + o_gap);
    const int64_t *d_dptr = dust_ptr ? (const int64_t *)(d_in + o_dptr) : nullptr;
    const int32_t *d_div = (const int32_t *)(d_in + o_div);
    // ---- bind, offsets
    CgSummary *d_sum;
    uint32_t *d_roff, *d_qoff, *d_sums;
    if (int rc = dh_scr(ctx, SLOT_CG_SUM, (size_t)count, &d_sum)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CG_ROFF, (size_t)count + 1, &d_roff)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CG_QOFF, (size_t)count + 1, &d_qoff)) return rc;
    const size_t nsums = (size_t)count / 2048 + 2;  // behind the scans' block sums: a word per pair, whether its query has a base
    if (int rc = dh_scr(ctx, SLOT_CG_SUMS, nsums + (size_t)count, &d_sums)) return rc;
    const CgEnv env{(const int32_t *)(d_in + o_mapped), (const CgMap *)(d_in + o_maps), d_gap, result_db->d_off, n_input, nmaps, crop, first_contig};
    dhk_cg_bind(st, env, count, d_sum, d_roff, d_qoff);
    HIPCHK(hipGetLastError());
    // the scans wrap at 2^32: the lengths are added up on the host first, from the summaries' own numbers
    std::vector<uint32_t> h_rlen((size_t)count + 1), h_qlen((size_t)count + 1);
    HIPCHK(hipMemcpyAsync(h_rlen.data(), d_roff, sizeof(uint32_t) * ((size_t)count + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_qlen.data(), d_qoff, sizeof(uint32_t) * ((size_t)count + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(rep->sum.data(), d_sum, sizeof(CgSummary) * (size_t)count, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::vector<DhNwSeq> seq((size_t)count);
    std::vector<int64_t> todo;
    int64_t rbytes = 0, qbytes = 0;
    for (int32_t g = 0; g < count; g++) {
        seq[(size_t)g] = DhNwSeq{NW_SEQ_PAD + rbytes, NW_SEQ_PAD + qbytes, (int32_t)h_rlen[(size_t)g], (int32_t)h_qlen[(size_t)g]};
        if (h_rlen[(size_t)g]) todo.push_back(g);
        rbytes += h_rlen[(size_t)g], qbytes += h_qlen[(size_t)g];
    }
    if (rbytes + qbytes >= ((int64_t)1 << 30)) return dh_fail(DH_EOVERFLOW, name + ": 2^30 bases of pairs or more");
    rep->aligned = (int64_t)todo.size();
    if (!todo.empty()) {
        dhk_scan(st, d_roff, (int64_t)count + 1, d_sums);
        dhk_scan(st, d_qoff, (int64_t)count + 1, d_sums);
        uint8_t *d_ref, *d_qry;
        if (int rc = dh_scr(ctx, SLOT_CG_REF, (size_t)rbytes + 2 * NW_SEQ_PAD, &d_ref)) return rc;
        if (int rc = dh_scr(ctx, SLOT_CG_QRY, (size_t)qbytes + 2 * NW_SEQ_PAD, &d_qry)) return rc;
        dhk_cg_gather(st, d_sum, count, d_roff, d_qoff, true_db->d_bases, true_db->d_off, result_db->d_bases, result_db->d_rc, result_db->d_off,
                      d_gap, d_ref, d_qry, d_sums + nsums);
        HIPCHK(hipGetLastError());
        // a query that is all n is not aligned (the early return of stretcher): only the gathered bytes tell
        std::vector<uint32_t> has_base((size_t)count);
        HIPCHK(hipMemcpyAsync(has_base.data(), d_sums + nsums, sizeof(uint32_t) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        size_t kept = 0;
        for (int64_t g : todo) {
            if (has_base[(size_t)g])
                todo[kept++] = g;
            else
                rep->sum[(size_t)g].align_status = DH_CG_EMPTY, h_rlen[(size_t)g] = 0;
        }
        todo.resize(kept);
        rep->aligned = (int64_t)kept;
        // ---- the alignments
        std::vector<DhNwPairOut> po((size_t)count);
        std::vector<uint8_t> stage;
        if (int rc = dh_nwa_run_pairs(ctx, d_ref, d_qry, seq.data(), todo, scoring, po, stage, &rep->groups)) return rc;
        std::vector<int64_t> &op_off = rep->paths.op_off;
        for (int32_t g = 0; g < count; g++) {
            const DhNwPairOut &o = po[(size_t)g];
            const bool ok = h_rlen[(size_t)g] && o.status == DH_NW_OK;
            if (h_rlen[(size_t)g] && !ok) rep->sum[(size_t)g].align_status = DH_CG_BAND_EXCEEDED;
            op_off[(size_t)g + 1] = op_off[(size_t)g] + (ok ? o.nops : 0);
            rep->paths.score[(size_t)g] = ok ? o.score : 0;
        }
        rep->paths.ops.resize((size_t)op_off[(size_t)count]);
        for (int32_t g = 0; g < count; g++)
            if (op_off[(size_t)g + 1] > op_off[(size_t)g])
                memcpy(rep->paths.ops.data() + op_off[(size_t)g], stage.data() + po[(size_t)g].at, (size_t)po[(size_t)g].nops);
        // ---- crop and count
        if (!rep->paths.ops.empty()) {
            const size_t off_bytes = (sizeof(int64_t) * ((size_t)count + 1) + 255) & ~(size_t)255,
                         st_bytes = (sizeof(CgStats) * (size_t)count + 255) & ~(size_t)255;
            char *d_ops;
            if (int rc = dh_scr(ctx, SLOT_CG_OPS, off_bytes + st_bytes + rep->paths.ops.size(), &d_ops)) return rc;
            HIPCHK(hipMemcpyAsync(d_ops, op_off.data(), sizeof(int64_t) * ((size_t)count + 1), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemcpyAsync(d_ops + off_bytes + st_bytes, rep->paths.ops.data(), rep->paths.ops.size(), hipMemcpyHostToDevice, st));
            dhk_cg_stats(st, d_sum, count, d_roff, d_qoff, d_ref, d_qry, (const int64_t *)d_ops, (const uint8_t *)(d_ops + off_bytes + st_bytes), d_dptr,
                         d_div, crop, d_ops + off_bytes);
            HIPCHK(hipGetLastError());
            std::vector<CgStats> hs((size_t)count);
            HIPCHK(hipMemcpyAsync(hs.data(), d_ops + off_bytes, sizeof(CgStats) * (size_t)count, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            for (int32_t g = 0; g < count; g++) {
                if (op_off[(size_t)g + 1] == op_off[(size_t)g]) continue;
                dh_gap_summary &s = rep->sum[(size_t)g];
                const CgStats &x = hs[(size_t)g];
                s.col_begin = x.col_begin, s.col_end = x.col_end, s.matches = x.matches;
                if (crop > 0) s.reference_length = x.reference_length, s.query_length = x.query_length;
                s.dust_ops = x.dust_ops, s.dust_matches = x.dust_matches, s.none_dust_ops = x.none_dust_ops, s.none_dust_matches = x.none_dust_matches;
            }
        }
    }
    if (getenv("DH_TRACE"))
        fprintf(stderr, "[checkgaps] %d gaps from contig %d, %d mappings, crop %d: %lld pairs, %lld + %lld bases, %lld launch groups, %lld ops; %.2f ms\n",
                count, first_contig, nmaps, crop, (long long)rep->aligned, (long long)rbytes, (long long)qbytes, (long long)rep->groups,
                (long long)rep->paths.ops.size(), dh_ms_since(t_call));
    *out = rep.release();
    return DH_OK;
}

extern "C" void dh_gap_report_destroy(dh_gap_report *r) { delete r; }
extern "C" int64_t dh_gap_report_count(const dh_gap_report *r) { return (int64_t)r->sum.size(); }
extern "C" const dh_gap_summary *dh_gap_report_summaries(const dh_gap_report *r) { return r->sum.data(); }
extern "C" const dh_edit_paths *dh_gap_report_paths(const dh_gap_report *r) { return &r->paths; }
extern "C" int64_t dh_gap_report_aligned(const dh_gap_report *r) { return r->aligned; }
extern "C" int64_t dh_gap_report_groups(const dh_gap_report *r) { return r->groups; }
