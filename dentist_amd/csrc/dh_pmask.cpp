// dh_pmask.cpp -- host side of dh_la_propagate_mask: `dentist propagate-mask` (commands/propagateMask.d:136-305) on the device,
// with the union taken on a bitmap of the destination bases.  Kernels: dh_pmask.hip; lane code, layouts and the plan: dh_pmask.h.
//
// The call: the mask, the records and the layout are checked on the host threads (all of it before the first launch); the
// compact records, the mask and the bit offsets are uploaded (the trace values too, unless the set holds them on the device);
// k_pm_plan counts every record's intersecting intervals, two scans per launch group place them and compact the records that
// have any; k_pm_translate writes the raw list once; then, per destination range, the bitmap is cleared, painted and read
// out as runs, which come back in one copy per range.  DH_TRACE prints a line per stage.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "dh_pmask.h"

using pm::Raw;
using pm::Rec;

extern "C" void dhk_pm_plan(hipStream_t st, const Rec *recs, int64_t n, const int64_t *mask_ptr, const int32_t *mask_iv, int64_t *lo,
                            uint32_t *cnt, uint32_t *off, uint32_t *has);
extern "C" void dhk_pm_compact(hipStream_t st, const uint32_t *cnt, const uint32_t *has, int64_t i0, int64_t n, int64_t *list);
extern "C" void dhk_pm_translate(hipStream_t st, const Rec *recs, const int64_t *list, int64_t nlist, const int64_t *lo, const uint32_t *cnt,
                                 const uint32_t *off, const uint16_t *trace, int32_t ts, const int32_t *mask_iv, Raw *raw,
                                 unsigned long long *bad, unsigned long long *nonempty);
extern "C" void dhk_pm_paint(hipStream_t st, const Raw *raw, int64_t n, const int64_t *boff, int32_t r0, int32_t r1, int64_t base_bit,
                             uint32_t *bm);
extern "C" void dhk_pm_runs_count(hipStream_t st, const uint32_t *bm, int64_t ngroups, uint32_t *cs, uint32_t *ce);
extern "C" void dhk_pm_runs_emit(hipStream_t st, const uint32_t *bm, int64_t ngroups, int64_t base_bit, const int64_t *boff, int32_t r0,
                                 int32_t r1, const uint32_t *soff, const uint32_t *eoff, int32_t *iv, int64_t k0, int64_t *ptr);

struct dh_mask_result {
    std::vector<int64_t> ptr;
    std::vector<int32_t> iv;
    int64_t raw = 0, hit = 0;
    int32_t passes = 0;
};
static_assert(sizeof(Rec) == 40 && sizeof(Raw) == 12, "dh_pmask.h states the layouts");

namespace {

// h_trace or d_trace: where the trace values are (exactly one is used when trace_len > 0)
int propagate(dh_ctx *ctx, const char *fn, const dh_la *las, int64_t n, const uint16_t *h_trace, const uint16_t *d_trace, int64_t trace_len,
              int32_t tspace, const int64_t *mask_ptr, const int32_t *mask_iv, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
              dh_mask_result **out)
{
    const std::string name(fn);
    if (!ctx || !out || n < 0 || (n > 0 && !las) || trace_len < 0 || (trace_len > 0 && !h_trace && !d_trace) || tspace < 1 || ncontigs < 0 ||
        nreads < 0 || !mask_ptr || !read_off || (ncontigs > 0 && mask_ptr[ncontigs] > mask_ptr[0] && !mask_iv))
        return dh_fail(DH_EINVAL, name + ": bad argument");
    *out = nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    const bool trace_on = getenv("DH_TRACE") != nullptr;
    const int64_t cap_bits = dh_env_knob("DH_PMASK_BITMAP_MB", 4096, 1, 65536) << 23;
    const int64_t group_raw = dh_env_knob("DH_PMASK_GROUP_RAW", (int64_t)1 << 31, 1, (int64_t)1 << 31);  // development
    // ---- the plan, before anything is launched
    pm::Plan pl;
    pm::Fault f;
    pm::build_plan(las, n, trace_len, tspace, mask_ptr, mask_iv, ncontigs, read_off, nreads, group_raw, cap_bits,
                   dh_plan_runner<DH_PLAN_GRAIN>, pl, f);
    if (f.contig >= 0) return dh_fail(DH_EINVAL, name + ": the mask of contig " + std::to_string(f.contig) + " has " + f.what);
    if (f.contig == -2) return dh_fail(DH_EINVAL, name + ": " + f.what);
    if (f.record >= 0) return dh_fail(DH_EINVAL, name + ": record " + std::to_string(f.record) + ": " + f.what);
    std::unique_ptr<dh_mask_result> res(new dh_mask_result);
    res->ptr.assign((size_t)nreads + 1, 0);
    const int64_t nmask = ncontigs > 0 ? mask_ptr[ncontigs] : 0;
    if (n == 0 || nmask == 0 || nreads == 0) {
        *out = res.release();
        return DH_OK;
    }
    const double ms_plan = dh_ms_since(t_call);
    // ---- upload
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const size_t ngr = pl.group_at.size() - 1;
    Rec *d_recs;
    int64_t *d_mask_ptr, *d_boff, *d_lo, *d_list, *d_ptr;
    int32_t *d_mask_iv, *d_iv;
    uint16_t *d_tr_up = nullptr;
    uint32_t *d_cnt, *d_off, *d_has, *d_sums, *d_bm, *d_cs, *d_ce;
    unsigned long long *d_total;
    Raw *d_raw;
    if (int rc = dh_upload(ctx, SLOT_PM_RECS, pl.recs.data(), (size_t)n, &d_recs)) return rc;
    if (int rc = dh_upload(ctx, SLOT_PM_MASK_PTR, mask_ptr, (size_t)ncontigs + 1, &d_mask_ptr)) return rc;
    if (int rc = dh_upload(ctx, SLOT_PM_MASK_IV, mask_iv, (size_t)(2 * mask_ptr[ncontigs]), &d_mask_iv)) return rc;
    if (int rc = dh_upload(ctx, SLOT_PM_BOFF, pl.boff.data(), pl.boff.size(), &d_boff)) return rc;
    if (!d_trace && trace_len > 0) {
        if (int rc = dh_upload(ctx, SLOT_PM_TRACE, h_trace, (size_t)trace_len, &d_tr_up)) return rc;
        d_trace = d_tr_up;
    }
    if (int rc = dh_scr(ctx, SLOT_PM_LO, (size_t)n, &d_lo)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_CNT, (size_t)n, &d_cnt)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_OFF, (size_t)n, &d_off)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_HAS, (size_t)n, &d_has)) return rc;
    // counters: [0] the lowest record whose trace runs past its read, [1] non-empty raw intervals, then per launch group its
    // raw intervals and its records with any
    if (int rc = dh_scr(ctx, SLOT_PM_TOTAL, 2 + 2 * ngr, &d_total)) return rc;
    HIPCHK(hipMemsetAsync(d_total, 0xFF, sizeof(unsigned long long), st));
    HIPCHK(hipMemsetAsync(d_total + 1, 0, sizeof(unsigned long long) * (1 + 2 * ngr), st));
    if (trace_on) HIPCHK(hipStreamSynchronize(st));
    const double ms_upload = dh_ms_since(t_call) - ms_plan;
    // ---- which intervals every record meets, and where they go
    auto t0 = std::chrono::steady_clock::now();
    int64_t max_group = 0;
    for (size_t g = 0; g < ngr; g++) max_group = std::max(max_group, pl.group_at[g + 1] - pl.group_at[g]);
    const int64_t max_words = pm::padded_words(pl.max_range_bits), max_groups = max_words / PM_GROUP_WORDS;
    if (int rc = dh_scr(ctx, SLOT_PM_SUMS, (size_t)std::max(max_groups, max_group) / 2048 + 1, &d_sums)) return rc;
    dhk_pm_plan(st, d_recs, n, d_mask_ptr, d_mask_iv, d_lo, d_cnt, d_off, d_has);
    for (size_t g = 0; g < ngr; g++) {
        const int64_t g0 = pl.group_at[g], ng = pl.group_at[g + 1] - g0;
        if (ng <= 0) continue;
        dhk_scan_total(st, d_off + g0, ng, d_sums, d_total + 2 + 2 * g);
        dhk_scan_total(st, d_has + g0, ng, d_sums, d_total + 3 + 2 * g);
    }
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> totals(2 + 2 * ngr);
    HIPCHK(hipMemcpyAsync(totals.data(), d_total, sizeof(unsigned long long) * totals.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    int64_t nraw = 0, nhit = 0;
    for (size_t g = 0; g < ngr; g++) {
        if (totals[2 + 2 * g] > (unsigned long long)UINT32_MAX) return dh_fail(DH_EOVERFLOW, name + ": a launch group has 2^32 raw intervals or more");
        nraw += (int64_t)totals[2 + 2 * g];
        nhit += (int64_t)totals[3 + 2 * g];
    }
    res->hit = nhit;
    const double ms_count = dh_ms_since(t0);
    if (nraw == 0) {
        *out = res.release();
        return DH_OK;
    }
    // ---- the raw list, written once
    t0 = std::chrono::steady_clock::now();
    if (int rc = dh_scr(ctx, SLOT_PM_RAW, (size_t)nraw, &d_raw)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_LIST, (size_t)nhit, &d_list)) return rc;
    int64_t raw_at = 0, list_at = 0;
    for (size_t g = 0; g < ngr; g++) {
        const int64_t g0 = pl.group_at[g], ng = pl.group_at[g + 1] - g0, hits = (int64_t)totals[3 + 2 * g];
        if (hits > 0) {
            dhk_pm_compact(st, d_cnt, d_has, g0, ng, d_list + list_at);
            dhk_pm_translate(st, d_recs, d_list + list_at, hits, d_lo, d_cnt, d_off, d_trace, tspace, d_mask_iv, d_raw + raw_at, d_total,
                             d_total + 1);
        }
        raw_at += (int64_t)totals[2 + 2 * g];
        list_at += hits;
    }
    HIPCHK(hipGetLastError());
    unsigned long long found[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(found, d_total, sizeof(found), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (found[0] != ~0ull) {
        const dh_la &l = las[found[0]];
        char msg[240];
        snprintf(msg, sizeof(msg), "%s: record %llu: a translated position lies outside [0, %lld]: the b-bases of its trace run past read %d "
                 "(bbpos %d)", fn, found[0], (long long)(read_off[l.bread + 1] - read_off[l.bread]), l.bread, l.bbpos);
        return dh_fail(DH_EINVAL, msg);
    }
    res->raw = (int64_t)found[1];
    const double ms_translate = dh_ms_since(t0);
    // ---- per destination range: clear, paint, read out
    const size_t npass = pl.range_at.size() - 1;
    if (int rc = dh_scr(ctx, SLOT_PM_BITMAP, (size_t)max_words, &d_bm)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_CS, (size_t)max_groups, &d_cs)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_CE, (size_t)max_groups, &d_ce)) return rc;
    if (int rc = dh_scr(ctx, SLOT_PM_PTR, (size_t)nreads + 1, &d_ptr)) return rc;
    double ms_paint = 0, ms_runs = 0, ms_down = 0;
    int64_t k0 = 0;
    for (size_t p = 0; p < npass; p++) {
        const int32_t r0 = pl.range_at[p], r1 = pl.range_at[p + 1];
        const int64_t base_bit = pl.boff[(size_t)r0], words = pm::padded_words(pl.boff[(size_t)r1] - base_bit), groups = words / PM_GROUP_WORDS;
        t0 = std::chrono::steady_clock::now();
        HIPCHK(dhk_memset(st, d_bm, 0, sizeof(uint32_t) * (size_t)words));
        HIPCHK(hipMemsetAsync(d_total, 0, 2 * sizeof(unsigned long long), st));
        dhk_pm_paint(st, d_raw, nraw, d_boff, r0, r1, base_bit, d_bm);
        HIPCHK(hipGetLastError());
        if (trace_on) {
            HIPCHK(hipStreamSynchronize(st));
            ms_paint += dh_ms_since(t0);
            t0 = std::chrono::steady_clock::now();
        }
        dhk_pm_runs_count(st, d_bm, groups, d_cs, d_ce);
        dhk_scan_total(st, d_cs, groups, d_sums, d_total);
        dhk_scan_total(st, d_ce, groups, d_sums, d_total + 1);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(found, d_total, sizeof(found), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (found[0] != found[1]) return dh_fail(DH_EHIP, name + ": the bitmap's run starts and ends disagree");
        if (found[0] > (unsigned long long)UINT32_MAX) return dh_fail(DH_EOVERFLOW, name + ": 2^32 intervals or more in one destination range");
        const int64_t runs = (int64_t)found[0];
        if (int rc = dh_scr(ctx, SLOT_PM_IV, (size_t)(2 * runs), &d_iv)) return rc;
        dhk_pm_runs_emit(st, d_bm, groups, base_bit, d_boff, r0, r1, d_cs, d_ce, d_iv, k0, d_ptr);
        HIPCHK(hipGetLastError());
        if (trace_on) {
            HIPCHK(hipStreamSynchronize(st));
            ms_runs += dh_ms_since(t0);
            t0 = std::chrono::steady_clock::now();
        }
        res->iv.resize((size_t)(2 * (k0 + runs)));
        if (runs > 0) HIPCHK(hipMemcpyAsync(res->iv.data() + 2 * k0, d_iv, sizeof(int32_t) * (size_t)(2 * runs), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));  // (the next range reuses the run buffer)
        if (trace_on) ms_down += dh_ms_since(t0);
        k0 += runs;
    }
    t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(res->ptr.data(), d_ptr, sizeof(int64_t) * (size_t)nreads, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    res->ptr[(size_t)nreads] = k0;
    res->passes = (int32_t)npass;
    ms_down += dh_ms_since(t0);
    if (trace_on)
        fprintf(stderr,
                "[pmask] %lld records (%zu launch groups), %lld with a mask interval, %lld raw intervals (%lld non-empty), %lld trace values %s; "
                "%zu destination ranges of up to %lld MB; plan %.2f ms, upload %.2f ms, count+scan %.2f ms, compact+translate %.2f ms, "
                "clear+paint %.2f ms, runs %.2f ms, download %.2f ms, total %.2f ms; %lld intervals\n",
                (long long)n, ngr, (long long)nhit, (long long)nraw, (long long)res->raw, (long long)trace_len,
                d_tr_up ? "uploaded" : "on the device", npass, (long long)(max_words >> 18), ms_plan, ms_upload, ms_count, ms_translate, ms_paint,
                ms_runs, ms_down, dh_ms_since(t_call), (long long)k0);
    *out = res.release();
    return DH_OK;
}

}  // namespace

extern "C" int dh_la_propagate_mask(dh_ctx *ctx, const dh_la *las, int64_t n, const uint16_t *trace, int64_t trace_len, int32_t tspace,
                                    const int64_t *mask_ptr, const int32_t *mask_iv, int32_t ncontigs, const int64_t *read_off,
                                    int32_t nreads, dh_mask_result **out)
{
    return propagate(ctx, "dh_la_propagate_mask", las, n, trace, nullptr, trace_len, tspace, mask_ptr, mask_iv, ncontigs, read_off, nreads, out);
}

extern "C" int dh_la_set_propagate_mask(dh_ctx *ctx, const dh_la_set *set, const int64_t *mask_ptr, const int32_t *mask_iv,
                                        int32_t ncontigs, const int64_t *read_off, int32_t nreads, dh_mask_result **out)
{
    const dh_la *las;
    int64_t n;
    if (int rc = dh_set_host_records("dh_la_set_propagate_mask", ctx != nullptr, set, &las, &n)) return rc;
    const bool on_device = set->trace.empty() && set->d_trace_own_len > 0;
    if (on_device && set->device != ctx->device)
        return dh_fail(DH_EINVAL, "dh_la_set_propagate_mask: the set's trace values are on another device than the context");
    return propagate(ctx, "dh_la_set_propagate_mask", las, n, on_device ? nullptr : set->trace.data(),
                     on_device ? set->d_trace_own : nullptr, on_device ? set->d_trace_own_len : (int64_t)set->trace.size(), set->tspace,
                     mask_ptr, mask_iv, ncontigs, read_off, nreads, out);
}

extern "C" void dh_mask_result_destroy(dh_mask_result *m) { delete m; }
extern "C" int64_t dh_mask_result_count(const dh_mask_result *m) { return m ? (int64_t)m->iv.size() / 2 : 0; }
extern "C" const int64_t *dh_mask_result_ptr(const dh_mask_result *m) { return m ? m->ptr.data() : nullptr; }
extern "C" const int32_t *dh_mask_result_iv(const dh_mask_result *m) { return m ? m->iv.data() : nullptr; }
extern "C" int64_t dh_mask_result_raw(const dh_mask_result *m) { return m ? m->raw : 0; }
extern "C" int64_t dh_mask_result_hit(const dh_mask_result *m) { return m ? m->hit : 0; }
extern "C" int32_t dh_mask_result_passes(const dh_mask_result *m) { return m ? m->passes : 0; }
