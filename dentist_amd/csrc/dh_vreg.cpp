// dh_vreg.cpp -- host side of dh_la_validate_regions: `dentist validate-regions` (commands/validateRegions.d:141-512) on the
// device, every record bound to the regions it touches in one pass.  Kernels: dh_vreg.hip; lane code, layouts and the plan:
// dh_vreg.h.
//
// The call: the records and the regions are checked on the host threads (all of it before the first launch) and the regions are
// put in plan order; the compact records and the regions are uploaded; k_vr_bind counts per region its pairs, its pairs with
// windows and its spanning records; the counts come back and cut the plan into launch groups whose lists and slab parts fit
// DH_VREG_SLAB_MB.  Per group: the lists are written, the spanning records ordered, the regions' weak intervals counted, placed
// by the host and emitted; intervals and spanning ids come back in one copy each.  The results are put in input order and the
// mask is merged on the host.  DH_TRACE prints a line per call.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "dh_vreg.h"

using vr::Job;
using vr::Pair;
using vr::Rec;
using vr::Reg;

typedef unsigned long long u64;

extern "C" void dhk_vr_bind(hipStream_t st, int emit, const Rec *recs, int64_t i0, int64_t n, const int64_t *rptr, const Reg *regs, int64_t s0,
                            int64_t s1, u64 *cnt, const int64_t *at, u64 *cur, Pair *pairs, int64_t *span_idx);
extern "C" void dhk_vr_span(hipStream_t st, const Rec *recs, const int64_t *at, const u64 *cnt, int64_t s0, int64_t nreg, const int64_t *span_idx,
                            int32_t *span_out);
extern "C" void dhk_vr_region(hipStream_t st, int emit, const Job *jobs, int64_t nsmall, int64_t njobs, int64_t lds_entries, const Pair *pairs,
                              int32_t *slab, int32_t min_cov, uint32_t *rcnt, int32_t *iv);

struct dh_region_result {
    std::vector<dh_region_report> reports;
    std::vector<int32_t> weak;  // (contig, begin, end) triples in region order
    std::vector<int64_t> span_off, mask_ptr;
    std::vector<int32_t> span_ids, mask_iv;
    int64_t pairs = 0, big_regions = 0, groups = 0;
};
static_assert(sizeof(Rec) == 16 && sizeof(Reg) == 24 && sizeof(Pair) == 8 && sizeof(Job) == 48, "dh_vreg.h states the layouts");
static_assert(sizeof(u64) == sizeof(uint64_t), "the counters are read as uint64_t");

namespace {

int validate(dh_ctx *ctx, const char *fn, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const dh_region *regions,
             int32_t nregions, int32_t region_context, int32_t window, int32_t min_cov, int32_t min_span, dh_region_result **out)
{
    const std::string name(fn);
    if (!ctx || !out || (n > 0 && !las) || !contig_off || ncontigs < 0 || (nregions > 0 && !regions) || n < 0 || nregions < 0 ||
        region_context < 0 || window < 1)
        return dh_fail(DH_EINVAL, name + ": bad argument");
    *out = nullptr;
    const auto t_call = std::chrono::steady_clock::now();
    // 8192 entries = 32 KB of the 160 KB of a CU: five workgroups of 256 lanes per CU, and every region of up to 6 690 bases
    // (the default context and window) stays in LDS.  Above 16 000 a workgroup's array would not fit the 64 KB of a launch.
    const int64_t lds_windows = dh_env_knob("DH_VREG_LDS_WINDOWS", 8192, 2, 16000);  // development
    const int64_t budget = dh_env_knob("DH_VREG_SLAB_MB", 1024, 1, 65536) << 20;
    // ---- the plan, before anything is launched
    vr::Plan pl;
    vr::Fault f;
    vr::build_plan(las, n, contig_off, ncontigs, regions, nregions, region_context, window,
                   dh_plan_runner<DH_PLAN_GRAIN>, pl, f);
    if (f.contig >= 0) return dh_fail(DH_EINVAL, name + ": contig " + std::to_string(f.contig) + ": " + f.what);
    if (f.record >= 0) return dh_fail(DH_EINVAL, name + ": record " + std::to_string(f.record) + ": " + f.what);
    if (f.region >= 0) return dh_fail(DH_EINVAL, name + ": region " + std::to_string(f.region) + ": " + f.what);
    std::unique_ptr<dh_region_result> res(new dh_region_result);
    const size_t nreg = (size_t)nregions;
    res->reports.resize(nreg);
    res->span_off.assign(nreg + 1, 0);
    res->mask_ptr.assign((size_t)ncontigs + 1, 0);
    for (size_t s = 0; s < nreg; s++) vr::fill_report(pl.regs[s], 0, 0, min_span, &res->reports[(size_t)pl.perm[s]]);
    if (n == 0 || nregions == 0) {
        *out = res.release();
        return DH_OK;
    }
    // ---- upload and count
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Rec *d_recs;
    Reg *d_regs;
    int64_t *d_rptr, *d_at, *d_span_idx;
    u64 *d_cnt, *d_cur;
    Job *d_jobs;
    Pair *d_pairs;
    int32_t *d_span_out, *d_slab, *d_iv;
    uint32_t *d_rcnt;
    if (int rc = dh_upload(ctx, SLOT_VR_RECS, pl.recs.data(), (size_t)n, &d_recs)) return rc;
    if (int rc = dh_upload(ctx, SLOT_VR_REGS, pl.regs.data(), nreg, &d_regs)) return rc;
    if (int rc = dh_upload(ctx, SLOT_VR_RPTR, pl.rptr.data(), pl.rptr.size(), &d_rptr)) return rc;
    if (int rc = dh_scr(ctx, SLOT_VR_CNT, 3 * nreg, &d_cnt)) return rc;
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(u64) * 3 * nreg, st));
    dhk_vr_bind(st, 0, d_recs, 0, n, d_rptr, d_regs, 0, (int64_t)nreg, d_cnt, nullptr, nullptr, nullptr, nullptr);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> cnt(3 * nreg);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, sizeof(uint64_t) * cnt.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const double ms_count = dh_ms_since(t_call);
    for (size_t s = 0; s < nreg; s++) {
        res->pairs += (int64_t)cnt[3 * s];
        res->big_regions += vr::is_big(vr::live_windows(pl.regs[s], cnt[3 * s]), lds_windows) ? 1 : 0;
        if (cnt[3 * s + 2] > (uint64_t)INT32_MAX) return dh_fail(DH_EOVERFLOW, name + ": 2^31 spanning records or more in one region");
    }
    std::vector<vr::Group> groups;
    vr::build_groups(pl, cnt.data(), lds_windows, budget, groups);
    res->groups = (int64_t)groups.size();
    // ---- per launch group: write the lists, order the spanning records, count, place and emit the weak intervals
    std::vector<std::vector<int32_t>> weak_of(nreg), span_of(nreg);  // per region of the plan
    std::vector<int64_t> at;
    std::vector<Job> jobs;
    std::vector<size_t> job_reg;
    std::vector<uint32_t> rcnt;
    std::vector<int32_t> iv, span_out;
    for (const vr::Group &g : groups) {
        const size_t ng = (size_t)(g.s1 - g.s0);
        at.assign(2 * ng, 0);
        int64_t npairs = 0, nspan = 0, nslab = 0, lds_entries = 1;
        for (size_t k = 0; k < ng; k++) {
            at[2 * k] = npairs, at[2 * k + 1] = nspan;
            npairs += (int64_t)cnt[3 * (g.s0 + k) + 1];
            nspan += (int64_t)cnt[3 * (g.s0 + k) + 2];
        }
        // the jobs: the regions whose array stays in LDS first, then those of the slab
        jobs.clear();
        job_reg.clear();
        int64_t nsmall = 0;
        for (int big = 0; big < 2; big++) {
            for (size_t k = 0; k < ng; k++) {
                const size_t s = (size_t)g.s0 + k;
                const int32_t nw = vr::live_windows(pl.regs[s], cnt[3 * s]);
                if ((int)vr::is_big(nw, lds_windows) != big) continue;
                jobs.push_back(Job{pl.regs[s].cb, pl.regs[s].wlen, nw, 0, at[2 * k], (int64_t)cnt[3 * s + 1], nslab, 0});
                job_reg.push_back(s);
                if (big)
                    nslab += vr::slab_entries(nw);
                else
                    lds_entries = std::max<int64_t>(lds_entries, (int64_t)nw + 1);
            }
            if (!big) nsmall = (int64_t)jobs.size();
        }
        if (int rc = dh_upload(ctx, SLOT_VR_AT, at.data(), at.size(), &d_at)) return rc;
        if (int rc = dh_upload(ctx, SLOT_VR_JOBS, jobs.data(), jobs.size(), &d_jobs)) return rc;
        if (int rc = dh_scr(ctx, SLOT_VR_CUR, 2 * ng, &d_cur)) return rc;
        if (int rc = dh_scr(ctx, SLOT_VR_PAIRS, (size_t)npairs, &d_pairs)) return rc;
        if (int rc = dh_scr(ctx, SLOT_VR_SPAN_IDX, (size_t)nspan, &d_span_idx)) return rc;
        if (int rc = dh_scr(ctx, SLOT_VR_SPAN_OUT, (size_t)nspan, &d_span_out)) return rc;
        if (int rc = dh_scr(ctx, SLOT_VR_SLAB, (size_t)nslab, &d_slab)) return rc;
        if (int rc = dh_scr(ctx, SLOT_VR_RCNT, 2 * ng, &d_rcnt)) return rc;
        HIPCHK(hipMemsetAsync(d_cur, 0, sizeof(u64) * 2 * ng, st));
        if (npairs + nspan > 0) {
            // the records of the group's contigs (the records are sorted by aread)
            const int32_t c0 = pl.regs[(size_t)g.s0].contig, c1 = pl.regs[(size_t)g.s1 - 1].contig;
            const Rec *r0 = pl.recs.data(), *r1 = r0 + n;
            const int64_t i0 = std::lower_bound(r0, r1, c0, [](const Rec &r, int32_t c) { return r.aread < c; }) - r0;
            const int64_t i1 = std::upper_bound(r0, r1, c1, [](int32_t c, const Rec &r) { return c < r.aread; }) - r0;
            dhk_vr_bind(st, 1, d_recs, i0, i1 - i0, d_rptr, d_regs, g.s0, g.s1, d_cnt, d_at, d_cur, d_pairs, d_span_idx);
        }
        if (nspan > 0) dhk_vr_span(st, d_recs, d_at, d_cnt, g.s0, (int64_t)ng, d_span_idx, d_span_out);
        dhk_vr_region(st, 0, d_jobs, nsmall, (int64_t)ng, lds_entries, d_pairs, d_slab, min_cov, d_rcnt, nullptr);
        HIPCHK(hipGetLastError());
        rcnt.resize(2 * ng);
        span_out.resize((size_t)nspan);
        HIPCHK(hipMemcpyAsync(rcnt.data(), d_rcnt, sizeof(uint32_t) * rcnt.size(), hipMemcpyDeviceToHost, st));
        if (nspan > 0) HIPCHK(hipMemcpyAsync(span_out.data(), d_span_out, sizeof(int32_t) * (size_t)nspan, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        int64_t niv = 0;
        for (size_t q = 0; q < ng; q++) {
            jobs[q].out_at = niv;
            niv += (int64_t)rcnt[2 * q];
        }
        if (niv > 0) {
            if (int rc = dh_upload(ctx, SLOT_VR_JOBS, jobs.data(), jobs.size(), &d_jobs)) return rc;
            if (int rc = dh_scr(ctx, SLOT_VR_IV, (size_t)(2 * niv), &d_iv)) return rc;
            dhk_vr_region(st, 1, d_jobs, nsmall, (int64_t)ng, lds_entries, d_pairs, d_slab, min_cov, d_rcnt, d_iv);
            HIPCHK(hipGetLastError());
            iv.resize((size_t)(2 * niv));
            HIPCHK(hipMemcpyAsync(iv.data(), d_iv, sizeof(int32_t) * iv.size(), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        for (size_t q = 0; q < ng; q++) {
            const size_t s = job_reg[q];
            if (rcnt[2 * q]) weak_of[s].assign(iv.begin() + 2 * jobs[q].out_at, iv.begin() + 2 * (jobs[q].out_at + (int64_t)rcnt[2 * q]));
            vr::fill_report(pl.regs[s], (int64_t)cnt[3 * s + 2], (int64_t)rcnt[2 * q + 1], min_span, &res->reports[(size_t)pl.perm[s]]);
        }
        for (size_t k = 0; k < ng; k++) {
            const size_t s = (size_t)g.s0 + k;
            span_of[s].assign(span_out.begin() + at[2 * k + 1], span_out.begin() + at[2 * k + 1] + (int64_t)cnt[3 * s + 2]);
        }
    }
    // ---- input order, and the merged mask
    std::vector<size_t> plan_of(nreg);
    for (size_t s = 0; s < nreg; s++) plan_of[(size_t)pl.perm[s]] = s;
    for (size_t r = 0; r < nreg; r++) {
        const size_t s = plan_of[r];
        for (size_t x = 0; x + 1 < weak_of[s].size(); x += 2) {
            res->weak.push_back(regions[r].contig);
            res->weak.push_back(weak_of[s][x]);
            res->weak.push_back(weak_of[s][x + 1]);
        }
        res->span_ids.insert(res->span_ids.end(), span_of[s].begin(), span_of[s].end());
        res->span_off[r + 1] = (int64_t)res->span_ids.size();
    }
    vr::merge_mask(res->weak, ncontigs, res->mask_ptr, res->mask_iv);
    if (getenv("DH_TRACE"))
        fprintf(stderr,
                "[vreg] %lld records, %d regions (%lld in the slab), %lld pairs, %zu launch groups; plan+upload+count %.2f ms, total %.2f ms; "
                "%zu weak intervals, %zu spanning ids\n",
                (long long)n, nregions, (long long)res->big_regions, (long long)res->pairs, groups.size(), ms_count,
                dh_ms_since(t_call), res->weak.size() / 3,
                res->span_ids.size());
    *out = res.release();
    return DH_OK;
}

}  // namespace

extern "C" int dh_la_validate_regions(dh_ctx *ctx, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                                      const dh_region *regions, int32_t nregions, int32_t region_context, int32_t weak_coverage_window,
                                      int32_t min_coverage_reads, int32_t min_spanning_reads, dh_region_result **out)
{
    return validate(ctx, "dh_la_validate_regions", las, n, contig_off, ncontigs, regions, nregions, region_context, weak_coverage_window,
                    min_coverage_reads, min_spanning_reads, out);
}

extern "C" int dh_la_set_validate_regions(dh_ctx *ctx, const dh_la_set *set, const int64_t *contig_off, int32_t ncontigs,
                                          const dh_region *regions, int32_t nregions, int32_t region_context, int32_t weak_coverage_window,
                                          int32_t min_coverage_reads, int32_t min_spanning_reads, dh_region_result **out)
{
    const dh_la *las;
    int64_t n;
    if (int rc = dh_set_host_records("dh_la_set_validate_regions", ctx != nullptr, set, &las, &n)) return rc;
    return validate(ctx, "dh_la_set_validate_regions", las, n, contig_off, ncontigs, regions, nregions, region_context, weak_coverage_window,
                    min_coverage_reads, min_spanning_reads, out);
}

extern "C" void dh_region_result_destroy(dh_region_result *r) { delete r; }
extern "C" int32_t dh_region_result_count(const dh_region_result *r) { return r ? (int32_t)r->reports.size() : 0; }
extern "C" const dh_region_report *dh_region_result_reports(const dh_region_result *r) { return r ? r->reports.data() : nullptr; }
extern "C" int64_t dh_region_result_weak_count(const dh_region_result *r) { return r ? (int64_t)r->weak.size() / 3 : 0; }
extern "C" const int32_t *dh_region_result_weak(const dh_region_result *r) { return r ? r->weak.data() : nullptr; }
extern "C" const int64_t *dh_region_result_span_off(const dh_region_result *r) { return r ? r->span_off.data() : nullptr; }
extern "C" const int32_t *dh_region_result_span_ids(const dh_region_result *r) { return r ? r->span_ids.data() : nullptr; }
extern "C" const int64_t *dh_region_result_mask_ptr(const dh_region_result *r) { return r ? r->mask_ptr.data() : nullptr; }
extern "C" const int32_t *dh_region_result_mask_iv(const dh_region_result *r) { return r ? r->mask_iv.data() : nullptr; }
extern "C" int64_t dh_region_result_mask_count(const dh_region_result *r) { return r ? (int64_t)r->mask_iv.size() / 2 : 0; }
extern "C" int64_t dh_region_result_pairs(const dh_region_result *r) { return r ? r->pairs : 0; }
extern "C" int64_t dh_region_result_big_regions(const dh_region_result *r) { return r ? r->big_regions : 0; }
extern "C" int64_t dh_region_result_groups(const dh_region_result *r) { return r ? r->groups : 0; }
