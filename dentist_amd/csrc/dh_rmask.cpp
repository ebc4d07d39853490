// dh_rmask.cpp -- host side of dh_la_repeat_mask: `dentist mask-repetitive-regions` (commands/maskRepetitiveRegions.d:129-430)
// on the device, from records and lengths to intervals, without a dh_db.  Kernels: dh_rmask.hip; lane code, layouts and the plan:
// dh_rmask.h.  dh_db_mask_coverage (dh_db.cpp) is untouched.
//
// The call: everything is checked on the host threads while the records are packed to 32 bytes in pooled page-locked memory (all
// of it before the first launch); the lengths go up once; then every launch group -- whole contigs, as many as DH_RMASK_CHUNK_MB
// hold -- uploads its records, finds its chains (flags and a scan), writes two keys per chain, classifies its contigs by their
// number of events (the counters come back: the one wait in front of the sort), sorts every contig's keys by its tier, walks them
// twice (count, scan, place) and merges the two lists per contig (count, scan, place); the three lists and their offsets come
// back and are appended to the result.  What the host decides is listed in DESIGN.md 5.7.  DH_TRACE prints a line per call.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "dh_rmask.h"

using rm::Opts;
using rm::Rec;
using rm::u64;

extern "C" void dhk_cf_start(hipStream_t st, const Rec *recs, int64_t n, int32_t *flag, int32_t *uid);
extern "C" void dhk_rm_events(hipStream_t st, const Rec *recs, int64_t m, const int32_t *flag, const int32_t *uid, const int32_t *alen,
                              const int32_t *blen, Opts o, u64 *ev, u64 *ctr);
extern "C" void dhk_rm_classify(hipStream_t st, const int32_t *roff, const int32_t *uid, int32_t nc, int32_t lds_events, int32_t *seg, u64 *ctr,
                                int32_t *l_wave, int32_t *l_lds, int32_t *l_glob, u64 *slab_at);
extern "C" void dhk_rm_sort(hipStream_t st, u64 *ev, const int32_t *seg, int64_t nwave, const int32_t *l_wave, int64_t nlds, const int32_t *l_lds,
                            int32_t lds_events, int64_t nglob, const int32_t *l_glob, const u64 *slab_at, u64 *slab, int64_t max_padded);
extern "C" void dhk_rm_cover(hipStream_t st, int place, const u64 *ev, const int32_t *seg, int32_t nc, const int32_t *alen, Opts o,
                             uint32_t *cnt_all, uint32_t *cnt_imp, int32_t *iv_all, int32_t *iv_imp);
extern "C" void dhk_rm_union(hipStream_t st, int place, int32_t nc, const uint32_t *ptr_all, const int32_t *iv_all, const uint32_t *ptr_imp,
                             const int32_t *iv_imp, uint32_t *cnt, int32_t *iv);

static_assert(sizeof(Rec) == 32 && sizeof(Opts) == sizeof(dh_repeat_opts) && sizeof(u64) == sizeof(uint64_t), "dh_rmask.h states the layouts");

enum { M_MASK = 0, M_ALL = 1, M_IMPROPER = 2 };
struct dh_repeat_result {
    int32_t ncontigs = 0;
    std::vector<int64_t> ptr[3];  // ncontigs + 1 each
    std::vector<int32_t> iv[3];   // (begin, end) pairs
    int64_t units = 0, improper_units = 0, tiers[4] = {0, 0, 0, 0}, groups = 0;
};

namespace {

int repeat_mask(dh_ctx *ctx, const char *fn, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                int32_t nreads, const dh_repeat_opts *opts, dh_repeat_result **out)
{
    const std::string name(fn);
    if (!ctx || (n > 0 && !las) || !contig_off || !opts || !out || n < 0 || ncontigs < 0 || nreads < 0 || (opts->with_improper && !read_off))
        return dh_fail(DH_EINVAL, name + ": bad argument");
    const Opts o{opts->lower, opts->upper, opts->improper_lower, opts->improper_upper, opts->allowance, opts->with_improper ? 1 : 0};
    if (const char *w = rm::check_opts(o)) return dh_fail(DH_EINVAL, name + ": " + w);
    if (n >= ((int64_t)1 << 30)) return dh_fail(DH_EOVERFLOW, name + ": 2^30 records or more");
    const auto t_call = std::chrono::steady_clock::now();
    const bool trace = getenv("DH_TRACE") != nullptr;
    const int32_t lds_events = (int32_t)dh_env_knob("DH_RMASK_LDS_EVENTS", RM_LDS_EVENTS, RM_LDS_EVENTS_MIN, RM_LDS_EVENTS);
    // ---- the plan, before anything is launched
    std::vector<Rec, PinnedAlloc<Rec>> h_recs((size_t)n);
    std::vector<int32_t, PinnedAlloc<int32_t>> h_alen((size_t)ncontigs), h_blen(o.with_improper ? (size_t)nreads : 0);
    rm::Plan pl;
    pl.recs = h_recs.data(), pl.alen = h_alen.data(), pl.blen = h_blen.data();
    rm::Fault f;
    rm::build_plan(las, n, contig_off, ncontigs, read_off, nreads, o, rm::chunk_bytes_of_env(), dh_plan_runner<DH_PLAN_GRAIN>, pl, f);
    if (f.record >= 0) return dh_fail(DH_EINVAL, name + ": record " + std::to_string(f.record) + ": " + f.what);
    if (f.contig >= 0) return dh_fail(DH_EINVAL, name + ": contig " + std::to_string(f.contig) + ": " + f.what);
    std::unique_ptr<dh_repeat_result> res(new dh_repeat_result);
    res->ncontigs = ncontigs;
    for (int k = 0; k < 3; k++) res->ptr[k].assign((size_t)ncontigs + 1, 0);
    if (n == 0) {
        *out = res.release();
        return DH_OK;
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    double ms[6] = {0, 0, 0, 0, 0, 0};
    auto t_lap = t_call;
    auto lap = [&](int k) -> int {  // (stage times only when asked for: each is a wait)
        if (!trace) return DH_OK;
        HIPCHK(hipStreamSynchronize(st));
        ms[k] += dh_ms_since(t_lap);
        t_lap = std::chrono::steady_clock::now();
        return DH_OK;
    };
    int32_t *d_alen, *d_blen = nullptr;
    if (int rc = dh_upload(ctx, SLOT_RM_ALEN, pl.alen, (size_t)ncontigs, &d_alen)) return rc;
    if (o.with_improper)
        if (int rc = dh_upload(ctx, SLOT_RM_BLEN, pl.blen, (size_t)nreads, &d_blen)) return rc;
    std::vector<int32_t> roff;
    std::vector<uint32_t> h_ptr[3];
    std::vector<int32_t> h_iv;
    for (const rm::Group &g : pl.groups) {
        const int64_t m = g.r1 - g.r0;
        const int32_t nc = g.c1 - g.c0;
        const size_t sm = (size_t)m, snc = (size_t)nc;
        res->groups++;
        // ---- upload
        roff.resize(snc + 1);
        for (int32_t c = 0; c <= nc; c++) roff[(size_t)c] = (int32_t)(pl.rec_off[(size_t)(g.c0 + c)] - g.r0);
        int64_t max_padded = 2;  // no contig of the group has more events, padded to a power of two
        for (int32_t c = 0; c < nc; c++) max_padded = std::max<int64_t>(max_padded, cf::pow2ceil(2 * (roff[(size_t)c + 1] - roff[(size_t)c])));
        Rec *d_recs;
        int32_t *d_roff, *d_flag, *d_uid, *d_seg, *d_lw, *d_ll, *d_lg, *d_iv[3];
        uint32_t *d_sums, *d_cnt[3];
        u64 *d_ev, *d_ctr, *d_slab_at, *d_slab = nullptr, *d_nunits;
        if (int rc = dh_upload(ctx, SLOT_RM_RECS, pl.recs + g.r0, sm, &d_recs)) return rc;
        if (int rc = dh_upload(ctx, SLOT_RM_ROFF, roff.data(), snc + 1, &d_roff)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_FLAG, sm, &d_flag)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_UID, sm + 1, &d_uid)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_SUMS, (std::max(sm, snc) + 1 + 2047) / 2048, &d_sums)) return rc;  // (dhk_scan: 2048 values per block)
        if (int rc = dh_scr(ctx, SLOT_RM_EV, 2 * sm, &d_ev)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_SEG, snc + 1, &d_seg)) return rc;
        // the counters of the group and, behind them, the number of units: the 64-bit total of the flag scan
        if (int rc = dh_scr(ctx, SLOT_RM_CTR, (size_t)rm::C_COUNT + 1, &d_ctr)) return rc;
        d_nunits = d_ctr + rm::C_COUNT;
        // a contig of the LDS tier has 65 events or more, one of the global tier lds_events + 1
        const size_t cap_l = std::min(snc, 2 * sm / (RM_WAVE_EVENTS + 1)), cap_g = std::min(snc, 2 * sm / ((size_t)lds_events + 1));
        if (int rc = dh_scr(ctx, SLOT_RM_LWAVE, snc, &d_lw)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_LLDS, cap_l, &d_ll)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_LGLOB, cap_g, &d_lg)) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_SLAB_AT, cap_g, &d_slab_at)) return rc;
        // a run of an assessor begins at base 0 or at an event's position and ends at one or at the contig's end, and the runs of
        // a contig share no position: a contig of u units has u + 1 runs at most, and its union twice that
        const size_t cap_iv = sm + snc;
        if (int rc = dh_scr(ctx, SLOT_RM_CNT_ALL, snc + 1, &d_cnt[M_ALL])) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_CNT_IMP, snc + 1, &d_cnt[M_IMPROPER])) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_CNT_MASK, snc + 1, &d_cnt[M_MASK])) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_IV_ALL, 2 * cap_iv, &d_iv[M_ALL])) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_IV_IMP, o.with_improper ? 2 * cap_iv : 0, &d_iv[M_IMPROPER])) return rc;
        if (int rc = dh_scr(ctx, SLOT_RM_IV_MASK, o.with_improper ? 4 * cap_iv : 0, &d_iv[M_MASK])) return rc;
        HIPCHK(hipMemsetAsync(d_uid + m, 0, sizeof(int32_t), st));
        HIPCHK(hipMemsetAsync(d_ctr, 0, sizeof(u64) * (rm::C_COUNT + 1), st));
        for (int k = 0; k < 3; k++) HIPCHK(hipMemsetAsync(d_cnt[k], 0, sizeof(uint32_t) * (snc + 1), st));
        if (int rc = lap(0)) return rc;
        // ---- chains and events
        dhk_cf_start(st, d_recs, m, d_flag, d_uid);
        dhk_scan_total(st, (uint32_t *)d_uid, m + 1, d_sums, d_nunits);  // (flags: never negative)
        dhk_rm_events(st, d_recs, m, d_flag, d_uid, d_alen, d_blen, o, d_ev, d_ctr);
        HIPCHK(hipGetLastError());
        if (int rc = lap(1)) return rc;
        dhk_rm_classify(st, d_roff, d_uid, nc, lds_events, d_seg, d_ctr, d_lw, d_ll, d_lg, d_slab_at);
        HIPCHK(hipGetLastError());
        uint64_t ctr[rm::C_COUNT + 1];
        HIPCHK(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = lap(2)) return rc;
        // ---- sort
        if (ctr[rm::C_ZERO] + ctr[rm::C_WAVE] + ctr[rm::C_LDS] + ctr[rm::C_GLOBAL] != (uint64_t)nc || ctr[rm::C_LDS] > cap_l ||
            ctr[rm::C_GLOBAL] > cap_g || ctr[rm::C_SLAB] > 4 * (uint64_t)m || ctr[rm::C_COUNT] > (uint64_t)m)
            return dh_fail(DH_EOVERFLOW, name + ": the tier lists do not add up");
        if (int rc = dh_scr(ctx, SLOT_RM_SLAB, (size_t)ctr[rm::C_SLAB], &d_slab)) return rc;
        dhk_rm_sort(st, d_ev, d_seg, (int64_t)ctr[rm::C_WAVE], d_lw, (int64_t)ctr[rm::C_LDS], d_ll, lds_events, (int64_t)ctr[rm::C_GLOBAL], d_lg,
                    d_slab_at, d_slab, max_padded);
        HIPCHK(hipGetLastError());
        if (int rc = lap(3)) return rc;
        // ---- coverage: count, scan, place
        const int32_t *d_galen = d_alen + g.c0;
        dhk_rm_cover(st, 0, d_ev, d_seg, nc, d_galen, o, d_cnt[M_ALL], d_cnt[M_IMPROPER], d_iv[M_ALL], d_iv[M_IMPROPER]);
        dhk_scan(st, d_cnt[M_ALL], (int64_t)nc + 1, d_sums);
        if (o.with_improper) dhk_scan(st, d_cnt[M_IMPROPER], (int64_t)nc + 1, d_sums);
        dhk_rm_cover(st, 1, d_ev, d_seg, nc, d_galen, o, d_cnt[M_ALL], d_cnt[M_IMPROPER], d_iv[M_ALL], d_iv[M_IMPROPER]);
        HIPCHK(hipGetLastError());
        if (int rc = lap(4)) return rc;
        // ---- union: count, scan, place
        if (o.with_improper) {
            dhk_rm_union(st, 0, nc, d_cnt[M_ALL], d_iv[M_ALL], d_cnt[M_IMPROPER], d_iv[M_IMPROPER], d_cnt[M_MASK], d_iv[M_MASK]);
            dhk_scan(st, d_cnt[M_MASK], (int64_t)nc + 1, d_sums);
            dhk_rm_union(st, 1, nc, d_cnt[M_ALL], d_iv[M_ALL], d_cnt[M_IMPROPER], d_iv[M_IMPROPER], d_cnt[M_MASK], d_iv[M_MASK]);
            HIPCHK(hipGetLastError());
        }
        // ---- download: the offsets, then as many intervals as they say
        const int first = o.with_improper ? M_MASK : M_ALL, last = o.with_improper ? M_IMPROPER : M_ALL;
        for (int k = first; k <= last; k++) {
            h_ptr[k].resize(snc + 1);
            HIPCHK(hipMemcpyAsync(h_ptr[k].data(), d_cnt[k], sizeof(uint32_t) * (snc + 1), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        for (int k = first; k <= last; k++) {
            const size_t total = h_ptr[k][snc];
            if (total > (k == M_MASK ? 2 : 1) * cap_iv) return dh_fail(DH_EOVERFLOW, name + ": more runs than events allow");
            h_iv.resize(2 * total);
            if (total) HIPCHK(hipMemcpyAsync(h_iv.data(), d_iv[k], sizeof(int32_t) * 2 * total, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            const int64_t at = (int64_t)res->iv[k].size() / 2;
            for (int32_t c = 0; c <= nc; c++) res->ptr[k][(size_t)(g.c0 + c)] = at + h_ptr[k][(size_t)c];
            res->iv[k].insert(res->iv[k].end(), h_iv.begin(), h_iv.end());
        }
        res->units += (int64_t)ctr[rm::C_COUNT];
        res->improper_units += (int64_t)ctr[rm::C_IMPROPER];
        for (int t = 0; t < 4; t++) res->tiers[t] += (int64_t)ctr[rm::C_ZERO + t];
        if (int rc = lap(5)) return rc;
    }
    // an assessor that counts no unit at all gives nothing (maskRepetitiveRegions.d:350-351), and without it the mask is `all`
    if (o.with_improper && res->improper_units == 0) {
        res->ptr[M_IMPROPER].assign((size_t)ncontigs + 1, 0);
        res->iv[M_IMPROPER].clear();
    }
    if (!o.with_improper || res->improper_units == 0) res->ptr[M_MASK] = res->ptr[M_ALL], res->iv[M_MASK] = res->iv[M_ALL];
    if (trace)
        fprintf(stderr,
                "[rmask] %lld records, %lld units (%lld improper), %d contigs in %lld groups; tiers: %lld none, %lld wave, %lld LDS (cap %d), "
                "%lld global; plan+upload %.2f, chains+events %.2f, classify %.2f, sort %.2f, cover %.2f, union+download %.2f ms, total %.2f ms; "
                "runs %lld all, %lld improper, %lld mask\n",
                (long long)n, (long long)res->units, (long long)res->improper_units, ncontigs, (long long)res->groups, (long long)res->tiers[0],
                (long long)res->tiers[1], (long long)res->tiers[2], lds_events, (long long)res->tiers[3], ms[0], ms[1], ms[2], ms[3], ms[4], ms[5],
                dh_ms_since(t_call), (long long)res->iv[M_ALL].size() / 2, (long long)res->iv[M_IMPROPER].size() / 2,
                (long long)res->iv[M_MASK].size() / 2);
    *out = res.release();
    return DH_OK;
}

}  // namespace

extern "C" int dh_la_repeat_mask(dh_ctx *ctx, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                                 int32_t nreads, const dh_repeat_opts *opts, dh_repeat_result **out)
{
    return repeat_mask(ctx, "dh_la_repeat_mask", las, n, contig_off, ncontigs, read_off, nreads, opts, out);
}

extern "C" int dh_la_set_repeat_mask(dh_ctx *ctx, const dh_la_set *set, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                                     int32_t nreads, const dh_repeat_opts *opts, dh_repeat_result **out)
{
    const dh_la *las;
    int64_t n;
    if (int rc = dh_set_host_records("dh_la_set_repeat_mask", ctx != nullptr, set, &las, &n)) return rc;
    return repeat_mask(ctx, "dh_la_set_repeat_mask", las, n, contig_off, ncontigs, read_off, nreads, opts, out);
}

extern "C" void dh_repeat_result_destroy(dh_repeat_result *r) { delete r; }
extern "C" const int64_t *dh_repeat_result_mask_ptr(const dh_repeat_result *r) { return r->ptr[M_MASK].data(); }
extern "C" const int32_t *dh_repeat_result_mask_iv(const dh_repeat_result *r) { return r->iv[M_MASK].data(); }
extern "C" int64_t dh_repeat_result_mask_count(const dh_repeat_result *r) { return (int64_t)r->iv[M_MASK].size() / 2; }
extern "C" const int64_t *dh_repeat_result_all_ptr(const dh_repeat_result *r) { return r->ptr[M_ALL].data(); }
extern "C" const int32_t *dh_repeat_result_all_iv(const dh_repeat_result *r) { return r->iv[M_ALL].data(); }
extern "C" int64_t dh_repeat_result_all_count(const dh_repeat_result *r) { return (int64_t)r->iv[M_ALL].size() / 2; }
extern "C" const int64_t *dh_repeat_result_improper_ptr(const dh_repeat_result *r) { return r->ptr[M_IMPROPER].data(); }
extern "C" const int32_t *dh_repeat_result_improper_iv(const dh_repeat_result *r) { return r->iv[M_IMPROPER].data(); }
extern "C" int64_t dh_repeat_result_improper_count(const dh_repeat_result *r) { return (int64_t)r->iv[M_IMPROPER].size() / 2; }
extern "C" int64_t dh_repeat_result_units(const dh_repeat_result *r) { return r->units; }
extern "C" int64_t dh_repeat_result_improper_units(const dh_repeat_result *r) { return r->improper_units; }
extern "C" int64_t dh_repeat_result_tier_contigs(const dh_repeat_result *r, int32_t tier) { return tier >= 0 && tier < 4 ? r->tiers[tier] : 0; }
extern "C" int64_t dh_repeat_result_groups(const dh_repeat_result *r) { return r->groups; }
