// dh_cfilt.cpp -- host side of dh_la_collect_filter: the six alignment filters of `dentist collect` (collectPileUps/filter.d:
// 122-356) on the device.  Kernels: dh_cfilt.hip; lane code, layouts and the plan: dh_cfilt.h.  The contract is the host function
// dh_collect_filter (dh_filter.cpp), which is untouched.
//
// The call: the ids and the mask are checked on the host threads while the records are packed to 32 bytes in pooled page-locked
// memory (all of it before the first launch; from pageable memory the upload alone took longer than the host function); records,
// lengths and the mask with its prefix sums are uploaded; chains are found (flags and a scan), judged by stages 1-3 and counted
// per read; the counts are scanned and the units scattered to their reads; reads of one unit are finished by their lane, the
// others listed by tier.  The counters come back (the one wait inside the call) and size the launches of the tiers and the slab.  k_cf_finish writes a byte per record and the six counts; those, and read_used, come back, and the
// host threads set DH_FLAG_DISABLED.  DH_TRACE prints a line per call.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "dh_cfilt.h"

using cf::Mask;
using cf::Opts;
using cf::Rec;
using cf::Unit;

typedef unsigned long long u64;

extern "C" void dhk_cf_start(hipStream_t st, const Rec *recs, int64_t n, int32_t *flag, int32_t *uid);
extern "C" void dhk_cf_units(hipStream_t st, const Rec *recs, int64_t n, const int32_t *flag, int32_t *uid, const u64 *nunits, int32_t *first,
                             Mask mask, const int32_t *alen, const int32_t *blen, Opts o, Unit *units, uint8_t *why, int32_t *cnt);
extern "C" void dhk_cf_group(hipStream_t st, const Unit *units, int64_t n, int32_t nreads, int32_t lds_units, const int32_t *goff, int32_t *cur,
                             int32_t *gidx, uint8_t *why, uint8_t *used, const u64 *nunits, uint32_t *ctr, int32_t *l_wave, int32_t *l_lds,
                             int32_t *l_glob, uint32_t *slab_at);
extern "C" void dhk_cf_tiers(hipStream_t st, const Unit *units, const int32_t *goff, const int32_t *gidx, int64_t nwave, const int32_t *l_wave,
                             int64_t nlds, const int32_t *l_lds, int32_t lds_units, int64_t nglob, const int32_t *l_glob,
                             const uint32_t *slab_at, int32_t *slab, uint8_t *why, uint8_t *used);
extern "C" void dhk_cf_finish(hipStream_t st, const int32_t *flag, const int32_t *uid, int64_t n, const Unit *units, const uint8_t *why, uint8_t *out,
                              u64 *cnt6);

static_assert(sizeof(Rec) == 32 && sizeof(Unit) == 40 && sizeof(Opts) == 16, "dh_cfilt.h states the layouts");
static_assert(sizeof(u64) == sizeof(uint64_t), "the counters are read as uint64_t");

namespace {

int collect_filter(dh_ctx *ctx, const char *fn, dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                   int32_t nreads, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts, int64_t *dropped6,
                   uint8_t *read_used)
{
    const std::string name(fn);
    if (!ctx || (n > 0 && !las) || !contig_off || !read_off || !opts || n < 0 || ncontigs < 0 || nreads < 0 ||
        (rep_ptr && !rep_iv && ncontigs > 0 && rep_ptr[ncontigs] > 0))
        return dh_fail(DH_EINVAL, name + ": bad argument");
    if (n >= ((int64_t)1 << 30)) return dh_fail(DH_EOVERFLOW, name + ": 2^30 records or more");
    const auto t_call = std::chrono::steady_clock::now();
    const bool trace = getenv("DH_TRACE") != nullptr;
    const int32_t lds_units = (int32_t)dh_env_knob("DH_CFILT_LDS_UNITS", CF_LDS_UNITS, CF_WAVE_UNITS, CF_LDS_UNITS);
    // ---- the plan, before anything is launched or written
    // (page-locked and pooled: the copies run at the speed of the link, and resize() fills nothing)
    std::vector<Rec, PinnedAlloc<Rec>> h_recs((size_t)n);
    std::vector<int32_t, PinnedAlloc<int32_t>> h_alen((size_t)ncontigs), h_blen((size_t)nreads);
    std::vector<uint8_t, PinnedAlloc<uint8_t>> out((size_t)n);
    cf::Plan pl;
    pl.recs = h_recs.data(), pl.alen = h_alen.data(), pl.blen = h_blen.data();
    cf::Fault f;
    cf::build_plan(las, n, contig_off, ncontigs, read_off, nreads, rep_ptr, rep_iv, dh_plan_runner<DH_PLAN_GRAIN>, pl, f);
    if (f.record >= 0) return dh_fail(DH_EINVAL, name + ": record " + std::to_string(f.record) + ": " + f.what);
    if (f.contig >= 0) return dh_fail(DH_EINVAL, name + ": contig " + std::to_string(f.contig) + ": " + f.what);
    if (dropped6) memset(dropped6, 0, 6 * sizeof(int64_t));
    if (read_used && nreads > 0) memset(read_used, 1, (size_t)nreads);
    if (n == 0) return DH_OK;
    // ---- upload
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    double ms[5] = {0, 0, 0, 0, 0};
    auto t_lap = t_call;
    auto lap = [&](int k) -> int {  // (stage times only when asked for: each is a wait)
        if (!trace) return DH_OK;
        HIPCHK(hipStreamSynchronize(st));
        ms[k] = dh_ms_since(t_lap);
        t_lap = std::chrono::steady_clock::now();
        return DH_OK;
    };
    const size_t sn = (size_t)n, sr = (size_t)nreads, nsums = (std::max(sn, sr + 1) + 2047) / 2048;  // (dhk_scan: 2048 values per block)
    const size_t nmask = rep_ptr ? pl.pre.size() - 1 : 0;
    Rec *d_recs;
    int32_t *d_alen, *d_blen, *d_iv = nullptr, *d_flag, *d_uid, *d_first, *d_cnt, *d_cur, *d_gidx, *d_lw, *d_ll, *d_lg, *d_slab = nullptr;
    int64_t *d_ptr = nullptr, *d_pre = nullptr;
    Unit *d_units;
    uint8_t *d_why, *d_used, *d_out;
    uint32_t *d_ctr, *d_slab_at, *d_sums;
    u64 *d_cnt6;
    if (int rc = dh_upload(ctx, SLOT_CF_RECS, pl.recs, sn, &d_recs)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CF_ALEN, pl.alen, (size_t)ncontigs, &d_alen)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CF_BLEN, pl.blen, sr, &d_blen)) return rc;
    if (rep_ptr) {
        if (int rc = dh_upload(ctx, SLOT_CF_MASK_PTR, rep_ptr, (size_t)ncontigs + 1, &d_ptr)) return rc;
        if (int rc = dh_upload(ctx, SLOT_CF_MASK_IV, rep_iv, 2 * nmask, &d_iv)) return rc;
        if (int rc = dh_upload(ctx, SLOT_CF_MASK_PRE, pl.pre.data(), nmask + 1, &d_pre)) return rc;
    }
    if (int rc = dh_scr(ctx, SLOT_CF_FLAG, sn, &d_flag)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_UID, sn, &d_uid)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_SUMS, nsums, &d_sums)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_FIRST, sn + 1, &d_first)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_UNITS, sn, &d_units)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_WHY, sn, &d_why)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_CNT, sr + 1, &d_cnt)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_CUR, sr, &d_cur)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_GIDX, sn, &d_gidx)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_USED, sr, &d_used)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_OUT, sn, &d_out)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_CTR, (size_t)cf::C_COUNT, &d_ctr)) return rc;
    // the six counts, and behind them the number of chains: the 64-bit total of the flag scan
    if (int rc = dh_scr(ctx, SLOT_CF_CNT6, 7, &d_cnt6)) return rc;
    u64 *d_nunits = d_cnt6 + 6;
    // a read of the wave tier has two units or more, one of the LDS tier 65, one of the global tier lds_units + 1
    const size_t cap_w = std::min(sr, sn / 2), cap_l = std::min(sr, sn / (CF_WAVE_UNITS + 1)), cap_g = std::min(sr, sn / ((size_t)lds_units + 1));
    if (int rc = dh_scr(ctx, SLOT_CF_LWAVE, cap_w, &d_lw)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_LLDS, cap_l, &d_ll)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_LGLOB, cap_g, &d_lg)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CF_SLAB_AT, cap_g, &d_slab_at)) return rc;
    HIPCHK(hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * (sr + 1), st));
    HIPCHK(hipMemsetAsync(d_cur, 0, sizeof(int32_t) * std::max<size_t>(sr, 1), st));
    HIPCHK(hipMemsetAsync(d_used, 1, std::max<size_t>(sr, 1), st));
    HIPCHK(hipMemsetAsync(d_ctr, 0, sizeof(uint32_t) * cf::C_COUNT, st));
    HIPCHK(hipMemsetAsync(d_cnt6, 0, sizeof(u64) * 7, st));
    if (int rc = lap(0)) return rc;
    // ---- chains, stages 1-3, the units of every read
    const Mask mask{d_ptr, d_iv, d_pre};
    const Opts o{opts->max_align_err_ppm, opts->allowance, opts->min_anchor, 0};
    dhk_cf_start(st, d_recs, n, d_flag, d_uid);
    dhk_scan_total(st, (uint32_t *)d_uid, n, d_sums, d_nunits);  // (flags: never negative)
    dhk_cf_units(st, d_recs, n, d_flag, d_uid, d_nunits, d_first, mask, d_alen, d_blen, o, d_units, d_why, d_cnt);
    HIPCHK(hipGetLastError());
    if (int rc = lap(1)) return rc;
    dhk_scan(st, (uint32_t *)d_cnt, (int64_t)nreads + 1, d_sums);  // (counts: never negative)
    dhk_cf_group(st, d_units, n, nreads, lds_units, d_cnt, d_cur, d_gidx, d_why, d_used, d_nunits, d_ctr, d_lw, d_ll, d_lg, d_slab_at);
    HIPCHK(hipGetLastError());
    uint32_t ctr[cf::C_COUNT];
    HIPCHK(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (int rc = lap(2)) return rc;
    // ---- stages 4-6 of the reads with more than one unit
    if (ctr[cf::C_WAVE] > cap_w || ctr[cf::C_LDS] > cap_l || ctr[cf::C_GLOBAL] > cap_g || ctr[cf::C_SLAB] > 2 * (uint64_t)n)
        return dh_fail(DH_EOVERFLOW, name + ": the tier lists do not add up");
    if (int rc = dh_scr(ctx, SLOT_CF_SLAB, (size_t)ctr[cf::C_SLAB], &d_slab)) return rc;
    dhk_cf_tiers(st, d_units, d_cnt, d_gidx, ctr[cf::C_WAVE], d_lw, ctr[cf::C_LDS], d_ll, lds_units, ctr[cf::C_GLOBAL], d_lg, d_slab_at, d_slab,
                 d_why, d_used);
    HIPCHK(hipGetLastError());
    if (int rc = lap(3)) return rc;
    dhk_cf_finish(st, d_flag, d_uid, n, d_units, d_why, d_out, d_cnt6);
    HIPCHK(hipGetLastError());
    uint64_t cnt6[7];
    HIPCHK(hipMemcpyAsync(out.data(), d_out, sn, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(cnt6, d_cnt6, sizeof(cnt6), hipMemcpyDeviceToHost, st));
    if (read_used && nreads > 0) HIPCHK(hipMemcpyAsync(read_used, d_used, sr, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const uint8_t *dis = out.data();
    dh_parallel_for(n, 1 << 14, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++)
            if (dis[i]) las[i].flags |= DH_FLAG_DISABLED;
    });
    if (dropped6)
        for (int k = 0; k < 6; k++) dropped6[k] = (int64_t)cnt6[k];
    if (int rc = lap(4)) return rc;
    if (trace)
        fprintf(stderr,
                "[cfilt] %lld records, %llu chains, %d reads; tiers: %u wave, %u LDS (cap %d), %u global (%u slab entries); plan+upload %.2f, "
                "chains+stages 1-3 %.2f, group %.2f, tiers %.2f, finish+download %.2f ms, total %.2f ms; dropped %llu %llu %llu %llu %llu %llu\n",
                (long long)n, (unsigned long long)cnt6[6], nreads, ctr[cf::C_WAVE], ctr[cf::C_LDS], lds_units, ctr[cf::C_GLOBAL], ctr[cf::C_SLAB], ms[0], ms[1],
                ms[2], ms[3], ms[4], dh_ms_since(t_call),
                (unsigned long long)cnt6[0], (unsigned long long)cnt6[1], (unsigned long long)cnt6[2], (unsigned long long)cnt6[3],
                (unsigned long long)cnt6[4], (unsigned long long)cnt6[5]);
    return DH_OK;
}

}  // namespace

extern "C" int dh_la_collect_filter(dh_ctx *ctx, dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                                    int32_t nreads, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                                    int64_t *dropped6, uint8_t *read_used)
{
    return collect_filter(ctx, "dh_la_collect_filter", las, n, contig_off, ncontigs, read_off, nreads, rep_ptr, rep_iv, opts, dropped6, read_used);
}

extern "C" int dh_la_set_collect_filter(dh_ctx *ctx, dh_la_set *set, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                                        int32_t nreads, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                                        int64_t *dropped6, uint8_t *read_used)
{
    dh_la *las;
    int64_t n;
    if (int rc = dh_set_host_records("dh_la_set_collect_filter", ctx != nullptr, set, &las, &n)) return rc;
    return collect_filter(ctx, "dh_la_set_collect_filter", las, n, contig_off, ncontigs, read_off, nreads, rep_ptr, rep_iv, opts, dropped6, read_used);
}
