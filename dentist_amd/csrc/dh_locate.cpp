// dh_locate.cpp -- host side of dh_exact_locate: every exact occurrence of every query and of its reverse complement in a
// reference of many records, what the reference's external/fm-index.cpp answers for `dentist check-results`
// (commands/checkResults.d:511-565).  Kernels: dh_locate.hip; lane code, layouts and the plan of the queries: dh_locate.h.
//
// The call: offsets are validated; the queries are packed (both strands), which finds a code above 3; the reference is
// packed by the host threads into a bounded page-locked staging buffer and uploaded slice by slice, which finds a code
// above 3 there -- all of it before the first launch.  Then word ranges of the text are scanned (k_locate_scan for the
// queries of 32 bases or more, k_locate_short for the rest) into the candidate buffer; a range whose candidates exceed the
// buffer is scanned again in halves (a range of one word that still overflows grows the buffer to the counted number:
// nothing is dropped).  The candidates the scan could not compare whole are cut into segments, one wavefront of
// k_locate_verify each.  The survivors are sorted on the host by (query, strand, position).
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>

#include "dh_locate.h"

extern "C" void dhk_locate_scan(hipStream_t st, int use_bitmap, const uint64_t *text, int64_t nbases, int64_t w0, int64_t w1,
                                const LocSlot *table, int32_t tbits, const uint32_t *bitmap, const uint32_t *memb, const LocPat *pats,
                                const uint64_t *pw, const int64_t *starts, int64_t nref, LocCand *cands, int64_t cap,
                                unsigned long long *counter);
extern "C" void dhk_locate_short(hipStream_t st, const uint64_t *text, int64_t nbases, int64_t p0, int64_t p1, const LocShort *shorts,
                                 int64_t nshort, const int64_t *starts, int64_t nref, LocCand *cands, int64_t cap,
                                 unsigned long long *counter);
extern "C" void dhk_locate_verify(hipStream_t st, const uint64_t *text, int64_t nbases, const uint64_t *pw, const LocPat *pats,
                                  LocCand *cands, int64_t ncands, const LocUnit *units, int64_t nunits, int64_t seg);

struct dh_exact_hits {
    std::vector<loc::Hit> hits;
};
static_assert(sizeof(dh_exact_hit) == 32 && sizeof(loc::Hit) == 32, "the header states the record's layout");

namespace {

const size_t kStageBytes = 8u << 20;        // the page-locked staging buffer of the uploads
const int64_t kUnitBatch = (int64_t)1 << 22;  // verify units per launch

struct Stage {  // bounded staging of host arrays
    void *p = nullptr;
    ~Stage() { dh_pinned_free(p, kStageBytes); }
};

// a host array to the device through the staging buffer, piece by piece with a wait behind each (not dh_upload: the
// source is pageable and may be large)
int upload_staged(dh_ctx *ctx, Stage &sg, void *dst, const void *src, size_t bytes)
{
    for (size_t at = 0; at < bytes; at += kStageBytes) {
        const size_t n = std::min(kStageBytes, bytes - at);
        memcpy(sg.p, (const char *)src + at, n);
        HIPCHK(hipMemcpyAsync((char *)dst + at, sg.p, n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return DH_OK;
}

template <typename T>
int upload_staged(dh_ctx *ctx, Stage &sg, DhSlot id, const std::vector<T> &v, T **out)
{
    if (int rc = dh_scr(ctx, id, v.size(), out)) return rc;
    return upload_staged(ctx, sg, *out, v.data(), sizeof(T) * v.size());
}

// the reference bytes checked for a code above 3 without a device: first bad position or -1
int64_t first_bad_code(const uint8_t *text, int64_t n)
{
    int64_t bad = -1;
    for (int64_t i = 0; i < n; i++)
        if (text[i] > 3) {
            bad = i;
            break;
        }
    return bad;
}

int bad_ref_code(const uint8_t *text, int64_t lo, int64_t hi, const int64_t *starts, int64_t nref)
{
    int64_t at = lo;
    while (at < hi && text[at] <= 3) at++;
    const int64_t r = loc::record_of(starts, nref, at);
    char msg[160];
    snprintf(msg, sizeof(msg), "dh_exact_locate: reference record %lld: code %d above 3 at base %lld", (long long)r, (int)text[at],
             (long long)(at - starts[r]));
    return dh_fail(DH_EINVAL, msg);
}

}  // namespace

extern "C" int dh_exact_locate(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off, int64_t nref, const uint8_t *qry,
                               const int64_t *qry_off, int64_t nqry, int32_t both_strands, dh_exact_hits **out)
{
    if (!ctx || !out || nref < 0 || nqry < 0 || (nref > 0 && !ref_off) || (nqry > 0 && !qry_off))
        return dh_fail(DH_EINVAL, "dh_exact_locate: bad argument");
    *out = nullptr;
    if (nref > INT32_MAX || nqry > INT32_MAX) return dh_fail(DH_EINVAL, "dh_exact_locate: more than 2^31 - 1 records or queries");
    const auto t_call = std::chrono::steady_clock::now();
    const bool trace = getenv("DH_TRACE") != nullptr;
    // ---- validation on the host, before anything is launched
    for (int side = 0; side < 2; side++) {
        const int64_t *off = side ? qry_off : ref_off, n = side ? nqry : nref;
        const char *what = side ? "query" : "reference record";
        if (n > 0 && off[0] < 0) return dh_fail(DH_EINVAL, std::string("dh_exact_locate: negative first offset of the ") + (side ? "queries" : "reference"));
        for (int64_t i = 0; i < n; i++)
            if (off[i + 1] < off[i]) {
                char msg[160];
                snprintf(msg, sizeof(msg), "dh_exact_locate: %s %lld: offsets decrease", what, (long long)i);
                return dh_fail(DH_EINVAL, msg);
            }
    }
    if ((nref > 0 && ref_off[nref] > ref_off[0] && !ref) || (nqry > 0 && qry_off[nqry] > qry_off[0] && !qry))
        return dh_fail(DH_EINVAL, "dh_exact_locate: sequences are NULL");
    const int64_t nbases = nref > 0 ? ref_off[nref] - ref_off[0] : 0;
    const uint8_t *text = nref > 0 ? ref + ref_off[0] : nullptr;
    std::vector<int64_t> starts((size_t)nref + 1, 0);
    int64_t longest = 0;
    for (int64_t i = 0; i < nref; i++) {
        starts[(size_t)i + 1] = ref_off[i + 1] - ref_off[0];
        longest = std::max(longest, ref_off[i + 1] - ref_off[i]);
    }
    loc::Plan pl;
    loc::build_plan(qry, qry_off, nqry, both_strands != 0, longest,
                    dh_plan_runner<64>, pl);
    if (pl.bad_query >= 0) {
        char msg[160];
        snprintf(msg, sizeof(msg), "dh_exact_locate: query %lld: a code above 3", (long long)pl.bad_query);
        return dh_fail(DH_EINVAL, msg);
    }
    std::unique_ptr<dh_exact_hits> res(new dh_exact_hits);
    if (pl.memb.empty() && pl.shorts.empty()) {  // nothing to search for: the reference is checked all the same
        const int64_t bad = first_bad_code(text, nbases);
        if (bad >= 0) return bad_ref_code(text, bad, nbases, starts.data(), nref);
        *out = res.release();
        return DH_OK;
    }
    // ---- the packed text, resident whole
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Stage sg;
    sg.p = dh_pinned_alloc(kStageBytes);
    if (!sg.p) return dh_fail(DH_ENOMEM, "dh_exact_locate: no staging buffer");
    const int64_t nwords = (nbases + 31) >> 5;
    uint64_t *d_text;
    if (int rc = dh_scr(ctx, SLOT_LOC_TEXT, (size_t)nwords + LOC_TEXT_PAD, &d_text)) return rc;
    const int64_t slice = (int64_t)(kStageBytes / 8);  // words
    for (int64_t w0 = 0; w0 < nwords; w0 += slice) {
        const int64_t n = std::min(slice, nwords - w0);
        uint64_t *dst = (uint64_t *)sg.p;
        int ok = 1;
        dh_parallel_for(n, 4096, [&](int64_t lo, int64_t hi) {
            if (!loc::pack_words(text, nbases, 32 * (w0 + lo), hi - lo, false, dst + lo)) __atomic_store_n(&ok, 0, __ATOMIC_RELAXED);
        });
        if (!ok) return bad_ref_code(text, 32 * w0, std::min(nbases, 32 * (w0 + n)), starts.data(), nref);
        HIPCHK(hipMemcpyAsync(d_text + w0, dst, sizeof(uint64_t) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipMemsetAsync(d_text + nwords, 0, sizeof(uint64_t) * LOC_TEXT_PAD, st));
    int64_t *d_starts;
    uint64_t *d_pw;
    LocPat *d_pats;
    uint32_t *d_memb, *d_bitmap;
    LocSlot *d_table;
    LocShort *d_shorts;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_STARTS, starts, &d_starts)) return rc;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_PW, pl.pw, &d_pw)) return rc;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_PATS, pl.pats, &d_pats)) return rc;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_MEMB, pl.memb, &d_memb)) return rc;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_TABLE, pl.table, &d_table)) return rc;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_BITMAP, pl.bitmap, &d_bitmap)) return rc;
    if (int rc = upload_staged(ctx, sg, SLOT_LOC_SHORTS, pl.shorts, &d_shorts)) return rc;
    const double ms_upload = dh_ms_since(t_call);
    // the pre-filter in LDS is used while at most one bit in eight of it is set: measured it takes the scan of
    // 2 002 groups from 0.58 to 0.21 ms and changes nothing at 798 408 groups, where it is full.  DH_LOCATE_BITMAP forces it
    size_t ngroups = 0;
    for (const LocSlot &s : pl.table) ngroups += s.count != 0;
    const int use_bitmap = (int)dh_env_knob("DH_LOCATE_BITMAP", ngroups * 8 <= LOC_BITMAP_BITS ? 1 : 0, 0, 1);
    // ---- scan, verify
    int64_t cap = dh_env_knob("DH_LOCATE_CAND_CAP", LOC_CAND_CAP_DEFAULT, 1, (int64_t)1 << 31);
    const int64_t seg = loc::round_seg(dh_env_knob("DH_LOCATE_SEG", LOC_SEG_DEFAULT, 1, (int64_t)1 << 40));
    LocCand *d_cands;
    unsigned long long *d_counter;
    if (int rc = dh_scr(ctx, SLOT_LOC_CANDS, (size_t)cap, &d_cands)) return rc;
    if (int rc = dh_scr(ctx, SLOT_LOC_COUNTER, 1, &d_counter)) return rc;
    std::vector<LocCand> all, part;
    std::vector<LocUnit> units;
    std::vector<std::pair<int64_t, int64_t>> todo{{0, nwords}};
    double ms_scan = 0, ms_verify = 0;
    int64_t nranges = 0, ncand_total = 0, nunit_total = 0;
    while (!todo.empty()) {
        const std::pair<int64_t, int64_t> r = todo.back();
        todo.pop_back();
        if (r.second <= r.first) continue;
        const auto t_scan = std::chrono::steady_clock::now();
        HIPCHK(hipMemsetAsync(d_counter, 0, sizeof(unsigned long long), st));
        if (!pl.memb.empty())
            dhk_locate_scan(st, use_bitmap, d_text, nbases, r.first, r.second, d_table, pl.tbits, d_bitmap, d_memb, d_pats, d_pw, d_starts,
                            nref, d_cands, cap, d_counter);
        dhk_locate_short(st, d_text, nbases, 32 * r.first, std::min(nbases, 32 * r.second), d_shorts, (int64_t)pl.shorts.size(), d_starts,
                         nref, d_cands, cap, d_counter);
        HIPCHK(hipGetLastError());
        unsigned long long count = 0;
        HIPCHK(hipMemcpyAsync(&count, d_counter, sizeof(count), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        ms_scan += dh_ms_since(t_scan);
        nranges++;
        if ((int64_t)count > cap) {
            if (r.second - r.first > 1) {  // the later half first on the stack, so that the ranges run in text order
                const int64_t mid = r.first + (r.second - r.first) / 2;
                todo.push_back({mid, r.second});
                todo.push_back({r.first, mid});
            } else {  // one word of positions: the buffer grows to what was counted
                if (count > 0xFFFFFFFFull) return dh_fail(DH_EOVERFLOW, "dh_exact_locate: more than 2^32 candidates at 32 positions");
                cap = (int64_t)count;
                if (int rc = dh_scr(ctx, SLOT_LOC_CANDS, (size_t)cap, &d_cands)) return rc;
                todo.push_back(r);
            }
            continue;
        }
        if (count == 0) continue;
        const auto t_verify = std::chrono::steady_clock::now();
        part.resize((size_t)count);
        HIPCHK(hipMemcpyAsync(part.data(), d_cands, sizeof(LocCand) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        loc::make_units(part.data(), (int64_t)count, pl, seg, units);
        if (!units.empty()) {
            LocUnit *d_units;
            if (int rc = dh_scr(ctx, SLOT_LOC_UNITS, (size_t)std::min<int64_t>((int64_t)units.size(), kUnitBatch), &d_units)) return rc;
            for (int64_t u0 = 0; u0 < (int64_t)units.size(); u0 += kUnitBatch) {
                const int64_t n = std::min<int64_t>(kUnitBatch, (int64_t)units.size() - u0);
                if (int rc = upload_staged(ctx, sg, d_units, units.data() + u0, sizeof(LocUnit) * (size_t)n)) return rc;
                dhk_locate_verify(st, d_text, nbases, d_pw, d_pats, d_cands, (int64_t)count, d_units, n, seg);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));  // (the staging buffer is written again by the next batch)
            }
            HIPCHK(hipMemcpyAsync(part.data(), d_cands, sizeof(LocCand) * (size_t)count, hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
        }
        for (const LocCand &c : part)
            if (c.ok) all.push_back(c);
        ncand_total += (int64_t)count;
        nunit_total += (int64_t)units.size();
        ms_verify += dh_ms_since(t_verify);
    }
    loc::finish(all, pl, starts.data(), nref, res->hits);
    if (trace)
        fprintf(stderr,
                "[locate] %lld bases in %lld records, %lld queries (%zu anchor groups, %zu short), bitmap %d: upload/pack %.2f ms, scan "
                "%.2f ms (%lld ranges), verify %.2f ms (%lld candidates, %lld units), total %.2f ms, %zu hits\n",
                (long long)nbases, (long long)nref, (long long)nqry, ngroups, pl.shorts.size(), use_bitmap, ms_upload, ms_scan,
                (long long)nranges, ms_verify, (long long)ncand_total, (long long)nunit_total, dh_ms_since(t_call), res->hits.size());
    *out = res.release();
    return DH_OK;
}

extern "C" void dh_exact_hits_destroy(dh_exact_hits *h) { delete h; }
extern "C" int64_t dh_exact_hits_count(const dh_exact_hits *h) { return h ? (int64_t)h->hits.size() : 0; }
extern "C" const dh_exact_hit *dh_exact_hits_records(const dh_exact_hits *h)
{
    return h ? (const dh_exact_hit *)h->hits.data() : nullptr;
}
