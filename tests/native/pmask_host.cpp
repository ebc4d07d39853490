// The lane code and the host plan of the mask propagation (dentist_amd/csrc/dh_pmask.h) compiled for the CPU.  A wavefront is
// played the way the kernels of dh_pmask.hip use these functions: one value per lane in arrays of 64, a shuffle is an index,
// a ballot a loop, an atomicOr an |=.  Every device buffer is a heap block of exactly the size the driver (dh_pmask.cpp) asks
// for, so an access behind the edge words of the bitmap or the last chunk of a trace is a report of the sanitizer.  The scans
// are the driver's; here they are loops.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../dentist_amd/csrc/dh_pmask.h"

using pm::Raw;
using pm::Rec;

namespace {

template <typename T>
std::unique_ptr<T[]> exact(const T *src, size_t n)  // an exact-size heap copy (n == 0: a block of no elements)
{
    std::unique_ptr<T[]> p(new T[n]);
    if (n) memcpy(p.get(), src, sizeof(T) * n);
    return p;
}

// k_pm_translate: one wavefront, one record
void play_translate(const Rec &r, uint32_t n_iv, int64_t m0, const uint16_t *trace, int32_t ts, const int32_t *mask_iv, Raw *out, int64_t i,
                    int64_t *bad, int64_t *nonempty, int64_t *chunks_walked)
{
    const uint16_t *tr = trace + r.toff;
    int32_t c = 0;
    int64_t carry = 0;
    for (uint32_t j0 = 0; j0 < n_iv; j0 += 64) {
        const int32_t nlive = (int32_t)std::min<uint32_t>(64u, n_iv - j0);
        int32_t ib[64], ie[64], incl[64];
        int64_t pb[64], pe[64];
        for (int l = 0; l < 64; l++) {
            ib[l] = ie[l] = 0;
            pb[l] = pe[l] = 0;
            if (l < nlive) pm::cut_indices(r, ts, mask_iv[2 * (m0 + j0 + l)], mask_iv[2 * (m0 + j0 + l) + 1], &ib[l], &ie[l]);
        }
        const int32_t c_last = pm::chunk_of(ie[nlive - 1]);
        int32_t c_next = -1;
        if (j0 + 64 < n_iv) {
            int32_t nb, ne;
            pm::cut_indices(r, ts, mask_iv[2 * (m0 + j0 + 64)], mask_iv[2 * (m0 + j0 + 64) + 1], &nb, &ne);
            c_next = pm::chunk_of(nb);
        }
        const int32_t c_end = std::max(c_last, c_next);
        int32_t keep_c = c;
        int64_t keep_carry = carry;
        for (; c <= c_end; c++) {
            if (c == c_next) keep_c = c, keep_carry = carry;
            int32_t run = 0;
            for (int l = 0; l < 64; l++) {  // the wave scan
                run += pm::tile_bases(tr, r.ntp, (int64_t)c * 64 + l);
                incl[l] = run;
            }
            for (int l = 0; l < 64; l++) {
                const int32_t at_b = incl[(ib[l] - 1) & 63], at_e = incl[(ie[l] - 1) & 63];
                if (ib[l] > 0 && pm::chunk_of(ib[l]) == c) pb[l] = carry + at_b;
                if (ie[l] > 0 && pm::chunk_of(ie[l]) == c) pe[l] = carry + at_e;
            }
            carry += incl[63];
            (*chunks_walked)++;
        }
        if (c_next >= 0) c = keep_c, carry = keep_carry;
        for (int l = 0; l < nlive; l++) {
            Raw x;
            if (!pm::finish(r, pb[l], pe[l], &x) && i < *bad) *bad = i;
            out[j0 + l] = x;
            if (x.b < x.e) (*nonempty)++;
        }
    }
}

// k_pm_paint: the wavefront that holds the raw intervals [i0, i0 + 64)
void play_paint_wave(const Raw *raw, int64_t n, int64_t i0, const int64_t *boff, int32_t r0, int32_t r1, int64_t base_bit, uint32_t *bm)
{
    bool wide[64];
    int64_t bit0[64], bit1[64];
    for (int l = 0; l < 64; l++) {
        const int64_t i = i0 + l;
        Raw x = Raw{-1, 0, 0};
        if (i < n) x = raw[i];
        const bool have = i < n && pm::paintable(x, boff, r0, r1);
        bit0[l] = bit1[l] = 0;
        if (have) {
            bit0[l] = boff[x.rd] - base_bit + x.b;
            bit1[l] = boff[x.rd] - base_bit + x.e;
        }
        wide[l] = have && ((bit1[l] - 1) >> 5) - (bit0[l] >> 5) >= PM_SHORT_WORDS;
        if (have && !wide[l])
            for (int64_t w = bit0[l] >> 5; w <= (bit1[l] - 1) >> 5; w++) bm[w] |= pm::word_mask(bit0[l], bit1[l], w);
    }
    for (int src = 0; src < 64; src++) {
        if (!wide[src]) continue;
        for (int l = 0; l < 64; l++)
            for (int64_t w = (bit0[src] >> 5) + l; w <= (bit1[src] - 1) >> 5; w += 64) bm[w] |= pm::word_mask(bit0[src], bit1[src], w);
    }
}

void exclusive_scan(std::vector<uint32_t> &v, int64_t at, int64_t n, uint64_t *total)
{
    uint64_t run = 0;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t x = v[(size_t)(at + i)];
        v[(size_t)(at + i)] = (uint32_t)run;
        run += x;
    }
    *total = run;
}

}  // namespace

// What dh_la_propagate_mask does, on the CPU.  cap_bits: the largest bitmap of a destination range; group_raw: the bound on a
// launch group's raw intervals.  Returns the number of intervals (out_ptr: nreads + 1, out_iv: up to cap pairs), or -1 with
// info[6] = the offending record or info[7] = the offending contig (-1 otherwise).  info[0] non-empty raw intervals, [1]
// records with a mask interval, [2] destination ranges, [3] launch groups, [4] raw intervals, [5] chunks of tiles walked.
extern "C" int64_t pmask_host(const dh_la *las, int64_t n, const uint16_t *trace_in, int64_t trace_len, int32_t tspace, const int64_t *mask_ptr,
                              const int32_t *mask_iv_in, int32_t ncontigs, const int64_t *read_off, int32_t nreads, int64_t cap_bits,
                              int64_t group_raw, int64_t *out_ptr, int32_t *out_iv, int64_t cap, int64_t *info)
{
    for (int k = 0; k < 8; k++) info[k] = 0;
    info[6] = info[7] = -1;
    pm::Plan pl;
    pm::Fault f;
    pm::build_plan(las, n, trace_len, tspace, mask_ptr, mask_iv_in, ncontigs, read_off, nreads, group_raw, cap_bits,
                   [](int64_t m, const std::function<void(int64_t, int64_t)> &body) {
                       for (int64_t lo = 0; lo < m; lo += 1000) body(lo, std::min(m, lo + 1000));
                   },
                   pl, f);
    if (f.contig != -1 || f.record >= 0) {
        info[6] = f.record;
        info[7] = f.contig;
        return -1;
    }
    for (int32_t r = 0; r <= nreads; r++) out_ptr[r] = 0;
    const int64_t nmask = ncontigs > 0 ? mask_ptr[ncontigs] : 0;
    if (n == 0 || nmask == 0 || nreads == 0) return 0;
    const auto trace = exact(trace_in, (size_t)trace_len);
    const auto mask_iv = exact(mask_iv_in, (size_t)(2 * nmask));
    const auto boff = exact(pl.boff.data(), pl.boff.size());
    const size_t ngr = pl.group_at.size() - 1;
    info[3] = (int64_t)ngr;
    // k_pm_plan and the scans per launch group
    std::vector<int64_t> lo((size_t)n);
    std::vector<uint32_t> cnt((size_t)n), off((size_t)n), has((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        pm::plan_lane(pl.recs[(size_t)i], mask_ptr, mask_iv.get(), &lo[(size_t)i], &cnt[(size_t)i]);
        off[(size_t)i] = cnt[(size_t)i];
        has[(size_t)i] = cnt[(size_t)i] ? 1u : 0u;
    }
    std::vector<uint64_t> traw(ngr), thit(ngr);
    int64_t nraw = 0, nhit = 0;
    for (size_t g = 0; g < ngr; g++) {
        const int64_t g0 = pl.group_at[g], ng = pl.group_at[g + 1] - g0;
        exclusive_scan(off, g0, ng, &traw[g]);
        exclusive_scan(has, g0, ng, &thit[g]);
        if (traw[g] > (uint64_t)group_raw && ng > 1) return -2;  // the bound of the plan does not hold
        nraw += (int64_t)traw[g];
        nhit += (int64_t)thit[g];
    }
    info[1] = nhit;
    info[4] = nraw;
    if (nraw == 0) return 0;
    // k_pm_compact, k_pm_translate
    std::unique_ptr<Raw[]> raw(new Raw[(size_t)nraw]);
    std::unique_ptr<int64_t[]> list(new int64_t[(size_t)nhit]);
    int64_t raw_at = 0, list_at = 0, bad = INT64_MAX;
    for (size_t g = 0; g < ngr; g++) {
        const int64_t g0 = pl.group_at[g], ng = pl.group_at[g + 1] - g0;
        for (int64_t i = 0; i < ng; i++)
            if (cnt[(size_t)(g0 + i)]) list[(size_t)(list_at + has[(size_t)(g0 + i)])] = g0 + i;
        for (int64_t k = 0; k < (int64_t)thit[g]; k++) {
            const int64_t i = list[(size_t)(list_at + k)];
            play_translate(pl.recs[(size_t)i], cnt[(size_t)i], lo[(size_t)i], trace.get(), tspace, mask_iv.get(), raw.get() + raw_at + off[(size_t)i],
                           i, &bad, &info[0], &info[5]);
        }
        raw_at += (int64_t)traw[g];
        list_at += (int64_t)thit[g];
    }
    if (bad != INT64_MAX) {
        info[6] = bad;
        return -1;
    }
    // per destination range: clear, paint, read out
    const size_t npass = pl.range_at.size() - 1;
    info[2] = (int64_t)npass;
    int64_t k0 = 0;
    for (size_t p = 0; p < npass; p++) {
        const int32_t r0 = pl.range_at[p], r1 = pl.range_at[p + 1];
        const int64_t base_bit = pl.boff[(size_t)r0], words = pm::padded_words(pl.boff[(size_t)r1] - base_bit), groups = words / PM_GROUP_WORDS;
        if (words > pm::padded_words(pl.max_range_bits)) return -3;
        std::unique_ptr<uint32_t[]> bm(new uint32_t[(size_t)words]);
        memset(bm.get(), 0, sizeof(uint32_t) * (size_t)words);
        for (int64_t i0 = 0; i0 < nraw; i0 += 64) play_paint_wave(raw.get(), nraw, i0, boff.get(), r0, r1, base_bit, bm.get());
        std::vector<uint32_t> cs((size_t)groups), ce((size_t)groups);
        for (int64_t g = 0; g < groups; g++) pm::runs_count_lane(bm.get(), g, &cs[(size_t)g], &ce[(size_t)g]);
        uint64_t ts_ = 0, te_ = 0;
        exclusive_scan(cs, 0, groups, &ts_);
        exclusive_scan(ce, 0, groups, &te_);
        if (ts_ != te_) return -4;
        std::unique_ptr<int32_t[]> iv(new int32_t[(size_t)(2 * ts_)]);
        for (int64_t g = 0; g < groups; g++)
            pm::runs_emit_lane(bm.get(), g, base_bit, boff.get(), r0, r1, cs[(size_t)g], ce[(size_t)g], iv.get());
        for (int32_t r = r0; r < r1; r++) out_ptr[r] = k0 + pm::runs_ptr_lane(bm.get(), cs.data(), base_bit, boff.get(), r);
        for (uint64_t k = 0; k < 2 * ts_; k++)
            if (2 * k0 + (int64_t)k < 2 * cap) out_iv[2 * k0 + (int64_t)k] = iv[(size_t)k];
        k0 += (int64_t)ts_;
    }
    out_ptr[nreads] = k0;
    return k0;
}
