// The lane code and the host plan of the region validation (dentist_amd/csrc/dh_vreg.h) compiled for the CPU.  A workgroup is
// played the way the kernels of dh_vreg.hip use these functions: one value per lane in arrays of VR_BLOCK, four wavefronts of
// 64, a shuffle is an index, an atomicAdd a +=.  The slots of a region's segments are claimed by the records in DESCENDING
// order, the opposite of what a device would tend to do: no result may depend on it.  Every device buffer is a heap block of
// exactly the size the driver (dh_vreg.cpp) asks for, so an access behind a difference array, a pair list or an interval list
// is a report of the sanitizer.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../dentist_amd/csrc/dh_vreg.h"

using vr::Job;
using vr::Pair;
using vr::Rec;
using vr::Reg;

namespace {

// block_scan of dh_vreg.hip: the shuffle steps per wavefront, the wave totals through ws
void play_block_scan(bool is_max, const int32_t *v_in, int32_t *excl, int32_t *total)
{
    const int32_t ident = is_max ? -1 : 0;
    auto op = [&](int32_t x, int32_t y) { return is_max ? (x > y ? x : y) : x + y; };
    int32_t v[VR_BLOCK], before[VR_BLOCK], ws[VR_BLOCK / 64];
    memcpy(v, v_in, sizeof(v));
    for (int wave = 0; wave < VR_BLOCK / 64; wave++) {
        int32_t *x = v + 64 * wave;
        for (int d = 1; d < 64; d <<= 1) {
            int32_t t[64];
            for (int l = 0; l < 64; l++) t[l] = x[l >= d ? l - d : l];
            for (int l = 0; l < 64; l++)
                if (l >= d) x[l] = op(x[l], t[l]);
        }
        for (int l = 0; l < 64; l++) before[64 * wave + l] = l == 0 ? ident : x[l - 1];
        ws[wave] = x[63];
    }
    int32_t tot = ident;
    for (int w = 0; w < VR_BLOCK / 64; w++) tot = op(tot, ws[w]);
    for (int t = 0; t < VR_BLOCK; t++) {
        int32_t pre = ident;
        for (int w = 0; w < t / 64; w++) pre = op(pre, ws[w]);
        excl[t] = op(pre, before[t]);
    }
    *total = tot;
}

// k_vr_region of one job.  emit == false: rcnt[0] = intervals, rcnt[1] = their bases; emit == true: iv gets the intervals
void play_region(bool emit, const Job &j, const Pair *pairs, int32_t *diff, int32_t min_cov, uint32_t *rcnt, int32_t *iv)
{
    if (j.nw <= 0) {
        if (!emit) rcnt[0] = rcnt[1] = 0u;
        return;
    }
    for (int64_t k = 0; k <= (int64_t)j.nw; k++) diff[k] = 0;
    for (int64_t k = 0; k < j.npairs; k++) {
        const Pair p = pairs[j.pair_at + k];
        if (p.w0 < 0 || p.w0 >= p.w1e || p.w1e > j.nw) continue;
        diff[p.w0] += 1;
        diff[p.w1e] -= 1;
    }
    int32_t cov_carry = 0, last_carry = -1;
    uint32_t rank_carry = 0u, bases = 0u;
    int32_t *out = iv + 2 * j.out_at;
    for (int64_t base = 0; base < (int64_t)j.nw; base += VR_BLOCK) {
        int32_t d[VR_BLOCK], m[VR_BLOCK], o[VR_BLOCK], excl[VR_BLOCK], last[VR_BLOCK], total;
        bool weak[VR_BLOCK];
        for (int t = 0; t < VR_BLOCK; t++) d[t] = base + t < (int64_t)j.nw ? diff[base + t] : 0;
        play_block_scan(false, d, excl, &total);
        for (int t = 0; t < VR_BLOCK; t++) {
            weak[t] = base + t < (int64_t)j.nw && cov_carry + excl[t] + d[t] < min_cov;
            m[t] = weak[t] ? (int32_t)(base + t) : -1;
        }
        cov_carry += total;
        play_block_scan(true, m, excl, &total);
        for (int t = 0; t < VR_BLOCK; t++) {
            last[t] = excl[t] > last_carry ? excl[t] : last_carry;
            o[t] = weak[t] && vr::opens(base + t, last[t], j.wlen) ? 1 : 0;
        }
        last_carry = total > last_carry ? total : last_carry;
        play_block_scan(false, o, excl, &total);
        for (int t = 0; t < VR_BLOCK; t++) {
            if (!o[t]) continue;
            const uint32_t rank = rank_carry + (uint32_t)excl[t];
            const int64_t w = base + t;
            if (emit) {
                out[2 * (int64_t)rank] = j.cb + (int32_t)w;
                if (last[t] >= 0) out[2 * (int64_t)rank - 1] = j.cb + last[t] + j.wlen;
            } else
                bases += (last[t] >= 0 ? (uint32_t)(last[t] + j.wlen) : 0u) - (uint32_t)w;
        }
        rank_carry += (uint32_t)total;
    }
    if (last_carry >= 0) {
        if (emit)
            out[2 * (int64_t)rank_carry - 1] = j.cb + last_carry + j.wlen;
        else
            bases += (uint32_t)(last_carry + j.wlen);
    }
    if (!emit) rcnt[0] = rank_carry, rcnt[1] = bases;
}

}  // namespace

// What dh_la_validate_regions does, on the CPU.  lds_windows / budget: DH_VREG_LDS_WINDOWS and DH_VREG_SLAB_MB << 20.  Returns the
// number of weak triples, or -1 with info[4] = the offending record, info[5] = region, info[6] = contig (-1 otherwise).  info[0]
// pairs, [1] regions of the global tier, [2] launch groups, [3] intervals of the merged mask.  weak / span_ids / mask_iv are
// filled up to their caps (triples, ids, pairs).
extern "C" int64_t vreg_host(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const dh_region *regions,
                             int32_t nregions, int32_t region_context, int32_t window, int32_t min_cov, int32_t min_span,
                             int64_t lds_windows, int64_t budget, dh_region_report *reports, int32_t *weak, int64_t weak_cap,
                             int64_t *span_off, int32_t *span_ids, int64_t span_cap, int64_t *mask_ptr, int32_t *mask_iv, int64_t mask_cap,
                             int64_t *info)
{
    for (int k = 0; k < 8; k++) info[k] = 0;
    info[4] = info[5] = info[6] = -1;
    vr::Plan pl;
    vr::Fault f;
    vr::build_plan(las, n, contig_off, ncontigs, regions, nregions, region_context, window,
                   [](int64_t m, const std::function<void(int64_t, int64_t)> &body) {
                       for (int64_t lo = 0; lo < m; lo += 1000) body(lo, std::min(m, lo + 1000));
                   },
                   pl, f);
    if (f.any()) {
        info[4] = f.record, info[5] = f.region, info[6] = f.contig;
        return -1;
    }
    const size_t nreg = (size_t)nregions;
    for (size_t s = 0; s < nreg; s++) vr::fill_report(pl.regs[s], 0, 0, min_span, &reports[pl.perm[s]]);
    for (size_t r = 0; r <= nreg; r++) span_off[r] = 0;
    for (int32_t c = 0; c <= ncontigs; c++) mask_ptr[c] = 0;
    if (n == 0 || nregions == 0) return 0;
    std::unique_ptr<Rec[]> recs(new Rec[(size_t)n]);
    memcpy(recs.get(), pl.recs.data(), sizeof(Rec) * (size_t)n);
    std::unique_ptr<Reg[]> regs(new Reg[nreg]);
    memcpy(regs.get(), pl.regs.data(), sizeof(Reg) * nreg);
    // k_vr_bind<false>
    std::vector<uint64_t> cnt(3 * nreg, 0);
    for (int64_t i = 0; i < n; i++) {
        int64_t lo, hi;
        vr::candidates(recs[(size_t)i], pl.rptr.data(), regs.get(), &lo, &hi);
        for (int64_t s = lo; s < hi; s++) {
            Pair p;
            const uint32_t what = vr::classify(recs[(size_t)i], regs[(size_t)s], &p);
            cnt[3 * s] += what & vr::PAIR ? 1 : 0;
            cnt[3 * s + 1] += what & vr::WINDOWS ? 1 : 0;
            cnt[3 * s + 2] += what & vr::SPANS ? 1 : 0;
        }
    }
    for (size_t s = 0; s < nreg; s++) {
        info[0] += (int64_t)cnt[3 * s];
        info[1] += vr::is_big(vr::live_windows(pl.regs[s], cnt[3 * s]), lds_windows) ? 1 : 0;
    }
    std::vector<vr::Group> groups;
    vr::build_groups(pl, cnt.data(), lds_windows, budget, groups);
    info[2] = (int64_t)groups.size();
    std::vector<std::vector<int32_t>> weak_of(nreg), span_of(nreg);
    for (const vr::Group &g : groups) {
        const size_t ng = (size_t)(g.s1 - g.s0);
        std::vector<int64_t> at(2 * ng, 0);
        int64_t npairs = 0, nspan = 0;
        for (size_t k = 0; k < ng; k++) {
            at[2 * k] = npairs, at[2 * k + 1] = nspan;
            npairs += (int64_t)cnt[3 * (g.s0 + k) + 1];
            nspan += (int64_t)cnt[3 * (g.s0 + k) + 2];
        }
        std::unique_ptr<Pair[]> pairs(new Pair[(size_t)npairs]);
        std::unique_ptr<int64_t[]> span_idx(new int64_t[(size_t)nspan]);
        std::unique_ptr<int32_t[]> span_out(new int32_t[(size_t)nspan]);
        std::vector<uint64_t> cur(2 * ng, 0);
        // k_vr_bind<true>, the records of the group's contigs, last record first
        const int32_t c0 = pl.regs[(size_t)g.s0].contig, c1 = pl.regs[(size_t)g.s1 - 1].contig;
        for (int64_t i = n - 1; i >= 0; i--) {
            const Rec &r = recs[(size_t)i];
            if (r.aread < c0 || r.aread > c1) continue;
            int64_t lo, hi;
            vr::candidates(r, pl.rptr.data(), regs.get(), &lo, &hi);
            lo = std::max(lo, g.s0), hi = std::min(hi, g.s1);
            for (int64_t s = lo; s < hi; s++) {
                Pair p;
                const uint32_t what = vr::classify(r, regs[(size_t)s], &p);
                const size_t k = (size_t)(s - g.s0);
                if (what & vr::WINDOWS) pairs[(size_t)(at[2 * k] + (int64_t)cur[2 * k]++)] = p;
                if (what & vr::SPANS) span_idx[(size_t)(at[2 * k + 1] + (int64_t)cur[2 * k + 1]++)] = i;
            }
        }
        for (size_t k = 0; k < ng; k++)
            if (cur[2 * k] != cnt[3 * (g.s0 + k) + 1] || cur[2 * k + 1] != cnt[3 * (g.s0 + k) + 2]) return -2;  // the two passes disagree
        // k_vr_span
        for (size_t k = 0; k < ng; k++) {
            const int64_t m = (int64_t)cnt[3 * (g.s0 + k) + 2], first = at[2 * k + 1];
            for (int64_t x = 0; x < m; x++)
                span_out[(size_t)(first + vr::rank_of(span_idx.get() + first, m, span_idx[(size_t)(first + x)]))] =
                    recs[(size_t)span_idx[(size_t)(first + x)]].bread;
            span_of[(size_t)g.s0 + k].assign(span_out.get() + first, span_out.get() + first + m);
        }
        // k_vr_region: count, place, emit.  The array of a region is of exactly its size in either tier
        std::vector<Job> jobs;
        std::vector<size_t> job_reg;
        int64_t cost = 0;
        for (int big = 0; big < 2; big++)
            for (size_t k = 0; k < ng; k++) {
                const size_t s = (size_t)g.s0 + k;
                const int32_t nw = vr::live_windows(pl.regs[s], cnt[3 * s]);
                if ((int)vr::is_big(nw, lds_windows) != big) continue;
                jobs.push_back(Job{pl.regs[s].cb, pl.regs[s].wlen, nw, 0, at[2 * k], (int64_t)cnt[3 * s + 1], 0, 0});
                job_reg.push_back(s);
                if (big) cost += vr::slab_entries(nw) * 4;
            }
        cost += npairs * (int64_t)sizeof(Pair) + nspan * 12;
        if (cost > budget && ng > 1) return -3;  // the bound of the groups does not hold
        std::vector<uint32_t> rcnt(2 * ng);
        int64_t niv = 0;
        for (size_t q = 0; q < ng; q++) {
            std::unique_ptr<int32_t[]> diff(new int32_t[(size_t)jobs[q].nw + 1]);
            play_region(false, jobs[q], pairs.get(), diff.get(), min_cov, &rcnt[2 * q], nullptr);
            jobs[q].out_at = niv;
            niv += (int64_t)rcnt[2 * q];
        }
        std::unique_ptr<int32_t[]> iv(new int32_t[(size_t)(2 * niv)]);
        for (size_t q = 0; q < ng; q++) {
            std::unique_ptr<int32_t[]> diff(new int32_t[(size_t)jobs[q].nw + 1]);
            play_region(true, jobs[q], pairs.get(), diff.get(), min_cov, nullptr, iv.get());
            const size_t s = job_reg[q];
            weak_of[s].assign(iv.get() + 2 * jobs[q].out_at, iv.get() + 2 * (jobs[q].out_at + (int64_t)rcnt[2 * q]));
            vr::fill_report(pl.regs[s], (int64_t)cnt[3 * s + 2], (int64_t)rcnt[2 * q + 1], min_span, &reports[pl.perm[s]]);
        }
    }
    std::vector<size_t> plan_of(nreg);
    for (size_t s = 0; s < nreg; s++) plan_of[(size_t)pl.perm[s]] = s;
    std::vector<int32_t> all_weak;
    int64_t nids = 0;
    for (size_t r = 0; r < nreg; r++) {
        const size_t s = plan_of[r];
        for (size_t x = 0; x + 1 < weak_of[s].size(); x += 2) {
            all_weak.push_back(regions[r].contig);
            all_weak.push_back(weak_of[s][x]);
            all_weak.push_back(weak_of[s][x + 1]);
        }
        for (int32_t id : span_of[s]) {
            if (nids < span_cap) span_ids[nids] = id;
            nids++;
        }
        span_off[r + 1] = nids;
    }
    for (size_t k = 0; k < all_weak.size() && (int64_t)k < 3 * weak_cap; k++) weak[k] = all_weak[k];
    std::vector<int64_t> mp;
    std::vector<int32_t> mi;
    vr::merge_mask(all_weak, ncontigs, mp, mi);
    for (int32_t c = 0; c <= ncontigs; c++) mask_ptr[c] = mp[(size_t)c];
    for (size_t k = 0; k < mi.size() && (int64_t)k < 2 * mask_cap; k++) mask_iv[k] = mi[k];
    info[3] = (int64_t)mi.size() / 2;
    return (int64_t)all_weak.size() / 3;
}
