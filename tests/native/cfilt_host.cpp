// The lane code and the host plan of the collect filters (dentist_amd/csrc/dh_cfilt.h) compiled for the CPU.  The kernels of
// dh_cfilt.hip are played the way they use these functions: a wavefront is 64 values in an array, a shuffle is an index, a ballot
// a loop, an atomicAdd a +=; a workgroup runs its threads one after the other between two barriers.  The slots of a read's
// segment are claimed by the units in DESCENDING order, the opposite of what a device would tend to do: no result may depend on
// it.  Every device buffer is a heap block of exactly the size the driver (dh_cfilt.cpp) asks for -- the order of a read in the
// workgroup tiers of exactly pow2ceil(units) entries -- so an access behind one is a report of the sanitizer.
#include <stdint.h>
#include <string.h>

#include <memory>
#include <vector>

#include "../../dentist_amd/csrc/dh_cfilt.h"

using cf::Mask;
using cf::Opts;
using cf::Rec;
using cf::Unit;

namespace {

// k_cf_wave for one read of 2..64 units
void play_wave(const Unit *units, const int32_t *goff, const int32_t *gidx, int32_t r, uint8_t *why, uint8_t *used)
{
    const int32_t g0 = goff[r], size = goff[r + 1] - g0;
    Unit me[64], moved[64];
    int32_t idx[64], rank[64], src[64], midx[64];
    bool in[64];
    for (int l = 0; l < 64; l++) {
        in[l] = l < size;
        idx[l] = in[l] ? gidx[g0 + l] : -1;
        me[l] = units[in[l] ? idx[l] : gidx[g0]];
        rank[l] = 0, src[l] = 0;
    }
    for (int32_t z = 0; z < size; z++)
        for (int l = 0; l < 64; l++) rank[l] += in[l] && cf::key_less(me[z], idx[z], me[l], idx[l]) ? 1 : 0;
    for (int32_t z = 0; z < size; z++)
        for (int l = 0; l < 64; l++)
            if (rank[z] == l) src[l] = z;
    for (int l = 0; l < 64; l++) {
        if (!in[l]) src[l] = 0;
        moved[l] = me[src[l]];
        midx[l] = in[l] ? idx[src[l]] : -1;
    }
    memcpy(me, moved, sizeof(me));
    memcpy(idx, midx, sizeof(idx));
    bool mark[64] = {false};
    for (int32_t x = 0; x + 1 < size; x++) {
        const Unit ux = me[x];
        if (ux.st & cf::DIS) continue;
        int32_t reach = size;
        for (int l = 63; l >= 0; l--)
            if (in[l] && l > x && !cf::scan_goes_on(ux, me[l])) reach = l;  // (the lowest set bit of the ballot)
        for (int l = 0; l < 64; l++)
            if (in[l] && l > x && l < reach && cf::drops(ux, me[l]) && !(me[l].st & cf::DIS)) mark[l] = true;
    }
    uint8_t w[64];
    bool en[64], amb[64], any_amb = false, any_red = false;
    for (int l = 0; l < 64; l++) {
        w[l] = in[l] ? why[idx[l]] : (uint8_t)cf::W_NONE;
        if (mark[l]) w[l] = cf::W_CONTAINED;
        en[l] = in[l] && cf::enabled(me[l], w[l]);
        amb[l] = false;
    }
    for (int32_t z = 0; z < size; z++)
        for (int l = 0; l < 64; l++)
            if (en[l] && en[z] && z != l && cf::intersect(me[l], me[z])) amb[l] = true;
    for (int l = 0; l < 64; l++) any_amb = any_amb || amb[l];
    if (!any_amb)
        for (int l = 0; l < 64; l++) any_red = any_red || (en[l] && (me[l].st & cf::RED));
    for (int l = 0; l < 64; l++) {
        if (en[l] && (any_amb || any_red)) w[l] = any_amb ? cf::W_AMBIGUOUS : cf::W_REDUNDANT;
        if (in[l] && w[l] != cf::W_NONE) why[idx[l]] = w[l];
    }
    if (any_amb || any_red) used[r] = 0;
}

// k_cf_block for one read: ord is the read's part of LDS or of the slab
void play_block(const Unit *units, const int32_t *goff, const int32_t *gidx, int32_t r, int32_t *ord, uint8_t *why, uint8_t *used)
{
    const int32_t g0 = goff[r], size = goff[r + 1] - g0, P = cf::pow2ceil(size);
    for (int32_t t = 0; t < P; t++) ord[t] = t < size ? gidx[g0 + t] : -1;
    for (int32_t k = 2; k <= P; k <<= 1)
        for (int32_t j = k >> 1; j > 0; j >>= 1)
            for (int32_t t = P / 2 - 1; t >= 0; t--) cf::bt_compare(ord, units, t, k, j);  // (the comparators of a step are disjoint)
    for (int32_t x = size - 2; x >= 0; x--) cf::bt_contained(ord, size, units, why, x);
    int32_t hit = 0;
    for (int32_t x = 0; x + 1 < size; x++)
        if (cf::bt_ambiguous(ord, size, units, why, x)) hit = 1;
    const bool any_amb = hit != 0;
    if (!any_amb)
        for (int32_t x = 0; x < size; x++)
            if (cf::enabled(units[ord[x]], why[ord[x]]) && (units[ord[x]].st & cf::RED)) hit = 1;
    if (!hit) return;
    for (int32_t x = 0; x < size; x++)
        if (cf::enabled(units[ord[x]], why[ord[x]])) why[ord[x]] = any_amb ? cf::W_AMBIGUOUS : cf::W_REDUNDANT;
    used[r] = 0;
}

}  // namespace

// What dh_la_collect_filter does, on the CPU; lds_units: DH_CFILT_LDS_UNITS.  Returns 0, or -1 with info[4] = the offending record,
// info[5] = contig (-1 otherwise), or -2 if the tiers do not add up.  info[0] chains, [1] reads of the wave tier, [2] of the LDS
// tier, [3] of the global tier.  rep_ptr, dropped6 and read_used may be NULL.
extern "C" int64_t cfilt_host(dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                              const int64_t *rep_ptr, const int32_t *rep_iv, int32_t ppm, int32_t allowance, int32_t min_anchor,
                              int32_t lds_units, int64_t *dropped6, uint8_t *read_used, int64_t *info)
{
    for (int k = 0; k < 8; k++) info[k] = 0;
    info[4] = info[5] = -1;
    std::unique_ptr<Rec[]> recs(new Rec[(size_t)std::max<int64_t>(n, 0)]);
    std::unique_ptr<int32_t[]> alen(new int32_t[(size_t)ncontigs]), blen(new int32_t[(size_t)nreads]);
    cf::Plan pl;
    pl.recs = recs.get(), pl.alen = alen.get(), pl.blen = blen.get();
    cf::Fault f;
    cf::build_plan(las, n, contig_off, ncontigs, read_off, nreads, rep_ptr, rep_iv,
                   [](int64_t m, const std::function<void(int64_t, int64_t)> &body) {
                       for (int64_t lo = 0; lo < m; lo += 1000) body(lo, std::min(m, lo + 1000));
                   },
                   pl, f);
    if (f.any()) {
        info[4] = f.record, info[5] = f.contig;
        return -1;
    }
    if (dropped6) memset(dropped6, 0, 6 * sizeof(int64_t));
    if (read_used && nreads > 0) memset(read_used, 1, (size_t)nreads);
    if (n == 0) return 0;
    const size_t sn = (size_t)n, sr = (size_t)nreads;
    // the mask as the driver uploads it: ncontigs + 1 offsets, the intervals of all contigs, their prefix sums
    const size_t nmask = rep_ptr ? pl.pre.size() - 1 : 0;
    std::unique_ptr<int64_t[]> m_ptr(new int64_t[(size_t)ncontigs + 1]), m_pre(new int64_t[nmask + 1]);
    std::unique_ptr<int32_t[]> m_iv(new int32_t[2 * nmask]);
    if (rep_ptr) {
        memcpy(m_ptr.get(), rep_ptr, sizeof(int64_t) * ((size_t)ncontigs + 1));
        if (nmask) memcpy(m_iv.get(), rep_iv, sizeof(int32_t) * 2 * nmask);
        memcpy(m_pre.get(), pl.pre.data(), sizeof(int64_t) * (nmask + 1));
    }
    const Mask mask{rep_ptr ? m_ptr.get() : nullptr, m_iv.get(), m_pre.get()};
    const Opts o{ppm, allowance, min_anchor, 0};
    // k_cf_start, the scan, k_cf_first
    std::unique_ptr<int32_t[]> flag(new int32_t[sn]), uid(new int32_t[sn]), first(new int32_t[sn + 1]);
    int32_t nu = 0;
    for (int64_t i = 0; i < n; i++) {
        flag[i] = i == 0 || !cf::continues(recs[i - 1], recs[i]) ? 1 : 0;
        nu += flag[i];
        uid[i] = nu - 1;
        if (flag[i]) first[nu - 1] = (int32_t)i;
    }
    first[nu] = (int32_t)n;
    info[0] = nu;
    // k_cf_unit
    std::unique_ptr<Unit[]> units(new Unit[sn]);
    std::unique_ptr<uint8_t[]> why(new uint8_t[sn]), used(new uint8_t[std::max<size_t>(sr, 1)]), out(new uint8_t[sn]);
    std::unique_ptr<int32_t[]> goff(new int32_t[sr + 1]), cur(new int32_t[std::max<size_t>(sr, 1)]), gidx(new int32_t[sn]);
    memset(goff.get(), 0, sizeof(int32_t) * (sr + 1));
    memset(cur.get(), 0, sizeof(int32_t) * std::max<size_t>(sr, 1));
    memset(used.get(), 1, std::max<size_t>(sr, 1));
    for (int32_t u = 0; u < nu; u++) {
        why[u] = cf::make_unit(recs.get(), first[u], first[u + 1], nu == n, mask, pl.alen, pl.blen, o, &units[u]);
        goff[units[u].bread]++;
    }
    for (int32_t r = 0, at = 0; r <= nreads; r++) {
        const int32_t c = goff[r];
        goff[r] = at;
        at += c;
    }
    // k_cf_scatter, the last unit first
    for (int32_t u = nu - 1; u >= 0; u--) gidx[goff[units[u].bread] + cur[units[u].bread]++] = u;
    // k_cf_classify and the tiers
    const size_t cap_w = std::min(sr, sn / 2), cap_l = std::min(sr, sn / (CF_WAVE_UNITS + 1)), cap_g = std::min(sr, sn / ((size_t)lds_units + 1));
    std::unique_ptr<int32_t[]> l_wave(new int32_t[cap_w]), l_lds(new int32_t[cap_l]), l_glob(new int32_t[cap_g]);
    size_t nw = 0, nl = 0, ng = 0;
    for (int32_t r = nreads - 1; r >= 0; r--) {
        const int32_t size = goff[r + 1] - goff[r];
        switch (cf::tier_of(size, lds_units)) {
        case 1: {
            const int32_t u = gidx[goff[r]];
            if (cf::single(units[u], &why[u])) used[r] = 0;
            break;
        }
        case 2: l_wave[nw++] = r; break;
        case 3: l_lds[nl++] = r; break;
        case 4: l_glob[ng++] = r; break;
        default: break;
        }
    }
    if (nw > cap_w || nl > cap_l || ng > cap_g) return -2;
    info[1] = (int64_t)nw, info[2] = (int64_t)nl, info[3] = (int64_t)ng;
    for (size_t k = 0; k < nw; k++) play_wave(units.get(), goff.get(), gidx.get(), l_wave[k], why.get(), used.get());
    for (int big = 0; big < 2; big++)
        for (size_t k = 0; k < (big ? ng : nl); k++) {
            const int32_t r = big ? l_glob[k] : l_lds[k];
            std::unique_ptr<int32_t[]> ord(new int32_t[(size_t)cf::pow2ceil(goff[r + 1] - goff[r])]);
            play_block(units.get(), goff.get(), gidx.get(), r, ord.get(), why.get(), used.get());
        }
    // k_cf_finish
    int64_t cnt6[6] = {0, 0, 0, 0, 0, 0};
    for (int64_t i = 0; i < n; i++) {
        const int32_t u = uid[i];
        out[i] = ((units[u].st & cf::DIS) || why[u] != cf::W_NONE) ? 1 : 0;
        if (flag[i] && why[u] != cf::W_NONE) cnt6[why[u] - 1]++;
    }
    for (int64_t i = 0; i < n; i++)
        if (out[i]) las[i].flags |= DH_FLAG_DISABLED;
    if (dropped6) memcpy(dropped6, cnt6, sizeof(cnt6));
    if (read_used && nreads > 0) memcpy(read_used, used.get(), sr);
    return 0;
}
