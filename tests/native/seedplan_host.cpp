// The plan of the seed stage (dentist_amd/csrc/dh_seed_plan.h: every decision plan_seeds, plan_mj_chunk and seed_chunk take,
// as functions of numbers) behind a C interface.  Test infrastructure (tests/test_seed_plan.py compares it with
// tests/seed_plan_ref.py; seedplan_host_main.cpp is the stand-alone program for a sanitizer build).
// Knobs travel as 16 integers and the percentage, constants as 13 integers and the rate, in the order of the structs.
#include <stdint.h>

#include <vector>

#include "../../dentist_amd/csrc/dh_seed_plan.h"

using namespace seedplan;

namespace {
SeedKnobs knobs_of(const int64_t *v, double big_pct)
{
    SeedKnobs kn;
    kn.has_seed_cap = v[0] != 0;
    kn.seed_cap = (int)v[1];
    kn.no16k = v[2] != 0;
    kn.no_wave_tier = v[3] != 0;
    kn.no_mid_tier = v[4] != 0;
    kn.has_big_pct = v[5] != 0;
    kn.big_pct = big_pct;
    kn.has_mjoin_min = v[6] != 0;
    kn.mjoin_min = v[7];
    kn.has_mjoin_pages = v[8] != 0;
    kn.mjoin_pages = v[9];
    kn.no_mjoin = v[10] != 0;
    kn.no_tjoin = v[11] != 0;
    kn.has_tjoin_cap = v[12] != 0;
    kn.tjoin_cap = v[13];
    kn.has_tjoin_hitcap = v[14] != 0;
    kn.tjoin_hitcap = v[15];
    return kn;
}
SeedConsts consts_of(const int64_t *v, double rate0)
{
    return SeedConsts{v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], rate0, v[10], v[11], v[12]};
}
struct Unit {
    int32_t g, r0, r1, zero;
};
}  // namespace

extern "C" {
double sp_chance_density(int64_t ix_n, int32_t kmer_mod, int32_t k, int32_t ngroups) { return chance_density(ix_n, kmer_mod, k, ngroups); }
int32_t sp_first_cap(int32_t max_len, int32_t kmer_mod, double dens, int32_t self, int32_t joined, const uint32_t *jhist, int32_t nreads,
                     const int64_t *kn, double pct)
{
    return first_cap(max_len, kmer_mod, dens, self != 0, joined != 0, jhist, nreads, knobs_of(kn, pct));
}
int64_t sp_mj_min_bases(const int64_t *kn, double pct) { return mj_min_bases(knobs_of(kn, pct)); }
int32_t sp_mj_chunk_size_ok(int64_t bases, int64_t min_bases) { return mj_chunk_size_ok(bases, min_bases); }
int64_t sp_tj_cap_entries(const int64_t *kn, double pct, const int64_t *k, double rate0)
{
    return tj_cap_entries(knobs_of(kn, pct), consts_of(k, rate0));
}
// out: tb, ntiles, ntiles_pad, ngroups, nseg, exp_ent, npages, fits
void sp_mj_geometry(int64_t bases, int32_t max_len, int32_t kmer_mod, double hit_frac, double dens, int32_t ncu, const int64_t *kn, double pct,
                    const int64_t *k, double rate0, int64_t *out)
{
    const MjGeom g = mj_geometry(bases, max_len, kmer_mod, hit_frac, dens, ncu, knobs_of(kn, pct), consts_of(k, rate0));
    const int64_t v[8] = {g.tb, g.ntiles, g.ntiles_pad, g.ngroups, g.nseg, g.exp_ent, g.npages, g.fits ? 1 : 0};
    for (int i = 0; i < 8; i++) out[i] = v[i];
}
// out: have, need, hit_frac; returns again
int32_t sp_mj_pool_regrow(int64_t npages, int64_t exp_ent, uint64_t hits, uint64_t unplaced, double hit_frac, const int64_t *k, double rate0,
                          double *out)
{
    const MjRegrow g = mj_pool_regrow(npages, exp_ent, hits, unplaced, hit_frac, consts_of(k, rate0));
    out[0] = g.have;
    out[1] = g.need;
    out[2] = g.hit_frac;
    return g.again ? 1 : 0;
}
// out: (group, first read, end read) per unit, room for cr1 - cr0 of them; returns their number
int32_t sp_tj_units(const int32_t *group, int32_t cr0, int32_t cr1, const int64_t *k, double rate0, int32_t *out)
{
    const std::vector<Unit> u = tj_units<Unit>(group, cr0, cr1, consts_of(k, rate0));
    for (size_t i = 0; i < u.size(); i++) {
        out[3 * i] = u[i].g;
        out[3 * i + 1] = u[i].r0;
        out[3 * i + 2] = u[i].r1;
        if (u[i].zero != 0) return -1;
    }
    return (int32_t)u.size();
}
int64_t sp_tj_first_hitcap(double rate, int64_t cbases, const int64_t *kn, double pct) { return tj_first_hitcap(rate, cbases, knobs_of(kn, pct)); }
double sp_tj_learned_rate(double rate, uint64_t hits, int64_t cbases, const int64_t *k, double rate0)
{
    return tj_learned_rate(rate, hits, cbases, consts_of(k, rate0));
}
double sp_mean_hits_expected(int64_t bases, int32_t ni, int32_t kmer_mod, double dens)
{
    return mean_hits_expected(kmers_per_read(bases, ni, kmer_mod), dens);
}
double sp_mean_hits_counted(uint64_t hits, int32_t ni) { return mean_hits_counted(hits, ni); }
// out: capj, wave_tier, mid_tier, fscr_words
void sp_first_tier(int32_t kind, int32_t cap, double mean_hits, int32_t nseg, int32_t ctx_wave, int32_t ctx_mid, const int64_t *kn, double pct,
                   const int64_t *k, double rate0, int64_t *out)
{
    const FirstTier t = first_tier((SourceKind)kind, cap, mean_hits, nseg, ctx_wave != 0, ctx_mid != 0, knobs_of(kn, pct), consts_of(k, rate0));
    out[0] = t.capj;
    out[1] = t.wave_tier ? 1 : 0;
    out[2] = t.mid_tier ? 1 : 0;
    out[3] = (int64_t)t.fscr_words;
}
int64_t sp_tier_fscr_words(int32_t tier, const int64_t *k, double rate0) { return (int64_t)tier_fscr_words(tier, consts_of(k, rate0)); }
int64_t sp_fscr_total_words(int64_t per_block, int32_t ncu, const int64_t *k, double rate0)
{
    return (int64_t)fscr_total_words((size_t)per_block, ncu, consts_of(k, rate0));
}
// out: room for 4 tiers; returns their number
int32_t sp_tier_ladder(int32_t held, const int64_t *kn, double pct, int32_t *out)
{
    const std::vector<int> t = tier_ladder(held, tier_max(knobs_of(kn, pct)));
    for (size_t i = 0; i < t.size() && i < 4; i++) out[i] = t[i];
    return (int32_t)t.size();
}
// reads: n reads of the chunk at item0; nhits: per item of the chunk; fits / left: room for n each; counts: their numbers
int32_t sp_split_rung(const int32_t *reads, int32_t n, const int32_t *nhits, int64_t item0, int32_t tier, int32_t *fits, int32_t *left,
                      int32_t *counts)
{
    const std::vector<int32_t> in(reads, reads + n);
    std::vector<int32_t> f(3, 7), l(5, 9);  // (what they held is dropped)
    const int32_t gcap = split_rung(in, nhits, item0, tier, f, l);
    for (size_t i = 0; i < f.size(); i++) fits[i] = f[i];
    for (size_t i = 0; i < l.size(); i++) left[i] = l[i];
    counts[0] = (int32_t)f.size();
    counts[1] = (int32_t)l.size();
    return gcap;
}
// big: room for ni / 2 reads; returns their number, *gcap the largest hit count
int32_t sp_list_overflowed(const int32_t *ncand, const int32_t *nhits, int32_t ni, int64_t item0, int32_t *big, int32_t *gcap)
{
    std::vector<int32_t> b;
    *gcap = list_overflowed(ncand, nhits, ni, item0, b);
    for (size_t i = 0; i < b.size(); i++) big[i] = b[i];
    return (int32_t)b.size();
}
int32_t sp_quarter_overflowed(int64_t nbig, int32_t ni) { return quarter_overflowed((size_t)nbig, ni); }
int64_t sp_redo_all_above(int32_t ni, int32_t cap, const int64_t *kn, double pct) { return (int64_t)redo_all_above(ni, cap, knobs_of(kn, pct)); }
int32_t sp_cap_doubles(int32_t kind, int64_t nbig, int64_t redo_all, int32_t cap)
{
    return cap_doubles((SourceKind)kind, (size_t)nbig, (size_t)redo_all, cap);
}
// out: pow2, slab_words, per_launch; returns refused
int32_t sp_hbm_pass(int32_t gcap, int64_t *out)
{
    const HbmPass p = hbm_pass(gcap);
    out[0] = p.pow2;
    out[1] = (int64_t)p.slab_words;
    out[2] = (int64_t)p.per_launch;
    return p.refused ? 1 : 0;
}
}
