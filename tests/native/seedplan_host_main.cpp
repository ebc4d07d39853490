// Stand-alone driver of tests/native/seedplan_host.cpp for a build under the host sanitizers (a program of its own: nothing
// is preloaded): a seeded sweep of random arguments through every function of the seed plan, under random switches, and a
// few of the anchors of tests/test_seed_plan.py.
#include <stdint.h>
#include <stdio.h>

#include <vector>

extern "C" {
double sp_chance_density(int64_t ix_n, int32_t kmer_mod, int32_t k, int32_t ngroups);
int32_t sp_first_cap(int32_t max_len, int32_t kmer_mod, double dens, int32_t self, int32_t joined, const uint32_t *jhist, int32_t nreads,
                     const int64_t *kn, double pct);
int64_t sp_mj_min_bases(const int64_t *kn, double pct);
int32_t sp_mj_chunk_size_ok(int64_t bases, int64_t min_bases);
int64_t sp_tj_cap_entries(const int64_t *kn, double pct, const int64_t *k, double rate0);
void sp_mj_geometry(int64_t bases, int32_t max_len, int32_t kmer_mod, double hit_frac, double dens, int32_t ncu, const int64_t *kn, double pct,
                    const int64_t *k, double rate0, int64_t *out);
int32_t sp_mj_pool_regrow(int64_t npages, int64_t exp_ent, uint64_t hits, uint64_t unplaced, double hit_frac, const int64_t *k, double rate0,
                          double *out);
int32_t sp_tj_units(const int32_t *group, int32_t cr0, int32_t cr1, const int64_t *k, double rate0, int32_t *out);
int64_t sp_tj_first_hitcap(double rate, int64_t cbases, const int64_t *kn, double pct);
double sp_tj_learned_rate(double rate, uint64_t hits, int64_t cbases, const int64_t *k, double rate0);
double sp_mean_hits_expected(int64_t bases, int32_t ni, int32_t kmer_mod, double dens);
double sp_mean_hits_counted(uint64_t hits, int32_t ni);
void sp_first_tier(int32_t kind, int32_t cap, double mean_hits, int32_t nseg, int32_t ctx_wave, int32_t ctx_mid, const int64_t *kn, double pct,
                   const int64_t *k, double rate0, int64_t *out);
int64_t sp_tier_fscr_words(int32_t tier, const int64_t *k, double rate0);
int64_t sp_fscr_total_words(int64_t per_block, int32_t ncu, const int64_t *k, double rate0);
int32_t sp_tier_ladder(int32_t held, const int64_t *kn, double pct, int32_t *out);
int32_t sp_split_rung(const int32_t *reads, int32_t n, const int32_t *nhits, int64_t item0, int32_t tier, int32_t *fits, int32_t *left,
                      int32_t *counts);
int32_t sp_list_overflowed(const int32_t *ncand, const int32_t *nhits, int32_t ni, int64_t item0, int32_t *big, int32_t *gcap);
int32_t sp_quarter_overflowed(int64_t nbig, int32_t ni);
int64_t sp_redo_all_above(int32_t ni, int32_t cap, const int64_t *kn, double pct);
int32_t sp_cap_doubles(int32_t kind, int64_t nbig, int64_t redo_all, int32_t cap);
int32_t sp_hbm_pass(int32_t gcap, int64_t *out);
}

namespace {
struct Rng {
    uint64_t s;
    uint64_t next()
    {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return s >> 17;
    }
    int64_t below(int64_t n) { return (int64_t)(next() % (uint64_t)n); }
    double unit() { return (double)below(1 << 30) / (double)(1 << 30); }
};
int bad = 0;
void expect(bool ok, const char *what)
{
    if (!ok) {
        printf("FAILED: %s\n", what);
        bad++;
    }
}
}  // namespace

int main()
{
    // the constants as dh_mjoin.h, dh_tjoin.h and dh_device.h have them
    const int64_t K[13] = {1024, 8192, 512, 17, 16, 64, 16384, 1024, 8192, 16, 6144, 24576, 4};
    const double rate0 = 0.14;
    const int64_t none[16] = {0};
    int64_t out[8];
    int32_t tiers[4];
    sp_first_tier(2, 4096, 140.0, 1, 1, 1, none, 0, K, rate0, out);
    expect(out[0] == 512 && out[1] == 1 && out[2] == 0 && out[3] == 0, "140 hits per read: the wavefront tier");
    sp_first_tier(2, 4096, 925.0, 257, 1, 1, none, 0, K, rate0, out);
    expect(out[0] == 2048 && out[1] == 0 && out[2] == 0, "925 hits per read over 257 segments: no middle tier");
    expect(sp_tier_ladder(0, none, 0, tiers) == 3 && tiers[0] == 2048 && tiers[1] == 8192 && tiers[2] == 16384, "ladder behind the middle tier");
    expect(sp_tier_ladder(16384, none, 0, tiers) == 0, "no ladder above 16384");
    expect(sp_hbm_pass(1 << 22, out) == 0 && out[0] == (1 << 22) && sp_hbm_pass((1 << 22) + 1, out) == 1, "4M hits pass, one more is refused");
    sp_mj_geometry(8193, 511 * 131072 + 1, 1, 0.2, 0.0, 256, none, 0, K, rate0, out);
    expect(out[0] == 8192 && out[1] == 2 && out[4] == 513 && out[7] == 0, "tb + 1 bases are two tiles; 513 segments do not fit");

    Rng rng{20261020};
    double sum = 0;
    for (int i = 0; i < 20000; i++) {
        int64_t kn[16];
        for (int j = 0; j < 16; j++) kn[j] = rng.below(3) == 0;
        const int64_t values[] = {-1, 0, 1, 100, 4096, 8192, 1ll << 20, 1ll << 30, 1ll << 31, 1ll << 33};
        kn[1] = 1024 << rng.below(5);
        for (int j : {7, 9, 13, 15}) kn[j] = values[rng.below(10)];
        const double pct = (double)rng.below(101);
        const int32_t kmer_mod = (int32_t)rng.below(66) - 1, ni = (int32_t)rng.below(1 << 20) + 1, cap = 1024 << rng.below(5);
        const int32_t max_len = (int32_t)rng.below(1 << 24) + 1, nreads = (int32_t)rng.below(1 << 20), ncu = (int32_t)rng.below(304) + 1;
        const double dens = sp_chance_density(rng.below(1 << 28) + 1, kmer_mod, 8 + (int32_t)rng.below(21), (int32_t)rng.below(5000));
        const uint32_t jhist[4] = {(uint32_t)rng.below(nreads + 1), (uint32_t)rng.below(nreads + 1), (uint32_t)rng.below(nreads + 1), 0};
        sum += sp_first_cap(max_len, kmer_mod, dens, (int32_t)rng.below(2), (int32_t)rng.below(2), jhist, nreads, kn, pct);
        sum += (double)sp_mj_min_bases(kn, pct) + (double)sp_tj_cap_entries(kn, pct, K, rate0);
        const int64_t bases = rng.below(2) ? rng.below(1ll << 40) + 1 : rng.below(1 << 20) + 1;
        sum += sp_mj_chunk_size_ok(bases, sp_mj_min_bases(kn, pct));
        const double hit_frac = 0.2 + 63.8 * rng.unit();
        sp_mj_geometry(bases, max_len, kmer_mod, hit_frac, dens, ncu, kn, pct, K, rate0, out);
        double d3[3];
        const uint64_t hits = (uint64_t)rng.below(1ll << 36), unplaced = (uint64_t)rng.below(1ll << 30);
        sum += sp_mj_pool_regrow(out[6], out[5], hits, unplaced, hit_frac, K, rate0, d3) + d3[2];
        const int32_t nr = (int32_t)rng.below(80);
        std::vector<int32_t> group((size_t)nr), units(3 * (size_t)nr + 3);
        for (int32_t j = 0, g = 0; j < nr; j++) group[(size_t)j] = g += rng.below(7) == 0;
        const int32_t cr0 = (int32_t)rng.below(nr + 1), cr1 = cr0 + (int32_t)rng.below(nr - cr0 + 1);
        const int32_t nu = sp_tj_units(group.data(), cr0, cr1, K, rate0, units.data());
        expect(nu >= 0 && nu <= cr1 - cr0 && (cr1 == cr0 || (nu > 0 && units[1] == cr0 && units[3 * (size_t)nu - 1] == cr1)), "units cover the chunk");
        const int64_t cbases = rng.below(3) ? rng.below(1ll << 36) : 0;
        sum += (double)sp_tj_first_hitcap(2.0 * rng.unit(), cbases, kn, pct) + sp_tj_learned_rate(rng.unit(), hits, cbases, K, rate0);
        const double mean = rng.below(2) ? sp_mean_hits_expected(bases, ni, kmer_mod, dens) : sp_mean_hits_counted(hits >> 16, ni);
        sp_first_tier((int32_t)rng.below(4), cap, mean, (int32_t)rng.below(514), (int32_t)rng.below(2), (int32_t)rng.below(2), kn, pct, K, rate0, out);
        sum += (double)sp_fscr_total_words(out[3], ncu, K, rate0) + (double)sp_tier_fscr_words((int32_t)out[0], K, rate0);
        const int32_t nt = sp_tier_ladder((int32_t)out[0], kn, pct, tiers);
        expect(nt >= 0 && nt <= 3, "at most three list tiers");
        const int32_t nit = (int32_t)rng.below(40);
        const int64_t item0 = 2 * rng.below(1 << 30);
        std::vector<int32_t> ncand((size_t)nit + 1), nhits((size_t)nit + 1), big((size_t)nit / 2 + 1), fits(big.size()), left(big.size());
        for (int32_t j = 0; j < nit; j++) {
            ncand[(size_t)j] = (int32_t)rng.below(3) - 2;
            nhits[(size_t)j] = (int32_t)rng.below(1 << 21);
        }
        int32_t gcap = 0, counts[2];
        const int32_t nbig = sp_list_overflowed(ncand.data(), nhits.data(), nit, item0, big.data(), &gcap);
        const int32_t gcap2 = sp_split_rung(big.data(), nbig, nhits.data(), item0, nt > 0 ? tiers[0] : 2048, fits.data(), left.data(), counts);
        expect(counts[0] + counts[1] == nbig && gcap2 <= gcap, "a rung splits the list");
        sum += sp_quarter_overflowed(nbig, ni);
        const int64_t redo_all = sp_redo_all_above(ni, cap, kn, pct);
        sum += sp_cap_doubles((int32_t)rng.below(4), nbig, redo_all, cap);
        sum += sp_hbm_pass(rng.below(2) ? gcap : (int32_t)rng.below(1 << 23), out) ? 0.0 : (double)out[2];
    }
    printf("checksum %.17g\n%s\n", sum, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
