// dh_seed_plan.h -- every decision of the seed stage of an alignment call (plan_seeds, plan_mj_chunk, seed_chunk in
// dh_align_seed.cpp) as functions of numbers: no HIP, no dh_ctx, no environment.  The development switches arrive as a
// SeedKnobs, the constants of the kernel headers (dh_mjoin.h, dh_tjoin.h, dh_device.h and dh_internal.h need HIP) as a
// SeedConsts, so that tests/native/seedplan_host.cpp compiles this file with plain g++ and tests/test_seed_plan.py checks
// it against a restatement in Python.  The comments that justify a constant with a measurement stand with the constant.
#ifndef DH_SEED_PLAN_H
#define DH_SEED_PLAN_H
#include <cstddef>
#include <cstdint>

#include <algorithm>
#include <cmath>
#include <vector>

#pragma GCC visibility push(hidden) /* (a copy the compiler does not inline is no export of the library) */
namespace seedplan {

// the development switches of the seed stage (read_seed_knobs, dh_align_seed.cpp: once per align_range call)
struct SeedKnobs {
    bool has_seed_cap = false;      // DH_SEED_CAP: the first LDS capacity, 1024 .. 16384, power of two
    int seed_cap = 0;
    bool no16k = false;             // DH_SEED_NO16K: without the 16384-entry tier
    bool no_wave_tier = false;      // DH_SEED_NO_WAVE_TIER: from 2048 as before
    bool no_mid_tier = false;       // DH_SEED_NO_MID_TIER: the 512-thread block as before
    bool has_big_pct = false;       // DH_SEED_BIG_PCT: per cent of the reads above which the whole chunk runs again
    double big_pct = 0;
    bool has_mjoin_min = false;     // DH_MJOIN_MIN: bases of a chunk from which the mapping join is used
    int64_t mjoin_min = 0;
    bool has_mjoin_pages = false;   // DH_MJOIN_PAGES: pages of the hit pool (tests: force the fall-back)
    int64_t mjoin_pages = 0;
    bool no_mjoin = false;          // DH_NO_MJOIN
    bool no_tjoin = false;          // DH_NO_TJOIN
    bool has_tjoin_cap = false;     // DH_TJOIN_CAP: entries per group the table is planned for (tests: the fall-back)
    int64_t tjoin_cap = 0;
    bool has_tjoin_hitcap = false;  // DH_TJOIN_HITCAP: the first hit buffer (tests: force the rerun)
    int64_t tjoin_hitcap = 0;
};

// the constants of the kernel headers the plan needs (seed_consts, dh_align_seed.cpp)
struct SeedConsts {
    int64_t mj_p, mj_cap, mj_threads, mj_posbits, mj_group, mj_batch, mj_page, mj_probe_threads;  // dh_mjoin.h
    int64_t tj_cap, tj_run;                                                                         // dh_tjoin.h
    double tj_hit_rate0;                                                                            // dh_internal.h
    int64_t fscr_words, fscr_words16, fscr_blocks_per_cu;                                           // dh_device.h
};

// where the hits of a chunk come from
enum SourceKind { SRC_DIRECTORY = 0, SRC_PILEUP_JOIN = 1, SRC_MAPPING_JOIN = 2, SRC_TABLE_JOIN = 3 };

// ---- the call

// chance matches of a sampled k-mer per strand
// (ix_n = indexed k-mers; a sampled k-mer of B meets ix_n / (4^k / kmer_mod) of them by chance)
inline double chance_density(int64_t ix_n, int kmer_mod, int k, int ngroups)
{
    return (double)ix_n * std::max(1, kmer_mod) / std::pow(4.0, k) / std::max(1, ngroups);
}

// the LDS hit capacity the call starts with (self: A == B; joined: the pile-up join has counted its hits -- jhist: reads
// with more than 2048 / 4096 / 8192 hits -- for nreads reads)
inline int first_cap(int32_t max_len, int kmer_mod, double dens, bool self, bool joined, const unsigned int *jhist, int32_t nreads,
                     const SeedKnobs &kn)
{
    // expected hits per read (both strands share the LDS buffer): random matches + true seeds (measured
    // 0.075 per sampled k-mer for 15 % error reads at k = 20; reads that need more are redone with their
    // hits in HBM, and a chunk with many of them restarts with the next capacity); pick the LDS hit capacity
    const double exp_hits = (double)max_len / std::max(1, kmer_mod) * (2.0 * dens + 0.1);
    int cap = 1024;
    while (cap < 16384 && exp_hits * 1.5 >= cap) cap *= 2;
    if (self) {
        // all-vs-all inside pile-ups: a read shares k-mers with every other read of its group; measured
        // ~0.5 hits per base, and the 2048-entry variant (8 blocks per CU) with a few items redone from
        // HBM beats the 8192-entry one by 40 %
        cap = 1024;
        while (cap < 8192 && 0.6 * max_len > cap) cap *= 2;
    }
    if (joined) {
        // the hits are counted already (a whole second pass with the next size cost 9.5 ms at configs[2] when the guess
        // was one size short)
        // (tiers: reads above the first capacity are redone by the 8192-entry variant, reads above that from HBM -- so
        // the first tier is the smallest one that serves at least 70 % of the reads)
        const unsigned int tol = (unsigned int)(0.3 * nreads);
        cap = jhist[0] <= tol ? 2048 : (jhist[1] <= tol ? 4096 : (jhist[2] <= tol ? 8192 : 16384));
    }
    if (kn.has_seed_cap) cap = kn.seed_cap;  // development: 1024 .. 16384, power of two
    return cap;
}

// Small chunks keep the directory path (the join's fixed costs: 1 024 partitions, a page per wavefront); DH_MJOIN_MIN
// sets the threshold (bases of a chunk)
inline int64_t mj_min_bases(const SeedKnobs &kn) { return kn.has_mjoin_min ? kn.mjoin_min : 64ll << 20; }
inline bool mj_chunk_size_ok(int64_t bases, int64_t min_bases) { return bases >= min_bases && bases < (1ll << 40); }

// entries of a group of A the table join takes (DH_TJOIN_CAP lowers it)
inline int64_t tj_cap_entries(const SeedKnobs &kn, const SeedConsts &k)
{
    return kn.has_tjoin_cap ? std::max<int64_t>(0, std::min<int64_t>(k.tj_cap, kn.tjoin_cap)) : k.tj_cap;
}

// ---- the mapping join of a chunk: tile and page geometry (bases: of the chunk; max_len: longest read of B)
struct MjGeom {
    int64_t tb, ntiles, ntiles_pad, ngroups, nseg, exp_ent, npages;
    bool fits;  // false: a limit of the join is exceeded, the chunk goes by the directory
};
inline MjGeom mj_geometry(int64_t bases, int32_t max_len, int kmer_mod, double hit_frac, double dens, int ncu, const SeedKnobs &kn,
                          const SeedConsts &k)
{
    MjGeom g;
    kmer_mod = std::max(1, kmer_mod);
    // bases per tile: 13/16 of the tile's capacity expected (modimer sampling is a hash), every
    // lane of the block rolls the same number of positions, positions fit MJ_POSBITS
    // (a wavefront stages its eighth of the tile's entries in its own 1 024 slots: 832 expected, 7 sigma of slack)
    int64_t tb = (int64_t)(k.mj_cap / 16 * 13) * kmer_mod;
    if (kmer_mod == 1) tb = k.mj_cap;
    tb = std::min<int64_t>(tb, (1ll << k.mj_posbits) - 64);
    tb = std::max<int64_t>(k.mj_threads * 8, tb / (k.mj_threads * 8) * (k.mj_threads * 8));
    g.tb = tb;
    g.ntiles = (bases + tb - 1) / tb;
    g.ntiles_pad = (g.ntiles + k.mj_batch - 1) / k.mj_batch * k.mj_batch;
    g.ngroups = g.ntiles_pad / k.mj_group;
    const int64_t tbg = tb * k.mj_group;
    g.nseg = (max_len + tbg - 1) / tbg + 1;
    // hit pool: 20 % of the sampled k-mers hit (measured 6 % at 13 % error and k = 20; raised when a pool ran out: low-error
    // reads) plus the chance matches, a page per wavefront
    // of the probe kernel on top; the same number of hits regrouped by read
    // (dens: chance matches of a sampled k-mer per strand, as for the LDS capacity above)
    g.exp_ent = bases / kmer_mod;
    // (a page is left when less than a quarter of it is free: a third more pages than hits)
    // (the pool holds the SURVIVORS of the filter: the hits' k-mers and a few per cent of the others)
    g.npages = (int64_t)(1.34 * (hit_frac + 0.06 + 2.5 * dens) * (double)g.exp_ent) / k.mj_page + (int64_t)ncu * (k.mj_probe_threads / 64) + 64;
    if (kn.has_mjoin_pages) g.npages = std::max<int64_t>(1, kn.mjoin_pages);  // development / tests: force the fall-back
    g.fits = !(g.ntiles >= (1ll << 30) / k.mj_p || g.npages >= (1ll << 31) / 2 || g.nseg > 512);
    return g;
}

// the hit pool ran out (more hits per k-mer than planned: low-error reads, short k-mers): sized by the pages
// the probe kernel asked for, the chunk runs through the join again -- and the later ones start with that rate
// (hits: counted for rhits; unplaced: survivors that found no page).  again == false: the rate is past what a pool can
// be planned for, the chunk goes by the directory.
struct MjRegrow {
    double have, need, hit_frac;
    bool again;
};
inline MjRegrow mj_pool_regrow(int64_t npages, int64_t exp_ent, unsigned long long hits, unsigned long long unplaced, double hit_frac,
                               const SeedConsts &k)
{
    MjRegrow g;
    g.have = (double)npages * k.mj_page / 1.34;
    g.need = 1.2 * std::max(g.have + (double)unplaced, (double)hits) / std::max<double>(1.0, (double)exp_ent);
    g.hit_frac = std::max(hit_frac * 1.5, g.need);
    g.again = g.hit_frac <= 64.0;
    return g;
}

// ---- the table join of a chunk: units (group, run of at most TJ_RUN consecutive reads of that group) of the reads
// [cr0, cr1); Unit is a {group, first read, end read, 0} aggregate (int4 on the device side)
template <class Unit>
inline std::vector<Unit> tj_units(const int32_t *group, int32_t cr0, int32_t cr1, const SeedConsts &k)
{
    std::vector<Unit> units;
    for (int32_t rd = cr0; rd < cr1;) {
        const int32_t g = group[(size_t)rd];
        int32_t e = rd + 1;
        while (e < cr1 && e - rd < k.tj_run && group[(size_t)e] == g) e++;
        units.push_back(Unit{g, rd, e, 0});
        rd = e;
    }
    return units;
}
// first attempt: the hits per base the context has seen (plus a quarter), exact from the cursor after that
inline int64_t tj_first_hitcap(double hit_rate, int64_t cbases, const SeedKnobs &kn)
{
    if (kn.has_tjoin_hitcap) return std::max<int64_t>(1, kn.tjoin_hitcap);  // development / tests: force the rerun
    return (int64_t)(1.25 * hit_rate * (double)cbases) + 4096;
}
// the next first attempt goes by what this call produced, never below the starting figure: one low-error call
// (0.87 hits per base at 1 %) does not make every later buffer of the context six times larger at 8 bytes per
// hit -- a call after it that needs more than it left pays one rerun
inline double tj_learned_rate(double hit_rate, unsigned long long hits, int64_t cbases, const SeedConsts &k)
{
    return cbases > 0 ? std::max(k.tj_hit_rate0, (double)hits / (double)cbases) : hit_rate;
}

// ---- the first tier of a chunk

// The first tier of a mapping chunk goes by the MEAN hits per read -- 0.075 true seeds per sampled k-mer at 13 % error
// plus the random matches -- with half as much again of room (first_cap goes by the longest read of the DB: right for
// the directory path, whose overflowing reads are staged in HBM, two sizes too large here, where the next tiers take
// them from a list: the unsampled mapping of configs[2] ran all reads through the 4096-entry variant for 1 100 hits per
// read).
inline double kmers_per_read(int64_t bases, int32_t ni, int kmer_mod)
{
    return (double)bases / std::max(1, ni / 2) / std::max(1, kmer_mod);
}
inline double mean_hits_expected(double kmers, double dens) { return kmers * (2.0 * dens + 0.075); }
// (the table join has counted its hits: the mean is known)
inline double mean_hits_counted(unsigned long long hits, int32_t ni) { return (double)hits / std::max(1, ni / 2); }

// (the back end fed from segments exists with 2048, 4096 and 8192 entries of LDS; the 8192-entry one scans in a slab)
inline int tier_max(const SeedKnobs &kn) { return kn.no16k ? 8192 : 16384; }  // development / tests: without the 16384-entry tier

// capj: the capacity the first launch of a join path runs with (512: the wavefront-per-read tier); fscr_words: 8-byte
// words of slab scratch per resident block the launch gets (0: none, a null pointer)
struct FirstTier {
    int capj;
    bool wave_tier, mid_tier;
    size_t fscr_words;
};
// cap: the call's LDS capacity (first_cap, doubled since); nseg: segments per read of the mapping join;
// ctx_wave / ctx_mid: the context still uses the wavefront-per-read / the middle tier
inline FirstTier first_tier(SourceKind kind, int cap, double mean_hits, int nseg, bool ctx_wave, bool ctx_mid, const SeedKnobs &kn,
                            const SeedConsts &k)
{
    const bool listed = kind == SRC_MAPPING_JOIN || kind == SRC_TABLE_JOIN;  // the mean decides, not the longest read
    const int tmax = tier_max(kn);
    FirstTier t;
    // (a mapping chunk through the partitioned join starts with the wavefront-per-read tier: 512 hits, 32 candidate band
    // pairs -- 140 hits per read at 1/8 sampling; a block of 512 threads per read kept 3 reads per CU in flight and spent
    // its time in barriers -- then 2048, 8192, 16384 for what overflows; DH_SEED_NO_WAVE_TIER=1: from 2048 as before)
    // The wavefront-per-read tier is switched off for the context once a quarter of a chunk's reads overflowed it.
    t.wave_tier = listed && ctx_wave && 1.5 * mean_hits <= 512.0 && !kn.no_wave_tier;
    t.capj = std::min(std::max(cap, 2048), tmax);
    if (listed) {
        t.capj = 2048;
        while (t.capj < tmax && 1.5 * mean_hits > t.capj) t.capj *= 2;
        if (t.wave_tier) t.capj = 512;
    }
    // (an unsampled mapping -- 925 hits per 15 kb read, 1.5 x the mean above 512 -- takes the middle tier: 2048 hits, four
    // wavefronts per read and 64 candidate band pairs, five blocks per CU where the 512-thread block keeps three.  A read
    // with more hits or more band pairs is marked like an overflow of the wavefront tier and redone from the list by the
    // 512-thread tiers; the context stops using the tier once a quarter of a chunk's reads were.  A block gathers one
    // segment per thread.  DH_SEED_NO_MID_TIER=1: the 512-thread block as before)
    t.mid_tier = listed && !t.wave_tier && t.capj == 2048 && ctx_mid && (kind != SRC_MAPPING_JOIN || nseg <= 256) && !kn.no_mid_tier;
    // slab scratch: the directory path's kernel takes it for 4096 < cap <= 8192 only (its 16384-entry variant none); a join
    // path's by capj, and below 4096 entries -- where the kernel does not look at it -- what the call's cap would get
    t.fscr_words = cap > 4096 && cap <= 8192 ? (size_t)k.fscr_words : 0;
    if (kind != SRC_DIRECTORY && t.capj > 4096) t.fscr_words = (size_t)(t.capj > 8192 ? k.fscr_words16 : k.fscr_words);
    return t;
}
// slab scratch of a list tier of the join path
inline size_t tier_fscr_words(int tier, const SeedConsts &k) { return (size_t)(tier > 8192 ? k.fscr_words16 : k.fscr_words); }
// the slot's size: one slab per resident block
inline size_t fscr_total_words(size_t per_block, int ncu, const SeedConsts &k) { return (size_t)ncu * k.fscr_blocks_per_cu * per_block; }

// ---- the reads that overflowed the first tier

// a read overflows with both of its strands (ncand == -1 on its forward item): the reads of the chunk's items
// [item0, item0 + ni) that did, and the largest number of hits among them
inline int32_t list_overflowed(const int32_t *ncand, const int32_t *nhits, int32_t ni, int64_t item0, std::vector<int32_t> &big)
{
    int32_t gcap = 0;
    for (int32_t it = 0; it + 1 < ni; it += 2)
        if (ncand[(size_t)it] == -1) {
            big.push_back((int32_t)((item0 + it) >> 1));
            gcap = std::max(gcap, nhits[(size_t)it] + nhits[(size_t)it + 1]);
        }
    return gcap;
}
// a quarter of the chunk's reads overflowed a tier: the context stops using it
inline bool quarter_overflowed(size_t nbig, int32_t ni) { return nbig * 4 > (size_t)(ni / 2); }
// many items overflow the LDS buffer: the next size is cheaper than HBM staging -- up to 8192; the 16384-entry
// variant keeps one block per CU resident and pays off only when most items need it
inline size_t redo_all_above(int32_t ni, int cap, const SeedKnobs &kn)
{
    size_t redo_all = (size_t)ni / 50 + 8;
    if (cap >= 8192) redo_all = (size_t)ni / 4;
    if (kn.has_big_pct) redo_all = (size_t)((double)ni * kn.big_pct / 200.0);  // development (reads = ni / 2)
    return redo_all;
}
// the directory path doubles its cap and runs the chunk again
inline bool cap_doubles(SourceKind kind, size_t nbig, size_t redo_all, int cap)
{
    return kind == SRC_DIRECTORY && nbig > redo_all && cap < 16384;
}

// further tiers of the join path: the reads above the first capacity that fit the 8192-entry variant, then the
// 16384-entry one (uncapped pile-ups: ~10 000 hits per read); what is left is staged in HBM.
// held: what the first tier held -- 0 behind the middle tier (its reads with too many band pairs have at most 2048 hits:
// the tiers start at 2048 again)
inline std::vector<int> tier_ladder(int held, int tmax)
{
    std::vector<int> tiers;
    for (int tier = held < 2048 ? 2048 : 8192; tier <= tmax; tier = tier < 8192 ? 8192 : tier * 2)
        if (tier > held) tiers.push_back(tier);
    return tiers;
}
// one rung: the reads of `reads` whose hits fit `tier`, the others, and the largest count among those
inline int32_t split_rung(const std::vector<int32_t> &reads, const int32_t *nhits, int64_t item0, int tier, std::vector<int32_t> &fits,
                          std::vector<int32_t> &left)
{
    int32_t gcap = 0;
    fits.clear();
    left.clear();
    for (int32_t rd : reads) {
        const size_t it = (size_t)(2 * (int64_t)rd - item0);
        const int32_t nh = nhits[it] + nhits[it + 1];
        if (nh <= tier)
            fits.push_back(rd);
        else {
            left.push_back(rd);
            gcap = std::max(gcap, nh);
        }
    }
    return gcap;
}

// ---- the HBM-staged pass: gcap = the largest hit count of a read in it
struct HbmPass {
    bool refused;  // more than 4M hits for one sequence
    int32_t pow2;
    size_t slab_words, per_launch;
};
inline HbmPass hbm_pass(int32_t gcap)
{
    HbmPass p = {gcap > (1 << 22), 1, 0, 0};
    if (p.refused) return p;
    while (p.pow2 < gcap) p.pow2 <<= 1;  // the bitonic sort pads to a power of two
    // per block: pow2 hits, pow2 64-bit prefix sums, pow2 32-bit band-head positions (k_seed<0>)
    p.slab_words = 2 * (size_t)p.pow2 + ((size_t)p.pow2 + 1) / 2;
    p.per_launch = std::max<size_t>(1, (size_t)(2ull << 30) / (p.slab_words * 8));  // launches of at most 2 GB
    return p;
}

}  // namespace seedplan
#pragma GCC visibility pop
#endif
