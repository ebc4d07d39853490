// dh_seed.hip -- the seed filter (K4) for gfx950 (CDNA4, wave64).
//
// k_seed<LCAP, JOIN, NT, CC>  persistent blocks, one read (both strands) at a time (seed_item):
//     fill        the hit buffer, either by k-mer lookups in the fat directory of A or (JOIN) gathered from the hit
//                 segments of a k-mer join (dh_join.hip, dh_mjoin.hip)
//     sort        by (strand, diagonal, position): ranks by a wavefront, ranks with one hit per thread, diagonal buckets
//                 with a second counting pass for heavy buckets, or the bitonic network
//     band pairs  coverage of neighbouring diagonal bands, local maxima become candidates with a seed
//     rank, write candidates ranked per strand, the best max_cand written
//   LCAP > 0: hits staged in LDS; LCAP == 0: in a slab of HBM (reads that overflowed every LDS tier).
//   Segment-fed tiers below the 512-thread blocks: <512, 64, 32> a wavefront per read (sampled mapping), <2048, 256, 64>
//   four wavefronts per read with a slim LDS layout (unsampled mapping).
// k_seed_summary  per-chunk sums of the per-item results
// dhk_seed, dhk_seed_big, dhk_seed_join, dhk_seed_big_join: tier tables over launch_seed
//
// The arithmetic specification is written down in DESIGN.md ("Algorithm DH-1").
#include <hip/hip_runtime.h>
#include <type_traits>
#include <algorithm>
#include <cstdlib>
#include <stdio.h>
#include <stdint.h>
#include <stdlib.h>

#include "dh_device.h"
#include "dh_join.h"

#define LANES 64

#include "dh_kmer.h"

// ------------------------------------------------------------------------------------ K4

// development / tests: 0 = reads with a bucket above SORT_BMAX hits take the bitonic network as before round 6
// (DH_SEED_NO_REFINE=1; the order is the same either way)
__device__ int g_seed_sort_refine = 1;
// development / tests: 1 = the band phase of the segment-fed 8192- and 16384-entry tiers keeps the per-hit sums and the band
// heads of every read in its slab of global scratch, as before the head table (DH_SEED_SLAB_BANDS=1; same candidates)
__device__ int g_seed_slab_bands = 0;
// reads of those two tiers whose band heads went to the table in LDS [0] and to the slab [1] (dh_get_seed_band_counts); a
// block counts in LDS and adds its counts when it ends
__device__ unsigned long long g_seed_band_reads[2];
__device__ __forceinline__ uint32_t *seed_band_lds()
{
    __shared__ uint32_t s_band_reads[2];
    return s_band_reads;
}
#define HIT_QBITS 24
#define HIT_QMASK ((1u << HIT_QBITS) - 1u)
#define SEED_THREADS 512
#define SEED_LOOKUP_THREADS 512 /* threads that roll k-mers (whole wavefronts; fewer = longer serial chains = slower) */
#define SEED_CCAP 256 /* candidate band pairs collected per (read, strand) before ranking */

__device__ __forceinline__ int64_t hitD(uint64_t h) { return (int64_t)(h >> HIT_QBITS); }
__device__ __forceinline__ int32_t hitQ(uint64_t h) { return (int32_t)(h & HIT_QMASK); }

// covered-base contribution of sorted hit i (needs hit i-1)
__device__ __forceinline__ int32_t hit_cov(const uint64_t *h, int32_t i, int32_t k)
{
    if (i > 0 && hitD(h[i - 1]) == hitD(h[i])) {
        const int32_t dq = hitQ(h[i]) - hitQ(h[i - 1]);
        return dq < k ? dq : k;
    }
    return k;
}

// LCAP > 0: hits are staged in LDS (LCAP entries); items that do not fit are marked with
// ncand = -1 and redone by the LCAP == 0 instantiation, whose hit buffer is a slab of HBM
// (gcap entries per block, items taken from item_list) -- same code, same results.
#ifdef DH_SEED_PROF
// (a row per tier class: the segment- or directory-fed 8192-entry tier [1], the 16384-entry tier [2], every other tier [0])
__device__ unsigned long long g_seed_prof_all[3][12];
#define g_seed_prof g_seed_prof_all[LCAP == 8192 ? 1 : (LCAP == 16384 ? 2 : 0)]
// (a block's clocks add up in LDS and reach g_seed_prof when the persistent block ends: as ten atomics per read on one
// cache line -- 10^7 per mapping launch at ~10 ns each -- the instrumentation was what the instrumented kernel waited for)
__device__ __forceinline__ unsigned long long *seed_prof_lds()
{
    __shared__ unsigned long long s_prof[12];
    return s_prof;
}
#define SP(i) if (tid == 0) { const unsigned long long t_ = wall_clock64(); seed_prof_lds()[i] += t_ - tp_; tp_ = t_; }
#else
#define SP(i)
#endif
// One READ (both strands), processed by the whole block; `work` = index of the read in this launch,
// `slab` = index of the block's HBM hit slab (LCAP == 0).  The k-mers are rolled once over the forward
// read together with their reverse complements; the index is keyed by canonical k-mers with the
// orientation of the A k-mer in bit 63 of the key, so ONE lookup yields the hits of both strands:
// equal orientations = the forward read matches A, opposite = its reverse complement does (at
// position blen - k - q of the reverse-complemented read).  Hits carry the strand in their top bit,
// the band filter therefore never mixes strands; candidates go to the items 2r (forward) and 2r + 1.
#define HIT_DBITS 39
// JOIN: the hits come from the per-pile-up k-mer join (dh_join.hip) -- the read's segments of the hit buffer are
// gathered instead of looking its k-mers up; everything after the hit buffer is filled is the same code.
template <int LCAP, bool JOIN, int NT, int CC>
__device__ void seed_item(const DbView &B, const IndexView &ix, const JoinView &jv,
                          const DhOpts &o, int32_t read0, int32_t work, int32_t slab,
                          DhCand *__restrict__ cand_out, int32_t *__restrict__ ncand_out,
                          int32_t *__restrict__ nhits_out, int32_t *__restrict__ status,
                          uint64_t *__restrict__ gbuf, int32_t gcap, const int32_t *__restrict__ read_list)
{
    // Which sort a tier takes goes by (LCAP, NT), not by the block size alone:
    //   RANK_ALL  one wavefront whose lanes rank each of their keys against all n hits (n x LCAP / NT compares: for the 512
    //             hits of the wavefront-per-read tier only)
    //   otherwise one hit per thread (n <= NT), the diagonal buckets, or the bitonic network
    // SLIM (the middle tier: four wavefronts per read, 2 048 hits, CC = 64): the segment tables of the gather and the
    // counters of the bucket sort overlay the prefix sums and band heads of the band phase (not live before the hits are
    // sorted) instead of the candidate arrays, which therefore need not hold 8 + 4 KB: 31.5 KB of LDS per block, five
    // blocks per CU where the 512-thread block of the same capacity keeps three.
    constexpr bool RANK_ALL = LCAP > 0 && NT <= LANES && LCAP <= 8 * NT;
    constexpr bool SLIM = LCAP > 0 && LCAP <= 4096 && NT > LANES && NT < SEED_THREADS;
    constexpr bool FB_LDS = LCAP > 0 && LCAP <= 4096;  // the band phase's prefix sums and heads live in LDS
    // HTAB (the segment-fed 8192- and 16384-entry tiers, the pile-up all-vs-all's): a table of the band heads in the unused
    // tail of the read's own hit buffer where it fits, and a lane group for every long range (both below)
    constexpr bool HTAB = JOIN && NT == SEED_THREADS && (LCAP == 8192 || LCAP == 16384);
    __shared__ uint64_t lhits[LCAP > 0 ? LCAP : 1];
    __shared__ DhCand cands[2 * CC];
    __shared__ int64_t cband[2 * CC];
    __shared__ __attribute__((aligned(8))) uint32_t bsum_l[FB_LDS ? LCAP : 1];   // inclusive prefix sums
    __shared__ __attribute__((aligned(8))) uint16_t bhead_l[FB_LDS ? LCAP : 1];  // positions of the band heads
    __shared__ int32_t s_n, s_nc;

    const int32_t r = read_list ? read_list[work] : read0 + work;  // (the HBM variant always works from a list)
    const int32_t item = 2 * r;
    // HBM variant: the block's slab holds gcap hits, gcap 64-bit prefix sums and gcap 32-bit head positions
    uint64_t *hits = LCAP > 0 ? lhits : gbuf + (int64_t)slab * (2 * (int64_t)gcap + (gcap + 1) / 2);
    const int32_t CAP = LCAP > 0 ? LCAP : gcap;
    const int tid = threadIdx.x;
#ifdef DH_SEED_PROF
    unsigned long long tp_ = wall_clock64();
#endif
    if (tid == 0) {
        s_n = 0;
        s_nc = 0;
    }
    __syncthreads();
    const int64_t bo = B.off[r];
    const int32_t blen = (int32_t)(B.off[r + 1] - bo);
    const uint8_t *b = B.bases + bo;
    const uint64_t grp = B.group ? (uint64_t)B.group[r] : 0ull;
    const int k = o.k;
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const int32_t npos = blen - k + 1;
    constexpr uint64_t ORI = 1ull << 63, PAL = 1ull << 62;

    // ---- k-mer lookups: thread t rolls over a contiguous chunk of positions.  Sampled k-mers are
    // queued in registers (SEED_QN per lane); when the queue of ANY lane of the wavefront is full
    // every lane looks up what it holds: the directory words of all queued k-mers are fetched
    // back to back, then the first (key, value) entry of every non-empty bucket -- two memory
    // round trips per flush for all lanes together.  Buckets hold one entry almost always (the
    // directory has ~8 buckets per indexed k-mer); longer ones take the generic loop.
    // The phase is bound by the latency of each lane's serial chain (measured: halving the number
    // of rolling threads makes it 40 % slower), so every thread of the block takes a chunk.
    if (JOIN) {
        // the read's segments: one per slice of its group (segtab row), first hit << 24 | count.  Their prefix sums
        // and first hits overlay the candidate arrays, which are not in use yet (SLIM: the band phase's arrays).
        static_assert(SLIM || (sizeof(cands) / 2 >= NT * sizeof(uint64_t) && sizeof(cands) / 2 >= (NT + 1) * sizeof(uint32_t)),
                      "segment tables overlay the candidate array");
        static_assert(!SLIM || (sizeof(bsum_l) >= NT * sizeof(uint64_t) && sizeof(bhead_l) >= (NT + 1) * sizeof(uint32_t)),
                      "segment tables overlay the band arrays");
        uint64_t *segb = SLIM ? (uint64_t *)bsum_l : (uint64_t *)cands;                        // [NT] first hit of segment s
        uint32_t *sego = (SLIM ? (uint32_t *)bhead_l : (uint32_t *)(cands + CC)) + 1;   // [-1 .. NT) exclusive prefix sums of the counts
        __shared__ uint32_t s_jw[NT / LANES];
        const int32_t ns = jv.gns ? jv.gns[B.group[r]] : jv.ns_fixed;
        const int64_t srow = jv.gns ? jv.segrow[r] : (int64_t)(r - jv.read0) * jv.ns_fixed;
        uint32_t c = 0;
        if (tid < ns) {
            const uint64_t sg = jv.segtab[srow + tid];
            c = (uint32_t)(sg & 0xFFFFFFull);
            segb[tid] = sg >> 24;
        }
        uint32_t incl = c;
        for (int off = 1; off < LANES; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, LANES);
            if ((tid & (LANES - 1)) >= off) incl += up;
        }
        if ((tid & (LANES - 1)) == LANES - 1) s_jw[tid / LANES] = incl;
        __syncthreads();
        uint32_t base = 0, tot = 0;
        for (int wv = 0; wv < NT / LANES; wv++) {
            if (wv < tid / LANES) base += s_jw[wv];
            tot += s_jw[wv];
        }
        sego[tid] = base + incl;  // inclusive: sego[s - 1] = hits before segment s
        if (tid == 0) {
            sego[-1] = 0;
            s_n = (int32_t)tot;
        }
        __syncthreads();
        if ((int32_t)tot <= CAP) {
            // the segment of hit e: the last s with sego[s - 1] <= e (sego[-1] = 0; empty segments repeat a value and lose to
            // the one behind them).  Four hits per thread at a time, their searches a fixed number of steps without a branch:
            // the LDS round trips of the four overlap and so do the four loads from the hit buffer (one hit per iteration
            // made the gather a chain of dependent round trips: 106 of the 170 us a block spent on a pile-up read of 166)
            constexpr int GU = 4;
            int32_t top = 1;
            while (top < ns) top <<= 1;
            for (int32_t e0 = tid; e0 < (int32_t)tot; e0 += NT * GU) {
                int32_t lo[GU];
#pragma unroll
                for (int u = 0; u < GU; u++) lo[u] = 0;
                for (int32_t step = top >> 1; step > 0; step >>= 1) {
#pragma unroll
                    for (int u = 0; u < GU; u++) {
                        const int32_t idx = lo[u] + step;
                        const uint32_t e = (uint32_t)(e0 + u * NT);
                        if (idx < ns && sego[idx - 1] <= e) lo[u] = idx;
                    }
                }
                uint64_t v[GU];
#pragma unroll
                for (int u = 0; u < GU; u++) {
                    const int32_t e = e0 + u * NT;
                    v[u] = 0;
                    if (e < (int32_t)tot) v[u] = jv.hits[segb[lo[u]] + ((uint32_t)e - sego[lo[u] - 1])];
                }
#pragma unroll
                for (int u = 0; u < GU; u++) {
                    const int32_t e = e0 + u * NT;
                    if (e < (int32_t)tot) hits[e] = v[u];
                }
            }
        }
    } else if (npos > 0 && tid < SEED_LOOKUP_THREADS) {
        constexpr int QN = 4;
        const int32_t per = (npos + SEED_LOOKUP_THREADS - 1) / SEED_LOOKUP_THREADS;
        const int32_t q0 = tid * per, q1 = min(npos, q0 + per);
        const KmerSampler smp = kmer_sampler(o.kmer_mod, k);
        uint64_t km = 0, rc = 0;
        int32_t valid = 0;
        const int32_t pend = q0 < q1 ? q1 + k - 1 : q0;
        uint64_t qk[QN];
        int32_t qq[QN];
        int32_t nq = 0;
#pragma unroll
        for (int u = 0; u < QN; u++) {
            qk[u] = 0;
            qq[u] = 0;
        }
        auto emit = [&](uint64_t v, int32_t q, int32_t strand) {
            if (!(o.strands & (1 << strand))) return;
            const int32_t aseq = (int32_t)(v >> 40);
            if (o.skip_self == 1 && aseq == r) return;
            // tandem (datander): a read against itself, below the main diagonal only (position on A > position on B)
            if (o.skip_self == 3 && (aseq != r || (int64_t)(v & ((1ull << 40) - 1)) - ix.goff[r] - q < 1)) return;
            // symmetric: each unordered pair once; which read plays B alternates with the
            // parity of a + b, so every read is B for about half of its partners
            if (o.skip_self == 2 && (aseq == r || ((aseq < r) != (((aseq + r) & 1) == 0)))) return;
            if (o.skip_self == 2 && B.pflags && !dh_pair_seeded(B.pflags, aseq, r)) return;  // neither record is wanted
            const int64_t gv = (int64_t)(v & ((1ull << 40) - 1));
            const int32_t qs = strand ? blen - k - q : q;  // position on the oriented read
            const int64_t D = gv + ix.sepv - qs;
            const int32_t slot = atomicAdd(&s_n, 1);
            if (slot < CAP) hits[slot] = ((uint64_t)strand << 63) | ((uint64_t)D << HIT_QBITS) | (uint32_t)qs;
        };
        auto flush = [&]() {
            // the fat directory word of every queued k-mer: one 16-byte load, one memory round trip per flush
            ulonglong2 f[QN];
#pragma unroll
            for (int u = 0; u < QN; u++) {
                f[u].x = DH_FAT_EMPTY;
                f[u].y = 0;
                if (u < nq) f[u] = ix.fat[(uint32_t)((qk[u] & ~(ORI | PAL)) >> ix.shift)];
            }
#pragma unroll
            for (int u = 0; u < QN; u++) {
                if (f[u].x == DH_FAT_EMPTY) continue;
                const uint64_t key = qk[u] & ~(ORI | PAL);
                const uint64_t bori = qk[u] & ORI;
                const bool pal = (qk[u] & PAL) != 0;
                if ((f[u].x >> 62) != 1ull) {  // the bucket's only entry
                    if ((f[u].x & ~ORI) == key && o.tcap >= 1) {
                        const bool same = (f[u].x & ORI) == bori;
                        if (same || pal) emit(f[u].y, qq[u], 0);
                        if (!same || pal) emit(f[u].y, qq[u], 1);
                    }
                    continue;
                }
                const uint32_t ss_u = (uint32_t)f[u].y, ee_u = ss_u + (uint32_t)(f[u].y >> 32);
                // -t cap: a k-mer occurring more than tcap times (per orientation) is skipped.  A bucket with at most
                // tcap entries cannot hold such a k-mer, so only larger buckets are counted first -- the count pass costs
                // one dependent load per entry, which for an unsampled index (the pile-up stage's: every intact k-mer of
                // a pile-up shares a bucket with its ~coverage copies) was half of the lookup phase
                bool dof = true, dor = true;
                if (ee_u - ss_u > (uint32_t)max(o.tcap, 0)) {
                    int32_t runf = 0, runr = 0;
                    for (uint32_t t = ss_u; t < ee_u; t++) {
                        const uint64_t ex = ix.ent[t].x;
                        if ((ex & ~ORI) != key) continue;
                        const bool same = (ex & ORI) == bori;
                        runf += (same || pal) ? 1 : 0;
                        runr += (!same || pal) ? 1 : 0;
                    }
                    dof = runf > 0 && runf <= o.tcap;
                    dor = runr > 0 && runr <= o.tcap;
                    if (!dof && !dor) continue;
                }
                // ... then emit its hits (the next entry is on its way while this one is handled)
                ulonglong2 nx = ix.ent[ss_u];
                for (uint32_t t = ss_u; t < ee_u; t++) {
                    const ulonglong2 en = nx;
                    if (t + 1 < ee_u) nx = ix.ent[t + 1];
                    if ((en.x & ~ORI) != key) continue;
                    const bool same = (en.x & ORI) == bori;
                    if (dof && (same || pal)) emit(en.y, qq[u], 0);
                    if (dor && (!same || pal)) emit(en.y, qq[u], 1);
                }
            }
            nq = 0;
        };
        const int rcsh = 2 * (k - 1);
        // warm-up: the first k - 1 bases of the chunk only fill the rolling k-mers
        uint64_t w = 0, wnext = q0 < pend ? load8(b + q0) : 0ull;
        for (int32_t t = 0; t < k - 1; t++) {
            const int32_t pp = q0 + t;
            if ((t & 7) == 0) {
                w = wnext;
                if (pp + 8 < pend) wnext = load8(b + pp + 8);
            }
            const uint8_t c = (uint8_t)w;
            w >>= 8;
            if (pp < pend) {
                if (c < 4) {
                    km = ((km << 2) | c) & mask;
                    rc = (rc >> 2) | ((uint64_t)(3 - c) << rcsh);
                    valid++;
                } else {
                    km = 0;
                    rc = 0;
                    valid = 0;
                }
            }
        }
        // uniform trip count so that the wavefront flushes together
        for (int32_t t = k - 1; t < per + k - 1; t++) {
            const int32_t pp = q0 + t;
            if ((t & 7) == 0) {
                w = wnext;
                if (pp + 8 < pend) wnext = load8(b + pp + 8);
            }
            const uint8_t c = (uint8_t)w;
            w >>= 8;
            if (pp < pend) {
                if (c < 4) {
                    km = ((km << 2) | c) & mask;
                    rc = (rc >> 2) | ((uint64_t)(3 - c) << rcsh);
                    valid++;
                } else {
                    km = 0;
                    rc = 0;
                    valid = 0;
                }
                const uint64_t canon = km < rc ? km : rc;
                bool em = valid >= k && kmer_sampled(canon, smp);
                if (em && B.mask_bits && mask_touch(B.mask_bits, bo + pp - k + 1, k)) em = false;
                if (em) {
                    const uint64_t key = ((grp << (2 * k)) | canon) | (km != canon ? ORI : 0ull) | (km == rc ? PAL : 0ull);
                    const int32_t q = pp - k + 1;
#pragma unroll
                    for (int u = 0; u < QN; u++)
                        if (u == nq) {
                            qk[u] = key;
                            qq[u] = q;
                        }
                    nq++;
                }
            }
            if (__ballot(nq == QN) != 0ull) flush();
        }
        if (__ballot(nq > 0) != 0ull) flush();
    }
    __syncthreads();
    SP(0)
    int32_t n = s_n;
    if (n > CAP) {
        // capacity exceeded: never silently truncated.  LDS variant: hand the read to the HBM
        // variant (ncand = -1); HBM variant: report
        if (tid == 0) {
            if (LCAP == 0) atomicOr(status, DH_ST_HIT_OVERFLOW);
            ncand_out[item] = ncand_out[item + 1] = LCAP > 0 ? -1 : 0;
            nhits_out[item] = n;  // what the HBM slab has to hold (both strands)
            nhits_out[item + 1] = 0;
        }
        return;
    }
    if (n == 0) {
        if (tid == 0) ncand_out[item] = ncand_out[item + 1] = nhits_out[item] = nhits_out[item + 1] = 0;
        return;
    }
    // ---- sort of the hit buffer (keys are distinct: a hit is (strand, diagonal, read position))
    int32_t N = 1;
    while (N < n) N <<= 1;
    if (RANK_ALL) {  // a wavefront per read (the sampled mapping's first tier)
        // every thread takes the (at most LCAP / NT) keys tid, tid + NT, ... and counts the keys below each of them: n
        // broadcast reads for all of its keys together; keys are distinct, the ranks a permutation
        // (as many keys per thread as the read needs: 140 hits at 1/8 sampling are three)
        constexpr int E8 = LCAP / NT > 0 ? LCAP / NT : 1;
        uint64_t ky[E8];
        int32_t rk8[E8];
#pragma unroll
        for (int u = 0; u < E8; u++) {
            const int32_t i = tid + u * NT;
            ky[u] = i < n ? hits[i] : ~0ull;
            rk8[u] = 0;
        }
#define DH_RANK_KEYS(M_)                                                   \
    for (int32_t x = 0; x < n; x++) {                                      \
        const uint64_t h = hits[x];                                        \
        _Pragma("unroll") for (int u = 0; u < (M_ < E8 ? M_ : E8); u++) rk8[u] += h < ky[u] ? 1 : 0; \
    }
        if (n <= 2 * NT) {
            DH_RANK_KEYS(2)
        } else if (n <= 4 * NT) {
            DH_RANK_KEYS(4)
        } else {
            DH_RANK_KEYS(E8)
        }
#undef DH_RANK_KEYS
        __syncthreads();
#pragma unroll
        for (int u = 0; u < E8; u++)
            if (tid + u * NT < n) hits[rk8[u]] = ky[u];
        N = 1;  // the network below has nothing left to do
    } else if (LCAP > 0 && n <= NT) {
        // at most one hit per thread (the mapping launches: 140 hits per read at kmer_mod 8): every thread counts the
        // keys below its own -- n broadcast reads that do not depend on each other -- and stores its key at that rank.
        // The bitonic network below takes log^2 N dependent LDS round trips (36 for N = 256: 8.6 of the 50 us a block
        // spent per read)
        uint64_t key = 0;
        int32_t rk = 0;
        if (tid < n) {
            key = hits[tid];
#pragma unroll 4
            for (int32_t x = 0; x < n; x++) rk += hits[x] < key ? 1 : 0;
        }
        __syncthreads();
        if (tid < n)
            hits[rk] = key;
        else if (tid < N)
            hits[tid] = ~0ull;
        N = 1;  // the network below has nothing left to do
    } else if (LCAP == 0 || ((LCAP <= 8192 || JOIN) && (JOIN || LCAP >= 4096))) {  // (not the mapping launches' small variants: registers)
        // More than one hit per thread (the pile-up all-vs-all: 2 500 hits per read, where the network below was 55 of the
        // 97 us a block spent per read): the hits of a read cluster on the diagonals of its overlaps, so they are dealt
        // into 2 x 1024 diagonal buckets (strand, then equal slices of the read's diagonal range: a counting pass, a scan,
        // a scatter through registers) and every hit takes its rank among the few hits of its bucket.  A bucket that grew
        // beyond SORT_BMAX hits (a repeat) sends the read through the network instead -- the same order either way.
        // The HBM variant (the few reads with more hits than any LDS buffer holds) scatters into the slab's prefix-sum area
        // instead of registers; its network is a chain of global round trips per exchange (8 ms for 4 reads of a
        // configs[2] part).  Ranking costs (n / 512) x bucket loads from L2 per thread, the network ~0.5 ms at 16 384
        // hits: measured break-even at buckets of ~340 hits.
        constexpr int E = LCAP >= NT ? LCAP / NT : 1;
        constexpr int NB = 2048, NBH = NB / 2, SORT_BMAX = LCAP == 0 ? 384 : 256;
        constexpr uint64_t DM = (1ull << HIT_DBITS) - 1;
        static_assert(NB % NT == 0 && NT % LANES == 0, "every thread scans NB / NT counters, whole wavefronts");
        static_assert(RANK_ALL || SLIM || sizeof(cands) >= NB * sizeof(uint32_t), "bucket counters overlay the candidate array");
        static_assert(!SLIM || sizeof(bsum_l) >= NB * sizeof(uint32_t), "bucket counters overlay the prefix sums");
        uint32_t *bcnt = SLIM ? (uint32_t *)bsum_l : (uint32_t *)cands;  // not in use yet (the join's segment table is done with it)
        __shared__ unsigned long long s_dmin, s_dmax;
        __shared__ uint32_t s_bw[NT / LANES];
        __shared__ uint32_t s_bmax;
        // REFINE (round 6): buckets above SORT_BMAX hits are sorted by a second counting pass over their own diagonal range
        // instead of sending the whole read through the network (below).  The mapping launches need it: a read's ~900 true
        // hits at kmer_mod 1 lie on a few hundred neighbouring diagonals while its handful of chance hits stretch the
        // diagonal range over the whole assembly, so the slices are 10^5 diagonals wide and one of them holds everything --
        // 88 % of the reads of configs[2] took the network, 25.6 of the 41 us a block spent per read.
        constexpr int HV = 8, NB2 = 1024;            // heavy buckets a read may have; slices of the second pass
        constexpr bool REFINE = LCAP > 0 && !RANK_ALL;
        static_assert(!REFINE || SLIM || sizeof(cband) >= NB2 * sizeof(uint32_t), "the second pass's counters overlay the band array");
        static_assert(!SLIM || sizeof(bhead_l) >= NB2 * sizeof(uint32_t), "the second pass's counters overlay the band heads");
        static_assert(NB2 % NT == 0 && (LCAP == 0 || LCAP % NT == 0 || LCAP < NT), "NB2 / NT counters, LCAP / NT hits per thread");
        uint32_t *fcnt = SLIM ? (uint32_t *)bhead_l : (uint32_t *)cband;  // not in use yet
        __shared__ uint32_t s_nheavy, s_heavy[HV];
        for (int32_t i = tid; i < NB; i += NT) bcnt[i] = 0;
        if (tid == 0) {
            s_dmin = ~0ull;
            s_dmax = 0ull;
            s_bmax = 0;
            s_nheavy = 0;
        }
        unsigned long long dmin = ~0ull, dmax = 0ull;
        for (int32_t i = tid; i < n; i += NT) {
            const unsigned long long d = (hits[i] >> HIT_QBITS) & DM;
            dmin = d < dmin ? d : dmin;
            dmax = d > dmax ? d : dmax;
        }
        for (int off = LANES / 2; off > 0; off >>= 1) {
            const unsigned long long a = __shfl_xor(dmin, off, LANES), c = __shfl_xor(dmax, off, LANES);
            dmin = a < dmin ? a : dmin;
            dmax = c > dmax ? c : dmax;
        }
        __syncthreads();
        if ((tid & (LANES - 1)) == 0) {
            atomicMin(&s_dmin, dmin);
            atomicMax(&s_dmax, dmax);
        }
        __syncthreads();
        // (slices aligned to their width: the hits of a bucket then differ in their low 24 + sh bits only)
        uint64_t d0 = s_dmin;
        int sh = 0;
        while (((s_dmax - d0) >> sh) >= (uint64_t)NBH) {
            sh++;
            d0 = s_dmin & ~((1ull << sh) - 1);
        }
        auto bucket = [&](uint64_t key) {
            return (uint32_t)(key >> 63) * NBH + (uint32_t)((((key >> HIT_QBITS) & DM) - d0) >> sh);
        };
        for (int32_t i = tid; i < n; i += NT) atomicAdd(&bcnt[bucket(hits[i])], 1u);
        __syncthreads();
        // exclusive scan of the counters (4 per thread), largest bucket
        uint32_t c4[NB / NT], sum = 0, mx = 0;
#pragma unroll
        for (int u = 0; u < NB / NT; u++) {
            c4[u] = bcnt[tid * (NB / NT) + u];
            sum += c4[u];
            mx = c4[u] > mx ? c4[u] : mx;
        }
        uint32_t incl = sum;
        for (int off = 1; off < LANES; off <<= 1) {
            const uint32_t up = __shfl_up(incl, off, LANES);
            if ((tid & (LANES - 1)) >= off) incl += up;
        }
        for (int off = LANES / 2; off > 0; off >>= 1) {
            const uint32_t a = __shfl_xor(mx, off, LANES);
            mx = a > mx ? a : mx;
        }
        if ((tid & (LANES - 1)) == LANES - 1) s_bw[tid / LANES] = incl;
        if ((tid & (LANES - 1)) == 0) atomicMax(&s_bmax, mx);
        __syncthreads();
        uint32_t base = incl - sum;
        for (int wv = 0; wv < tid / LANES; wv++) base += s_bw[wv];
#pragma unroll
        for (int u = 0; u < NB / NT; u++) {
            bcnt[tid * (NB / NT) + u] = base;
            base += c4[u];
        }
        if (REFINE) {
#pragma unroll
            for (int u = 0; u < NB / NT; u++)
                if (c4[u] > (uint32_t)SORT_BMAX) {
                    const uint32_t slot = atomicAdd(&s_nheavy, 1u);
                    if (slot < (uint32_t)HV) s_heavy[slot] = (uint32_t)(tid * (NB / NT) + u);
                }
        }
        uint64_t ke[E];
        if (LCAP > 0) {
#pragma unroll
            for (int u = 0; u < E; u++) {
                const int32_t i = tid + u * NT;
                ke[u] = i < n ? hits[i] : 0ull;
            }
        }
        __syncthreads();
        SP(5)
        const bool refine = REFINE && g_seed_sort_refine && s_bmax > (uint32_t)SORT_BMAX && s_nheavy <= (uint32_t)HV;
        if (LCAP == 0 && s_bmax <= (uint32_t)SORT_BMAX) {
            uint64_t *tmp = hits + gcap;  // the block's prefix sums live here later
            for (int32_t i = tid; i < n; i += NT) {
                const uint64_t key = hits[i];
                tmp[atomicAdd(&bcnt[bucket(key)], 1u)] = key;
            }
            __syncthreads();
            for (int32_t i = tid; i < n; i += NT) {
                const uint64_t key = tmp[i];
                const uint32_t bk = bucket(key);
                const uint32_t b0 = bk ? bcnt[bk - 1] : 0u, b1 = bcnt[bk];
                uint32_t rk = b0, x = b0;
                for (; x + 8 <= b1; x += 8) {
                    uint64_t h[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) h[j] = tmp[x + j];
#pragma unroll
                    for (int j = 0; j < 8; j++) rk += h[j] < key ? 1u : 0u;
                }
                for (; x < b1; x++) rk += tmp[x] < key ? 1u : 0u;
                hits[rk] = key;
            }
            N = 1;
        } else if (LCAP > 0 && (s_bmax <= (uint32_t)SORT_BMAX || refine)) {
            // scatter: a bucket's hits in arrival order; the counters end up at the buckets' ends
#pragma unroll
            for (int u = 0; u < E; u++) {
                const int32_t i = tid + u * NT;
                if (i < n) hits[atomicAdd(&bcnt[bucket(ke[u])], 1u)] = ke[u];
            }
            __syncthreads();
            SP(6)
            uint32_t dst[E];
            // keys below `key` among hits[x0, x1) (keys are distinct; eight loads in flight: one at a time made every compare
            // a full LDS round trip; `low`: the keys of the range agree above their low words, which then decide -- half the
            // LDS traffic of this loop, which is bound by it)
            auto count_below = [&](uint32_t x0, uint32_t x1, uint64_t key, bool low) {
                uint32_t rk = 0, x = x0;
                if (low) {
                    const uint32_t *h32 = (const uint32_t *)hits;
                    const uint32_t key32 = (uint32_t)key;
                    for (; x + 8 <= x1; x += 8) {
                        uint32_t h[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) h[j] = h32[2 * (x + j)];
#pragma unroll
                        for (int j = 0; j < 8; j++) rk += h[j] < key32 ? 1u : 0u;
                    }
                }
                for (; x + 8 <= x1; x += 8) {
                    uint64_t h[8];
#pragma unroll
                    for (int j = 0; j < 8; j++) h[j] = hits[x + j];
#pragma unroll
                    for (int j = 0; j < 8; j++) rk += h[j] < key ? 1u : 0u;
                }
                for (; x + 4 <= x1; x += 4) {
                    const uint64_t h0 = hits[x], h1 = hits[x + 1], h2 = hits[x + 2], h3 = hits[x + 3];
                    rk += (h0 < key ? 1u : 0u) + (h1 < key ? 1u : 0u) + (h2 < key ? 1u : 0u) + (h3 < key ? 1u : 0u);
                }
                for (; x < x1; x++) rk += hits[x] < key ? 1u : 0u;
                return rk;
            };
            const uint32_t nheavy = refine ? s_nheavy : 0u;
            if (REFINE) {
                // ---- second pass, one heavy bucket at a time: its hits [hb0, hb1) are dealt into NB2 slices of the bucket's
                // own diagonal range (counting pass, scan, scatter through registers) and ranked inside their slice; the
                // bucket ends up sorted in place.  A slice that is still long (hundreds of hits on one diagonal: a
                // low-complexity read) only makes its ranking loop longer.
                for (uint32_t hv = 0; hv < nheavy; hv++) {
                    const uint32_t hb = s_heavy[hv];
                    const uint32_t hb0 = hb ? bcnt[hb - 1] : 0u, hb1 = bcnt[hb];
                    if (tid == 0) {
                        s_dmin = ~0ull;
                        s_dmax = 0ull;
                    }
                    for (int32_t i = tid; i < NB2; i += NT) fcnt[i] = 0;
                    unsigned long long lmin = ~0ull, lmax = 0ull;
                    for (uint32_t i = hb0 + tid; i < hb1; i += NT) {
                        const unsigned long long d = (hits[i] >> HIT_QBITS) & DM;
                        lmin = d < lmin ? d : lmin;
                        lmax = d > lmax ? d : lmax;
                    }
                    for (int off = LANES / 2; off > 0; off >>= 1) {
                        const unsigned long long a = __shfl_xor(lmin, off, LANES), c = __shfl_xor(lmax, off, LANES);
                        lmin = a < lmin ? a : lmin;
                        lmax = c > lmax ? c : lmax;
                    }
                    __syncthreads();
                    if ((tid & (LANES - 1)) == 0) {
                        atomicMin(&s_dmin, lmin);
                        atomicMax(&s_dmax, lmax);
                    }
                    __syncthreads();
                    // (slices aligned to their width, as the buckets are: the hits of a slice then agree above their low
                    // 24 + sh2 bits, which is what lets count_below compare low words)
                    uint64_t e0 = s_dmin;
                    int sh2 = 0;
                    while (((s_dmax - e0) >> sh2) >= (uint64_t)NB2) {
                        sh2++;
                        e0 = s_dmin & ~((1ull << sh2) - 1);
                    }
                    auto slice = [&](uint64_t key) { return (uint32_t)((((key >> HIT_QBITS) & DM) - e0) >> sh2); };
                    for (uint32_t i = hb0 + tid; i < hb1; i += NT) atomicAdd(&fcnt[slice(hits[i])], 1u);
                    __syncthreads();
                    uint32_t f2[NB2 / NT > 0 ? NB2 / NT : 1], fsum = 0;
#pragma unroll
                    for (int u = 0; u < NB2 / NT; u++) {
                        f2[u] = fcnt[tid * (NB2 / NT) + u];
                        fsum += f2[u];
                    }
                    uint32_t fincl = fsum;
                    for (int off = 1; off < LANES; off <<= 1) {
                        const uint32_t up = __shfl_up(fincl, off, LANES);
                        if ((tid & (LANES - 1)) >= off) fincl += up;
                    }
                    if ((tid & (LANES - 1)) == LANES - 1) s_bw[tid / LANES] = fincl;
                    __syncthreads();
                    uint32_t fbase = hb0 + fincl - fsum;
                    for (int wv = 0; wv < tid / LANES; wv++) fbase += s_bw[wv];
#pragma unroll
                    for (int u = 0; u < NB2 / NT; u++) {
                        fcnt[tid * (NB2 / NT) + u] = fbase;
                        fbase += f2[u];
                    }
#pragma unroll
                    for (int u = 0; u < E; u++) {
                        const uint32_t i = hb0 + (uint32_t)tid + (uint32_t)u * NT;
                        ke[u] = i < hb1 ? hits[i] : 0ull;
                    }
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < E; u++) {
                        const uint32_t i = hb0 + (uint32_t)tid + (uint32_t)u * NT;
                        if (i < hb1) hits[atomicAdd(&fcnt[slice(ke[u])], 1u)] = ke[u];
                    }
                    __syncthreads();  // fcnt[f] = end of slice f (absolute positions)
#pragma unroll
                    for (int u = 0; u < E; u++) {
                        const uint32_t i = hb0 + (uint32_t)tid + (uint32_t)u * NT;
                        dst[u] = 0;
                        if (i < hb1) {
                            const uint64_t key = hits[i];
                            ke[u] = key;
                            const uint32_t f = slice(key);
                            const uint32_t f0 = f ? fcnt[f - 1] : hb0, f1 = fcnt[f];
                            dst[u] = f0 + count_below(f0, f1, key, sh2 <= 32 - HIT_QBITS);
                        }
                    }
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < E; u++)
                        if (hb0 + (uint32_t)tid + (uint32_t)u * NT < hb1) hits[dst[u]] = ke[u];
                    __syncthreads();
                }
            }
#pragma unroll
            for (int u = 0; u < E; u++) {
                const int32_t i = tid + u * NT;
                dst[u] = 0;
                if (i < n) {
                    const uint64_t key = hits[i];
                    ke[u] = key;
                    const uint32_t bk = bucket(key);
                    const uint32_t b0 = bk ? bcnt[bk - 1] : 0u, b1 = bcnt[bk];
                    bool heavy = false;
                    if (REFINE)
                        for (uint32_t hv = 0; hv < nheavy; hv++) heavy = heavy || s_heavy[hv] == bk;
                    if (heavy)  // sorted by the second pass
                        dst[u] = (uint32_t)i;
                    else
                        dst[u] = b0 + count_below(b0, b1, key, sh <= 32 - HIT_QBITS);
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < E; u++)
                if (tid + u * NT < n) hits[dst[u]] = ke[u];
            N = 1;
        } else {
#ifdef DH_SEED_PROF
            if (tid == 0) seed_prof_lds()[10] += 1ull;
#endif
            for (int32_t i = n + tid; i < N; i += NT) hits[i] = ~0ull;
        }
    } else {
        for (int32_t i = n + tid; i < N; i += NT) hits[i] = ~0ull;
    }
    __syncthreads();
    // Pair p exchanges elements i = insert-zero-bit(p, j) and i | j.  Pairs are dealt to threads in
    // runs of 64, so for strides j < 128 both elements of every pair of a wavefront live in that
    // wavefront's own 128-element blocks: those rounds need no block barrier (LDS operations of
    // one wavefront execute in order), only the rounds with j >= 128 do.
    for (int32_t kk = 2; kk <= N; kk <<= 1) {
        for (int32_t j = kk >> 1; j > 0; j >>= 1) {
            const bool cross = j >= 128;
            if (cross) __syncthreads();
            // pairs in batches of SORT_U: all loads of a batch are issued before the first exchange is stored (the pairs
            // of a round are disjoint).  One pair at a time made every pair a full memory round trip -- 64 of them in a
            // row per thread and round when 50 000 hits of a repeat-rich read are sorted in the HBM slab (17 ms for the
            // 27 such reads of a configs[2] half)
            constexpr int SORT_U = (LCAP == 0 || LCAP >= 4096) ? 8 : 4;
            for (int32_t p0 = tid; p0 < (N >> 1); p0 += NT * SORT_U) {
                uint64_t xs[SORT_U], ys[SORT_U];
#pragma unroll
                for (int u = 0; u < SORT_U; u++) {
                    const int32_t p = p0 + u * NT;
                    if (p < (N >> 1)) {
                        const int32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                        xs[u] = hits[i];
                        ys[u] = hits[i | j];
                    }
                }
#pragma unroll
                for (int u = 0; u < SORT_U; u++) {
                    const int32_t p = p0 + u * NT;
                    if (p < (N >> 1)) {
                        const int32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                        const bool up = (i & kk) == 0;
                        if ((xs[u] > ys[u]) == up) {
                            hits[i] = ys[u];
                            hits[i | j] = xs[u];
                        }
                    }
                }
            }
            if (cross)
                __syncthreads();
            else
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
    }
    __syncthreads();
    if (tid == 0) {  // hits per strand: the forward strand sorts first
        int32_t lo = 0, hi = n;
        while (lo < hi) {
            const int32_t mid = (lo + hi) >> 1;
            if (hits[mid] >> 63)
                hi = mid;
            else
                lo = mid + 1;
        }
        nhits_out[item] = lo;
        nhits_out[item + 1] = n - lo;
    }
    SP(1)
    // ---- band pairs.  Small variants (FASTB): one block-wide inclusive scan over
    // (band-head flag << 18 | covered-base contribution) gives every band its coverage as a
    // difference of two prefix sums and the compacted list of band heads, so the work is spread
    // over all threads instead of one serial walk per band; large variants (no LDS to spare) walk
    // the four bands from every band head.
    // The 8192-entry variant has no LDS to spare either, but its two arrays fit a per-block slab of
    // global scratch (48 KB, L2 resident since the persistent block reuses it): the parallel scan beats
    // the serial walks by far (pile-up all-vs-all: 183 -> about 30 us per read).  18 bits of coverage and
    // 14 bits of head count hold up to 8192 hits of k <= 28.
    // The HBM variant (LCAP == 0: the few reads whose hits -- tens of thousands for a repeat-rich read -- overflow the
    // LDS buffer) scans as well, with 64-bit sums (32 bits of coverage, 32 of head count) and 32-bit head positions in
    // the block's slab behind the hits: the serial walks cost a chain of dependent L2 round trips per hit of a band,
    // 5 - 21 ms for the 27 such reads of a configs[2] half (one block each).
    // (the 16384-entry variant fed from segments -- uncapped pile-ups: 166 reads, ~10 000 hits per read -- scans as well,
    // with the wide sums of the HBM variant in a slab of 24 576 words per block; the directory-fed one keeps the walks)
    // HTAB: only band heads are ever looked up, and a head needs its position and the coverage summed before it.  The
    // number of heads is known after the first pass of the scan; a read of n hits leaves hits[n .. LCAP) unused, so where
    // nheads + 1 entries (position << HSH | coverage before the head: the layout of the sums; the last entry is (n, total))
    // fit behind the hits the second pass writes those and nothing per hit: a band's coverage is the difference of two
    // neighbouring entries, and the head loop's six to eight dependent loads per head are LDS round trips instead of L2's.
    // 14 + 18 bits hold every read the table has room for at 8192 (positions <= n <= 8191, k <= 28); the 16384-entry tier
    // takes 32 + 32.  A read whose table does not fit (n + table > LCAP) keeps the slab.
    constexpr bool FASTB = LCAP <= 8192 || (JOIN && LCAP == 16384);
    constexpr bool FB_BIG = LCAP == 0;
    constexpr bool FB_WIDE = LCAP == 0 || LCAP == 16384;
    using bsum_t = typename std::conditional<FB_WIDE, uint64_t, uint32_t>::type;
    using bhead_t = typename std::conditional<FB_WIDE, uint32_t, uint16_t>::type;
    constexpr int HSH = FB_WIDE ? 32 : 18;
    constexpr bsum_t CMASK = ((bsum_t)1 << HSH) - 1;
    bsum_t *bsum = FB_LDS ? (bsum_t *)bsum_l
                          : (FB_BIG ? (bsum_t *)(hits + gcap) : (bsum_t *)(gbuf + (int64_t)slab * gcap));
    bhead_t *bhead = FB_LDS ? (bhead_t *)bhead_l : (bhead_t *)(bsum + (LCAP > 0 ? LCAP : gcap));
    __shared__ bsum_t s_wsum[NT / LANES];
    __shared__ int32_t s_nbig;
    constexpr int NBIG = NT <= LANES ? 8 : (SLIM ? 16 : ((LCAP > 0 && LCAP <= 4096) ? 128 : 64));  // (the 8192-entry variant has no LDS to spare; what does not fit walks serially)
    __shared__ int32_t bigc[HTAB ? 1 : NBIG][4];  // candidate band pairs with long hit ranges: (first, end, P, slot)
    __shared__ unsigned long long s_bestkeys[HTAB ? 1 : NBIG];
    // HTAB: every long range gets lanes.  Its descriptor is parked in the candidate's own record, which is not final before
    // emit_cand (score = P, aseq = first, apos = end, then bpos = first hit of the best run); biglist names those slots
    __shared__ uint16_t biglist[HTAB ? 2 * CC : 1];
    static_assert(2 * CC <= 65536, "a candidate slot fits a biglist entry");
    const int bs = o.band_shift;
    // seed of a band pair [i, e1): first hit of the same-diagonal run (steps <= k) covering most
    // bases; then the candidate record
    auto emit_cand = [&](int32_t slot, int32_t best_first, int32_t P, int64_t band) {
        const int64_t D = hitD(hits[best_first]) & ((1ll << HIT_DBITS) - 1);  // without the strand bit
        const int32_t q = hitQ(hits[best_first]);
        const int64_t gv = D - ix.sepv + q;
        // sequences start on 4096-base pages of the virtual axis: the page names the sequence (the binary search
        // over goff this replaces was a chain of ten dependent loads per candidate)
        const int32_t lo = ix.page_seq[gv >> 12];
        cands[slot].score = P;
        cands[slot].aseq = lo;
        cands[slot].apos = (int32_t)(gv - ix.goff[lo]);
        cands[slot].bpos = q;
        cband[slot] = band;
    };
    auto serial_seed = [&](int32_t i, int32_t e1) {
        int32_t best_first = i, best_cov = -1, run_first = i;
        for (int32_t x = i; x < e1; x++) {
            bool linked = false;
            if (x > i && hitD(hits[x]) == hitD(hits[x - 1]))
                linked = (hitQ(hits[x]) - hitQ(hits[x - 1])) <= k;
            if (!linked) run_first = x;
            const int32_t cov = k + hitQ(hits[x]) - hitQ(hits[run_first]);
            if (cov > best_cov) {
                best_cov = cov;
                best_first = run_first;
            }
        }
        return best_first;
    };
    if (FASTB) {
        if (tid == 0) s_nbig = 0;
        // -- scan: thread t owns the elements [t * per, t * per + per)
        const int32_t per = (n + NT - 1) / NT;
        const int32_t x0 = tid * per, x1 = min(n, x0 + per);
        // (LCAP > 0: the first pass only sums -- the hits are in LDS, the sums of the 8192 / 16384-entry variants in a slab of
        // global memory: storing the partial sums here and loading them back below was a chain of dependent round trips per
        // element; the second pass recomputes an element's term from the hits instead)
        bsum_t acc = 0;
        for (int32_t i = x0; i < x1; i++) {
            const bool head = i == 0 || (hitD(hits[i - 1]) >> bs) != (hitD(hits[i]) >> bs);
            acc += ((bsum_t)(head ? 1u : 0u) << HSH) | (bsum_t)hit_cov(hits, i, k);
            if (LCAP == 0) bsum[i] = acc;
        }
        bsum_t incl = acc;  // inclusive scan of the per-thread totals: inside the wavefront ...
        for (int off = 1; off < LANES; off <<= 1) {
            const bsum_t up = __shfl_up(incl, off, LANES);
            if ((tid & (LANES - 1)) >= off) incl += up;
        }
        if ((tid & (LANES - 1)) == LANES - 1) s_wsum[tid / LANES] = incl;
        __syncthreads();
        bsum_t base = incl - acc;  // ... plus the wavefronts before this one
        for (int wv = 0; wv < tid / LANES; wv++) base += s_wsum[wv];
        bsum_t run = base;
        // HTAB: the head table behind the hits, where it fits (the whole block decides alike: n and the block's total)
        constexpr int TPW = (int)(sizeof(uint64_t) / sizeof(bsum_t));  // table entries per entry of the hit buffer
        bsum_t *htab = (bsum_t *)(hits + n);
        bool use_tab = false;
        int32_t nheads_tab = 0;
        if constexpr (HTAB) {
            static_assert(HTAB ? sizeof(bsum_t) * 8 - HSH >= (LCAP == 8192 ? 14 : 15) : true, "a position <= LCAP - 1 (and n) fits an entry");
            bsum_t tot = 0;
            for (int wv = 0; wv < NT / LANES; wv++) tot += s_wsum[wv];
            nheads_tab = (int32_t)(tot >> HSH);
            use_tab = !g_seed_slab_bands && n + (nheads_tab + 1 + TPW - 1) / TPW <= LCAP;
            if (tid == 0) {
                seed_band_lds()[use_tab ? 0 : 1]++;
                if (use_tab) htab[nheads_tab] = ((bsum_t)n << HSH) | (tot & CMASK);
            }
        }
        if (HTAB && use_tab) {
            for (int32_t i = x0; i < x1; i++) {
                const bool head = i == 0 || (hitD(hits[i - 1]) >> bs) != (hitD(hits[i]) >> bs);
                // (run: heads and coverage before hit i)
                if (head) htab[(int32_t)(run >> HSH)] = ((bsum_t)i << HSH) | (run & CMASK);
                run += ((bsum_t)(head ? 1u : 0u) << HSH) | (bsum_t)hit_cov(hits, i, k);
            }
        } else
        for (int32_t i = x0; i < x1; i++) {
            const bool head = i == 0 || (hitD(hits[i - 1]) >> bs) != (hitD(hits[i]) >> bs);
            bsum_t v;
            if (LCAP == 0)
                v = bsum[i] + base;
            else {
                run += ((bsum_t)(head ? 1u : 0u) << HSH) | (bsum_t)hit_cov(hits, i, k);
                v = run;
            }
            bsum[i] = v;
            if (head) bhead[(v >> HSH) - 1] = (bhead_t)i;
        }
        __syncthreads();
        SP(2)
        if constexpr (HTAB) {
            // the head loop over (position of head r, coverage of band r): from the slab's arrays or from the head table
            auto head_loop = [&](const int32_t nheads, auto hpos, auto band_cov) {
                for (int32_t rnk = tid; rnk < nheads; rnk += NT) {
                    const int32_t i = hpos(rnk);
                    const int64_t band = hitD(hits[i]) >> bs;
                    int32_t covm1 = 0, cov1 = 0, cov2 = 0, e1;
                    const int32_t cov0 = band_cov(rnk);
                    if (rnk > 0 && (hitD(hits[hpos(rnk - 1)]) >> bs) == band - 1) covm1 = band_cov(rnk - 1);
                    int32_t nx = rnk + 1;  // head number of the next band present
                    e1 = nx < nheads ? hpos(nx) : n;
                    if (nx < nheads && (hitD(hits[hpos(nx)]) >> bs) == band + 1) {
                        cov1 = band_cov(nx);
                        nx++;
                        e1 = nx < nheads ? hpos(nx) : n;
                    }
                    if (nx < nheads && (hitD(hits[hpos(nx)]) >> bs) == band + 2) cov2 = band_cov(nx);
                    const int32_t P = cov0 + cov1, Pm1 = covm1 + cov0, Pp1 = cov1 + cov2;
                    if (P < o.hmin || P < Pm1 || P <= Pp1) continue;
                    const int32_t slot = atomicAdd(&s_nc, 1);
                    if (slot >= 2 * CC) continue;
                    if (e1 - i > 16) {
                        // long range: the whole block picks the seed below
                        const int32_t bslot = atomicAdd(&s_nbig, 1);
                        // (at most 2 CC slots are handed out, so bslot < 2 CC)
                        cands[slot].score = P;
                        cands[slot].aseq = i;
                        cands[slot].apos = e1;
                        biglist[bslot] = (uint16_t)slot;
                        continue;
                    }
                    emit_cand(slot, serial_seed(i, e1), P, band);
                }
            };
            if (use_tab) {
                head_loop(
                    nheads_tab, [&](int32_t rnk) { return (int32_t)(htab[rnk] >> HSH); },
                    [&](int32_t rnk) { return (int32_t)((htab[rnk + 1] & CMASK) - (htab[rnk] & CMASK)); });
            } else {
                const int32_t nheads = (int32_t)(bsum[n - 1] >> HSH);
                head_loop(
                    nheads, [&](int32_t rnk) { return (int32_t)bhead[rnk]; },
                    [&](int32_t rnk) {  // coverage of the band with head number rnk
                        const int32_t st_ = bhead[rnk], en_ = rnk + 1 < nheads ? bhead[rnk + 1] : n;
                        return (int32_t)((bsum[en_ - 1] & CMASK) - (st_ ? (bsum[st_ - 1] & CMASK) : (bsum_t)0));
                    });
            }
        } else {
            const int32_t nheads = (int32_t)(bsum[n - 1] >> HSH);
            auto band_cov = [&](int32_t rnk) {  // coverage of the band with head number rnk
                const int32_t st_ = bhead[rnk], en_ = rnk + 1 < nheads ? bhead[rnk + 1] : n;
                return (int32_t)((bsum[en_ - 1] & CMASK) - (st_ ? (bsum[st_ - 1] & CMASK) : (bsum_t)0));
            };
            for (int32_t rnk = tid; rnk < nheads; rnk += NT) {
                const int32_t i = bhead[rnk];
                const int64_t band = hitD(hits[i]) >> bs;
                int32_t covm1 = 0, cov1 = 0, cov2 = 0, e1;
                const int32_t cov0 = band_cov(rnk);
                if (rnk > 0 && (hitD(hits[bhead[rnk - 1]]) >> bs) == band - 1) covm1 = band_cov(rnk - 1);
                int32_t nx = rnk + 1;  // head number of the next band present
                e1 = nx < nheads ? bhead[nx] : n;
                if (nx < nheads && (hitD(hits[bhead[nx]]) >> bs) == band + 1) {
                    cov1 = band_cov(nx);
                    nx++;
                    e1 = nx < nheads ? bhead[nx] : n;
                }
                if (nx < nheads && (hitD(hits[bhead[nx]]) >> bs) == band + 2) cov2 = band_cov(nx);
                const int32_t P = cov0 + cov1, Pm1 = covm1 + cov0, Pp1 = cov1 + cov2;
                if (P < o.hmin || P < Pm1 || P <= Pp1) continue;
                const int32_t slot = atomicAdd(&s_nc, 1);
                if (slot >= 2 * CC) continue;
                if (e1 - i > 16) {
                    // long range: the whole block picks the seed below
                    const int32_t bslot = atomicAdd(&s_nbig, 1);
                    if (bslot < NBIG) {
                        bigc[bslot][0] = i;
                        bigc[bslot][1] = e1;
                        bigc[bslot][2] = P;
                        bigc[bslot][3] = slot;
                        continue;
                    }
                }
                emit_cand(slot, serial_seed(i, e1), P, band);
            }
        }
        __syncthreads();
        SP(8)
        // long ranges: 16 lanes per candidate, 16 consecutive hits at a time.  The first hit of the run a hit belongs to
        // (a run = hits of one diagonal at most k apart) is the running maximum of the run heads' positions -- a scan
        // over the 16 lanes plus the carry of the lanes before --, not a walk back from every run end: the walks were a
        // chain of dependent LDS round trips as long as the longest run of the wavefront (13 of the 97 us per read)
        // (SLIM: a wavefront per candidate -- an unsampled mapping read has two or three candidates whose band pairs hold
        // most of its ~900 hits: at 16 lanes the walk was 56 dependent rounds by one quarter of a wavefront, 9.4 of the
        // 31 us a 512-thread block spent per read, while every other lane waited at the barrier below; 3.7 us this way)
        // (HTAB: all of them -- a read of a deep pile-up has a long range per partner it plays B for, 80 and more; beyond
        // 64 slots they walked serially, one lane each, while the block waited at the barrier above)
        constexpr int GW = SLIM ? LANES : 16;
        const int32_t nbig = HTAB ? s_nbig : min(s_nbig, NBIG);
        const int gl = tid & (GW - 1);
        for (int32_t bc = tid / GW; bc < nbig; bc += NT / GW) {
            const int32_t i = HTAB ? cands[biglist[bc]].aseq : bigc[bc][0], e1 = HTAB ? cands[biglist[bc]].apos : bigc[bc][1];
            unsigned long long best = 0ull;
            int32_t carry = i;
            for (int32_t base = i; base < e1; base += GW) {
                const int32_t x = base + gl;
                const bool valid = x < e1;
                const uint64_t h = valid ? hits[x] : 0ull;
                const uint64_t hp = valid && x > i ? hits[x - 1] : 0ull;
                const uint64_t hn = x + 1 < e1 ? hits[x + 1] : 0ull;
                const bool linked = valid && x > i && hitD(h) == hitD(hp) && (hitQ(h) - hitQ(hp)) <= k;
                int32_t f = valid && !linked ? x : -1;
                for (int off = 1; off < GW; off <<= 1) {
                    const int32_t up = __shfl_up(f, off, GW);
                    if (gl >= off) f = up > f ? up : f;
                }
                f = carry > f ? carry : f;
                carry = __shfl(f, GW - 1, GW);
                // a run ends where the next hit is not linked; its coverage is the largest of the run
                const bool last = valid && (x + 1 >= e1 || hitD(hn) != hitD(h) || (hitQ(hn) - hitQ(h)) > k);
                if (last) {
                    const uint32_t cov = (uint32_t)(k + hitQ(h) - hitQ(hits[f]));
                    // largest coverage, then the earliest run
                    const unsigned long long key = ((unsigned long long)cov << 32) | (uint32_t)(0x7FFFFFFF - f);
                    best = key > best ? key : best;
                }
            }
            for (int off = GW / 2; off > 0; off >>= 1) {
                const unsigned long long ot = __shfl_xor(best, off, GW);
                best = ot > best ? ot : best;
            }
            if (gl == 0) {
                if constexpr (HTAB)
                    cands[biglist[bc]].bpos = 0x7FFFFFFF - (int32_t)(uint32_t)best;
                else
                    s_bestkeys[bc] = best;
            }
        }
        __syncthreads();
        SP(9)
        for (int32_t bc = tid; bc < nbig; bc += NT) {
            if constexpr (HTAB) {
                const int32_t slot = biglist[bc];
                const DhCand d = cands[slot];  // the parked descriptor, read before emit_cand overwrites it
                emit_cand(slot, d.bpos, d.score, hitD(hits[d.aseq]) >> bs);
            } else
                emit_cand(bigc[bc][3], 0x7FFFFFFF - (int32_t)(uint32_t)s_bestkeys[bc], bigc[bc][2], hitD(hits[bigc[bc][0]]) >> bs);
        }
    } else {
        for (int32_t i = tid; i < n; i += NT) {
            const int64_t band = hitD(hits[i]) >> bs;
            if (i > 0 && (hitD(hits[i - 1]) >> bs) == band) continue;  // not a band head
            int32_t covm1 = 0, cov0 = 0, cov1 = 0, cov2 = 0, e1;
            for (int32_t j = i - 1; j >= 0 && (hitD(hits[j]) >> bs) == band - 1; j--)
                covm1 += hit_cov(hits, j, k);
            int32_t j = i;
            for (; j < n && (hitD(hits[j]) >> bs) == band; j++) cov0 += hit_cov(hits, j, k);
            for (; j < n && (hitD(hits[j]) >> bs) == band + 1; j++) cov1 += hit_cov(hits, j, k);
            e1 = j;
            for (; j < n && (hitD(hits[j]) >> bs) == band + 2; j++) cov2 += hit_cov(hits, j, k);
            const int32_t P = cov0 + cov1, Pm1 = covm1 + cov0, Pp1 = cov1 + cov2;
            if (P < o.hmin || P < Pm1 || P <= Pp1) continue;
            const int32_t slot = atomicAdd(&s_nc, 1);
            if (slot < 2 * CC) emit_cand(slot, serial_seed(i, e1), P, band);
        }
    }
    __syncthreads();
    SP(3)
    int32_t nc = s_nc;
    if (nc > 2 * CC) {
        // more candidate band pairs than one read can sensibly have (a repeat the -t cap did not
        // catch): the read yields no alignments and is reported (ncand = -2), the launch goes on
        // (the wavefront-per-read tier and the middle tier hold fewer: the read goes to a tier with the full SEED_CCAP,
        // where the rule above decides)
        if (tid == 0) {
            ncand_out[item] = ncand_out[item + 1] = CC < SEED_CCAP ? -1 : -2;
            if (CC < SEED_CCAP) {
                nhits_out[item] = n;
                nhits_out[item + 1] = 0;
            }
        }
        return;
    }
    // ---- rank per strand by (score desc, band asc); bands are distinct so ranks are a permutation
    // (the strand is the top bit of the band).  Symmetric all-vs-all: the kept candidates
    // (rank < max_cand) are then grouped by A read, rank order inside a group -- groups are the only
    // candidates that depend on each other (coverage skip), which makes each of them a separate work
    // unit of the wave kernel (k_units).
    // (the ranks overlay the hit buffer, which nobody reads any more: the 2 KB they took kept the 8192-entry variant at 81.5 KB
    // of LDS -- one block per CU instead of two)
    __shared__ int32_t crank_s[LCAP > 0 ? 1 : 2 * CC];
    int32_t *crank = LCAP > 0 ? (int32_t *)lhits : crank_s;
    __shared__ int32_t s_ncs[2];
    constexpr int BSTR = HIT_DBITS;  // strand bit of a band = bit HIT_DBITS - band_shift
    auto strand_of = [&](int32_t c) { return (int32_t)((cband[c] >> (BSTR - bs)) & 1); };
    if (tid < 2) s_ncs[tid] = 0;
    __syncthreads();
    if constexpr (HTAB) {
        // A read of a deep pile-up has a candidate band pair per partner, 80 to 160 of them: one thread per candidate left
        // most of the block idle behind a chain of nc LDS round trips, twice.  G lanes share a candidate's loop over the
        // others and add their counts up (sums of integers: the same ranks).
        int G = 4;
        while (G < LANES && nc * 2 * G <= NT) G <<= 1;
        const int gl = tid & (G - 1);
        for (int32_t c0 = 0; c0 < nc; c0 += NT / G) {  // (every lane of a group takes part in the shuffles)
            const int32_t c = c0 + tid / G;
            const bool on = c < nc;
            const int32_t cc = on ? c : 0;
            const int32_t st = strand_of(cc);
            const int32_t sc = cands[cc].score;
            const int64_t bc = cband[cc];
            int32_t rank = 0;
#pragma unroll 4
            for (int32_t x = gl; x < nc; x += G) {
                const int64_t bx = cband[x];
                const int32_t sx = cands[x].score;
                rank += ((int32_t)((bx >> (BSTR - bs)) & 1) == st && (sx > sc || (sx == sc && bx < bc))) ? 1 : 0;
            }
            for (int off = G >> 1; off > 0; off >>= 1) rank += __shfl_xor(rank, off, G);
            if (on && gl == 0) {
                crank[c] = rank;
                atomicAdd(&s_ncs[st], 1);
            }
        }
        __syncthreads();
        for (int32_t c0 = 0; c0 < nc; c0 += NT / G) {
            const int32_t c = c0 + tid / G;
            const bool on = c < nc;
            const int32_t cc = on ? c : 0;
            const int32_t rank = crank[cc], st = strand_of(cc);
            const bool kept = on && rank < o.max_cand;
            int32_t pos = 0;
            if (o.skip_self == 2) {
                const int32_t ac = cands[cc].aseq;
                if (kept) {
#pragma unroll 4
                    for (int32_t x = gl; x < nc; x += G) {
                        const int32_t ax = cands[x].aseq, rx = crank[x];
                        pos += (strand_of(x) == st && rx < o.max_cand && (ax < ac || (ax == ac && rx < rank))) ? 1 : 0;
                    }
                }
                for (int off = G >> 1; off > 0; off >>= 1) pos += __shfl_xor(pos, off, G);
            } else
                pos = rank;
            if (kept && gl == 0) cand_out[(int64_t)(item + st) * o.max_cand + pos] = cands[cc];
        }
    } else {
        for (int32_t c = tid; c < nc; c += NT) {
            const int32_t st = strand_of(c);
            const int32_t sc = cands[c].score;
            const int64_t bc = cband[c];
            int32_t rank = 0;
            // (no branches, loads of four candidates in flight: the loop is a chain of LDS round trips otherwise)
#pragma unroll 4
            for (int32_t x = 0; x < nc; x++) {
                const int64_t bx = cband[x];
                const int32_t sx = cands[x].score;
                rank += ((int32_t)((bx >> (BSTR - bs)) & 1) == st && (sx > sc || (sx == sc && bx < bc))) ? 1 : 0;
            }
            crank[c] = rank;
            atomicAdd(&s_ncs[st], 1);
        }
        __syncthreads();
        for (int32_t c = tid; c < nc; c += NT) {
            const int32_t rank = crank[c], st = strand_of(c);
            if (rank >= o.max_cand) continue;
            int32_t pos = rank;
            if (o.skip_self == 2) {
                pos = 0;
                const int32_t ac = cands[c].aseq;
#pragma unroll 4
                for (int32_t x = 0; x < nc; x++) {
                    const int32_t ax = cands[x].aseq, rx = crank[x];
                    pos += (strand_of(x) == st && rx < o.max_cand && (ax < ac || (ax == ac && rx < rank))) ? 1 : 0;
                }
            }
            cand_out[(int64_t)(item + st) * o.max_cand + pos] = cands[c];
        }
    }
    if (tid < 2) ncand_out[item + tid] = s_ncs[tid] < o.max_cand ? s_ncs[tid] : o.max_cand;
    SP(4)
#ifdef DH_SEED_PROF
    if (tid == 0) seed_prof_lds()[7] += 1ull;
#endif
}
// Persistent blocks: the grid is sized to the resident capacity of the chip and every block pulls
// items from an atomic queue (no per-item block launch, dynamic balance over ragged read lengths).
template <int LCAP, bool JOIN, int NT = SEED_THREADS, int CC = SEED_CCAP>
__global__ void __launch_bounds__(NT, NT <= LANES ? 4 : (NT < SEED_THREADS ? 5 : ((LCAP > 0 && LCAP <= 2048) ? 6 : (LCAP == 16384 ? 2 : 4))))
k_seed(DbView B, IndexView ix, JoinView jv, DhOpts o, int32_t read0,
       int32_t nreads, DhCand *__restrict__ cand_out, int32_t *__restrict__ ncand_out,
       int32_t *__restrict__ nhits_out, int32_t *__restrict__ status, uint64_t *__restrict__ gbuf,
       int32_t gcap, const int32_t *__restrict__ read_list, uint32_t *__restrict__ queue)
{
    __shared__ int32_t s_work;
    // (the queue is ONE address: half a million reads of a mapping chunk were half a million returning atomics on it, ~11 ns
    // each whatever the kernel did in between -- 5.7 of the wavefront-per-read tier's 5.7 ms, SQ_WAIT_ANY 88 %.  The small
    // tiers of the segment-fed back end take eight reads per atomic.)
    constexpr int32_t BATCH = (JOIN && LCAP > 0 && LCAP <= 2048) ? 8 : 1;
#ifdef DH_SEED_PROF
    if (threadIdx.x == 0)
        for (int i = 0; i < 12; i++) seed_prof_lds()[i] = 0;
#endif
    constexpr bool HTAB = JOIN && NT == SEED_THREADS && (LCAP == 8192 || LCAP == 16384);  // (as in seed_item)
    if constexpr (HTAB)
        if (threadIdx.x < 2) seed_band_lds()[threadIdx.x] = 0;
    for (;;) {
        __syncthreads();  // the previous read is finished by every thread (shared state is reused)
        if (threadIdx.x == 0) s_work = (int32_t)atomicAdd(queue, (uint32_t)BATCH);
        __syncthreads();
        const int32_t work0 = s_work;
        if (work0 >= nreads) break;
#pragma unroll 1
        for (int32_t wi = 0; wi < BATCH; wi++) {
            const int32_t work = work0 + wi;
            if (work >= nreads) break;
            if (wi) __syncthreads();
            // (HTAB: inlined by force.  Left to itself the compiler makes seed_item<16384, true> a function of its own and
            // keeps the four views it takes by reference in 272 bytes of scratch per lane, read back field by field)
            if constexpr (HTAB) {
                [[clang::always_inline]] seed_item<LCAP, JOIN, NT, CC>(B, ix, jv, o, read0, work, (int32_t)blockIdx.x, cand_out,
                                                                       ncand_out, nhits_out, status, gbuf, gcap, read_list);
            } else
                seed_item<LCAP, JOIN, NT, CC>(B, ix, jv, o, read0, work, (int32_t)blockIdx.x, cand_out, ncand_out, nhits_out,
                                              status, gbuf, gcap, read_list);
        }
    }
#ifdef DH_SEED_PROF
    if (threadIdx.x == 0)
        for (int i = 0; i < 12; i++)
            if (seed_prof_lds()[i]) atomicAdd(&g_seed_prof[i], seed_prof_lds()[i]);
#endif
    if constexpr (HTAB)
        if (threadIdx.x < 2 && seed_band_lds()[threadIdx.x]) atomicAdd(&g_seed_band_reads[threadIdx.x], (unsigned long long)seed_band_lds()[threadIdx.x]);
}
#define SEED_INST(C, J)                                                                           \
    template __global__ void k_seed<C, J>(DbView, IndexView, JoinView, DhOpts, int32_t, int32_t,  \
                                          DhCand *, int32_t *, int32_t *, int32_t *, uint64_t *, int32_t, \
                                          const int32_t *, uint32_t *);
SEED_INST(1024, false)
SEED_INST(2048, false)
SEED_INST(4096, false)
SEED_INST(8192, false)
SEED_INST(16384, false)
SEED_INST(0, false)
SEED_INST(2048, true)
template __global__ void k_seed<512, true, 64, 32>(DbView, IndexView, JoinView, DhOpts, int32_t, int32_t, DhCand *, int32_t *, int32_t *,
                                                   int32_t *, uint64_t *, int32_t, const int32_t *, uint32_t *);
template __global__ void k_seed<2048, true, 256, 64>(DbView, IndexView, JoinView, DhOpts, int32_t, int32_t, DhCand *, int32_t *, int32_t *,
                                                     int32_t *, uint64_t *, int32_t, const int32_t *, uint32_t *);
SEED_INST(4096, true)
SEED_INST(8192, true)
SEED_INST(16384, true)
SEED_INST(0, true)

// ------------------------------------------------------------------------------------ launchers

// resident blocks of a seed variant on the whole chip (persistent grid size)
template <int C, bool J, int NT, int CC>
static int seed_grid(int32_t nitems, int32_t ncu)
{
    static int per_cu = 0;
    if (per_cu == 0) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_seed<C, J, NT, CC>, NT, 0) != hipSuccess || nb < 1)
            nb = 1;
        per_cu = nb;
        if (getenv("DH_TRACE"))
            fprintf(stderr, "[seeds] k_seed<%d, %s, %d, %d>: %d resident blocks per CU\n", C, J ? "true" : "false", NT, CC, nb);
    }
    int use = per_cu;
    if (const char *e = getenv("DH_SEED_BLOCKS_PER_CU")) use = std::max(1, std::min(per_cu, atoi(e)));  // development
    const int64_t g = (int64_t)use * ncu;
    return (int)(g < nitems ? g : nitems);
}

// what every tier of a seed launch shares.  queue: one zeroed uint32 (work counter of the persistent blocks);
// read_list (device, absolute read ids): only those reads, else the reads [read0, read0 + nreads)
struct SeedLaunch {
    hipStream_t st;
    DbView B;
    IndexView ix;
    JoinView jv;
    DhOpts o;
    int32_t read0, nreads;
    DhCand *cand;
    int32_t *ncand, *nhits, *status;
    const int32_t *read_list;
    uint32_t *queue;
    int32_t ncu;
};
// gbuf / gcap: the tier's global scratch per block and its size in 8-byte words (LCAP == 0: the hit slabs)
template <int C, bool J, int NT = SEED_THREADS, int CC = SEED_CCAP>
static void launch_seed(const SeedLaunch &a, uint64_t *gbuf, int32_t gcap)
{
    hipLaunchKernelGGL((k_seed<C, J, NT, CC>), dim3(seed_grid<C, J, NT, CC>(a.nreads, a.ncu)), dim3(NT), 0, a.st, a.B, a.ix,
                       a.jv, a.o, a.read0, a.nreads, a.cand, a.ncand, a.nhits, a.status, gbuf, gcap, a.read_list, a.queue);
}

// development / tests: DH_SEED_NO_REFINE=1 switches the second counting pass of the seed sort off, DH_SEED_SLAB_BANDS=1 the
// head table of the segment-fed 8192- and 16384-entry tiers (read per launch)
static void seed_sort_switch()
{
    static int cur = 1, cur_slab = 0;
    const int want = getenv("DH_SEED_NO_REFINE") ? 0 : 1;
    if (want != cur) {
        (void)hipDeviceSynchronize();
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_seed_sort_refine), &want, sizeof(int));
        cur = want;
    }
    const int want_slab = getenv("DH_SEED_SLAB_BANDS") ? 1 : 0;
    if (want_slab != cur_slab) {
        (void)hipDeviceSynchronize();
        (void)hipMemcpyToSymbol(HIP_SYMBOL(g_seed_slab_bands), &want_slab, sizeof(int));
        cur_slab = want_slab;
    }
}

// reads of the segment-fed 8192- and 16384-entry tiers since the last reset, on the current device: out[0] took the head
// table in LDS, out[1] the slab (every launch that counted has finished behind the synchronisation)
extern "C" int dhk_seed_band_counts(unsigned long long *out, int reset)
{
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_seed_band_reads), 2 * sizeof(unsigned long long)) != hipSuccess) return 1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_seed_band_reads), z, sizeof(z)) != hipSuccess) return 1;
    }
    return 0;
}

// item0 / nitems: even (both strands of the reads [item0 / 2, (item0 + nitems) / 2))
extern "C" void dhk_seed(hipStream_t st, int cap, DbView B, IndexView ix, DhOpts o,
                         int32_t item0, int32_t nitems, DhCand *cand, int32_t *ncand, int32_t *nhits,
                         int32_t *status, uint32_t *queue, int32_t ncu, uint64_t *fscr)
{
    if (nitems <= 0) return;
    seed_sort_switch();
    const SeedLaunch a = {st, B, ix, JoinView{}, o, item0 / 2, nitems / 2, cand, ncand, nhits, status, nullptr, queue, ncu};
    if (cap <= 1024)
        launch_seed<1024, false>(a, nullptr, 0);
    else if (cap <= 2048)
        launch_seed<2048, false>(a, nullptr, 0);
    else if (cap <= 4096)
        launch_seed<4096, false>(a, nullptr, 0);
    else if (cap <= 8192)
        launch_seed<8192, false>(a, fscr, DH_SEED_FSCR_WORDS);
    else
        launch_seed<16384, false>(a, nullptr, 0);
}

// the reads listed in read_list (device, absolute read ids) with their hits staged in HBM: block x owns the slab of
// 2 gcap + (gcap + 1) / 2 words that starts at gbuf[x * that]; gbuf holds one slab per block of the persistent grid
extern "C" void dhk_seed_big(hipStream_t st, DbView B, IndexView ix, DhOpts o,
                             const int32_t *read_list, int32_t nreads, uint64_t *gbuf, int32_t gcap, DhCand *cand,
                             int32_t *ncand, int32_t *nhits, int32_t *status, uint32_t *queue, int32_t ncu)
{
    if (nreads <= 0) return;
    const SeedLaunch a = {st, B, ix, JoinView{}, o, 0, nreads, cand, ncand, nhits, status, read_list, queue, ncu};
    launch_seed<0, false>(a, gbuf, gcap);
}

// the same back end fed from the hit segments of the per-pile-up k-mer join (dh_join.hip)
extern "C" void dhk_seed_join(hipStream_t st, int cap, DbView B, IndexView ix, DhOpts o, JoinView jv, int32_t item0,
                              int32_t nitems, DhCand *cand, int32_t *ncand, int32_t *nhits, int32_t *status,
                              uint32_t *queue, int32_t ncu, uint64_t *fscr, const int32_t *read_list, int32_t nlist,
                              int32_t mid_tier)
{
    if (nitems <= 0 || (read_list && nlist <= 0)) return;
    seed_sort_switch();
    // read_list (device, nlist absolute read ids): only those reads -- the second tier of the join path, the reads whose
    // hits overflowed the first tier's LDS buffer
    const SeedLaunch a = {st,     B,     ix,     jv,        o,     item0 / 2, read_list ? nlist : nitems / 2, cand, ncand,
                          nhits,  status, read_list, queue, ncu};
    if (cap <= 512)  // the first tier of a mapping: a wavefront per read (140 hits at 1/8 sampling), 32 candidate band pairs
        launch_seed<512, true, 64, 32>(a, nullptr, 0);
    else if (cap <= 2048 && mid_tier)  // an unsampled mapping (~900 hits per read): four wavefronts per read, 64 band pairs
        launch_seed<2048, true, 256, 64>(a, nullptr, 0);
    else if (cap <= 2048)
        launch_seed<2048, true>(a, nullptr, 0);
    else if (cap <= 4096)
        launch_seed<4096, true>(a, nullptr, 0);
    else if (cap <= 8192)
        launch_seed<8192, true>(a, fscr, DH_SEED_FSCR_WORDS);
    else
        launch_seed<16384, true>(a, fscr, DH_SEED_FSCR_WORDS16);
}

extern "C" void dhk_seed_big_join(hipStream_t st, DbView B, IndexView ix, DhOpts o, JoinView jv, const int32_t *read_list,
                                  int32_t nreads, uint64_t *gbuf, int32_t gcap, DhCand *cand, int32_t *ncand,
                                  int32_t *nhits, int32_t *status, uint32_t *queue, int32_t ncu)
{
    if (nreads <= 0) return;
    const SeedLaunch a = {st, B, ix, jv, o, 0, nreads, cand, ncand, nhits, status, read_list, queue, ncu};
    launch_seed<0, true>(a, gbuf, gcap);
}

#ifdef DH_SEED_PROF
#undef g_seed_prof
extern "C" void dhk_seed_prof_dump()
{
    unsigned long long all[3][12];
    (void)hipMemcpyFromSymbol(all, HIP_SYMBOL(g_seed_prof_all), sizeof(all));
    static const char *const row[3] = {"other tiers", "8192-entry tier", "16384-entry tier"};
    for (int t = 0; t < 3; t++) {
        const unsigned long long *h = all[t];
        if (!h[7]) continue;
        // (a clock runs from the one before it: the sort is buckets + scatter + ranks, the bands are heads + long ranges + emit)
        const double per = 1.0 / 100.0 / (double)h[7];
        fprintf(stderr, "[seed prof] %s, reads %llu: fill %.1f sort %.1f (buckets %.1f scatter %.1f ranks %.1f) bcov %.1f bands %.1f (heads %.1f long ranges %.1f emit %.1f) rank %.1f us/read; %llu reads through the network\n",
                row[t], h[7], h[0] * per, (h[5] + h[6] + h[1]) * per, h[5] * per, h[6] * per, h[1] * per, h[2] * per, (h[8] + h[9] + h[3]) * per,
                h[8] * per, h[9] * per, h[3] * per, h[4] * per, h[10]);
    }
    unsigned long long z[3][12] = {{0}};
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_seed_prof_all), z, sizeof(z));
}
#endif

// per-chunk summary of the seed filter's per-item results, so that the host fetches the per-item arrays only when it
// has to: out[0] = sum of hits, out[1] = sum of candidates, out[2] = items handed to the HBM variant (-1),
// out[3] = items the filter gave up on (-2)
extern "C" __global__ void __launch_bounds__(256)
k_seed_summary(const int32_t *__restrict__ ncand, const int32_t *__restrict__ nhits, int32_t n, unsigned long long *__restrict__ out)
{
    unsigned long long h = 0, c = 0, big = 0, gave = 0;
    for (int32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int32_t nc = ncand[i];
        h += (unsigned long long)max(nhits[i], 0);
        c += (unsigned long long)max(nc, 0);
        big += nc == -1 ? 1ull : 0ull;
        gave += nc == -2 ? 1ull : 0ull;
    }
    for (int off = 32; off > 0; off >>= 1) {
        h += __shfl_xor(h, off, 64);
        c += __shfl_xor(c, off, 64);
        big += __shfl_xor(big, off, 64);
        gave += __shfl_xor(gave, off, 64);
    }
    // one atomic per block and counter: per wavefront they were 16 000 returning-order atomics on four addresses for a
    // mapping chunk (2.7 ms for a kernel that reads 16 MB)
    __shared__ unsigned long long s_part[4][4];
    if ((threadIdx.x & 63) == 0) {
        s_part[threadIdx.x >> 6][0] = h;
        s_part[threadIdx.x >> 6][1] = c;
        s_part[threadIdx.x >> 6][2] = big;
        s_part[threadIdx.x >> 6][3] = gave;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const unsigned long long v = s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
        if (v) atomicAdd(&out[threadIdx.x], v);
    }
}

extern "C" void dhk_seed_summary(hipStream_t st, const int32_t *ncand, const int32_t *nhits, int32_t n, unsigned long long *out)
{
    (void)hipMemsetAsync(out, 0, 4 * sizeof(unsigned long long), st);
    if (n <= 0) return;
    hipLaunchKernelGGL(k_seed_summary, dim3(std::min((n + 255) / 256, 512)), dim3(256), 0, st, ncand, nhits, n, out);
}
