// dh_wave.hip -- the DH-1 alignment kernels (K5, K5b) for gfx950 (CDNA4, wave64).  DH-1 is algo = 0: the benchmarked
// path aligns with DH-2 (algo = 1, dh_tile.hip) and launches nothing from this file.
//
// K5   k_wave<SYM, PK>      per (B read, strand): O(ND) furthest-reaching wave, one 64-lane wavefront per alignment
//                           (lane == diagonal), trace points every tspace A-bases
// K5b  k_wave2<SYM, PK, G>  the same arithmetic with G = 32 or 16 lanes per alignment: two (width <= 30) or four
//                           (width <= 14) alignments per wavefront
// k_compact, which both of them (and DH-2) feed, is in dh_kernels.hip.
//
// The arithmetic specification is written down in DESIGN.md ("Algorithm DH-1"); reference call sites:
// source/dentist/dazzler.d:6121-6170.

#include <hip/hip_runtime.h>
#include <cstdlib>
#include <stdio.h>
#include <stdint.h>

#include "dh_device.h"

#define LANES 64

#include "dh_kmer.h"

// ------------------------------------------------------------------------------------ K5

// ballot straight from the compare (llvm.amdgcn.ballot): no bool -> int -> compare round trip
__device__ __forceinline__ unsigned long long wballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
// ---- wave64 primitives (verified on gfx950 by scripts/dpp_probe.cpp)
// value of lane-1 / lane+1 (rotation over the whole wave): one DPP mov each, no LDS crossbar
__device__ __forceinline__ int32_t from_lower_lane(int32_t v)
{
    return __builtin_amdgcn_mov_dpp(v, 0x13C, 0xF, 0xF, false);  // wave_ror:1, every lane has a source
}
__device__ __forceinline__ int32_t from_upper_lane(int32_t v)
{
    return __builtin_amdgcn_mov_dpp(v, 0x134, 0xF, 0xF, false);  // wave_rol:1
}
// max over the 64 lanes, result uniform: 4 DPP steps inside each row of 16, then 4 readlanes
__device__ __forceinline__ int32_t wave_max_i32(int32_t v)
{
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, false));  // row_half_mirror
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, false));  // row_mirror
    const int32_t r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int32_t r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return max(max(r0, r1), max(r2, r3));
}
// a wave-uniform global pointer pinned to an SGPR pair (explicit global address space so that
// the loads stay global_load with SGPR base + 32-bit VGPR offset)
typedef const __attribute__((address_space(1))) uint8_t *gptr_t;
struct __attribute__((packed)) PackedU64 {
    uint64_t v;
};
__device__ __forceinline__ gptr_t uniform_ptr(const uint8_t *p)
{
    const uint64_t v = (uint64_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (gptr_t)(((uint64_t)hi << 32) | lo);
}
__device__ __forceinline__ uint64_t load8g(gptr_t base, uint32_t off)
{
    return ((const __attribute__((address_space(1))) PackedU64 *)(base + off))->v;
}
// extend a run of matches: element i of A' is ap[i * step], 8 bases per compare.
// DB buffers carry 64 bytes of padding on both sides, so the wide loads stay inside them.
// lim = min(an, bn + k) bounds i on diagonal k.  ar/br = ap - an - 7 / bp - bn - 7 (reverse only):
// offsets are unsigned 32-bit values on wave-uniform bases.
template <int STEP>
__device__ __forceinline__ void slide(gptr_t ap, gptr_t ar, int32_t an, gptr_t bp, gptr_t br,
                                      int32_t bn, int32_t lim, int32_t &i, int32_t &j)
{
    for (;;) {
        const int32_t rem = lim - i;
        if (rem <= 0) break;
        int32_t m;
        if (STEP > 0) {
            const uint64_t x = load8g(ap, (uint32_t)i) ^ load8g(bp, (uint32_t)j);
            m = x ? ((__ffsll((long long)x) - 1) >> 3) : 8;
        } else {
            const uint64_t x = load8g(ar, (uint32_t)(an - i)) ^ load8g(br, (uint32_t)(bn - j));
            m = x ? (__clzll((long long)x) >> 3) : 8;
        }
        m = min(m, rem);
        i += m;
        j += m;
        if (m < 8) break;
    }
}

// The same on 2-bit packed sequences: 32 bases per 8-byte load.  Forward: element i of A' is
// base (4 * qa + ra + i) and pa points at byte qa; reverse: element i is base (4 * qa + ra - i),
// par points at byte qa - 7 - na4 and the window is the 32 bases ENDING at that base (na4 keeps
// the unsigned load offsets non-negative).  The window of a load starts at an arbitrary base of
// its first byte, so only 32 - max(phase) bases of a compare are valid.
template <int STEP>
__device__ __forceinline__ void slide_pk(gptr_t pa, int32_t ra, int32_t na4, gptr_t pb, int32_t rb,
                                         int32_t nb4, int32_t lim, int32_t &i, int32_t &j)
{
    for (;;) {
        const int32_t rem = lim - i;
        if (rem <= 0) break;
        int32_t m, valid;
        if (STEP > 0) {
            const int32_t ta = ra + i, tb = rb + j;
            const int32_t sa = (ta & 3) << 1, sb = (tb & 3) << 1;
            const uint64_t x = (load8g(pa, (uint32_t)ta >> 2) >> sa) ^ (load8g(pb, (uint32_t)tb >> 2) >> sb);
            valid = 32 - (max(sa, sb) >> 1);
            m = x ? ((__ffsll((long long)x) - 1) >> 1) : 32;
        } else {
            const int32_t ta = ra - i, tb = rb - j;
            const int32_t sa = (3 - (ta & 3)) << 1, sb = (3 - (tb & 3)) << 1;
            const uint64_t x = (load8g(pa, (uint32_t)((ta >> 2) + na4)) << sa) ^
                               (load8g(pb, (uint32_t)((tb >> 2) + nb4)) << sb);
            valid = 32 - (max(sa, sb) >> 1);
            m = x ? (__clzll((long long)x) >> 1) : 32;
        }
        m = min(min(m, valid), rem);
        i += m;
        j += m;
        if (m < valid) break;
    }
}

struct ExtResult {
    int32_t i, j, d, head, nb, headb, nbb;
};

// One-directional greedy extension by one wavefront; lane (k & 63) owns diagonal k.
// All lanes execute every cross-lane operation.  SYM additionally records the crossings of the
// B-offsets tpb_first + m*ts (value = i when j first reaches the boundary): the same path then
// also yields the trace of the transposed record (symmetric all-vs-all, each pair aligned once).
// PK: ap_ / bp_ are the 2-bit packed arrays and ag / bg the absolute base index of element 0
// (slide_pk); otherwise ap_ / bp_ point at element 0 of the byte arrays.
template <int STEP, bool SYM, bool PK>
__device__ ExtResult ext_wave(const uint8_t *ap_, int64_t ag, int32_t an, const uint8_t *bp_, int64_t bg,
                              int32_t bn, int32_t tp_first,
                              int32_t tpb_first, const DhOpts &o, DhNode *__restrict__ pool,
                              int32_t poolcap, int32_t &pool_n, unsigned long long &cells,
                              int32_t &err)
{
    const int lane = threadIdx.x & (LANES - 1);
    const int32_t ts = o.tspace, pen = o.pen, xdrop = o.xdrop;
    an = __builtin_amdgcn_readfirstlane(an);
    bn = __builtin_amdgcn_readfirstlane(bn);
    // byte arrays: forward base ap / bp, reverse base ar / br (slide); packed: one base per
    // direction in ap / bp plus the phases ra / rb and the offset biases na4 / nb4 (slide_pk)
    const int32_t ra = PK ? __builtin_amdgcn_readfirstlane((int32_t)(ag & 3)) : 0;
    const int32_t rb = PK ? __builtin_amdgcn_readfirstlane((int32_t)(bg & 3)) : 0;
    const int32_t na4 = (PK && STEP < 0) ? (an >> 2) + 2 : 0, nb4 = (PK && STEP < 0) ? (bn >> 2) + 2 : 0;
    const gptr_t ap = uniform_ptr(PK ? ap_ + (ag >> 2) - (STEP < 0 ? 7 + na4 : 0) : ap_);
    const gptr_t bp = uniform_ptr(PK ? bp_ + (bg >> 2) - (STEP < 0 ? 7 + nb4 : 0) : bp_);
    const gptr_t ar = uniform_ptr(PK ? ap_ : ap_ - an - 7), br = uniform_ptr(PK ? bp_ : bp_ - bn - 7);
    tp_first = __builtin_amdgcn_readfirstlane(tp_first);
    tpb_first = __builtin_amdgcn_readfirstlane(tpb_first);
    // per-lane state of diagonal k: R = furthest i (DEAD when dead), H = head of its trace chain,
    // NB = the first trace boundary above R (tp_first + #boundaries * ts, carried along so that the
    // loop needs neither a division nor a multiplication); HB / NBB the same for the B-offset
    // boundaries (SYM only)
    constexpr int32_t DEAD = -(1 << 30);
    int32_t R = DEAD, H = -1, NB = tp_first, HB = -1, NBB = tpb_first;
    int32_t L = 0;

    // d = 0: the seed diagonal, slid by lane 0
    int32_t i0 = 0, h0 = -1, nb0 = 0, hb0 = -1, nbb0 = 0;
    if (lane == 0) {
        int32_t j0 = 0;
        if (PK)
            slide_pk<STEP>(ap, ra, na4, bp, rb, nb4, min(an, bn), i0, j0);
        else
            slide<STEP>(ap, ar, an, bp, br, bn, min(an, bn), i0, j0);
        int32_t cnt = 0;
        for (int32_t nextb = tp_first; nextb <= i0; nextb += ts) {
            const int32_t idx = pool_n + cnt;
            if (idx < poolcap) {
                pool[idx].parent = h0;
                pool[idx].d = 0;
                pool[idx].j = nextb;
            }
            h0 = idx;
            nb0++;
            cnt++;
        }
        if (SYM)
            for (int32_t nextb = tpb_first; nextb <= i0; nextb += ts) {
                const int32_t idx = pool_n + cnt;
                if (idx < poolcap) {
                    pool[idx].parent = hb0;
                    pool[idx].d = 0;
                    pool[idx].j = nextb;
                }
                hb0 = idx;
                nbb0++;
                cnt++;
            }
        R = i0;
        H = h0;
        NB = tp_first + nb0 * ts;
        HB = hb0;
        NBB = tpb_first + nbb0 * ts;
    }
    // wave-uniform values are pinned to SGPRs (readfirstlane) so that the window arithmetic,
    // mask rotations and find-first-set below run on the scalar unit
    i0 = __builtin_amdgcn_readfirstlane(i0);
    h0 = __builtin_amdgcn_readfirstlane(h0);
    nb0 = __builtin_amdgcn_readfirstlane(nb0);
    hb0 = __builtin_amdgcn_readfirstlane(hb0);
    nbb0 = __builtin_amdgcn_readfirstlane(nbb0);
    pool_n = __builtin_amdgcn_readfirstlane(pool_n + nb0 + nbb0);
    int32_t best_score = 2 * i0, best_i = i0, best_k = 0, best_d = 0, best_head = h0;
    int32_t best_nb = tp_first + nb0 * ts, best_headb = hb0, best_nbb = tpb_first + nbb0 * ts;
    unsigned long long ncell = 1;

    for (int32_t d = 1; d <= o.dmax; d++) {
        const int32_t nL = L - 1;
        const int32_t kidx = (lane - nL) & (LANES - 1);
        const int32_t k = nL + kidx;
        const int32_t Rm = from_lower_lane(R), Hm = from_lower_lane(H), Nm = from_lower_lane(NB);
        const int32_t Rp = from_upper_lane(R), Hp = from_upper_lane(H), Np = from_upper_lane(NB);
        int32_t HBm = -1, NBm = tpb_first, HBp = -1, NBp = tpb_first;
        if (SYM) {
            HBm = from_lower_lane(HB);
            NBm = from_lower_lane(NBB);
            HBp = from_upper_lane(HB);
            NBp = from_upper_lane(NBB);
        }
        // substitution on k, deletion from k-1 (consumes A), insertion from k+1 (consumes B); ties
        // prefer sub, then del.  Dead diagonals carry R = DEAD (very negative), so a candidate from
        // a dead source never beats ni = -1; sources are valid points, hence j >= 0 holds for all
        // three moves and only i <= an, j <= bn (i <= lim) has to be checked.  Lanes outside the
        // window see dead sources only (width <= 62) and stay dead.
        int32_t ni = -1, hd = -1, nbp = tp_first, hb = -1, nbbp = tpb_first;
        const int32_t lim = min(an, bn + k);  // i <= an and i - k <= bn
        {
            const int32_t cs = R + 1, cd = Rm + 1, ci = Rp;
            if (cs <= lim && cs > ni) {
                ni = cs;
                hd = H;
                nbp = NB;
                hb = HB;
                nbbp = NBB;
            }
            if (cd <= lim && cd > ni) {
                ni = cd;
                hd = Hm;
                nbp = Nm;
                hb = HBm;
                nbbp = NBm;
            }
            if (ci <= lim && ci > ni) {
                ni = ci;
                hd = Hp;
                nbp = Np;
                hb = HBp;
                nbbp = NBp;
            }
        }
        bool alive = ni >= 0;
        int32_t j = ni - k;
        if (alive) {
            if (PK)
                slide_pk<STEP>(ap, ra, na4, bp, rb, nb4, lim, ni, j);
            else
                slide<STEP>(ap, ar, an, bp, br, bn, lim, ni, j);
        }
        const unsigned long long amask = wballot(alive);
        if (amask == 0ull) break;
        ncell += __popcll(amask);
        // trace nodes for the boundaries crossed in (prev_i, ni]: nbp is the first one above prev_i
        int32_t nextb = nbp;
        bool cross = alive && ni >= nextb;
        for (;;) {
            const unsigned long long m = wballot(cross);
            if (m == 0ull) break;
            if (cross) {
                const int32_t idx = pool_n + __popcll(m & ((1ull << lane) - 1ull));
                if (idx < poolcap) {
                    pool[idx].parent = hd;
                    pool[idx].d = d;
                    pool[idx].j = nextb - k;
                }
                hd = idx;
                nextb += ts;
                cross = ni >= nextb;
            }
            pool_n = __builtin_amdgcn_readfirstlane(pool_n + __popcll(m));
        }
        int32_t nextbb_out = nbbp;
        if (SYM) {
            int32_t nextbb = nbbp;
            bool crossb = alive && j >= nextbb;
            for (;;) {
                const unsigned long long m = wballot(crossb);
                if (m == 0ull) break;
                if (crossb) {
                    const int32_t idx = pool_n + __popcll(m & ((1ull << lane) - 1ull));
                    if (idx < poolcap) {
                        pool[idx].parent = hb;
                        pool[idx].d = d;
                        pool[idx].j = nextbb + k;
                    }
                    hb = idx;
                    nextbb += ts;
                    crossb = j >= nextbb;
                }
                pool_n = __builtin_amdgcn_readfirstlane(pool_n + __popcll(m));
            }
            nextbb_out = nextbb;
        }
        if (pool_n > poolcap) {
            err |= DH_ST_POOL_OVERFLOW;
            break;
        }
        R = alive ? ni : DEAD;
        H = hd;
        NB = nextb;
        HB = hb;
        NBB = SYM ? nextbb_out : NBB;
        // best of this step: highest score, then lowest diagonal (ballot of the max holders,
        // rotated so that bit x is diagonal nL + x)
        const int32_t sc = alive ? 2 * ni - k - pen * d : INT32_MIN;
        const int32_t step_best = wave_max_i32(sc);
        const int rot = nL & (LANES - 1);
        if (step_best > best_score) {
            const unsigned long long hm = wballot(alive && sc == step_best);
            const unsigned long long hr = rot ? ((hm >> rot) | (hm << (LANES - rot))) : hm;
            const int32_t step_kidx = __ffsll((long long)hr) - 1;
            const int src = __builtin_amdgcn_readfirstlane((nL + step_kidx) & (LANES - 1));
            best_score = step_best;
            best_k = nL + step_kidx;
            best_i = __builtin_amdgcn_readlane(R, src);
            best_head = __builtin_amdgcn_readlane(H, src);
            best_nb = __builtin_amdgcn_readlane(NB, src);
            if (SYM) {
                best_headb = __builtin_amdgcn_readlane(HB, src);
                best_nbb = __builtin_amdgcn_readlane(NBB, src);
            }
            best_d = d;
        }
        // trim to xdrop of the best
        if (alive && sc < best_score - xdrop) {
            alive = false;
            R = DEAD;
        }
        unsigned long long lm = wballot(alive);
        if (lm == 0ull) break;
        unsigned long long rm = rot ? ((lm >> rot) | (lm << (LANES - rot))) : lm;
        int32_t l2 = __builtin_amdgcn_readfirstlane(nL + (__ffsll((long long)rm) - 1));
        int32_t u2 = __builtin_amdgcn_readfirstlane(nL + (63 - __clzll((long long)rm)));
        while (u2 - l2 + 1 > o.width) {
            // drop the lower-scoring edge (same d: compare 2R - k), ties drop the low edge
            const int32_t val = 2 * R - k;
            const int32_t sl = __builtin_amdgcn_readlane(val, l2 & (LANES - 1));
            const int32_t su = __builtin_amdgcn_readlane(val, u2 & (LANES - 1));
            const int32_t kill = sl <= su ? l2 : u2;
            if (k == kill) {
                alive = false;
                R = DEAD;
            }
            lm = wballot(alive);
            rm = rot ? ((lm >> rot) | (lm << (LANES - rot))) : lm;
            l2 = __builtin_amdgcn_readfirstlane(nL + (__ffsll((long long)rm) - 1));
            u2 = __builtin_amdgcn_readfirstlane(nL + (63 - __clzll((long long)rm)));
        }
        L = l2;
    }
    cells += ncell;
    ExtResult res;
    res.i = best_i;
    res.j = best_i - best_k;
    res.d = best_d;
    res.head = best_head;
    res.nb = (best_nb - tp_first) / ts;
    res.headb = best_headb;
    res.nbb = SYM ? (best_nbb - tpb_first) / ts : 0;
    return res;
}

// walk a trace chain (serial, one lane); writes cd/cj[m], returns diagonal excursion
__device__ void walk_chain(const DhNode *__restrict__ pool, int32_t head, int32_t nb,
                           int32_t tp_first, int32_t ts, int32_t best_k, int32_t *cd, int32_t *cj,
                           int32_t &lo, int32_t &hi)
{
    lo = best_k < 0 ? best_k : 0;
    hi = best_k > 0 ? best_k : 0;
    int32_t h = head;
    for (int32_t m = nb - 1; m >= 0 && h >= 0; m--) {
        const DhNode nd = pool[h];
        cd[m] = nd.d;
        cj[m] = nd.j;
        const int32_t kk = (tp_first + m * ts) - nd.j;
        lo = kk < lo ? kk : lo;
        hi = kk > hi ? kk : hi;
        h = nd.parent;
    }
}

// the pairs (delta diffs, delta other) of a trace between consecutive grid boundaries, written by
// the whole wavefront.  grid = the coordinate the trace spacing refers to (boundaries at
// grid = res mod ts), other = the opposite sequence; gs/os = seed on the two axes; rd/ro, fd/fo =
// boundary records of the reverse / forward extension (diffs, offset on `other`).  `reverse`
// writes the pairs back to front (transposed record of a complemented alignment).
__device__ int32_t emit_trace(int lane, int stride, int32_t ts, int32_t res, int32_t gs, int32_t os,
                              int32_t gbeg, int32_t gend, int32_t obeg, int32_t oend, int32_t rdv,
                              int32_t fdv, int32_t rev_first, int32_t nr, const int32_t *rd,
                              const int32_t *ro, int32_t fwd_first, int32_t nf, const int32_t *fd,
                              const int32_t *fo, bool reverse, uint16_t *__restrict__ tr)
{
    const int32_t nrv = nr - ((nr > 0 && rev_first + (nr - 1) * ts == gs - gbeg) ? 1 : 0);
    const int32_t nfv = nf - ((nf > 0 && fwd_first + (nf - 1) * ts == gend - gs) ? 1 : 0);
    int32_t gm = (gs - res) % ts;
    gm = gm < 0 ? gm + ts : gm;
    const int32_t seedb = (gm == 0 && gs > gbeg && gs < gend) ? 1 : 0;
    // (a zero-length alignment -- two empty extensions, kept at min_len 0 -- has no pair at all, as in the oracle)
    const int32_t npairs = nrv + seedb + nfv + (gend > gbeg ? 1 : 0);
    for (int32_t e = lane; e < npairs; e += stride) {
        int32_t po[2], pD[2];
#pragma unroll
        for (int w = 0; w < 2; w++) {
            const int32_t idx = e + w;
            if (idx == 0) {
                po[w] = obeg;
                pD[w] = -rdv;
            } else if (idx <= nrv) {
                const int32_t m = nrv - idx;
                po[w] = os - ro[m];
                pD[w] = -rd[m];
            } else if (idx <= nrv + seedb) {
                po[w] = os;
                pD[w] = 0;
            } else if (idx <= nrv + seedb + nfv) {
                const int32_t m = idx - 1 - nrv - seedb;
                po[w] = os + fo[m];
                pD[w] = fd[m];
            } else {
                po[w] = oend;
                pD[w] = fdv;
            }
        }
        const int32_t pos = reverse ? npairs - 1 - e : e;
        tr[2 * pos] = (uint16_t)(pD[1] - pD[0]);
        tr[2 * pos + 1] = (uint16_t)(po[1] - po[0]);
    }
    return npairs;
}

// SYM (all-vs-all inside one DB, skip_self == 2): each unordered pair has candidates in one item only; every
// accepted alignment emits the record (a, b) into the slots of item (a, strand) and the transposed
// record (b, a) into the slots of item (b, strand); slots are claimed with atomics because any
// wavefront may add records to any item (the final LAsort makes the output order unique).
// PK: the wave slides over the 2-bit packed copies apk (A), bpk / brcpk (B, B reverse-complemented)
template <bool SYM, bool PK>
__global__ void __launch_bounds__(LANES)
k_wave(DbView A, DbView B, const uint8_t *__restrict__ brc, const uint8_t *__restrict__ apk,
       const uint8_t *__restrict__ bpk, const uint8_t *__restrict__ brcpk, DhOpts o, int32_t item0,
       int32_t nitems, const DhCand *__restrict__ cand, const int32_t *__restrict__ ncand,
       WaveScratch ws, DhLa *__restrict__ out_la, uint16_t *__restrict__ out_trace,
       int32_t trmax, int32_t *__restrict__ out_nla, int32_t *__restrict__ out_ntr,
       unsigned long long *__restrict__ counters,
       int32_t *__restrict__ status)
{
    const int lane = threadIdx.x;
    DhNode *pool = ws.pool + (int64_t)blockIdx.x * ws.poolcap;
    int32_t *cdj = ws.cdj + (int64_t)blockIdx.x * 8 * ws.nbmax;
    int32_t *fd = cdj, *fj = cdj + ws.nbmax, *rd = cdj + 2 * ws.nbmax, *rj = cdj + 3 * ws.nbmax;
    int32_t *fdb = cdj + 4 * ws.nbmax, *fib = cdj + 5 * ws.nbmax, *rdb = cdj + 6 * ws.nbmax,
            *rib = cdj + 7 * ws.nbmax;
    const int32_t ts = o.tspace;
    unsigned long long cells = 0, naln = 0;
    int32_t err = 0;

    for (;;) {
        int32_t it = 0;
        if (lane == 0) it = (int32_t)atomicAdd(ws.queue, 1u);
        it = __builtin_amdgcn_readfirstlane(it);
        if (it >= (ws.units ? (int32_t)*ws.nunits : nitems)) break;
        // work unit: a whole item, or (symmetric mode) one group of candidates of an item
        int32_t c0 = 0, c1 = INT32_MAX, ui = it;
        if (ws.units) {
            const int4 u = ws.units[it];
            ui = u.x;
            c0 = u.y;
            c1 = u.z;
        }
        const int32_t item = item0 + ui;
        const int32_t r = item >> 1, strand = item & 1;
        const int32_t nc = min(max(ncand[item], 0), c1);
        const int64_t bo = B.off[r];
        const int32_t blen = (int32_t)(B.off[r + 1] - bo);
        const uint8_t *b = (strand ? brc : B.bases) + bo;
        // regions already aligned for this (read, strand): kept in registers of lanes 0..nd-1
        int32_t g_aseq = -1, g_ab = 0, g_ae = 0, g_bb = 0, g_be = 0, g_lo = 0, g_hi = 0;
        int32_t nd = 0, nacc = 0, ntr = 0;
        for (int32_t c = c0; c < nc && (SYM || nacc < o.max_la) && nd < LANES; c++) {
            const DhCand cd = cand[(int64_t)item * o.max_cand + c];
            const int32_t sd = cd.apos - cd.bpos;
            const bool cov = lane < nd && g_aseq == cd.aseq && cd.apos >= g_ab && cd.apos < g_ae &&
                             cd.bpos >= g_bb && cd.bpos < g_be && sd >= g_lo - 64 && sd <= g_hi + 64;
            if (wballot(cov) != 0ull) continue;
            const int64_t ao = A.off[cd.aseq];
            const int32_t alen = (int32_t)(A.off[cd.aseq + 1] - ao);
            const uint8_t *a = A.bases + ao;
            const int32_t as = cd.apos, bs = cd.bpos;
            const int32_t fwd_first = ts - (as % ts);
            const int32_t rev_first = (as % ts) ? (as % ts) : ts;
            // B grid of the transposed record: forward strand of the read behind B
            const int32_t resb = strand ? blen % ts : 0;
            int32_t bm = (bs - resb) % ts;
            bm = bm < 0 ? bm + ts : bm;
            const int32_t fwdb_first = ts - bm, revb_first = bm ? bm : ts;
            int32_t pool_n = 0;
            const uint8_t *bsrc = PK ? (strand ? brcpk : bpk) : b;
            const ExtResult fw = ext_wave<1, SYM, PK>(PK ? apk : a + as, ao + as, alen - as,
                                                      PK ? bsrc : b + bs, bo + bs, blen - bs, fwd_first,
                                                      fwdb_first, o, pool, ws.poolcap, pool_n, cells, err);
            const ExtResult rv = ext_wave<-1, SYM, PK>(PK ? apk : a + as - 1, ao + as - 1, as,
                                                       PK ? bsrc : b + bs - 1, bo + bs - 1, bs, rev_first,
                                                       revb_first, o, pool, ws.poolcap, pool_n, cells, err);
            naln++;
            if (err || fw.nb > ws.nbmax || rv.nb > ws.nbmax || fw.nbb > ws.nbmax || rv.nbb > ws.nbmax) {
                err |= DH_ST_POOL_OVERFLOW;
                break;
            }
            // chains: lanes 0..3 walk the forward / reverse chains of the two boundary families
            int32_t flo = 0, fhi = 0, rlo = 0, rhi = 0;
            if (lane == 0)
                walk_chain(pool, fw.head, fw.nb, fwd_first, ts, fw.i - fw.j, fd, fj, flo, fhi);
            if (lane == 1)
                walk_chain(pool, rv.head, rv.nb, rev_first, ts, rv.i - rv.j, rd, rj, rlo, rhi);
            if (SYM) {
                int32_t x0, x1;
                if (lane == 2) walk_chain(pool, fw.headb, fw.nbb, fwdb_first, ts, 0, fdb, fib, x0, x1);
                if (lane == 3) walk_chain(pool, rv.headb, rv.nbb, revb_first, ts, 0, rdb, rib, x0, x1);
            }
            __threadfence_block();
            flo = __shfl(flo, 0, LANES);
            fhi = __shfl(fhi, 0, LANES);
            rlo = __shfl(rlo, 1, LANES);
            rhi = __shfl(rhi, 1, LANES);
            const int32_t abpos = as - rv.i, bbpos = bs - rv.j, aepos = as + fw.i, bepos = bs + fw.j;
            const int32_t diffs = fw.d + rv.d;
            int32_t lo = sd + flo, hi = sd + fhi;
            lo = (sd - rhi) < lo ? (sd - rhi) : lo;
            hi = (sd - rlo) > hi ? (sd - rlo) : hi;
            if (lane == nd) {
                g_aseq = cd.aseq;
                g_ab = abpos;
                g_ae = aepos;
                g_bb = bbpos;
                g_be = bepos;
                g_lo = lo;
                g_hi = hi;
            }
            nd++;
            const int64_t al = aepos - abpos, bl = bepos - bbpos;
            const bool accept = al >= o.min_len &&
                                (int64_t)2 * diffs * 1000000ll <= (int64_t)o.max_err_ppm * (al + bl);
            if (!accept) continue;
            // ---- the record (a, b): trace on the grid of A.  SYM: it goes to the slots of item
            // (a, strand) and the transposed record to those of (b, strand), so that the output
            // is grouped by A read.
            const int32_t item_a = SYM ? 2 * cd.aseq + strand : item;
            int32_t s1 = nacc;
            if (SYM) {
                if (lane == 0) s1 = atomicAdd(&out_nla[item_a], 1);
                s1 = __shfl(s1, 0, LANES);
                if (s1 >= o.max_la) {  // more overlaps than slots: drop the pair, report both items
                    if (lane == 0) {
                        atomicSub(&out_nla[item_a], 1);
                        ws.item_ovf[item_a] = 1;
                        ws.item_ovf[item] = 1;
                    }
                    continue;
                }
            }
            const int64_t slot = (int64_t)item_a * o.max_la + s1;
            const int32_t npairs = emit_trace(lane, LANES, ts, 0, as, bs, abpos, aepos, bbpos, bepos, rv.d, fw.d,
                                              rev_first, rv.nb, rd, rj, fwd_first, fw.nb, fd, fj, false,
                                              out_trace + slot * trmax);
            if (lane == 0) {
                DhLa la;
                la.tlen = 2 * npairs;
                la.diffs = diffs;
                la.abpos = abpos;
                la.bbpos = bbpos;
                la.aepos = aepos;
                la.bepos = bepos;
                la.flags = strand ? 1u : 0u;
                la.aread = cd.aseq;
                la.bread = r;
                la.pad = 0;
                la.toff = 0;
                out_la[slot] = la;
                if (SYM) atomicAdd(&out_ntr[item_a], 2 * npairs);
            }
            nacc++;
            ntr += 2 * npairs;
            if (SYM) {
                // ---- the transposed record (b, a): same path, trace on the grid of B
                const int32_t item2 = item;
                int32_t s2 = 0;
                if (lane == 0) s2 = atomicAdd(&out_nla[item2], 1);
                s2 = __shfl(s2, 0, LANES);
                if (s2 >= o.max_la) {
                    if (lane == 0) {
                        atomicSub(&out_nla[item2], 1);
                        ws.item_ovf[item2] = 1;
                        ws.item_ovf[item_a] = 1;
                    }
                    continue;
                }
                const int64_t slot2 = (int64_t)item2 * o.max_la + s2;
                const int32_t np2 = emit_trace(lane, LANES, ts, resb, bs, as, bbpos, bepos, abpos, aepos, rv.d, fw.d,
                                               revb_first, rv.nbb, rdb, rib, fwdb_first, fw.nbb, fdb, fib,
                                               strand != 0, out_trace + slot2 * trmax);
                if (lane == 0) {
                    DhLa la;
                    la.tlen = 2 * np2;
                    la.diffs = diffs;
                    la.abpos = strand ? blen - bepos : bbpos;
                    la.aepos = strand ? blen - bbpos : bepos;
                    la.bbpos = strand ? alen - aepos : abpos;
                    la.bepos = strand ? alen - abpos : aepos;
                    la.flags = strand ? 1u : 0u;
                    la.aread = r;
                    la.bread = cd.aseq;
                    la.pad = 0;
                    la.toff = 0;
                    out_la[slot2] = la;
                    atomicAdd(&out_ntr[item2], 2 * np2);
                }
            }
        }
        if (!SYM && lane == 0) {
            out_nla[item] = nacc;
            out_ntr[item] = ntr;
        }
        if (err) break;
    }
    if (lane == 0) {
        atomicAdd(&counters[0], cells);
        atomicAdd(&counters[1], naln);
        if (err) atomicOr(status, err);
    }
}

// ------------------------------------------------------------------------------------ K5b
//
// k_wave2: two alignments per wavefront.  On average only ~19 of the 64 diagonals of a wavefront
// are alive and the kernel is bound by VALU issue, so with a wave width of at most 30 diagonals
// (DhOpts.width <= 30) each 32-lane half runs its own alignment: lane (k & 31) of a half owns
// diagonal k.  The halves are independent state machines sharing one instruction stream -- a half
// that finishes an extension runs its bookkeeping (next candidate, chains, trace, records, next
// item) while the other half keeps stepping -- and everything that is wave-uniform in k_wave is
// half-uniform here (kept per lane, broadcast with readlane pairs / ds_bpermute, ballots split
// into their 32-bit halves).  Reverse extensions are forward extensions over the
// reverse-complemented copies, so both halves always run the same slide code.
// The arithmetic is that of ext_wave / k_wave, bit for bit.

enum { W2_FETCH = 0, W2_CAND = 1, W2_EXT = 2, W2_EXT_END = 3, W2_DONE = 4, W2_POST_CHAIN = 5, W2_POST_REC1 = 6,
       W2_POST_REC2 = 7 };

// G lanes per alignment (32: two per wavefront, 16: four); hb = first lane of my group
template <int G>
__device__ __forceinline__ uint32_t hballot(bool p, int hb)
{
    const uint64_t m = wballot(p);
    if (G == 32) return hb ? (uint32_t)(m >> 32) : (uint32_t)m;
    return (uint32_t)(m >> hb) & 0xFFFFu;
}
// value of lane `l` (constant) of my group
template <int G, int L>
__device__ __forceinline__ int32_t hlane(int32_t v, int hb)
{
    if (G == 32) {
        const int32_t a = __builtin_amdgcn_readlane(v, L), b = __builtin_amdgcn_readlane(v, 32 + L);
        return hb ? b : a;
    }
    // four groups: one trip through the LDS crossbar (the group's lanes are all active wherever this
    // is used) instead of four readlanes and three selects
    return __builtin_amdgcn_ds_bpermute((hb | L) << 2, v);
}
// value of lane l (group-uniform, 0..G-1) of my group; every lane of the group must be active
__device__ __forceinline__ int32_t hread(int32_t v, int32_t l, int hb)
{
    return __builtin_amdgcn_ds_bpermute((hb | l) << 2, v);
}
// the same for the serial edge trimming.  Two groups: two readlanes per group on scalar indices
// (no LDS crossbar round trip on the critical path); four groups: the crossbar after all (eight
// readlanes plus selects cost more issue slots than the round trip costs latency)
template <int G>
__device__ __forceinline__ int32_t hread_fast(int32_t v, int32_t l, int hb)
{
    if (G == 32) {
        const int32_t l0 = __builtin_amdgcn_readlane(l, 0) & 31, l1 = __builtin_amdgcn_readlane(l, 32) & 31;
        const int32_t a = __builtin_amdgcn_readlane(v, l0), b = __builtin_amdgcn_readlane(v, 32 + l1);
        return hb ? b : a;
    }
    return __builtin_amdgcn_ds_bpermute((hb | (l & 15)) << 2, v);
}
// max over the G lanes of my group
template <int G>
__device__ __forceinline__ int32_t hmax_i32(int32_t v, int hb)
{
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x141, 0xF, 0xF, true));
    v = max(v, __builtin_amdgcn_mov_dpp(v, 0x140, 0xF, 0xF, true));
    if (G == 16) return v;  // a DPP row is a group: every lane holds its row's maximum
    const int32_t r0 = __builtin_amdgcn_readlane(v, 0), r1 = __builtin_amdgcn_readlane(v, 16);
    const int32_t r2 = __builtin_amdgcn_readlane(v, 32), r3 = __builtin_amdgcn_readlane(v, 48);
    return hb ? max(r2, r3) : max(r0, r1);
}
// rotate the G-bit group mask right by r (0 <= r < G)
template <int G>
__device__ __forceinline__ uint32_t hrotr(uint32_t x, uint32_t r)
{
    if (G == 32) return __builtin_rotateright32(x, r);
    return ((x | (x << 16)) >> r) & 0xFFFFu;
}
// forward slide with per-lane base pointers (bytes: p + i; packed: base index 4 * q + r + i,
// p points at byte q)
template <bool PK>
__device__ __forceinline__ void slide2(const uint8_t *pa, int32_t ra, const uint8_t *pb, int32_t rb,
                                       int32_t lim, int32_t &i, int32_t &j)
{
    for (;;) {
        const int32_t rem = lim - i;
        if (rem <= 0) break;
        int32_t m, valid;
        if (PK) {
            const int32_t ta = ra + i, tb = rb + j;
            const int32_t sa = (ta & 3) << 1, sb = (tb & 3) << 1;
            const uint64_t x = (load8(pa + ((uint32_t)ta >> 2)) >> sa) ^ (load8(pb + ((uint32_t)tb >> 2)) >> sb);
            valid = 32 - (max(sa, sb) >> 1);
            m = x ? ((__ffsll((long long)x) - 1) >> 1) : 32;
        } else {
            const uint64_t x = load8(pa + (uint32_t)i) ^ load8(pb + (uint32_t)j);
            valid = 8;
            m = x ? ((__ffsll((long long)x) - 1) >> 3) : 8;
        }
        m = min(min(m, valid), rem);
        i += m;
        j += m;
        if (m < valid) break;
    }
}

struct W2Cold {
    int32_t item, r, strand, nc, c, blen, nd, nacc, ntr;
    int32_t c_aseq, as, bs, alen, sd;
    int32_t fwd_first, rev_first, fwdb_first, revb_first, resb;
    int64_t bo, ao;
    int32_t fw_i, fw_j, fw_d, fw_head, fw_nb, fw_headb, fw_nbb;
    int32_t rv_i, rv_j, rv_d, rv_head, rv_nb, rv_headb, rv_nbb;
    int32_t abpos, bbpos, aepos, bepos, diffs;
    unsigned long long cells, naln;
};

template <bool SYM, bool PK, int G>
__global__ void __launch_bounds__(LANES, G == 16 ? 5 : 6)  // G = 32: 80 VGPRs, measured best of 4 / 5 / 6 / 8 waves per SIMD
k_wave2(DbView A, DbView B, const uint8_t *__restrict__ arc, const uint8_t *__restrict__ brc,
        const uint8_t *__restrict__ apk, const uint8_t *__restrict__ arcpk,
        const uint8_t *__restrict__ bpk, const uint8_t *__restrict__ brcpk, DhOpts o, int32_t item0,
        int32_t nitems, const DhCand *__restrict__ cand, const int32_t *__restrict__ ncand,
        WaveScratch ws, DhLa *__restrict__ out_la, uint16_t *__restrict__ out_trace,
        int32_t trmax, int32_t *__restrict__ out_nla, int32_t *__restrict__ out_ntr,
        unsigned long long *__restrict__ counters, int32_t *__restrict__ status)
{
    constexpr int NG = LANES / G;  // alignments per wavefront
    const int lane = threadIdx.x, hl = lane & (G - 1), hb = lane & (LANES - G), grp = lane / G;
    const int64_t slot = (int64_t)blockIdx.x * NG + grp;
    DhNode *pool = ws.pool + slot * ws.poolcap;
    // every lane pushes its trace nodes into its own stretch of the slot's pool (node = lbase + pn):
    // no ballot / prefix count per boundary crossing, and a level on which nothing crosses costs
    // one compare per family
    const int32_t ts = o.tspace, pen = o.pen, xdrop = o.xdrop, lanecap = ws.poolcap / G, lbase = hl * lanecap;
    const int32_t addr_lo = (hb | ((hl - 1) & (G - 1))) << 2, addr_hi = (hb | ((hl + 1) & (G - 1))) << 2;
    constexpr int32_t DEAD = -(1 << 30);

    int32_t st = W2_FETCH, err = 0;
    // ---- cold state of the half (item, candidate, results, counters): half-uniform values that
    // only the bookkeeping touches live in LDS (every lane of the half writes the same value), so
    // that the stepping loop keeps its registers -- two alignments per wavefront at 8 waves/SIMD
    __shared__ W2Cold cold_[NG];
    __shared__ int32_t greg_[NG][7 * NG][G];  // regions already aligned: region x in lane x % G, set x / G
    W2Cold &cs = cold_[grp];
    int32_t(*gr)[G] = greg_[grp];
    cs.cells = 0;
    cs.naln = 0;
    // ---- the running extension (hot)
    int32_t dir = 0, ra = 0, rb = 0, an = 0, bn = 0, tp_first = 0, tpb_first = 0;
    const uint8_t *pa = nullptr, *pb = nullptr;
    int32_t R = DEAD, H = -1, NB = 0, HB = -1, NBB = 0;  // per lane
    int32_t L = 0, d = 0, pn = 0;  // pn: nodes of this lane (per candidate, both extensions)
    int32_t best_score = 0, best_i = 0, best_k = 0, best_d = 0, best_head = -1, best_nb = 0, best_headb = -1,
            best_nbb = 0;
    uint32_t ncell = 0;

    // start the extension `dir` (0 forward, 1 reverse) of the current candidate
    auto ext_begin = [&](int32_t nd_) {
        dir = nd_;
        // reverse = forward over the reverse complements: base (len - pos) of the rc copy
        const int32_t as = cs.as, bs = cs.bs, alen = cs.alen, blen = cs.blen;
        const int64_t ga = cs.ao + (dir ? alen - as : as), gb = cs.bo + (dir ? blen - bs : bs);
        an = dir ? as : alen - as;
        bn = dir ? bs : blen - bs;
        const bool brc_side = (cs.strand != 0) != (dir != 0);
        if (PK) {
            pa = (dir ? arcpk : apk) + (ga >> 2);
            pb = (brc_side ? brcpk : bpk) + (gb >> 2);
            ra = (int32_t)(ga & 3);
            rb = (int32_t)(gb & 3);
        } else {
            pa = (dir ? arc : A.bases) + ga;
            pb = (brc_side ? brc : B.bases) + gb;
            ra = rb = 0;
        }
        tp_first = dir ? cs.rev_first : cs.fwd_first;
        tpb_first = dir ? cs.revb_first : cs.fwdb_first;
        R = DEAD;
        H = -1;
        NB = tp_first;
        HB = -1;
        NBB = tpb_first;
        L = 0;
        // d = 0: the seed diagonal, slid by lane 0 of the half
        int32_t i0 = 0, h0 = -1, nb0 = 0, hb0 = -1, nbb0 = 0;
        if (hl == 0) {
            int32_t j0 = 0;
            slide2<PK>(pa, ra, pb, rb, min(an, bn), i0, j0);
            int32_t cnt = 0;
            for (int32_t nextb = tp_first; nextb <= i0; nextb += ts) {
                const int32_t idx = lbase + pn + cnt;
                if (pn + cnt < lanecap) {
                    pool[idx].parent = h0;
                    pool[idx].d = 0;
                    pool[idx].j = nextb;
                }
                h0 = idx;
                nb0++;
                cnt++;
            }
            if (SYM)
                for (int32_t nextb = tpb_first; nextb <= i0; nextb += ts) {
                    const int32_t idx = lbase + pn + cnt;
                    if (pn + cnt < lanecap) {
                        pool[idx].parent = hb0;
                        pool[idx].d = 0;
                        pool[idx].j = nextb;
                    }
                    hb0 = idx;
                    nbb0++;
                    cnt++;
                }
            R = i0;
            H = h0;
            NB = tp_first + nb0 * ts;
            HB = hb0;
            NBB = tpb_first + nbb0 * ts;
            pn += cnt;
        }
        i0 = hlane<G, 0>(i0, hb);
        h0 = hlane<G, 0>(h0, hb);
        nb0 = hlane<G, 0>(nb0, hb);
        hb0 = hlane<G, 0>(hb0, hb);
        nbb0 = hlane<G, 0>(nbb0, hb);
        best_score = 2 * i0;
        best_i = i0;
        best_k = 0;
        best_d = 0;
        best_head = h0;
        best_nb = tp_first + nb0 * ts;
        best_headb = hb0;
        best_nbb = tpb_first + nbb0 * ts;
        ncell = hl == 0 ? 1u : 0u;
        d = 1;
        st = d <= o.dmax ? W2_EXT : W2_EXT_END;
    };

#ifdef DH_WAVE_GUARD
    uint32_t guard_ = 0;
#endif
    for (;;) {
#ifdef DH_WAVE_GUARD
        if (++guard_ > (1u << 22)) {  // debug builds: a stuck state machine reports instead of hanging
            if (hl == 0) printf("k_wave2 guard: block %d grp %d st %d d %d L %d item %d c %d nc %d nd %d\n", (int)blockIdx.x, grp,
                                st, d, L, cs.item, cs.c, cs.nc, cs.nd);
            err |= 8;
            break;
        }
#endif
        // the stepping loop proper: left only when a half needs bookkeeping (or both are done)
        if (wballot(st != W2_EXT && st != W2_DONE) == 0ull && wballot(st == W2_EXT) != 0ull) do {
          {
            // ======================================================== one difference level
            // (executed by every lane: a half that is done carries dead diagonals only, so the
            // step is a no-op for it and the loop body needs no divergent region)
            R = st == W2_EXT ? R : DEAD;
            const int32_t nL = L - 1;
            const int32_t kidx = (hl - nL) & (G - 1);
            const int32_t k = nL + kidx;
            const int32_t Rm = __builtin_amdgcn_ds_bpermute(addr_lo, R), Hm = __builtin_amdgcn_ds_bpermute(addr_lo, H),
                          Nm = __builtin_amdgcn_ds_bpermute(addr_lo, NB);
            const int32_t Rp = __builtin_amdgcn_ds_bpermute(addr_hi, R), Hp = __builtin_amdgcn_ds_bpermute(addr_hi, H),
                          Np = __builtin_amdgcn_ds_bpermute(addr_hi, NB);
            int32_t HBm = -1, NBm = tpb_first, HBp = -1, NBp = tpb_first;
            if (SYM) {
                HBm = __builtin_amdgcn_ds_bpermute(addr_lo, HB);
                NBm = __builtin_amdgcn_ds_bpermute(addr_lo, NBB);
                HBp = __builtin_amdgcn_ds_bpermute(addr_hi, HB);
                NBp = __builtin_amdgcn_ds_bpermute(addr_hi, NBB);
            }
            int32_t ni = -1, hd = -1, nbp = tp_first, hbn = -1, nbbp = tpb_first;
            const int32_t lim = min(an, bn + k);
            {
                const int32_t cs = R + 1, cdl = Rm + 1, ci = Rp;
                if (cs <= lim && cs > ni) {
                    ni = cs;
                    hd = H;
                    nbp = NB;
                    hbn = HB;
                    nbbp = NBB;
                }
                if (cdl <= lim && cdl > ni) {
                    ni = cdl;
                    hd = Hm;
                    nbp = Nm;
                    hbn = HBm;
                    nbbp = NBm;
                }
                if (ci <= lim && ci > ni) {
                    ni = ci;
                    hd = Hp;
                    nbp = Np;
                    hbn = HBp;
                    nbbp = NBp;
                }
            }
            bool alive = ni >= 0;
            int32_t j = ni - k;
            if (alive) slide2<PK>(pa, ra, pb, rb, lim, ni, j);
            // live diagonals of this level are counted per lane and summed when the extension ends;
            // a level without any falls through: nothing crosses, nothing beats the best, and the
            // window test below ends the extension
            ncell += alive ? 1u : 0u;
            bool ended = false;
            {
                // trace nodes for the boundaries crossed in (prev_i, ni]
                int32_t nextb = nbp;
                if (alive)
                    while (ni >= nextb) {
                        const int32_t idx = lbase + pn;
                        if (pn < lanecap) {
                            pool[idx].parent = hd;
                            pool[idx].d = d;
                            pool[idx].j = nextb - k;
                        }
                        hd = idx;
                        pn++;
                        nextb += ts;
                    }
                int32_t nextbb = nbbp;
                if (SYM && alive)
                    while (j >= nextbb) {
                        const int32_t idx = lbase + pn;
                        if (pn < lanecap) {
                            pool[idx].parent = hbn;
                            pool[idx].d = d;
                            pool[idx].j = nextbb + k;
                        }
                        hbn = idx;
                        pn++;
                        nextbb += ts;
                    }
                {
                    R = alive ? ni : DEAD;
                    H = hd;
                    NB = nextb;
                    HB = hbn;
                    NBB = nextbb;
                    const int32_t sc = alive ? 2 * ni - k - pen * d : INT32_MIN;
                    const int32_t step_best = hmax_i32<G>(sc, hb);
                    const uint32_t rot = (uint32_t)nL & (uint32_t)(G - 1);
                    if (step_best > best_score) {
                        const uint32_t hm = hballot<G>(alive && sc == step_best, hb);
                        const uint32_t hr = hrotr<G>(hm, rot);
                        const int32_t step_kidx = __ffs((int)hr) - 1;
                        const int32_t src = (nL + step_kidx) & (G - 1);
                        best_score = step_best;
                        best_k = nL + step_kidx;
                        best_i = hread(R, src, hb);
                        best_head = hread(H, src, hb);
                        best_nb = hread(NB, src, hb);
                        if (SYM) {
                            best_headb = hread(HB, src, hb);
                            best_nbb = hread(NBB, src, hb);
                        }
                        best_d = d;
                    }
                    if (alive && sc < best_score - xdrop) {
                        alive = false;
                        R = DEAD;
                    }
                    uint32_t lm = hballot<G>(alive, hb);
                    if (lm == 0u) {
                        ended = true;
                    } else {
                        uint32_t rm = hrotr<G>(lm, rot);
                        int32_t l2 = nL + (__ffs((int)rm) - 1);
                        int32_t u2 = nL + (31 - __clz((int)rm));
                        if (u2 - l2 + 1 > o.width) {
                            // Narrow windows trim on most levels.  A level adds at most one diagonal on
                            // each side, so at most two edges go: fetch the scores of the two lowest and
                            // the two highest live diagonals in one crossbar round trip and replay the
                            // rule (drop the lower-scoring edge, ties the low edge) on them.
                            const uint32_t rml = rm & (rm - 1u);
                            const int32_t pl0 = __ffs((int)rm) - 1, pu0 = 31 - __clz((int)rm);
                            const int32_t pl1 = __ffs((int)rml) - 1, pu1 = 31 - __clz((int)(rm & ~(1u << pu0)));
                            const int32_t val = 2 * R - k;
                            const int32_t sl0 = hread(val, (nL + pl0) & (G - 1), hb), sl1 = hread(val, (nL + pl1) & (G - 1), hb);
                            const int32_t su0 = hread(val, (nL + pu0) & (G - 1), hb), su1 = hread(val, (nL + pu1) & (G - 1), hb);
                            const bool low1 = sl0 <= su0;
                            const int32_t kill1 = low1 ? pl0 : pu0;
                            const int32_t nl = low1 ? pl1 : pl0, nu = low1 ? pu0 : pu1;
                            const bool low2 = (low1 ? sl1 : sl0) <= (low1 ? su0 : su1);
                            const int32_t kill2 = nu - nl + 1 > o.width ? (low2 ? nl : nu) : -1;
                            if (kidx == kill1 || kidx == kill2) {
                                alive = false;
                                R = DEAD;
                            }
                            lm = hballot<G>(alive, hb);
                            rm = hrotr<G>(lm, rot);
                            l2 = nL + (__ffs((int)rm) - 1);
                            u2 = nL + (31 - __clz((int)rm));
                        }
                        while (u2 - l2 + 1 > o.width) {
                            const int32_t val = 2 * R - k;
                            const int32_t sl = hread_fast<G>(val, l2, hb);
                            const int32_t su = hread_fast<G>(val, u2, hb);
                            const int32_t kill = sl <= su ? l2 : u2;
                            if (k == kill) {
                                alive = false;
                                R = DEAD;
                            }
                            lm = hballot<G>(alive, hb);
                            rm = hrotr<G>(lm, rot);
                            l2 = nL + (__ffs((int)rm) - 1);
                            u2 = nL + (31 - __clz((int)rm));
                        }
                        L = l2;
                    }
                }
            }
            d++;
            st = ((ended || d > o.dmax) && st == W2_EXT) ? W2_EXT_END : st;
          }
        } while (wballot(st == W2_EXT_END) == 0ull);  // (no half can run out of work inside the loop)
        if (st != W2_EXT && st != W2_DONE) {
            // ======================================================== bookkeeping of this half
            while (st != W2_EXT && st != W2_DONE) {
                if (st == W2_FETCH) {
                    int32_t it = 0;
                    if (hl == 0) it = (int32_t)atomicAdd(ws.queue, 1u);
                    it = hlane<G, 0>(it, hb);
                    if (it >= (ws.units ? (int32_t)*ws.nunits : nitems)) {
                        st = W2_DONE;
                        break;
                    }
                    // work unit: a whole item, or (symmetric mode) one group of candidates of an item
                    int32_t c0 = 0, c1 = INT32_MAX, ui = it;
                    if (ws.units) {
                        const int4 u = ws.units[it];
                        ui = u.x;
                        c0 = u.y;
                        c1 = u.z;
                    }
                    const int32_t item = item0 + ui;
                    cs.item = item;
                    cs.r = item >> 1;
                    cs.strand = item & 1;
                    cs.nc = min(max(ncand[item], 0), c1);
                    const int64_t bo = B.off[item >> 1];
                    cs.bo = bo;
                    cs.blen = (int32_t)(B.off[(item >> 1) + 1] - bo);
#pragma unroll
                    for (int sx = 0; sx < NG; sx++) gr[7 * sx][hl] = -1;
                    cs.nd = cs.nacc = cs.ntr = 0;
                    cs.c = c0;
                    st = W2_CAND;
                } else if (st == W2_CAND) {
                    bool started = false;
                    const int32_t item = cs.item, nc = cs.nc, nd = cs.nd;
                    int32_t c = cs.c;
                    while (c < nc && (SYM || cs.nacc < o.max_la) && nd < LANES) {
                        const DhCand cd = cand[(int64_t)item * o.max_cand + c];
                        const int32_t sdc = cd.apos - cd.bpos;
                        bool covd = false;
#pragma unroll 1
                        for (int sx = 0; sx < NG; sx++)
                            covd = covd || (hl + sx * G < nd && gr[7 * sx][hl] == cd.aseq && cd.apos >= gr[7 * sx + 1][hl] &&
                                            cd.apos < gr[7 * sx + 2][hl] && cd.bpos >= gr[7 * sx + 3][hl] &&
                                            cd.bpos < gr[7 * sx + 4][hl] && sdc >= gr[7 * sx + 5][hl] - 64 &&
                                            sdc <= gr[7 * sx + 6][hl] + 64);
                        if (hballot<G>(covd, hb) != 0u) {
                            c++;
                            continue;
                        }
                        const int32_t as = cd.apos, bs = cd.bpos;
                        cs.c_aseq = cd.aseq;
                        cs.as = as;
                        cs.bs = bs;
                        cs.sd = sdc;
                        const int64_t ao = A.off[cd.aseq];
                        cs.ao = ao;
                        cs.alen = (int32_t)(A.off[cd.aseq + 1] - ao);
                        cs.fwd_first = ts - (as % ts);
                        cs.rev_first = (as % ts) ? (as % ts) : ts;
                        const int32_t resb = cs.strand ? cs.blen % ts : 0;
                        cs.resb = resb;
                        int32_t bm = (bs - resb) % ts;
                        bm = bm < 0 ? bm + ts : bm;
                        cs.fwdb_first = ts - bm;
                        cs.revb_first = bm ? bm : ts;
                        pn = 0;
                        ext_begin(0);
                        started = true;
                        break;
                    }
                    cs.c = c;
                    if (!started) {
                        if (!SYM && hl == 0) {
                            out_nla[item] = cs.nacc;
                            out_ntr[item] = cs.ntr;
                        }
                        st = W2_FETCH;
                    }
                } else if (st == W2_EXT_END) {
                    {
                        // sum of the per-lane counts over the half
                        uint32_t tot = ncell;
                        for (int off = G / 2; off > 0; off >>= 1) tot += (uint32_t)__shfl_xor((int)tot, off, LANES);
                        cs.cells += tot;
                        // a lane that ran out of node slots wrote nothing past its stretch; its chains are
                        // broken, so the alignment is reported instead of used
                        if (hballot<G>(pn > lanecap, hb) != 0u) err |= DH_ST_POOL_OVERFLOW;
                    }
                    const int32_t r_nb = (best_nb - tp_first) / ts, r_nbb = SYM ? (best_nbb - tpb_first) / ts : 0;
                    if (dir == 0 && !err) {
                        cs.fw_i = best_i;
                        cs.fw_j = best_i - best_k;
                        cs.fw_d = best_d;
                        cs.fw_head = best_head;
                        cs.fw_nb = r_nb;
                        cs.fw_headb = best_headb;
                        cs.fw_nbb = r_nbb;
                        ext_begin(1);
                        continue;
                    }
                    cs.rv_i = best_i;
                    cs.rv_j = best_i - best_k;
                    cs.rv_d = best_d;
                    cs.rv_head = best_head;
                    cs.rv_nb = r_nb;
                    cs.rv_headb = best_headb;
                    cs.rv_nbb = r_nbb;
                    cs.naln += 1;
                    if (err || cs.fw_nb > ws.nbmax || r_nb > ws.nbmax || cs.fw_nbb > ws.nbmax || r_nbb > ws.nbmax) {
                        err |= DH_ST_POOL_OVERFLOW;
                        st = W2_DONE;
                        break;
                    }
                    st = W2_POST_CHAIN;
                } else if (st == W2_POST_CHAIN) {
                    // chains: lane 0 forward, lane 1 reverse, lanes 2 / 3 the B-boundary families (SYM)
                    int32_t *cdj = ws.cdj + slot * 8 * ws.nbmax;
                    int32_t clo = 0, chi = 0;
                    if (hl < (SYM ? 4 : 2)) {
                        const bool isf = (hl & 1) == 0, isb = hl >= 2;
                        const int32_t head = isb ? (isf ? cs.fw_headb : cs.rv_headb) : (isf ? cs.fw_head : cs.rv_head);
                        const int32_t nb = isb ? (isf ? cs.fw_nbb : cs.rv_nbb) : (isf ? cs.fw_nb : cs.rv_nb);
                        const int32_t first = isb ? (isf ? cs.fwdb_first : cs.revb_first)
                                                  : (isf ? cs.fwd_first : cs.rev_first);
                        const int32_t bk = isb ? 0 : (isf ? cs.fw_i - cs.fw_j : cs.rv_i - cs.rv_j);
                        // layout of cdj: fd fj rd rj fdb fib rdb rib (nbmax each)
                        int32_t *cd = cdj + (int64_t)((isb ? 4 : 0) + (isf ? 0 : 2)) * ws.nbmax;
                        walk_chain(pool, head, nb, first, ts, bk, cd, cd + ws.nbmax, clo, chi);
                    }
                    __threadfence_block();
                    const int32_t flo = hlane<G, 0>(clo, hb), fhi = hlane<G, 0>(chi, hb);
                    const int32_t rlo = hlane<G, 1>(clo, hb), rhi = hlane<G, 1>(chi, hb);
                    const int32_t as = cs.as, bs = cs.bs, sd = cs.sd, nd = cs.nd;
                    const int32_t abpos = as - cs.rv_i, bbpos = bs - cs.rv_j, aepos = as + cs.fw_i, bepos = bs + cs.fw_j;
                    const int32_t diffs = cs.fw_d + cs.rv_d;
                    int32_t lo = sd + flo, hi = sd + fhi;
                    lo = (sd - rhi) < lo ? (sd - rhi) : lo;
                    hi = (sd - rlo) > hi ? (sd - rlo) : hi;
                    if (hl == (nd & (G - 1))) {
                        const int g0 = 7 * (nd / G);
                        gr[g0 + 0][hl] = cs.c_aseq;
                        gr[g0 + 1][hl] = abpos;
                        gr[g0 + 2][hl] = aepos;
                        gr[g0 + 3][hl] = bbpos;
                        gr[g0 + 4][hl] = bepos;
                        gr[g0 + 5][hl] = lo;
                        gr[g0 + 6][hl] = hi;
                    }
                    cs.nd = nd + 1;
                    cs.c = cs.c + 1;
                    cs.abpos = abpos;
                    cs.bbpos = bbpos;
                    cs.aepos = aepos;
                    cs.bepos = bepos;
                    cs.diffs = diffs;
                    const int64_t al = aepos - abpos, bl = bepos - bbpos;
                    const bool accept = al >= o.min_len &&
                                        (int64_t)2 * diffs * 1000000ll <= (int64_t)o.max_err_ppm * (al + bl);
                    st = accept ? W2_POST_REC1 : W2_CAND;
                } else if (st == W2_POST_REC1) {
                    // ---- the record (a, b): trace on the grid of A
                    int32_t *cdj = ws.cdj + slot * 8 * ws.nbmax;
                    const int32_t item = cs.item, strand = cs.strand, c_aseq = cs.c_aseq;
                    const int32_t item_a = SYM ? 2 * c_aseq + strand : item;
                    int32_t s1 = cs.nacc;
                    if (SYM) {
                        if (hl == 0) s1 = atomicAdd(&out_nla[item_a], 1);
                        s1 = hlane<G, 0>(s1, hb);
                        if (s1 >= o.max_la) {
                            // more overlaps than slots: the pair is dropped, both items are reported
                            // (their pile-up is skipped by the caller), everything else goes on
                            if (hl == 0) {
                                atomicSub(&out_nla[item_a], 1);
                                ws.item_ovf[item_a] = 1;
                                ws.item_ovf[item] = 1;
                            }
                            st = W2_CAND;
                            continue;
                        }
                    }
                    const int64_t oslot = (int64_t)item_a * o.max_la + s1;
                    const int32_t npairs = emit_trace(hl, G, ts, 0, cs.as, cs.bs, cs.abpos, cs.aepos, cs.bbpos,
                                                      cs.bepos, cs.rv_d, cs.fw_d, cs.rev_first, cs.rv_nb,
                                                      cdj + 2 * (int64_t)ws.nbmax, cdj + 3 * (int64_t)ws.nbmax,
                                                      cs.fwd_first, cs.fw_nb, cdj, cdj + ws.nbmax, false,
                                                      out_trace + oslot * trmax);
                    if (hl == 0) {
                        DhLa la;
                        la.tlen = 2 * npairs;
                        la.diffs = cs.diffs;
                        la.abpos = cs.abpos;
                        la.bbpos = cs.bbpos;
                        la.aepos = cs.aepos;
                        la.bepos = cs.bepos;
                        la.flags = strand ? 1u : 0u;
                        la.aread = c_aseq;
                        la.bread = cs.r;
                        la.pad = 0;
                        la.toff = 0;
                        out_la[oslot] = la;
                        if (SYM) atomicAdd(&out_ntr[item_a], 2 * npairs);
                    }
                    cs.nacc = cs.nacc + 1;
                    cs.ntr = cs.ntr + 2 * npairs;
                    st = SYM ? W2_POST_REC2 : W2_CAND;
                } else {  // W2_POST_REC2: the transposed record (b, a), trace on the grid of B
                    int32_t *cdj = ws.cdj + slot * 8 * ws.nbmax;
                    const int32_t item = cs.item, strand = cs.strand;
                    int32_t s2 = 0;
                    if (hl == 0) s2 = atomicAdd(&out_nla[item], 1);
                    s2 = hlane<G, 0>(s2, hb);
                    if (s2 >= o.max_la) {
                        if (hl == 0) {
                            atomicSub(&out_nla[item], 1);
                            ws.item_ovf[item] = 1;
                            ws.item_ovf[2 * cs.c_aseq + strand] = 1;
                        }
                        st = W2_CAND;
                        continue;
                    }
                    const int64_t slot2 = (int64_t)item * o.max_la + s2;
                    const int32_t np2 = emit_trace(hl, G, ts, cs.resb, cs.bs, cs.as, cs.bbpos, cs.bepos, cs.abpos,
                                                   cs.aepos, cs.rv_d, cs.fw_d, cs.revb_first, cs.rv_nbb,
                                                   cdj + 6 * (int64_t)ws.nbmax, cdj + 7 * (int64_t)ws.nbmax,
                                                   cs.fwdb_first, cs.fw_nbb, cdj + 4 * (int64_t)ws.nbmax,
                                                   cdj + 5 * (int64_t)ws.nbmax, strand != 0, out_trace + slot2 * trmax);
                    if (hl == 0) {
                        const int32_t blen = cs.blen, alen = cs.alen;
                        DhLa la;
                        la.tlen = 2 * np2;
                        la.diffs = cs.diffs;
                        la.abpos = strand ? blen - cs.bepos : cs.bbpos;
                        la.aepos = strand ? blen - cs.bbpos : cs.bepos;
                        la.bbpos = strand ? alen - cs.aepos : cs.abpos;
                        la.bepos = strand ? alen - cs.abpos : cs.aepos;
                        la.flags = strand ? 1u : 0u;
                        la.aread = cs.r;
                        la.bread = cs.c_aseq;
                        la.pad = 0;
                        la.toff = 0;
                        out_la[slot2] = la;
                        atomicAdd(&out_ntr[item], 2 * np2);
                    }
                    st = W2_CAND;
                }
            }
        }
        if (wballot(st != W2_DONE) == 0ull) break;
    }
    if (hl == 0) {
        atomicAdd(&counters[0], cs.cells);
        atomicAdd(&counters[1], cs.naln);
        if (err) atomicOr(status, err);
    }
}

// ------------------------------------------------------------------------------------ launchers

// apk / bpk / brcpk: 2-bit packed copies (all three or none)
extern "C" void dhk_wave(hipStream_t st, int32_t nslots, DbView A, DbView B, const uint8_t *brc, const uint8_t *apk,
              const uint8_t *bpk, const uint8_t *brcpk, DhOpts o,
              int32_t item0, int32_t nitems, const DhCand *cand, const int32_t *ncand,
              WaveScratch ws, DhLa *out_la, uint16_t *out_trace, int32_t trmax, int32_t *out_nla,
              int32_t *out_ntr, unsigned long long *counters, int32_t *status)
{
    if (nitems <= 0) return;
    const bool pk = apk && bpk && brcpk;
#define WAVE_LAUNCH(S, P)                                                                          \
    hipLaunchKernelGGL((k_wave<S, P>), dim3(nslots), dim3(LANES), 0, st, A, B, brc, apk, bpk, brcpk, o, item0, \
                       nitems, cand, ncand, ws, out_la, out_trace, trmax, out_nla, out_ntr, counters, status)
    if (o.skip_self == 2) {
        if (pk)
            WAVE_LAUNCH(true, true);
        else
            WAVE_LAUNCH(true, false);
    } else {
        if (pk)
            WAVE_LAUNCH(false, true);
        else
            WAVE_LAUNCH(false, false);
    }
#undef WAVE_LAUNCH
}

// two (o.width <= 30) or four (o.width <= 14) alignments per wavefront: nslots blocks with 2 or 4
// scratch slots each; needs the reverse complement of A as well (arc, arcpk); apk / arcpk / bpk /
// brcpk all four or none
extern "C" void dhk_wave2(hipStream_t st, int32_t nslots, DbView A, DbView B, const uint8_t *arc, const uint8_t *brc,
               const uint8_t *apk, const uint8_t *arcpk, const uint8_t *bpk, const uint8_t *brcpk, DhOpts o,
               int32_t item0, int32_t nitems, const DhCand *cand, const int32_t *ncand, WaveScratch ws,
               DhLa *out_la, uint16_t *out_trace, int32_t trmax, int32_t *out_nla, int32_t *out_ntr,
               unsigned long long *counters, int32_t *status)
{
    if (nitems <= 0) return;
    const bool pk = apk && arcpk && bpk && brcpk;
    // four alignments per wavefront at width <= 14 unless DH_WAVE_G32 is set (development): the same rule as the caller's
    // slots per block (dh_api.cpp: per_wave)
    const bool g16 = o.width <= 14 && !getenv("DH_WAVE_G32");
#define WAVE2_LAUNCH(S, P)                                                                         \
    do {                                                                                           \
        if (g16)                                                                                   \
            hipLaunchKernelGGL((k_wave2<S, P, 16>), dim3(nslots), dim3(LANES), 0, st, A, B, arc, brc, apk, arcpk, bpk, \
                               brcpk, o, item0, nitems, cand, ncand, ws, out_la, out_trace, trmax, out_nla, out_ntr,  \
                               counters, status);                                                  \
        else                                                                                       \
            hipLaunchKernelGGL((k_wave2<S, P, 32>), dim3(nslots), dim3(LANES), 0, st, A, B, arc, brc, apk, arcpk, bpk, \
                               brcpk, o, item0, nitems, cand, ncand, ws, out_la, out_trace, trmax, out_nla, out_ntr,  \
                               counters, status);                                                  \
    } while (0)
    if (o.skip_self == 2) {
        if (pk)
            WAVE2_LAUNCH(true, true);
        else
            WAVE2_LAUNCH(true, false);
    } else {
        if (pk)
            WAVE2_LAUNCH(false, true);
        else
            WAVE2_LAUNCH(false, false);
    }
#undef WAVE2_LAUNCH
}
