// bitvec_host.cpp -- k_tile's column loop on 32-bit words (dh_tile.h: tile_block / tile_col_h, three-input functions
// through dh_bitvec.h: b3) compiled for the CPU, against the 64-bit reference step dh_tile.h: tile_col.
//
// TEST INFRASTRUCTURE: one lane's view of the kernel's column loop -- blocks of 32 columns, the wave-uniform bounds
// (the longest and the shortest tile of the wavefront), the first block's lv, the wild / no-wild choice, the bulk
// update of dbot -- on random tiles: random Pv / Mv / dbot / tandem mask / sequence words, tiles of 1 .. 128 columns,
// B' ending before, inside or after the tile (z crossing zero inside it).
// Build: g++ -O2 -shared -fPIC -I/opt/rocm/include -D__HIP_PLATFORM_AMD__ (Makefile target tests/native/libdh_bitvec_host.so)
#include <cstdint>
#include <cstdio>

#include "../../dentist_amd/csrc/dh_tile.h"

using namespace dhtile;

static uint64_t rng(uint64_t &s)
{
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
    return s;
}

// stats: [0] tiles, [1] columns, [2] tiles run without wild, [3] tiles in which z crosses zero, [4] tiles whose columns
// all ran without the per-lane test (cols == cmin), [5] tiles with columns past 32, [6] lanes that did not run
template <bool TAN, int WB>
static long check(uint64_t seed, long ntiles, long *stats)
{
    typedef typename BandVec<WB>::U V;
    constexpr int W = WB;
    long bad = 0;
    uint64_t r = seed * 0x9E3779B97F4A7C15ull + 1;
    for (long it = 0; it < ntiles; it++) {
        uint32_t q[NTW];
        for (int i = 0; i < NTW; i++) q[i] = (uint32_t)rng(r);
        TileT<WB> t;
        t.Pv = (V)rng(r);
        t.Mv = (V)rng(r);
        if (rng(r) & 1) t.Mv &= (V)~t.Pv;  // the states the recurrence reaches have Pv & Mv == 0; the identities hold for any
        t.dbot = (int32_t)(rng(r) % 200) - 50;
        t.T = 1 + (int32_t)(rng(r) % TS_MAX);
        t.cols = (rng(r) & 3) ? t.T : 1 + (int32_t)(rng(r) % t.T);
        t.bnr = (int32_t)(rng(r) % (TS_MAX + 2 * W));
        t.lv = (V)(~(V)0 << (W / 2 + 1));
        const int32_t th = t.bnr + W / 2 + 1;
        t.wild = th >= W ? (V)0 : (V)(~(V)0 << th);
        t.z = t.bnr - W / 2 + 1;
        t.dm = TAN ? (V)rng(r) : (V)~(V)0;
        const bool run = (rng(r) % 16) != 0;
        // the wavefront's other lanes: the longest and the shortest tile among the running ones
        const int32_t cmax = t.cols + (int32_t)(rng(r) % (TS_MAX + 1 - t.cols)) * (int32_t)(rng(r) & 1);
        const int32_t cmin = (rng(r) & 1) ? t.cols : 1 + (int32_t)(rng(r) % t.cols);
        const bool need = t.wild != (V)0 || t.z < t.cols;
        const bool wild = need || (rng(r) & 1);  // another lane may need it

        TileT<WB> ref = t;
        if (run)
            for (int32_t c = 1; c <= t.cols; c++) {
                V p0, p1;
                uint32_t x;
                tile_window<WB>(q, c, p0, p1, x);
                tile_col<TAN, WB>(ref, p0, p1, x);
            }

        TileT<WB> n = t;
        TileH<WB> s;
        tile_split(n, s);
        for (int32_t blk = 0; 32 * blk < cmax; blk++) {  // as k_tile, q standing for its LDS words
            const uint32_t w[6] = {q[blk], q[blk + 1], WB == 64 ? q[blk + 2] : 0u, q[NQ + blk], q[NQ + blk + 1],
                                   WB == 64 ? q[NQ + blk + 2] : 0u};
            const uint32_t nab0 = ~q[2 * NQ + 2 * blk], nab1 = ~q[2 * NQ + 2 * blk + 1];
            const int32_t nsh = cmax - 32 * blk < 32 ? cmax - 32 * blk : 32;
            const int32_t nfull = cmin - 32 * blk < 0 ? 0 : (cmin - 32 * blk < nsh ? cmin - 32 * blk : nsh);
            const int32_t left = n.cols - 32 * blk, lim = run ? (left < 0 ? 0 : (left < nsh ? left : nsh)) : 0;
            tile_block<TAN, WB>(s, w, nab0, nab1, blk == 0, wild, nfull, nsh, run, lim);
            if (run) tile_dtop_flush(s, n.dbot, lim);
        }
        if (run) {
            tile_join(s, n);
            if (!wild) n.z -= n.cols;
        }

        // lv: the kernel stops shifting it after the first block (all ones from column W/2 + 1 on, never read after the tile)
        const bool lv_ok = !run || t.cols > 32 || n.lv == ref.lv;
        if (n.Pv != ref.Pv || n.Mv != ref.Mv || n.wild != ref.wild || n.z != ref.z || n.dbot != ref.dbot || !lv_ok) {
            if (bad < 5)
                fprintf(stderr, "tile %ld (WB %d TAN %d): cols %d cmin %d cmax %d bnr %d wild %d run %d: Pv %d Mv %d wild %d z %d/%d dbot %d/%d lv %d\n",
                        it, WB, (int)TAN, t.cols, cmin, cmax, t.bnr, (int)wild, (int)run, n.Pv == ref.Pv, n.Mv == ref.Mv,
                        n.wild == ref.wild, n.z, ref.z, n.dbot, ref.dbot, (int)lv_ok);
            bad++;
        }
        stats[0]++;
        stats[1] += run ? t.cols : 0;
        stats[2] += run && !wild;
        stats[3] += run && t.z > 0 && t.z - t.cols < 0;
        stats[4] += run && cmin == t.cols;
        stats[5] += run && t.cols > 32;
        stats[6] += !run;
    }
    return bad;
}

extern "C" long dh_bitvec_tile_check(uint64_t seed, long ntiles, int wb, int tan, long *stats)
{
    if (wb == 64) return tan ? check<true, 64>(seed, ntiles, stats) : check<false, 64>(seed, ntiles, stats);
    if (wb == 32) return tan ? check<true, 32>(seed, ntiles, stats) : check<false, 32>(seed, ntiles, stats);
    return -1;
}

// b3 on the host against the formulas its tables are composed from
extern "C" long dh_bitvec_b3_check(uint64_t seed, long n)
{
    using namespace dhbv;
    long bad = 0;
    uint64_t r = seed * 0x9E3779B97F4A7C15ull + 1;
    for (long i = 0; i < n; i++) {
        const uint32_t a = (uint32_t)rng(r), b = (uint32_t)rng(r), c = (uint32_t)rng(r);
        bad += b3<BA & (BB ^ BC)>(a, b, c) != (a & (b ^ c));
        bad += b3<(BA | BB) & BC>(a, b, c) != ((a | b) & c);
        bad += b3<(BA ^ BB) | BC>(a, b, c) != ((a ^ b) | c);
        bad += b3<BA | ~(BB | BC)>(a, b, c) != (a | ~(b | c));
        bad += b3<(BA ^ BB) & BC>(a, b, c) != ((a ^ b) & c);
        bad += b3<BA>(a, b, c) != a || b3<BB>(a, b, c) != b || b3<BC>(a, b, c) != c;
    }
    return bad;
}
