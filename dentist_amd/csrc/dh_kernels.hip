// dh_kernels.hip -- gfx950 (CDNA4, wave64) kernels around the alignment pass that are neither the seed filter
// (dh_seed.hip), the DH-1 wave kernels (dh_wave.hip) nor DH-2 (dh_tile.hip); every launcher follows its kernel.
//
// K1   k_revcomp, k_pack2<PLANES>, k_pack2_rc(+_bounds), k_planes_rc(+ k_pack2_rc_bounds32)
//                        copies of a DB: reverse complement, 2-bit packed, plane-packed       (HBM streams)
// K2   k_kmer_pass       k-mer extraction of A: count pass and fill pass                     (HBM stream + atomics)
//      k_group_index     the same two passes for a grouped DB with LDS counters
//      k_fat_dir         the fat directory word of every bucket
//      k_scan_*          exclusive scan of the bucket directory
// K4b  k_units           work units of the symmetric alignment launch (candidates grouped by A read)
//      k_compact         compaction of the per-item record and trace slots (DH-1 and DH-2)
//      k_dust            low-complexity mask (DBdust)
//      k_mask_slices, k_cov_events, k_cov_mask_at
//                        mask bits of slices, alignment-coverage mask
//      k_fill16, k_or_words
//                        memset for large buffers, OR of two bitmaps
//
// What they compute is written down in DESIGN.md (§3 algorithms, §4 data layout).

#include <hip/hip_runtime.h>
#include <algorithm>
#include <stdint.h>

#include "dh_device.h"

#define LANES 64

#include "dh_kmer.h"

// ------------------------------------------------------------------------------------ K1

// 8 bases per thread and step: unaligned 8-byte load of the mirrored window, byte swap,
// complement of the codes 0..3 (c ^ 3; other codes are kept), unaligned 8-byte store.
__global__ void __launch_bounds__(256)
k_revcomp(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int64_t *__restrict__ off,
          int32_t n)
{
    // blockIdx.y = sequence, grid-stride over its 8-base words
    const int32_t s = blockIdx.y;
    if (s >= n) return;
    const int64_t o = off[s], len = off[s + 1] - o;
    const int64_t nw = len >> 3;
    for (int64_t wd = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; wd < nw;
         wd += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = wd << 3;
        uint64_t x;
        __builtin_memcpy(&x, src + o + len - 8 - i, 8);
        x = __builtin_bswap64(x);
        const uint64_t hi = x & 0xFCFCFCFCFCFCFCFCull;  // bytes >= 4 are not bases
        const uint64_t nz = (((hi & 0x7F7F7F7F7F7F7F7Full) + 0x7F7F7F7F7F7F7F7Full) | hi) & 0x8080808080808080ull;
        const uint64_t keep = (nz >> 7) * 0xFFull;
        x ^= 0x0303030303030303ull & ~keep;
        __builtin_memcpy(dst + o + i, &x, 8);
    }
    // tail (len % 8 bases): the first threads of block x == 0
    if (blockIdx.x == 0) {
        const int64_t i = (nw << 3) + threadIdx.x;
        if (i < len) {
            const uint8_t c = src[o + len - 1 - i];
            dst[o + i] = c < 4 ? (uint8_t)(3 - c) : c;
        }
    }
}

extern "C" void dhk_revcomp(hipStream_t st, const uint8_t *src, uint8_t *dst, const int64_t *off, int32_t n,
                 int32_t max_len)
{
    if (n <= 0) return;
    int gx = (max_len + 2047) / 2048;  // 256 threads x 8 bases per block and step
    if (gx > 64) gx = 64;
    if (gx < 1) gx = 1;
    // grid.y is limited to 65535: loop in slabs
    for (int32_t s0 = 0; s0 < n; s0 += 65535) {
        const int32_t cnt = n - s0 < 65535 ? n - s0 : 65535;
        // shifted views: off + s0 keeps absolute offsets into src/dst
        hipLaunchKernelGGL(k_revcomp, dim3(gx, cnt), dim3(256), 0, st, src, dst, off + s0, cnt);
    }
}

// 2-bit packed copy of a base array for the wave kernel: base g sits in byte g >> 2 at bits
// 2 * (g & 3), so a little-endian 8-byte load holds 32 consecutive bases, low bits first.
// One thread per 8-byte word; flag is raised when a code outside 0..3 is met (such DBs are
// aligned from the byte arrays instead).  The source is readable 63 bytes past `total` (DB_PAD).
// PLANES: the word is stored plane-packed for k_tile (dh_tile.h: PlanePair -- low bits of the 32 bases in the low
// half, high bits in the high half) instead of being converted by a pass of its own over the copy
__device__ __forceinline__ uint32_t squeeze_even64(uint64_t x)
{
    x &= 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (uint32_t)x;
}
__device__ __forceinline__ uint64_t pk_to_planes(uint64_t x) { return (uint64_t)squeeze_even64(x) | ((uint64_t)squeeze_even64(x >> 1) << 32); }
template <bool PLANES>
__global__ void __launch_bounds__(256)
k_pack2(const uint8_t *__restrict__ src, int64_t total, uint64_t *__restrict__ dst,
        int32_t *__restrict__ flag)
{
    const int64_t wd = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nw = (total + 31) >> 5;
    if (wd >= nw) return;
    uint64_t out = 0;
    bool bad = false;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint64_t x = load8(src + (wd << 5) + 8 * q);
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t c = (uint32_t)(x >> (8 * u)) & 0xFFu;
            const int64_t g = (wd << 5) + 8 * q + u;
            if (c > 3u && g < total) bad = true;
            out |= (uint64_t)(c & 3u) << (2 * (8 * q + u));
        }
    }
    dst[wd] = PLANES ? pk_to_planes(out) : out;
    if (bad) atomicOr(flag, 1);
}
template __global__ void k_pack2<false>(const uint8_t *, int64_t, uint64_t *, int32_t *);
template __global__ void k_pack2<true>(const uint8_t *, int64_t, uint64_t *, int32_t *);

extern "C" void dhk_pack2(hipStream_t st, const uint8_t *src, int64_t total, uint8_t *dst, int32_t *flag)
{
    const int64_t nw = (total + 31) >> 5;
    if (nw <= 0) return;
    hipLaunchKernelGGL(k_pack2<false>, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, src, total, (uint64_t *)dst,
                       flag);
}
// plane-packed forward / reverse-complement copies of a chunk for k_tile, straight from the bytes
extern "C" void dhk_pack2_planes(hipStream_t st, const uint8_t *src, int64_t total, uint8_t *dst, int32_t *flag)
{
    const int64_t nw = (total + 31) >> 5;
    if (nw <= 0) return;
    hipLaunchKernelGGL(k_pack2<true>, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, st, src, total, (uint64_t *)dst,
                       flag);
}

// 2-bit packed reverse complements straight from the forward bytes: sequence s occupies the same base
// range [off[s], off[s+1]) in the packed copy, mirrored inside it.  One thread per 16-base word of the
// destination that the sequence touches: whole words are stored, the (at most two) words a sequence
// shares with its neighbours are ORed into the zeroed buffer.  `a0` (multiple of 32) = base position of
// dst word 0.  Codes outside 0..3 pack as (c ^ 3) & 3; such DBs are not aligned from the packed copies.
__device__ __forceinline__ uint32_t pack8_rc(uint64_t y)
{
    uint64_t t = (y ^ 0x0303030303030303ull) & 0x0303030303030303ull;
    t = (t | (t >> 6)) & 0x000F000F000F000Full;
    t = (t | (t >> 12)) & 0x000000FF000000FFull;
    t = (t | (t >> 24)) & 0xFFFFull;
    return (uint32_t)t;
}
__global__ void __launch_bounds__(256)
k_pack2_rc(const uint8_t *__restrict__ src, const int64_t *__restrict__ off, int32_t n, int64_t a0,
           uint32_t *__restrict__ dst)
{
    const int32_t s = blockIdx.y;
    if (s >= n) return;
    const int64_t o = off[s], len = off[s + 1] - o;
    if (len <= 0) return;
    const int64_t w0 = (o - a0) >> 4, w1 = (o + len - 1 - a0) >> 4;  // first / last destination word
    const int64_t sbase = 2 * o + len - 1;                           // source of base g is src[sbase - g]
    for (int64_t w = w0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= w1; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gw = a0 + (w << 4);
        if (gw >= o && gw + 16 <= o + len) {
            const uint8_t *A = src + (sbase - gw - 15);
            uint64_t x0, x1;
            __builtin_memcpy(&x0, A, 8);      // positions 15 .. 8
            __builtin_memcpy(&x1, A + 8, 8);  // positions 7 .. 0
            dst[w] = pack8_rc(__builtin_bswap64(x1)) | (pack8_rc(__builtin_bswap64(x0)) << 16);
        } else {
            const int64_t g0 = gw > o ? gw : o, g1 = gw + 16 < o + len ? gw + 16 : o + len;
            uint32_t out = 0;
            for (int64_t g = g0; g < g1; g++) out |= (uint32_t)((src[sbase - g] ^ 3u) & 3u) << (2 * (int)(g - gw));
            atomicOr(&dst[w], out);
        }
    }
}

// zeroes the (at most two) destination words every sequence shares with its neighbours: what k_pack2_rc ORs into.
// Interior words are stored whole, so the rest of the buffer needs no memset (2 GB per chunk of the mapping).
extern "C" __global__ void __launch_bounds__(256)
k_pack2_rc_bounds(const int64_t *__restrict__ off, int32_t n, int64_t a0, uint32_t *__restrict__ dst)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t o = off[s], len = off[s + 1] - o;
    if (len <= 0) return;
    const int64_t w0 = (o - a0) >> 4, w1 = (o + len - 1 - a0) >> 4;
    const int64_t g0 = a0 + (w0 << 4), g1 = a0 + (w1 << 4);
    if (!(g0 >= o && g0 + 16 <= o + len)) dst[w0] = 0;
    if (!(g1 >= o && g1 + 16 <= o + len)) dst[w1] = 0;
}

extern "C" void dhk_pack2_rc_bounds(hipStream_t st, const int64_t *off, int32_t n, int64_t a0, uint8_t *dst)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pack2_rc_bounds, dim3((n + 255) / 256), dim3(256), 0, st, off, n, a0, (uint32_t *)dst);
}

extern "C" void dhk_pack2_rc(hipStream_t st, const uint8_t *src, const int64_t *off, int32_t n, int32_t max_len, int64_t a0,
                  uint8_t *dst)
{
    if (n <= 0) return;
    int gx = (max_len / 16 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int32_t s0 = 0; s0 < n; s0 += 65535) {
        const int32_t cnt = n - s0 < 65535 ? n - s0 : 65535;
        hipLaunchKernelGGL(k_pack2_rc, dim3(gx, cnt), dim3(256), 0, st, src, off + s0, cnt, a0, (uint32_t *)dst);
    }
}

// the plane-packed reverse complements from the plane-packed FORWARD copy (made just before by k_pack2<true>) instead of
// from the bytes again: 8 bytes read per 32 bases instead of 32 -- base g of the reverse complement of sequence s is the
// complement of forward base sbase - g, so the 32 bases of a destination word are a run of 32 forward bases in reverse
// order: two funnel shifts over two forward words per plane, a bit reversal, a complement.  Words shared with a
// neighbouring sequence are ORed in, as in k_pack2_rc.  fwd / dst: word 0 = base a0 (a multiple of 32), readable /
// zeroed PK_PAD bytes beyond both ends.
__global__ void __launch_bounds__(256)
k_planes_rc(const unsigned long long *__restrict__ fwd, const int64_t *__restrict__ off, int32_t n, int64_t a0,
            unsigned long long *__restrict__ dst)
{
    const int32_t s = blockIdx.y;
    if (s >= n) return;
    const int64_t o = off[s], len = off[s + 1] - o;
    if (len <= 0) return;
    const int64_t w0 = (o - a0) >> 5, w1 = (o + len - 1 - a0) >> 5;  // first / last destination word
    const int64_t sbase = 2 * o + len - 1;                           // source of base g is forward base sbase - g
    for (int64_t w = w0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w <= w1; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t gw = a0 + (w << 5);
        const int64_t p = sbase - gw - 31 - a0;  // first forward base of the run, relative to word 0 (may lie in the padding)
        const int64_t ws = p >> 5;               // (arithmetic shift: floor)
        const uint32_t sh = (uint32_t)(p & 31);
        const unsigned long long f0 = fwd[ws], f1 = fwd[ws + 1];
        const uint32_t lo = __builtin_amdgcn_alignbit((uint32_t)f1, (uint32_t)f0, sh);
        const uint32_t hi = __builtin_amdgcn_alignbit((uint32_t)(f1 >> 32), (uint32_t)(f0 >> 32), sh);
        // (run position i = forward base p + i = destination base 31 - i; complement = both planes inverted)
        unsigned long long out = (unsigned long long)(~__brev(lo)) | ((unsigned long long)(~__brev(hi)) << 32);
        if (gw >= o && gw + 32 <= o + len)
            dst[w] = out;
        else {
            const int64_t g0 = gw > o ? gw : o, g1 = gw + 32 < o + len ? gw + 32 : o + len;
            const uint32_t m = (uint32_t)(((g1 - g0) >= 32 ? ~0ull : ((1ull << (g1 - g0)) - 1)) << (g0 - gw));
            out &= (unsigned long long)m | ((unsigned long long)m << 32);
            atomicOr(&dst[w], out);
        }
    }
}
__global__ void __launch_bounds__(256)
k_pack2_rc_bounds32(const int64_t *__restrict__ off, int32_t n, int64_t a0, uint64_t *__restrict__ dst)
{
    const int32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n) return;
    const int64_t o = off[s], len = off[s + 1] - o;
    if (len <= 0) return;
    const int64_t w0 = (o - a0) >> 5, w1 = (o + len - 1 - a0) >> 5;
    const int64_t g0 = a0 + (w0 << 5), g1 = a0 + (w1 << 5);
    if (!(g0 >= o && g0 + 32 <= o + len)) dst[w0] = 0;
    if (!(g1 >= o && g1 + 32 <= o + len)) dst[w1] = 0;
}

// the plane-packed reverse complements from the plane-packed forward copy `fwd` of the chunk (dhk_pack2_planes ran before on
// this stream)
extern "C" void dhk_planes_rc(hipStream_t st, const uint8_t *fwd, const int64_t *off, int32_t n, int32_t max_len, int64_t a0, uint8_t *dst)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_pack2_rc_bounds32, dim3((n + 255) / 256), dim3(256), 0, st, off, n, a0, (uint64_t *)dst);
    int gx = (max_len / 32 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int32_t s0 = 0; s0 < n; s0 += 65535) {
        const int32_t cnt = n - s0 < 65535 ? n - s0 : 65535;
        hipLaunchKernelGGL(k_planes_rc, dim3(gx, cnt), dim3(256), 0, st, (const unsigned long long *)fwd, off + s0, cnt, a0,
                           (unsigned long long *)dst);
    }
}

// ------------------------------------------------------------------------------------ K2

// tiles: (sequence, start) pairs, KM_TILE positions each; 256 threads x 16 positions.
template <bool FILL>
__global__ void __launch_bounds__(256)
k_kmer_pass(DbView A, const int2 *__restrict__ tiles, int32_t ntiles, int32_t k, int32_t kmer_mod,
            int32_t shift,
            uint32_t *__restrict__ dir, ulonglong2 *__restrict__ ent, const int64_t *__restrict__ goff)
{
    const int32_t t = blockIdx.x;
    if (t >= ntiles) return;
    const int32_t s = tiles[t].x;
    const int64_t o = A.off[s];
    const int32_t len = (int32_t)(A.off[s + 1] - o);
    const uint64_t grp = A.group ? (uint64_t)A.group[s] : 0ull;
    const uint64_t mask = (1ull << (2 * k)) - 1;
    const int32_t p0 = tiles[t].y + threadIdx.x * (KM_TILE / 256);
    const KmerSampler smp = kmer_sampler(kmer_mod, k);
    uint64_t km = 0, rc = 0;
    int32_t valid = 0;
    const uint8_t *a = A.bases + o;
    const int rcsh = 2 * (k - 1);
    for (int32_t x = 0; x < KM_TILE / 256 + k - 1; x++) {
        const int32_t p = p0 + x;
        if (p >= len) break;
        const uint8_t c = a[p];
        if (c < 4) {
            km = ((km << 2) | c) & mask;
            rc = (rc >> 2) | ((uint64_t)(3 - c) << rcsh);
            valid++;
        } else {
            km = 0;
            rc = 0;
            valid = 0;
        }
        // the index is keyed by the canonical k-mer; bit 63 of the stored key says that the k-mer of A
        // is the reverse complement of its key (the lookup tells the strands apart with it)
        const uint64_t canon = km < rc ? km : rc;
        if (x >= k - 1 && valid >= k && kmer_sampled(canon, smp) &&
            !(A.mask_bits && mask_touch(A.mask_bits, o + p - k + 1, k))) {
            const uint64_t key = (grp << (2 * k)) | canon;
            const uint32_t b = (uint32_t)(key >> shift);
            if (FILL) {
                const uint32_t slot = atomicAdd(&dir[b], 1u);
                ent[slot] = make_ulonglong2(key | (km != canon ? 1ull << 63 : 0ull),
                                            ((uint64_t)s << 40) | (uint64_t)(goff[s] + (p - k + 1)));
            } else
                atomicAdd(&dir[b], 1u);
        }
    }
}
template __global__ void k_kmer_pass<false>(DbView, const int2 *, int32_t, int32_t, int32_t, int32_t,
                                            uint32_t *, ulonglong2 *, const int64_t *);
template __global__ void k_kmer_pass<true>(DbView, const int2 *, int32_t, int32_t, int32_t, int32_t,
                                           uint32_t *, ulonglong2 *, const int64_t *);

extern "C" void dhk_kmer_pass(hipStream_t st, int fill, DbView A, const int2 *tiles, int32_t ntiles, int32_t k,
                   int32_t kmer_mod, int32_t shift, uint32_t *dir, ulonglong2 *ent, const int64_t *goff)
{
    if (ntiles <= 0) return;
    if (fill)
        hipLaunchKernelGGL(k_kmer_pass<true>, dim3(ntiles), dim3(256), 0, st, A, tiles, ntiles, k,
                           kmer_mod, shift, dir, ent, goff);
    else
        hipLaunchKernelGGL(k_kmer_pass<false>, dim3(ntiles), dim3(256), 0, st, A, tiles, ntiles, k,
                           kmer_mod, shift, dir, ent, goff);
}

// The same two passes for a GROUPED DB (the pile-up stage: group = pile-up) without global atomics.  Keys carry the
// group in their top bits, so a group owns the contiguous bucket range [g * nbg, (g + 1) * nbg), nbg = 4^k >> shift.
// A block takes (group, slice of `slice` <= GI_SLICE buckets), rolls every k-mer of the group -- its tiles are
// tiles[gtile[g] .. gtile[g + 1]) -- and counts (FILL: places) those of its slice with LDS atomics; the counts / the
// advanced cursors go to dir[] in one coalesced pass.  170 M device-scope atomics on random counters took 19 ms per
// step (configs[2], 1 000 pile-ups); the price here is that a group's k-mers are rolled once per slice (8 times at
// k = 14 with 2^27 buckets), which is VALU work of about a millisecond.
#define GI_SLICE 32768
#define GI_THREADS 1024
// KT = the rolling k-mers' word: uint32_t when k <= 16 (the pile-up stage's k = 14: half the instructions of the
// 64-bit roll), uint64_t otherwise.  The bucket of a k-mer relative to the slice needs no group bits: the group's
// first bucket is ((g << 2k) >> shift) exactly (shift <= 2k), so rel = (canon >> shift) - sl * slice.
template <bool FILL, typename KT>
__global__ void __launch_bounds__(GI_THREADS)
k_group_index(DbView A, const int2 *__restrict__ tiles, const int32_t *__restrict__ gtile, int32_t slices_per_group,
              int32_t slice, int32_t k, int32_t kmer_mod, int32_t shift, uint32_t *__restrict__ dir,
              ulonglong2 *__restrict__ ent, const int64_t *__restrict__ goff)
{
    __shared__ uint32_t cnt[GI_SLICE];
    const int32_t g = blockIdx.x / slices_per_group, sl = blockIdx.x % slices_per_group;
    const int tid = threadIdx.x;
    const uint32_t sl0 = (uint32_t)sl * (uint32_t)slice;
    const uint32_t b0 = (uint32_t)((((uint64_t)g) << (2 * k)) >> shift) + sl0;
    for (int32_t i = tid; i < slice; i += GI_THREADS) cnt[i] = FILL ? dir[b0 + i] : 0u;
    __syncthreads();
    const uint64_t grp = (uint64_t)g;
    const KT mask = (KT)(((uint64_t)1 << (2 * k)) - 1);  // 2k == 32 with a 32-bit word: all ones
    const KmerSampler smp = kmer_sampler(kmer_mod, k);
    const int rcsh = 2 * (k - 1);
    // a wavefront per tile (16 tiles of the group in flight), a lane per 64 positions: 64 + k - 1 roll steps yield 64
    // k-mers (a thread per 16 positions spent 16 + k - 1 on 16), and the chain tile -> offsets -> bases is walked a
    // quarter as often.  Bases stream through one 8-byte word per 8 steps, the next word in flight.
    constexpr int32_t PER = KM_TILE / LANES;
    const int32_t nroll = PER + k - 1;
    const uint64_t kones = (1ull << k) - 1ull;
    for (int32_t t = gtile[g] + (tid / LANES); t < gtile[g + 1]; t += GI_THREADS / LANES) {
        const int32_t s = tiles[t].x;
        const int64_t o = A.off[s];
        const int32_t len = (int32_t)(A.off[s + 1] - o);
        const int32_t p0 = tiles[t].y + (tid & (LANES - 1)) * PER;
        if (p0 >= len) continue;
        const uint8_t *a = A.bases + o;
        KT km = 0, rc = 0;
        int32_t valid = 0;
        // soft-mask bits of the lane's k-mers (starts p0 .. p0 + 63, up to 64 + k - 1 <= 91 bits) in two words
        uint64_t mw0 = 0, mw1 = 0;
        if (A.mask_bits) {
            const int64_t gb = o + p0;
            mw0 = load8(A.mask_bits + (gb >> 3)) >> (gb & 7);
            const uint64_t hi = load8(A.mask_bits + (gb >> 3) + 8);
            if (gb & 7) mw0 |= hi << (64 - (gb & 7));
            mw1 = hi >> (gb & 7);  // bits 64 .. 64 + 56 of the window: k - 1 <= 27 are needed
        }
        uint64_t cur = load8(a + p0);
        for (int32_t wi = 0; wi * 8 < nroll; wi++) {
            const int32_t pn = p0 + 8 * (wi + 1);
            const uint64_t nxt = (8 * (wi + 1) < nroll && pn < len) ? load8(a + pn) : 0ull;
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int32_t x = wi * 8 + u, p = p0 + x;
                if (x >= nroll || p >= len) continue;
                const uint32_t c = (uint32_t)(cur >> (8 * u)) & 0xFFu;
                if (c < 4u) {
                    km = ((km << 2) | (KT)c) & mask;
                    rc = (rc >> 2) | ((KT)(3u - c) << rcsh);
                    valid++;
                } else {
                    km = 0;
                    rc = 0;
                    valid = 0;
                }
                const KT canon = km < rc ? km : rc;
                if (x < k - 1 || valid < k) continue;
                const uint32_t rel = (uint32_t)(canon >> shift) - sl0;
                if (rel >= (uint32_t)slice) continue;  // another slice's bucket
                const int32_t d = x - (k - 1);         // offset of the k-mer's first base in the lane's window
                const uint64_t mb = d == 0 ? mw0 : ((mw0 >> d) | (mw1 << (64 - d)));
                if (!kmer_sampled((uint64_t)canon, smp) || (mb & kones) != 0ull) continue;
                const uint32_t slot = atomicAdd(&cnt[rel], 1u);
                if (FILL)
                    ent[slot] = make_ulonglong2(((grp << (2 * k)) | (uint64_t)canon) | (km != canon ? 1ull << 63 : 0ull),
                                                ((uint64_t)s << 40) | (uint64_t)(goff[s] + (p - k + 1)));
            }
            cur = nxt;
        }
    }
    __syncthreads();
    for (int32_t i = tid; i < slice; i += GI_THREADS) dir[b0 + i] = cnt[i];
}
#define GI_INST(F, T)                                                                                               \
    template __global__ void k_group_index<F, T>(DbView, const int2 *, const int32_t *, int32_t, int32_t, int32_t, int32_t, \
                                                 int32_t, uint32_t *, ulonglong2 *, const int64_t *);
GI_INST(false, uint32_t)
GI_INST(true, uint32_t)
GI_INST(false, uint64_t)
GI_INST(true, uint64_t)
#undef GI_INST

extern "C" void dhk_group_index(hipStream_t st, int fill, DbView A, const int2 *tiles, const int32_t *gtile, int32_t ngroups,
                     int32_t slices_per_group, int32_t slice, int32_t k, int32_t kmer_mod, int32_t shift, uint32_t *dir,
                     ulonglong2 *ent, const int64_t *goff)
{
    if (ngroups <= 0) return;
    const dim3 grid((uint32_t)ngroups * (uint32_t)slices_per_group);
#define GI_LAUNCH(F, T)                                                                                              \
    hipLaunchKernelGGL((k_group_index<F, T>), grid, dim3(GI_THREADS), 0, st, A, tiles, gtile, slices_per_group, slice, k, \
                       kmer_mod, shift, dir, ent, goff)
    if (k <= 16 && shift < 32) {  // (a 32-bit word shifted by 32 would be undefined)
        if (fill)
            GI_LAUNCH(true, uint32_t);
        else
            GI_LAUNCH(false, uint32_t);
    } else {
        if (fill)
            GI_LAUNCH(true, uint64_t);
        else
            GI_LAUNCH(false, uint64_t);
    }
#undef GI_LAUNCH
}

// fat directory (dh_device.h): thread per bucket
__global__ void __launch_bounds__(256)
k_fat_dir(const uint32_t *__restrict__ dir, const ulonglong2 *__restrict__ ent, int64_t nb, ulonglong2 *__restrict__ fat)
{
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= nb) return;
    const uint32_t s0 = dir[b - 1], e0 = dir[b];
    ulonglong2 f;
    if (e0 == s0) {
        f.x = DH_FAT_EMPTY;
        f.y = 0;
    } else if (e0 - s0 == 1u)
        f = ent[s0];
    else {
        f.x = 1ull << 62;
        f.y = (unsigned long long)s0 | ((unsigned long long)(e0 - s0) << 32);
    }
    fat[b] = f;
}

extern "C" void dhk_fat_dir(hipStream_t st, const uint32_t *dir, const ulonglong2 *ent, int64_t nb, ulonglong2 *fat)
{
    if (nb <= 0) return;
    hipLaunchKernelGGL(k_fat_dir, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, st, dir, ent, nb, fat);
}

// exclusive scan of n uint32 in place: block sums, scan of sums, add-back
#define SCAN_PER_BLOCK 2048
__global__ void __launch_bounds__(256) k_scan_sums(const uint32_t *__restrict__ v, int64_t n,
                                                   uint32_t *__restrict__ sums)
{
    __shared__ uint32_t red[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_BLOCK;
    uint32_t acc = 0;
    for (int i = threadIdx.x; i < SCAN_PER_BLOCK; i += 256)
        if (base + i < n) acc += v[base + i];
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = red[0];
}

// total64 (optional): the sum of all elements in 64 bits -- the caller's check that the 32-bit prefix sums did not wrap
__global__ void __launch_bounds__(1024) k_scan_top(uint32_t *__restrict__ sums, int32_t nb, unsigned long long *__restrict__ total64)
{
    // single block: serial chunks per thread then a block scan of the 1024 partials
    __shared__ uint32_t part[1024];
    const int32_t per = (nb + 1023) / 1024;
    const int32_t lo = threadIdx.x * per, hi = min(nb, lo + per);
    uint32_t acc = 0;
    unsigned long long acc64 = 0;
    for (int32_t i = lo; i < hi; i++) {
        acc += sums[i];
        acc64 += sums[i];
    }
    if (total64 && acc64) atomicAdd(total64, acc64);
    part[threadIdx.x] = acc;
    __syncthreads();
    // Hillis-Steele inclusive scan
    for (int s = 1; s < 1024; s <<= 1) {
        uint32_t add = (int)threadIdx.x >= s ? part[threadIdx.x - s] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int32_t i = lo; i < hi; i++) {
        const uint32_t x = sums[i];
        sums[i] = run;
        run += x;
    }
}

__global__ void __launch_bounds__(256) k_scan_apply(uint32_t *__restrict__ v, int64_t n,
                                                    const uint32_t *__restrict__ sums)
{
    __shared__ uint32_t part[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_BLOCK;
    const int per = SCAN_PER_BLOCK / 256;
    uint32_t loc[SCAN_PER_BLOCK / 256];
    uint32_t acc = 0;
    for (int i = 0; i < per; i++) {
        const int64_t idx = base + threadIdx.x * per + i;
        loc[i] = idx < n ? v[idx] : 0;
        acc += loc[i];
    }
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 1; s < 256; s <<= 1) {
        uint32_t add = (int)threadIdx.x >= s ? part[threadIdx.x - s] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    uint32_t run = sums[blockIdx.x] + (threadIdx.x ? part[threadIdx.x - 1] : 0);
    for (int i = 0; i < per; i++) {
        const int64_t idx = base + threadIdx.x * per + i;
        if (idx < n) v[idx] = run;
        run += loc[i];
    }
}

// exclusive scan in place; sums must hold ceil(n / 2048) uint32
extern "C" void dhk_scan(hipStream_t st, uint32_t *v, int64_t n, uint32_t *sums)
{
    const int32_t nb = (int32_t)((n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK);
    hipLaunchKernelGGL(k_scan_sums, dim3(nb), dim3(256), 0, st, v, n, sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, sums, nb, (unsigned long long *)nullptr);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, st, v, n, sums);
}

// the same, adding the 64-bit total of the elements to *total64 (zeroed by the caller): a block's sum of SCAN_PER_BLOCK
// counters fits 32 bits as long as the counters themselves did not wrap, so the total tells whether the prefix sums did
extern "C" void dhk_scan_total(hipStream_t st, uint32_t *v, int64_t n, uint32_t *sums, unsigned long long *total64)
{
    const int32_t nb = (int32_t)((n + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK);
    hipLaunchKernelGGL(k_scan_sums, dim3(nb), dim3(256), 0, st, v, n, sums);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(1024), 0, st, sums, nb, total64);
    hipLaunchKernelGGL(k_scan_apply, dim3(nb), dim3(256), 0, st, v, n, sums);
}

// ------------------------------------------------------------------------------------ K4b
// Work units of the symmetric wave launch: the candidates of an item are grouped by A read
// (k_seed), and only candidates of one group depend on each other, so every group is a unit
// (item, first candidate, end candidate) of its own -- the heavy items of an all-vs-all no longer
// serialise dozens of alignments in one wavefront.  Items with more than 64 candidates stay whole
// (the cap of 64 attempted alignments per item must see them in order).
__global__ void __launch_bounds__(256)
k_units(const DhCand *__restrict__ cand, const int32_t *__restrict__ ncand, int32_t item0, int32_t nitems,
        int32_t max_cand, int4 *__restrict__ units, uint32_t *__restrict__ nunits)
{
    const int32_t it = blockIdx.x * blockDim.x + threadIdx.x;
    if (it >= nitems) return;
    const int32_t item = item0 + it;
    const int32_t nc = max(ncand[item], 0);
    if (nc == 0) return;
    const DhCand *cl = cand + (int64_t)item * max_cand;
    if (nc > LANES) {
        units[atomicAdd(nunits, 1u)] = make_int4(it, 0, nc, 0);
        return;
    }
    int32_t c0 = 0;
    while (c0 < nc) {
        int32_t c1 = c0 + 1;
        while (c1 < nc && cl[c1].aseq == cl[c0].aseq) c1++;
        units[atomicAdd(nunits, 1u)] = make_int4(it, c0, c1, 0);
        c0 = c1;
    }
}

extern "C" void dhk_units(hipStream_t st, const DhCand *cand, const int32_t *ncand, int32_t item0, int32_t nitems,
               int32_t max_cand, void *units, uint32_t *nunits)
{
    if (nitems <= 0) return;
    hipLaunchKernelGGL(k_units, dim3((nitems + 255) / 256), dim3(256), 0, st, cand, ncand, item0, nitems, max_cand,
                       (int4 *)units, nunits);
}

// ------------------------------------------------------------------------------------ compaction
// compaction of the per-item output slots: la_off / tr_off are the exclusive scans of the
// per-item LA counts and trace lengths; one wavefront per item copies its records and traces.
// ordered != 0 (symmetric mode: slots are claimed in racy order): the records of an item with at
// most 64 of them are written ordered by (bread, strand, abpos, bbpos, aepos, bepos), which makes
// the output deterministic and hands the host (A, B) pairs that are already adjacent.
__global__ void __launch_bounds__(LANES)
k_compact(const DhLa *__restrict__ la_slots, const uint16_t *__restrict__ tr_slots, int32_t trmax,
          int32_t max_la, int32_t ordered, int32_t nitems, const uint32_t *__restrict__ la_off,
          const uint32_t *__restrict__ tr_off, int64_t tr_base, DhLa *__restrict__ la_out,
          uint16_t *__restrict__ tr_out)
{
    const int32_t it = blockIdx.x;
    if (it >= nitems) return;
    const int lane = threadIdx.x;
    const uint32_t l0 = la_off[it], n = la_off[it + 1] - l0;
    uint32_t t = tr_off[it];
    if (ordered && n <= 256u) {
        // keys of the item's records in LDS; lane l ranks the records l, l + 64, ...
        __shared__ uint64_t sk1[256], sk2[256];
        __shared__ int32_t stl[256], sso[256];
        for (uint32_t x = (uint32_t)lane; x < n; x += LANES) {
            const DhLa la = la_slots[(int64_t)it * max_la + x];
            sk1[x] = ((uint64_t)(uint32_t)la.bread << 32) | ((uint64_t)(la.flags & 1u) << 31) | (uint32_t)la.abpos;
            sk2[x] = ((uint64_t)(uint32_t)la.bbpos << 32) | (uint32_t)la.aepos;
            stl[x] = la.tlen;
            sso[x] = (int32_t)la.toff;  // where the pairs start inside the slot (k_tile; 0 for the wave kernels)
        }
        __syncthreads();
        // rank among the records of the item, trace offset = prefix sum of the slot order
        for (uint32_t x = (uint32_t)lane; x < n; x += LANES) {
            const uint64_t k1 = sk1[x], k2 = sk2[x];
            int32_t rank = 0, toff = 0;
            for (uint32_t y = 0; y < n; y++) {
                const uint64_t y1 = sk1[y], y2 = sk2[y];
                const bool less = y1 < k1 || (y1 == k1 && (y2 < k2 || (y2 == k2 && y < x)));
                rank += less ? 1 : 0;
                toff += y < x ? stl[y] : 0;
            }
            DhLa la = la_slots[(int64_t)it * max_la + x];
            la.toff = tr_base + t + toff;
            la_out[l0 + rank] = la;
        }
        for (uint32_t x = 0; x < n; x++) {
            const int32_t xl = stl[x];
            const uint16_t *src = tr_slots + ((int64_t)it * max_la + x) * trmax + sso[x];
            for (int32_t e = lane; e < xl; e += LANES) tr_out[t + e] = src[e];
            t += xl;
        }
        return;
    }
    for (uint32_t x = 0; x < n; x++) {
        const int64_t slot = (int64_t)it * max_la + x;
        DhLa la = la_slots[slot];
        const uint16_t *src = tr_slots + slot * trmax + la.toff;
        for (int32_t e = lane; e < la.tlen; e += LANES) tr_out[t + e] = src[e];
        if (lane == 0) {
            la.toff = tr_base + t;
            la_out[l0 + x] = la;
        }
        t += la.tlen;
    }
}

extern "C" void dhk_compact(hipStream_t st, const DhLa *la_slots, const uint16_t *tr_slots, int32_t trmax,
                 int32_t max_la, int32_t ordered, int32_t nitems, const uint32_t *la_off,
                 const uint32_t *tr_off, int64_t tr_base, DhLa *la_out, uint16_t *tr_out)
{
    if (nitems <= 0) return;
    hipLaunchKernelGGL(k_compact, dim3(nitems), dim3(LANES), 0, st, la_slots, tr_slots, trmax, max_la, ordered,
                       nitems, la_off, tr_off, tr_base, la_out, tr_out);
}

// ------------------------------------------------------------------------------------ DUST
// Low-complexity mask (the role of DBdust, symmetric DUST with -w64 -t2.0 -m10): a window of L bases
// (L = 16, 32, 64) is low-complexity when the triplets inside it repeat too often,
//     S = sum over triplet codes of c (c - 1) / 2  >  2 (l - 1),   l = L - 2 triplets,
// i.e. a DUST score above 2.0; the mask is the union of all such windows (windows holding a
// non-ACGT base are skipped).  The score depends on the multiset of triplets only, so a sequence and
// its reverse complement get mirrored masks.  One launch per window length; a thread slides its
// window over a chunk of `chunk` starts (a tile = 256 chunks) with byte counters in LDS ([code][thread]).
template <int L>
__global__ void __launch_bounds__(256)
k_dust(const uint8_t *__restrict__ bases, const int64_t *__restrict__ off, const int2 *__restrict__ tiles,
       int32_t ntiles, int32_t chunk, uint32_t *__restrict__ bits)
{
    __shared__ uint8_t cnt[64][256];
    const int32_t t = blockIdx.x;
    if (t >= ntiles) return;
    const int tid = threadIdx.x;
    const int32_t s = tiles[t].x;
    const int64_t o = off[s];
    const int32_t len = (int32_t)(off[s + 1] - o);
    const int32_t a0 = tiles[t].y + tid * chunk;      // first window start of this thread
    const int32_t a1 = min(a0 + chunk, len - L + 1);  // end of its window starts
    if (a0 >= a1) return;
    for (int c = 0; c < 64; c++) cnt[c][tid] = 0;
    const uint8_t *b = bases + o;
    // the triplets that enter and leave the window are two sequential streams: each keeps 8 bases in a register (one
    // unaligned 8-byte load per 6 triplets; the DB is padded) instead of three byte loads per triplet
    struct Stream {
        uint64_t w;
        int32_t p;
    };
    Stream sin{0, INT32_MIN / 2}, sout{0, INT32_MIN / 2};
    auto trip_of = [&](Stream &st, int32_t i) -> int32_t {  // code of the triplet at i, -1 when it holds a non-base
        if (i < st.p || i + 2 >= st.p + 8) {
            __builtin_memcpy(&st.w, b + i, 8);
            st.p = i;
        }
        const uint32_t v = (uint32_t)(st.w >> (8 * (i - st.p)));
        const uint32_t x = v & 0xFFu, y = (v >> 8) & 0xFFu, z = (v >> 16) & 0xFFu;
        return (x | y | z) > 3u ? -1 : (int32_t)(x << 4 | y << 2 | z);
    };
    auto trip = [&](int32_t i) -> int32_t { return trip_of(sin, i); };
    int32_t S = 0, bad = 0;
    for (int32_t i = a0; i < a0 + L - 2; i++) {
        const int32_t c = trip(i);
        if (c < 0)
            bad++;
        else
            S += cnt[c][tid]++;
    }
    for (int32_t a = a0; a < a1; a++) {
        if (bad == 0 && S > 2 * (L - 3)) {
            const int64_t g0 = o + a, g1 = g0 + L;  // mask [g0, g1)
            for (int64_t wd = g0 >> 5; wd <= (g1 - 1) >> 5; wd++) {
                const int64_t lo = max(g0, wd << 5), hi = min(g1, (wd + 1) << 5);
                const uint32_t m = (hi - lo == 32) ? 0xFFFFFFFFu : (((1u << (hi - lo)) - 1u) << (lo & 31));
                if ((bits[wd] & m) != m) atomicOr(&bits[wd], m);
            }
        }
        if (a + 1 < a1) {  // slide: triplet a leaves, triplet a + L - 2 enters
            const int32_t c0 = trip_of(sout, a), c1 = trip(a + L - 2);
            if (c0 < 0)
                bad--;
            else
                S -= --cnt[c0][tid];
            if (c1 < 0)
                bad++;
            else
                S += cnt[c1][tid]++;
        }
    }
}

extern "C" void dhk_dust(hipStream_t st, const uint8_t *bases, const int64_t *off, const int2 *tiles, int32_t ntiles,
              int32_t chunk, uint32_t *bits)
{
    if (ntiles <= 0) return;
    hipLaunchKernelGGL(k_dust<16>, dim3(ntiles), dim3(256), 0, st, bases, off, tiles, ntiles, chunk, bits);
    hipLaunchKernelGGL(k_dust<32>, dim3(ntiles), dim3(256), 0, st, bases, off, tiles, ntiles, chunk, bits);
    hipLaunchKernelGGL(k_dust<64>, dim3(ntiles), dim3(256), 0, st, bases, off, tiles, ntiles, chunk, bits);
}

// mask bits of slices: destination sequence i = source sequence sidx[i] from sbeg[i] on
__global__ void __launch_bounds__(256)
k_mask_slices(const uint32_t *__restrict__ src_bits, const int64_t *__restrict__ src_off,
              const int32_t *__restrict__ sidx, const int32_t *__restrict__ sbeg,
              const int64_t *__restrict__ dst_off, int32_t n, uint32_t *__restrict__ dst_bits)
{
    const int32_t i = blockIdx.y;
    if (i >= n) return;
    const int64_t d0 = dst_off[i], len = dst_off[i + 1] - d0, s0 = src_off[sidx[i]] + sbeg[i];
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < len; x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g = s0 + x;
        if (src_bits[g >> 5] >> (g & 31) & 1u) atomicOr(&dst_bits[(d0 + x) >> 5], 1u << ((d0 + x) & 31));
    }
}

extern "C" void dhk_mask_slices(hipStream_t st, const uint32_t *src_bits, const int64_t *src_off, const int32_t *sidx,
                     const int32_t *sbeg, const int64_t *dst_off, int32_t n, int32_t max_len, uint32_t *dst_bits)
{
    if (n <= 0) return;
    int gx = (max_len + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int32_t s0 = 0; s0 < n; s0 += 65535) {
        const int32_t cnt = n - s0 < 65535 ? n - s0 : 65535;
        hipLaunchKernelGGL(k_mask_slices, dim3(gx, cnt), dim3(256), 0, st, src_bits, src_off, sidx + s0, sbeg + s0,
                           dst_off + s0, cnt, dst_bits);
    }
}

// ---- alignment-coverage mask (maskRepetitiveRegions.d:238-430 BadAlignmentCoverageAssessor): the
// alignment intervals become +1 / -1 events in a difference array laid out like the DB plus one slot
// per sequence (an interval may end at the sequence's length); the event of position p sits at slot
// p + 1, so the exclusive scan leaves the coverage of base p at slot p + 2; coverage drops to zero at every sequence end, so
// one scan over the whole array serves all sequences.
__global__ void __launch_bounds__(256)
k_cov_events(const DhLa *__restrict__ las, int64_t n, const int64_t *__restrict__ off,
             const int64_t *__restrict__ roff, int32_t improper_only, int32_t allowance,
             uint32_t *__restrict__ diff)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DhLa l = las[i];
    const int64_t o = off[l.aread];
    if (improper_only) {  // AlignmentChain.isProper, base.d:537-557
        const int32_t alen = (int32_t)(off[l.aread + 1] - o), blen = (int32_t)(roff[l.bread + 1] - roff[l.bread]);
        const bool proper = (l.abpos <= allowance || l.bbpos <= allowance) &&
                            (l.aepos + allowance >= alen || l.bepos + allowance >= blen);
        if (proper) return;
    }
    if (l.aepos <= l.abpos) return;
    const int64_t slot = o - off[0] + l.aread + 1;
    atomicAdd(&diff[slot + l.abpos], 1u);
    atomicAdd(&diff[slot + l.aepos], 0xFFFFFFFFu);
}

extern "C" void dhk_cov_events(hipStream_t st, const DhLa *las, int64_t n, const int64_t *off, const int64_t *roff,
                    int32_t improper_only, int32_t allowance, uint32_t *diff)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_cov_events, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, las, n, off, roff, improper_only,
                       allowance, diff);
}

// bases whose coverage is outside [lower, upper] get their mask bit (runs of them are the intervals
// the assessor's event machine emits: it masks from an event entering a bad zone to the next event
// entering the ok zone, sequence ends closing a run)
__global__ void __launch_bounds__(256)
k_cov_mask_at(const uint32_t *__restrict__ cov, const int64_t *__restrict__ off, int32_t s0, int32_t nseq, int32_t lower,
              int32_t upper, uint32_t *__restrict__ bits)
{
    if ((int32_t)blockIdx.y >= nseq) return;
    const int32_t s = s0 + blockIdx.y;
    const int64_t o = off[s], e = off[s + 1], slot = o - off[0] + s + 1;
    // one thread per 32-bit word of the bitmap that the sequence touches
    const int64_t w0 = o >> 5, w1 = (e + 31) >> 5;
    for (int64_t w = w0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < w1; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t g0 = max(o, w << 5), g1 = min(e, (w << 5) + 32);
        uint32_t m = 0;
        for (int64_t g = g0; g < g1; g++) {
            const int32_t c = (int32_t)cov[slot + (g - o) + 1];  // exclusive scan: events at positions <= g - o
            if (c < lower || c > upper) m |= 1u << (g & 31);
        }
        if (m) atomicOr(&bits[w], m);
    }
}

extern "C" void dhk_cov_mask(hipStream_t st, const uint32_t *cov, const int64_t *off, int32_t nseq, int32_t max_len, int32_t lower,
                  int32_t upper, uint32_t *bits)
{
    if (nseq <= 0) return;
    int gx = (max_len / 32 + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    for (int32_t s0 = 0; s0 < nseq; s0 += 65535) {
        const int32_t cnt = nseq - s0 < 65535 ? nseq - s0 : 65535;
        // shifted views keep absolute offsets; the slot formula needs off[0] of the whole DB
        hipLaunchKernelGGL(k_cov_mask_at, dim3(gx, cnt), dim3(256), 0, st, cov, off, s0, cnt, lower, upper, bits);
    }
}

// ------------------------------------------------------------------------------------ utilities
// memset for large buffers: the runtime's fill kernel runs a fixed grid of 256 workgroups (one wavefront per SIMD on a
// quarter of the SIMDs) -- 2 GB took 5.6 ms = 0.36 TB/s in the chunk set-up of the mapping.  16-byte stores, a grid that
// fills the chip.
__global__ void __launch_bounds__(256) k_fill16(uint4 *__restrict__ p, int64_t n16, uint32_t v)
{
    const uint4 w = make_uint4(v, v, v, v);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) p[i] = w;
}

// head and tail up to the next 16-byte boundary go through the runtime, the body through k_fill16
extern "C" hipError_t dhk_memset(hipStream_t st, void *ptr, int value, size_t nbytes)
{
    if (nbytes < (1u << 20)) return hipMemsetAsync(ptr, value, nbytes, st);
    uint8_t *p = (uint8_t *)ptr;
    const size_t head = (size_t)((16 - ((uintptr_t)p & 15)) & 15);
    if (head) {
        const hipError_t e = hipMemsetAsync(p, value, head, st);
        if (e != hipSuccess) return e;
    }
    const size_t body = (nbytes - head) & ~(size_t)15, tail = nbytes - head - body;
    const uint32_t v = 0x01010101u * (uint32_t)(value & 255);
    const int64_t n16 = (int64_t)(body / 16);
    const int grid = (int)std::min<int64_t>((n16 + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(k_fill16, dim3(grid), dim3(256), 0, st, (uint4 *)(p + head), n16, v);
    if (tail) return hipMemsetAsync(p + head + body, value, tail, st);
    return hipGetLastError();
}

extern "C" __global__ void __launch_bounds__(256) k_or_words(uint32_t *__restrict__ dst, const uint32_t *__restrict__ a,
                                                    const uint32_t *__restrict__ b, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = a[i] | b[i];
}
extern "C" void dhk_or_words(hipStream_t st, uint32_t *dst, const uint32_t *a, const uint32_t *b, int64_t n)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_or_words, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, dst, a, b, n);
}
