// dh_maskops.hip -- the kernels of dh_mask_combine and dh_la_tandem_mask (lane code and layouts: dh_maskops.h; driver:
// dh_maskops.cpp).  gfx950, wave64.  All of them work on one launch group and on one lane per element of the whole group: no
// kernel knows where a contig begins.
//
//   k_mo_events<PLACE>     one lane per interval (the lane finds its mask and contig by a binary search in the segment
//                          offsets): counts the non-empty ones, then (after a scan) writes their two keys.
//   k_mo_events_la<PLACE>  the same, one lane per alignment record, by the tandem rule.
//   k_mo_events_runs       one lane per run of the normalised masks: its two keys on its contig.
//   k_rx_hist              one workgroup per tile of keys: 256 bins in LDS (LDS atomics), written digit-major.
//   k_rx_scatter           one workgroup per tile, rounds of 256 keys in the tile's order: the lanes of a wavefront with the
//                          same digit by eight ballots, a count per wavefront and digit through LDS, a running count per digit
//                          over the rounds; destination = scanned hist[digit][tile] + the stable rank in the tile.
//   k_mo_deltas            one lane per event: the two deltas and the boundary flag (entry n: 0, so that the scan ends in the total).
//   k_mo_bounds            the boundary lanes: (unit, pos) and the kept state behind it, compacted.
//   k_mo_edges, k_mo_runs  one lane per boundary: differs from the boundary in front; edge 2r begins run r, edge 2r + 1 ends it.
//   k_mo_heads, k_mo_join  one lane per run: starts a group; the head writes begin, the tail end.
//   k_mo_sizes, k_mo_pick  one lane per run: long enough; compaction.
//   k_mo_output            one lane per run: the (begin, end) pair; one lane per contig: a binary search for its first run.
//
// The counts that only the device knows (boundaries, runs) stay there: the kernels are launched over the capacity and read
// the count.  Every index is bounded by it: an event index by n, a boundary by the scanned flags' total <= n, a run by half the
// edges <= n / 2 = the capacity of the run arrays.  No global atomics.
#include <hip/hip_runtime.h>

#include "dh_maskops.h"

using mo::u64;

static inline dim3 mo_grid(int64_t n) { return dim3((unsigned)((n + MO_BLOCK - 1) / MO_BLOCK)); }
#define MO_LANE const int64_t i = (int64_t)blockIdx.x * MO_BLOCK + threadIdx.x

// segoff[nseg + 1]: the first interval of every (mask, contig) of the group, mask-major, the subtract mask last; lanes [i0, i0 + n);
// unit_masks: the key's unit is mask * ncg + contig (normalising) or the contig; base (may be NULL): runs whose keys lie in front
template <bool PLACE>
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_events(const int32_t *__restrict__ iv, const int32_t *__restrict__ segoff, int32_t nseg, int64_t i0, int64_t n, int32_t ncg, int32_t nmasks,
            bool unit_masks, int32_t posbits, uint32_t *idx, const uint32_t *__restrict__ base, u64 *__restrict__ keys)
{
    MO_LANE;
    if (i > n) return;
    if (i == n) {
        if (!PLACE) idx[n] = 0;
        return;
    }
    const int32_t b = iv[2 * (i0 + i)], e = iv[2 * (i0 + i) + 1];
    if (!PLACE) {
        idx[i] = b < e;
        return;
    }
    if (b >= e) return;
    const int32_t s = (int32_t)mo::upper_bound(segoff, (int64_t)nseg + 1, (int32_t)(i0 + i)) - 1;
    const int32_t mask = s / ncg, c = s - mask * ncg;
    const u64 unit = unit_masks ? (u64)s : (u64)c;
    const int64_t at = 2 * ((int64_t)idx[i] + (base ? (int64_t)*base : 0));
    keys[at] = mo::event_key(unit, b, mask == nmasks, false, posbits);
    keys[at + 1] = mo::event_key(unit, e, mask == nmasks, true, posbits);
}

template <bool PLACE>
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_events_la(const dh_la *__restrict__ las, int64_t n, int32_t first_read, int32_t min_len, int32_t posbits, uint32_t *idx, u64 *__restrict__ keys)
{
    MO_LANE;
    if (i > n) return;
    if (i == n) {
        if (!PLACE) idx[n] = 0;
        return;
    }
    int32_t b, e;
    const bool counts = mo::tandem_interval(las[i], min_len, &b, &e);
    if (!PLACE) {
        idx[i] = counts;
        return;
    }
    if (!counts) return;
    const u64 unit = (u64)(las[i].aread - first_read);
    keys[2 * (int64_t)idx[i]] = mo::event_key(unit, b, false, false, posbits);
    keys[2 * (int64_t)idx[i] + 1] = mo::event_key(unit, e, false, true, posbits);
}

__global__ void __launch_bounds__(MO_BLOCK)
k_mo_events_runs(const u64 *__restrict__ rb, const u64 *__restrict__ re, const uint32_t *__restrict__ nr, int32_t ncg, int32_t posbits,
                 u64 *__restrict__ keys)
{
    MO_LANE;
    if (i >= (int64_t)*nr) return;
    const u64 unit = mo::at_unit(rb[i], posbits) % (u64)ncg;
    keys[2 * i] = mo::event_key(unit, mo::at_pos(rb[i], posbits), false, false, posbits);
    keys[2 * i + 1] = mo::event_key(unit, mo::at_pos(re[i], posbits), false, true, posbits);
}

// ---------------------------------------------------------------------------------------------------------------- the sort
__global__ void __launch_bounds__(MO_BLOCK)
k_rx_hist(const u64 *__restrict__ in, int64_t n, int32_t pass, int32_t tile_keys, uint32_t *__restrict__ hist, int32_t ntiles)
{
    __shared__ uint32_t h[256];
    const int32_t tid = (int32_t)threadIdx.x, tile = (int32_t)blockIdx.x;
    const int64_t base = (int64_t)tile * tile_keys;
    h[tid] = 0;
    __syncthreads();
    for (int32_t r0 = 0; r0 < tile_keys; r0 += MO_BLOCK) {
        const int64_t i = base + r0 + tid;
        if (i < n) atomicAdd(&h[rx::digit(in[i], pass)], 1u);
    }
    __syncthreads();
    hist[(int64_t)tid * ntiles + tile] = h[tid];
}

// hist: scanned.  A key's place: the keys of lower digits, those of its digit in the tiles in front, those of its digit in
// front of it in its tile -- the rounds in front (run), the wavefronts in front in its round (wcnt), the lanes below (ballots).
__global__ void __launch_bounds__(MO_BLOCK)
k_rx_scatter(const u64 *__restrict__ in, u64 *__restrict__ out, int64_t n, int32_t pass, int32_t tile_keys, const uint32_t *__restrict__ hist,
             int32_t ntiles)
{
    __shared__ uint32_t run[256], wcnt[MO_BLOCK / 64][256];
    const int32_t tid = (int32_t)threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = (int32_t)blockIdx.x;
    const int64_t base = (int64_t)tile * tile_keys;
    run[tid] = hist[(int64_t)tid * ntiles + tile];
    for (int w = 0; w < MO_BLOCK / 64; w++) wcnt[w][tid] = 0;
    __syncthreads();
    for (int32_t r0 = 0; r0 < tile_keys; r0 += MO_BLOCK) {  // (the same rounds for the whole workgroup)
        const int64_t i = base + r0 + tid;
        const bool active = i < n;
        const u64 key = active ? in[i] : 0;
        const int32_t d = rx::digit(key, pass);
        u64 ball[8];
        for (int b = 0; b < 8; b++) ball[b] = __ballot(active && ((d >> b) & 1));
        const u64 m = rx::peers(ball, d, __ballot(active));
        if (active && rx::leads(m, lane)) wcnt[wave][d] = (uint32_t)__popcll(m);
        __syncthreads();
        if (active) {
            uint32_t dst = run[d] + (uint32_t)rx::below(m, lane);
            for (int w = 0; w < wave; w++) dst += wcnt[w][d];
            if ((int64_t)dst < n) out[dst] = key;
        }
        __syncthreads();
        uint32_t s = 0;
        for (int w = 0; w < MO_BLOCK / 64; w++) s += wcnt[w][tid], wcnt[w][tid] = 0;
        run[tid] += s;
        __syncthreads();
    }
}

// --------------------------------------------------------------------------------------------------------------- the sweep
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_deltas(const u64 *__restrict__ keys, int64_t n, bool has_sub, uint32_t *__restrict__ da, uint32_t *__restrict__ ds, uint32_t *__restrict__ bf)
{
    MO_LANE;
    if (i > n) return;
    const u64 k = i < n ? keys[i] : 0;
    da[i] = i < n ? mo::delta_add(k) : 0;
    if (has_sub) ds[i] = i < n ? mo::delta_sub(k) : 0;
    bf[i] = i < n && mo::boundary(k, i + 1 < n ? keys[i + 1] : 0, i + 1 == n);
}

// da, ds, bf: scanned (exclusive), n + 1 entries
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_bounds(const u64 *__restrict__ keys, int64_t n, bool has_sub, int32_t min_count, const uint32_t *__restrict__ da,
            const uint32_t *__restrict__ ds, const uint32_t *__restrict__ bf, u64 *__restrict__ bat, uint8_t *__restrict__ bkept)
{
    MO_LANE;
    if (i >= n || bf[i + 1] == bf[i]) return;
    const u64 k = keys[i];
    const uint32_t b = bf[i];  // < n
    bat[b] = mo::key_at(k);
    bkept[b] = mo::kept(da[i] + mo::delta_add(k), has_sub ? ds[i] + mo::delta_sub(k) : 0u, min_count);
}

// nb: the number of boundaries; edge: n + 1 entries
__global__ void __launch_bounds__(MO_BLOCK) k_mo_edges(const uint8_t *__restrict__ bkept, const uint32_t *__restrict__ nb, int64_t n, uint32_t *__restrict__ edge)
{
    MO_LANE;
    if (i > n) return;
    edge[i] = i < (int64_t)*nb && bkept[i] != (i > 0 ? bkept[i - 1] : 0);
}

// edge: scanned.  Coverage is 0 behind a unit's last boundary, so the edges alternate begin, end and their number is even.
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_runs(const u64 *__restrict__ bat, const uint32_t *__restrict__ edge, int64_t n, u64 *__restrict__ rb, u64 *__restrict__ re, uint32_t *nr)
{
    MO_LANE;
    if (i == 0) *nr = edge[n] >> 1;
    if (i >= n || edge[i + 1] == edge[i]) return;
    const uint32_t j = edge[i];  // < n: j >> 1 < the capacity (n + 1) / 2
    (j & 1 ? re : rb)[j >> 1] = bat[i];
}

// -------------------------------------------------------------------------------------------------------------- the filter
// head: cap + 1 entries
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_heads(const u64 *__restrict__ rb, const u64 *__restrict__ re, const uint32_t *__restrict__ nr, int64_t cap, int32_t posbits, int32_t min_gap,
           uint32_t *__restrict__ head)
{
    MO_LANE;
    if (i > cap) return;
    head[i] = i < (int64_t)*nr && (i == 0 || mo::heads(re[i - 1], rb[i], posbits, min_gap));
}
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_join(const u64 *__restrict__ rb, const u64 *__restrict__ re, const uint32_t *__restrict__ nr, int64_t cap, const uint32_t *__restrict__ head,
          u64 *__restrict__ ob, u64 *__restrict__ oe, uint32_t *nout)
{
    MO_LANE;
    const int64_t m = (int64_t)*nr;  // <= cap
    if (i == 0) *nout = head[cap];
    if (i >= m) return;
    const uint32_t g = head[i + 1] - 1;  // the groups up to and with this run, less one
    if (head[i + 1] != head[i]) ob[g] = rb[i];
    if (i + 1 == m || head[i + 2] != head[i + 1]) oe[g] = re[i];
}
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_sizes(const u64 *__restrict__ rb, const u64 *__restrict__ re, const uint32_t *__restrict__ nr, int64_t cap, int32_t posbits, int32_t min_interval,
           uint32_t *__restrict__ keep)
{
    MO_LANE;
    if (i > cap) return;
    keep[i] = i < (int64_t)*nr && mo::long_enough(rb[i], re[i], posbits, min_interval);
}
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_pick(const u64 *__restrict__ rb, const u64 *__restrict__ re, const uint32_t *__restrict__ nr, int64_t cap, const uint32_t *__restrict__ keep,
          u64 *__restrict__ ob, u64 *__restrict__ oe, uint32_t *nout)
{
    MO_LANE;
    if (i == 0) *nout = keep[cap];
    if (i >= (int64_t)*nr || keep[i + 1] == keep[i]) return;
    ob[keep[i]] = rb[i], oe[keep[i]] = re[i];
}

// ptr: ncg + 1 entries; iv: a pair per run
__global__ void __launch_bounds__(MO_BLOCK)
k_mo_output(const u64 *__restrict__ rb, const u64 *__restrict__ re, const uint32_t *__restrict__ nr, int32_t ncg, int32_t posbits,
            uint32_t *__restrict__ ptr, int32_t *__restrict__ iv)
{
    MO_LANE;
    const int64_t m = (int64_t)*nr;
    if (i <= ncg) ptr[i] = (uint32_t)mo::lower_bound(rb, m, (u64)i << posbits);
    if (i < m) iv[2 * i] = mo::at_pos(rb[i], posbits), iv[2 * i + 1] = mo::at_pos(re[i], posbits);
}

// ------------------------------------------------------------------------------------------------------------ the launchers
extern "C" void dhk_scan(hipStream_t st, uint32_t *v, int64_t n, uint32_t *sums);

extern "C" void dhk_mo_events(hipStream_t st, int place, const int32_t *iv, const int32_t *segoff, int32_t nseg, int64_t i0, int64_t n, int32_t ncg,
                              int32_t nmasks, int unit_masks, int32_t posbits, uint32_t *idx, const uint32_t *base, u64 *keys)
{
    if (place)
        hipLaunchKernelGGL(k_mo_events<true>, mo_grid(n + 1), dim3(MO_BLOCK), 0, st, iv, segoff, nseg, i0, n, ncg, nmasks, unit_masks != 0, posbits, idx,
                           base, keys);
    else
        hipLaunchKernelGGL(k_mo_events<false>, mo_grid(n + 1), dim3(MO_BLOCK), 0, st, iv, segoff, nseg, i0, n, ncg, nmasks, unit_masks != 0, posbits, idx,
                           base, keys);
}
extern "C" void dhk_mo_events_la(hipStream_t st, int place, const dh_la *las, int64_t n, int32_t first_read, int32_t min_len, int32_t posbits,
                                 uint32_t *idx, u64 *keys)
{
    if (place)
        hipLaunchKernelGGL(k_mo_events_la<true>, mo_grid(n + 1), dim3(MO_BLOCK), 0, st, las, n, first_read, min_len, posbits, idx, keys);
    else
        hipLaunchKernelGGL(k_mo_events_la<false>, mo_grid(n + 1), dim3(MO_BLOCK), 0, st, las, n, first_read, min_len, posbits, idx, keys);
}
extern "C" void dhk_mo_events_runs(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t ncg, int32_t posbits, u64 *keys)
{
    if (cap > 0) hipLaunchKernelGGL(k_mo_events_runs, mo_grid(cap), dim3(MO_BLOCK), 0, st, rb, re, nr, ncg, posbits, keys);
}

// The stable LSD radix sort of n > 0 keys of `bits` bits in use: a and b are n keys each, hist 256 * ceil(n / tile_keys) words,
// sums ceil(that / 2048).  Returns the buffer that holds the sorted keys.
extern "C" u64 *dhk_rx_sort(hipStream_t st, u64 *a, u64 *b, int64_t n, int32_t bits, int32_t tile_keys, uint32_t *hist, uint32_t *sums)
{
    const int32_t ntiles = (int32_t)((n + tile_keys - 1) / tile_keys);
    for (int32_t pass = 0; pass < rx::passes_of_bits(bits); pass++) {
        hipLaunchKernelGGL(k_rx_hist, dim3(ntiles), dim3(MO_BLOCK), 0, st, a, n, pass, tile_keys, hist, ntiles);
        dhk_scan(st, hist, (int64_t)256 * ntiles, sums);
        hipLaunchKernelGGL(k_rx_scatter, dim3(ntiles), dim3(MO_BLOCK), 0, st, a, b, n, pass, tile_keys, hist, ntiles);
        std::swap(a, b);
    }
    return a;
}

// n > 0 sorted keys -> the runs rb / re ((n + 1) / 2 each) and their number *nr.  da, ds, bf: n + 1 words each; bat: n; bkept: n bytes
extern "C" void dhk_mo_sweep(hipStream_t st, const u64 *keys, int64_t n, int has_sub, int32_t min_count, uint32_t *da, uint32_t *ds, uint32_t *bf,
                             uint32_t *sums, u64 *bat, uint8_t *bkept, u64 *rb, u64 *re, uint32_t *nr)
{
    const dim3 g = mo_grid(n + 1), blk(MO_BLOCK);
    hipLaunchKernelGGL(k_mo_deltas, g, blk, 0, st, keys, n, has_sub != 0, da, ds, bf);
    dhk_scan(st, da, n + 1, sums);
    if (has_sub) dhk_scan(st, ds, n + 1, sums);
    dhk_scan(st, bf, n + 1, sums);
    hipLaunchKernelGGL(k_mo_bounds, g, blk, 0, st, keys, n, has_sub != 0, min_count, da, ds, bf, bat, bkept);
    uint32_t *edge = da;  // (free again)
    hipLaunchKernelGGL(k_mo_edges, g, blk, 0, st, bkept, bf + n, n, edge);
    dhk_scan(st, edge, n + 1, sums);
    hipLaunchKernelGGL(k_mo_runs, g, blk, 0, st, bat, edge, n, rb, re, nr);
}

// *nr runs of capacity cap in rb / re -> joined over gaps up to min_gap in ob / oe, *nout of them.  head: cap + 1 words
extern "C" void dhk_mo_close_gaps(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t posbits, int32_t min_gap,
                                  uint32_t *head, uint32_t *sums, u64 *ob, u64 *oe, uint32_t *nout)
{
    hipLaunchKernelGGL(k_mo_heads, mo_grid(cap + 1), dim3(MO_BLOCK), 0, st, rb, re, nr, cap, posbits, min_gap, head);
    dhk_scan(st, head, cap + 1, sums);
    hipLaunchKernelGGL(k_mo_join, mo_grid(cap + 1), dim3(MO_BLOCK), 0, st, rb, re, nr, cap, head, ob, oe, nout);
}
extern "C" void dhk_mo_drop_short(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t posbits, int32_t min_interval,
                                  uint32_t *keep, uint32_t *sums, u64 *ob, u64 *oe, uint32_t *nout)
{
    hipLaunchKernelGGL(k_mo_sizes, mo_grid(cap + 1), dim3(MO_BLOCK), 0, st, rb, re, nr, cap, posbits, min_interval, keep);
    dhk_scan(st, keep, cap + 1, sums);
    hipLaunchKernelGGL(k_mo_pick, mo_grid(cap + 1), dim3(MO_BLOCK), 0, st, rb, re, nr, cap, keep, ob, oe, nout);
}
extern "C" void dhk_mo_output(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t ncg, int32_t posbits, uint32_t *ptr,
                              int32_t *iv)
{
    hipLaunchKernelGGL(k_mo_output, mo_grid(std::max<int64_t>(cap, (int64_t)ncg + 1)), dim3(MO_BLOCK), 0, st, rb, re, nr, ncg, posbits, ptr, iv);
}
