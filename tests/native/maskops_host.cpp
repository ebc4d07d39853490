// TEST INFRASTRUCTURE -- the lane code and the host plan of dh_mask_combine / dh_la_tandem_mask (dentist_amd/csrc/dh_maskops.h)
// compiled for the CPU and played the way the kernels of dh_maskops.hip run it: one loop iteration per lane, 64-lane wavefronts
// whose ballots are loops over the lanes, workgroups whose barriers are the ends of loops over the threads, whole workgroup
// tiles for the rank of the sort.  Every device buffer is a heap block of exactly the size the driver (dh_maskops.cpp, mo::Sizes)
// gives it, so an access behind the keys, the scanned words, the runs or the output is a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../dentist_amd/csrc/dh_maskops.h"

using mo::u64;

namespace {

template <typename T>
struct Buf {  // exactly `n` elements (at least one, as the scratch slots are)
    std::unique_ptr<T[]> p;
    explicit Buf(size_t n) : p(new T[n ? n : 1]()) {}
    T *get() { return p.get(); }
    T &operator[](size_t i) { return p[i]; }
};

void serial(int64_t m, const std::function<void(int64_t, int64_t)> &body)
{
    // chunks in descending order: the lowest offending index must win whatever the order
    const int64_t grain = 7;
    for (int64_t lo = (m - 1) / grain * grain; m > 0 && lo >= 0; lo -= grain) body(lo, std::min(m, lo + grain));
}

void scan(uint32_t *v, int64_t n)  // dhk_scan: exclusive, in place, 32 bits that wrap
{
    uint32_t run = 0;
    for (int64_t i = 0; i < n; i++) {
        const uint32_t x = v[i];
        v[i] = run, run += x;
    }
}

// k_mo_events<PLACE>
void events(bool place, const int32_t *iv, const int32_t *segoff, int32_t nseg, int64_t i0, int64_t n, int32_t ncg, int32_t nmasks, bool unit_masks,
            int32_t posbits, uint32_t *idx, const uint32_t *base, u64 *keys)
{
    for (int64_t i = 0; i <= n; i++) {
        if (i == n) {
            if (!place) idx[n] = 0;
            continue;
        }
        const int32_t b = iv[2 * (i0 + i)], e = iv[2 * (i0 + i) + 1];
        if (!place) {
            idx[i] = b < e;
            continue;
        }
        if (b >= e) continue;
        const int32_t s = (int32_t)mo::upper_bound(segoff, (int64_t)nseg + 1, (int32_t)(i0 + i)) - 1;
        const int32_t mask = s / ncg, c = s - mask * ncg;
        const u64 unit = unit_masks ? (u64)s : (u64)c;
        const int64_t at = 2 * ((int64_t)idx[i] + (base ? (int64_t)*base : 0));
        keys[at] = mo::event_key(unit, b, mask == nmasks, false, posbits);
        keys[at + 1] = mo::event_key(unit, e, mask == nmasks, true, posbits);
    }
}

// k_mo_events_la<PLACE>
void events_la(bool place, const dh_la *las, int64_t n, int32_t first_read, int32_t min_len, int32_t posbits, uint32_t *idx, u64 *keys)
{
    for (int64_t i = 0; i <= n; i++) {
        if (i == n) {
            if (!place) idx[n] = 0;
            continue;
        }
        int32_t b, e;
        const bool counts = mo::tandem_interval(las[i], min_len, &b, &e);
        if (!place) {
            idx[i] = counts;
            continue;
        }
        if (!counts) continue;
        const u64 unit = (u64)(las[i].aread - first_read);
        keys[2 * (int64_t)idx[i]] = mo::event_key(unit, b, false, false, posbits);
        keys[2 * (int64_t)idx[i] + 1] = mo::event_key(unit, e, false, true, posbits);
    }
}

// k_rx_hist and k_rx_scatter for one pass; hist: 256 * ntiles
void rx_pass(const u64 *in, u64 *out, int64_t n, int32_t pass, int32_t tile_keys, uint32_t *hist, int32_t ntiles)
{
    for (int32_t tile = 0; tile < ntiles; tile++) {
        uint32_t h[256] = {0};
        const int64_t base = (int64_t)tile * tile_keys;
        for (int32_t r0 = 0; r0 < tile_keys; r0 += MO_BLOCK)
            for (int32_t tid = 0; tid < MO_BLOCK; tid++)
                if (base + r0 + tid < n) h[rx::digit(in[base + r0 + tid], pass)]++;
        for (int32_t tid = 0; tid < 256; tid++) hist[(int64_t)tid * ntiles + tile] = h[tid];
    }
    scan(hist, (int64_t)256 * ntiles);
    for (int32_t tile = 0; tile < ntiles; tile++) {
        uint32_t run[256], wcnt[MO_BLOCK / 64][256];
        const int64_t base = (int64_t)tile * tile_keys;
        for (int32_t tid = 0; tid < 256; tid++) run[tid] = hist[(int64_t)tid * ntiles + tile];
        memset(wcnt, 0, sizeof(wcnt));
        for (int32_t r0 = 0; r0 < tile_keys; r0 += MO_BLOCK) {
            u64 peers[MO_BLOCK];
            for (int32_t wave = 0; wave < MO_BLOCK / 64; wave++) {  // up to the first barrier
                u64 ball[8] = {0, 0, 0, 0, 0, 0, 0, 0}, act = 0;
                for (int32_t lane = 0; lane < 64; lane++) {
                    const int64_t i = base + r0 + wave * 64 + lane;
                    if (i >= n) continue;
                    act |= (u64)1 << lane;
                    for (int b = 0; b < 8; b++)
                        if ((rx::digit(in[i], pass) >> b) & 1) ball[b] |= (u64)1 << lane;
                }
                for (int32_t lane = 0; lane < 64; lane++) {
                    const int64_t i = base + r0 + wave * 64 + lane;
                    const int32_t d = i < n ? rx::digit(in[i], pass) : 0;
                    const u64 m = rx::peers(ball, d, act);
                    peers[wave * 64 + lane] = m;
                    if (i < n && rx::leads(m, lane)) wcnt[wave][d] = (uint32_t)__builtin_popcountll(m);
                }
            }
            for (int32_t tid = 0; tid < MO_BLOCK; tid++) {  // up to the second
                const int64_t i = base + r0 + tid;
                if (i >= n) continue;
                const int32_t d = rx::digit(in[i], pass), wave = tid >> 6;
                uint32_t dst = run[d] + (uint32_t)rx::below(peers[tid], tid & 63);
                for (int w = 0; w < wave; w++) dst += wcnt[w][d];
                out[dst] = in[i];  // (no guard here: a place behind the keys is a report)
            }
            for (int32_t tid = 0; tid < 256; tid++) {
                uint32_t s = 0;
                for (int w = 0; w < MO_BLOCK / 64; w++) s += wcnt[w][tid], wcnt[w][tid] = 0;
                run[tid] += s;
            }
        }
    }
}

// dhk_rx_sort
u64 *rx_sort(u64 *a, u64 *b, int64_t n, int32_t bits, int32_t tile_keys, uint32_t *hist)
{
    const int32_t ntiles = (int32_t)((n + tile_keys - 1) / tile_keys);
    for (int32_t pass = 0; pass < rx::passes_of_bits(bits); pass++) {
        rx_pass(a, b, n, pass, tile_keys, hist, ntiles);
        std::swap(a, b);
    }
    return a;
}

struct Dev {
    mo::Sizes z;
    Buf<uint32_t> idx, da, ds, bf, hist, ctr, ptr;
    Buf<u64> ka, kb, rb0, re0, rb1, re1;
    Buf<uint8_t> bkept;
    Buf<int32_t> iv;
    Dev(int64_t n_in, int64_t cap_ev, int32_t ncg, int32_t tile_keys)
        : z(n_in, cap_ev, ncg, tile_keys), idx(z.idx), da(z.ev1), ds(z.ev1), bf(z.ev1), hist(z.hist), ctr(z.ctr), ptr(z.ptr), ka(z.keys), kb(z.keys),
          rb0(z.runs), re0(z.runs), rb1(z.runs), re1(z.runs), bkept(z.bkept), iv(z.iv)
    {
    }
};

// dhk_mo_sweep
void sweep(const u64 *keys, int64_t n, bool has_sub, int32_t min_count, Dev &d, u64 *bat, u64 *rb, u64 *re, uint32_t *nr)
{
    uint32_t *da = d.da.get(), *ds = d.ds.get(), *bf = d.bf.get();
    for (int64_t i = 0; i <= n; i++) {  // k_mo_deltas
        const u64 k = i < n ? keys[i] : 0;
        da[i] = i < n ? mo::delta_add(k) : 0;
        if (has_sub) ds[i] = i < n ? mo::delta_sub(k) : 0;
        bf[i] = i < n && mo::boundary(k, i + 1 < n ? keys[i + 1] : 0, i + 1 == n);
    }
    scan(da, n + 1);
    if (has_sub) scan(ds, n + 1);
    scan(bf, n + 1);
    for (int64_t i = 0; i < n; i++) {  // k_mo_bounds
        if (bf[i + 1] == bf[i]) continue;
        const u64 k = keys[i];
        bat[bf[i]] = mo::key_at(k);
        d.bkept[bf[i]] = mo::kept(da[i] + mo::delta_add(k), has_sub ? ds[i] + mo::delta_sub(k) : 0u, min_count);
    }
    uint32_t *edge = da;
    const int64_t nb = bf[n];
    for (int64_t i = 0; i <= n; i++) edge[i] = i < nb && d.bkept[i] != (i > 0 ? d.bkept[i - 1] : 0);  // k_mo_edges
    scan(edge, n + 1);
    *nr = edge[n] >> 1;  // k_mo_runs
    for (int64_t i = 0; i < n; i++) {
        if (edge[i + 1] == edge[i]) continue;
        const uint32_t j = edge[i];
        (j & 1 ? re : rb)[j >> 1] = bat[i];
    }
}

// the filters and the output of finish_group; returns the number of runs
int64_t finish(Dev &d, int64_t cap_ev, int32_t ncg, int32_t posbits, const mo::Opts &o, int64_t *out_ptr, int32_t *out_iv, int64_t out_cap, int64_t at)
{
    const int64_t cap = cap_ev / 2;
    u64 *rb[2] = {d.rb0.get(), d.rb1.get()}, *re[2] = {d.re0.get(), d.re1.get()};
    int cur = 0, ctr = 0;
    if (o.min_gap > 0) {  // dhk_mo_close_gaps
        uint32_t *head = d.ds.get();
        const int64_t m = d.ctr[ctr];
        for (int64_t i = 0; i <= cap; i++) head[i] = i < m && (i == 0 || mo::heads(re[cur][i - 1], rb[cur][i], posbits, o.min_gap));
        scan(head, cap + 1);
        d.ctr[ctr + 1] = head[cap];
        for (int64_t i = 0; i < m; i++) {
            const uint32_t g = head[i + 1] - 1;
            if (head[i + 1] != head[i]) rb[cur ^ 1][g] = rb[cur][i];
            if (i + 1 == m || head[i + 2] != head[i + 1]) re[cur ^ 1][g] = re[cur][i];
        }
        cur ^= 1, ctr++;
    }
    if (o.min_interval > 1) {  // dhk_mo_drop_short
        uint32_t *keep = d.bf.get();
        const int64_t m = d.ctr[ctr];
        for (int64_t i = 0; i <= cap; i++) keep[i] = i < m && mo::long_enough(rb[cur][i], re[cur][i], posbits, o.min_interval);
        scan(keep, cap + 1);
        d.ctr[ctr + 1] = keep[cap];
        for (int64_t i = 0; i < m; i++)
            if (keep[i + 1] != keep[i]) rb[cur ^ 1][keep[i]] = rb[cur][i], re[cur ^ 1][keep[i]] = re[cur][i];
        cur ^= 1, ctr++;
    }
    const int64_t m = d.ctr[ctr];  // k_mo_output
    for (int64_t i = 0; i <= ncg; i++) d.ptr[i] = (uint32_t)mo::lower_bound(rb[cur], m, (u64)i << posbits);
    for (int64_t i = 0; i < m; i++) d.iv[2 * i] = mo::at_pos(rb[cur][i], posbits), d.iv[2 * i + 1] = mo::at_pos(re[cur][i], posbits);
    if (at + m > out_cap) return -2;
    for (int32_t c = 0; c <= ncg; c++) out_ptr[c] = at + d.ptr[c];
    memcpy(out_iv + 2 * at, d.iv.get(), sizeof(int32_t) * 2 * (size_t)m);
    return m;
}

int fail(char *msg, int32_t msg_cap, const std::string &s)
{
    snprintf(msg, (size_t)msg_cap, "%s", s.c_str());
    return -1;
}

}  // namespace

// dh_mask_combine as dh_maskops.cpp drives it.  opts4: min_count, min_gap, min_interval, 0.  out_ptr: ncontigs + 1; out_iv: cap
// pairs; info: events, sort passes, groups.  Returns the number of runs, -1 for a refusal (msg), -2 when cap is too small.
extern "C" int64_t maskops_host(const int64_t *const *ptr, const int32_t *const *iv, int32_t nmasks, const int64_t *sub_ptr, const int32_t *sub_iv,
                                const int64_t *contig_off, int32_t ncontigs, const int32_t *opts4, int32_t tile_keys, int64_t chunk_bytes,
                                int64_t *out_ptr, int32_t *out_iv, int64_t cap, int64_t *info, char *msg, int32_t msg_cap)
{
    const mo::Opts o{opts4[0], opts4[1], opts4[2], 0};
    if (const char *w = mo::check_opts(o, nmasks)) return fail(msg, msg_cap, w);
    std::vector<const int64_t *> mp(ptr, ptr + nmasks);
    std::vector<const int32_t *> mi(iv, iv + nmasks);
    mp.push_back(sub_ptr), mi.push_back(sub_iv);
    mo::Fault f;
    std::vector<int64_t> ne_in, ne_sub;
    mo::check_masks(mp.data(), mi.data(), nmasks, contig_off, ncontigs, serial, ne_in, ne_sub, f);
    if (f.any()) return fail(msg, msg_cap, mo::fault_text(f, nmasks));
    mo::Plan pl;
    mo::make_groups(mp.data(), nmasks, contig_off, ncontigs, ne_in, ne_sub, chunk_bytes, pl);
    info[0] = info[1] = info[2] = 0;
    for (const mo::Group &g : pl.groups) info[0] += 2 * g.nonempty;
    const bool normalise = o.min_count > 1;
    int64_t total = 0;
    out_ptr[0] = 0;
    for (const mo::Group &g : pl.groups) {
        const int32_t ncg = g.c1 - g.c0, nseg = (nmasks + 1) * ncg;
        const int64_t n_all = g.intervals, n_sub = g.sub_intervals, n_in = n_all - n_sub, ne_in = g.nonempty - g.sub_nonempty;
        if (ne_in == 0) {
            for (int32_t c = g.c0; c <= g.c1; c++) out_ptr[c] = total;
            continue;
        }
        const int32_t posbits = mo::bits_of((u64)g.maxlen);
        const int32_t bits1 = mo::bits_of((u64)nmasks * (u64)ncg - 1) + posbits + 2, bits2 = mo::bits_of((u64)ncg - 1) + posbits + 2;
        if (normalise && bits1 > 64) return fail(msg, msg_cap, "masks times contigs times the longest contig do not fit a key");
        info[2]++;
        Buf<int32_t> in((size_t)(2 * n_all + nseg + 1));
        int32_t *segoff = in.get() + 2 * n_all;
        int64_t at = 0;
        for (int32_t k = 0; k <= nmasks; k++)
            for (int32_t c = g.c0; c < g.c1; c++) {
                segoff[(size_t)k * ncg + (c - g.c0)] = (int32_t)at;
                if (!mp[(size_t)k]) continue;
                const int64_t i0 = mp[(size_t)k][c], m = mp[(size_t)k][c + 1] - i0;
                if (m) memcpy(in.get() + 2 * at, mi[(size_t)k] + 2 * i0, sizeof(int32_t) * 2 * (size_t)m);
                at += m;
            }
        segoff[nseg] = (int32_t)at;
        const int64_t cap_ev = 2 * g.nonempty;
        Dev d(n_all, cap_ev, ncg, tile_keys);
        int64_t ev;
        if (!normalise) {
            events(false, in.get(), segoff, nseg, 0, n_all, ncg, nmasks, false, posbits, d.idx.get(), nullptr, d.ka.get());
            scan(d.idx.get(), n_all + 1);
            events(true, in.get(), segoff, nseg, 0, n_all, ncg, nmasks, false, posbits, d.idx.get(), nullptr, d.ka.get());
            ev = 2 * g.nonempty;
        } else {
            events(false, in.get(), segoff, nseg, 0, n_in, ncg, nmasks, true, posbits, d.idx.get(), nullptr, d.ka.get());
            scan(d.idx.get(), n_in + 1);
            events(true, in.get(), segoff, nseg, 0, n_in, ncg, nmasks, true, posbits, d.idx.get(), nullptr, d.ka.get());
            u64 *sorted = rx_sort(d.ka.get(), d.kb.get(), 2 * ne_in, bits1, tile_keys, d.hist.get());
            info[1] += rx::passes_of_bits(bits1);
            sweep(sorted, 2 * ne_in, false, 1, d, sorted == d.ka.get() ? d.kb.get() : d.ka.get(), d.rb0.get(), d.re0.get(), d.ctr.get());
            const int64_t nruns = d.ctr[0];
            for (int64_t i = 0; i < nruns; i++) {  // k_mo_events_runs
                const u64 unit = mo::at_unit(d.rb0[i], posbits) % (u64)ncg;
                d.ka[2 * i] = mo::event_key(unit, mo::at_pos(d.rb0[i], posbits), false, false, posbits);
                d.ka[2 * i + 1] = mo::event_key(unit, mo::at_pos(d.re0[i], posbits), false, true, posbits);
            }
            if (n_sub > 0) {
                events(false, in.get(), segoff, nseg, n_in, n_sub, ncg, nmasks, false, posbits, d.idx.get(), d.ctr.get(), d.ka.get());
                scan(d.idx.get(), n_sub + 1);
                events(true, in.get(), segoff, nseg, n_in, n_sub, ncg, nmasks, false, posbits, d.idx.get(), d.ctr.get(), d.ka.get());
            }
            ev = 2 * (nruns + g.sub_nonempty);
        }
        if (ev == 0) {
            for (int32_t c = g.c0; c <= g.c1; c++) out_ptr[c] = total;
            continue;
        }
        u64 *sorted = rx_sort(d.ka.get(), d.kb.get(), ev, bits2, tile_keys, d.hist.get());
        info[1] += rx::passes_of_bits(bits2);
        sweep(sorted, ev, g.sub_nonempty > 0, o.min_count, d, sorted == d.ka.get() ? d.kb.get() : d.ka.get(), d.rb0.get(), d.re0.get(), d.ctr.get());
        const int64_t m = finish(d, cap_ev, ncg, posbits, o, out_ptr + g.c0, out_iv, cap, total);
        if (m < 0) return m;
        total += m;
    }
    return total;
}

// dh_la_tandem_mask as dh_maskops.cpp drives it
extern "C" int64_t maskops_tandem_host(const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads, int32_t first_read, int32_t min_len,
                                       int32_t tile_keys, int64_t *out_ptr, int32_t *out_iv, int64_t cap, int64_t *info, char *msg, int32_t msg_cap)
{
    int64_t maxlen = 0;
    std::string why;
    const int64_t counted = mo::check_tandem(las, n, read_off, nreads, first_read, min_len, &maxlen, why);
    if (counted < 0) return fail(msg, msg_cap, why);
    info[0] = 2 * counted, info[1] = 0, info[2] = counted > 0;
    for (int32_t r = 0; r <= nreads; r++) out_ptr[r] = 0;
    if (counted == 0) return 0;
    const int32_t posbits = mo::bits_of((u64)maxlen), bits = mo::bits_of((u64)nreads - 1) + posbits + 2;
    Dev d(n, 2 * counted, nreads, tile_keys);
    Buf<dh_la> in((size_t)n);
    memcpy(in.get(), las, sizeof(dh_la) * (size_t)n);
    events_la(false, in.get(), n, first_read, min_len, posbits, d.idx.get(), d.ka.get());
    scan(d.idx.get(), n + 1);
    events_la(true, in.get(), n, first_read, min_len, posbits, d.idx.get(), d.ka.get());
    u64 *sorted = rx_sort(d.ka.get(), d.kb.get(), 2 * counted, bits, tile_keys, d.hist.get());
    info[1] = rx::passes_of_bits(bits);
    sweep(sorted, 2 * counted, false, 1, d, sorted == d.ka.get() ? d.kb.get() : d.ka.get(), d.rb0.get(), d.re0.get(), d.ctr.get());
    return finish(d, 2 * counted, nreads, posbits, mo::Opts{1, 0, 0, 0}, out_ptr, out_iv, cap, 0);
}

// the sort alone: n keys sorted in place by their low `bits` bits, stable (whatever lies above them keeps its order)
extern "C" void maskops_rx_sort_host(u64 *keys, int64_t n, int32_t bits, int32_t tile_keys)
{
    if (n <= 0) return;
    const mo::Sizes z(0, n, 0, tile_keys);
    Buf<u64> a((size_t)n), b((size_t)n);
    Buf<uint32_t> hist(z.hist);
    memcpy(a.get(), keys, sizeof(u64) * (size_t)n);
    memcpy(keys, rx_sort(a.get(), b.get(), n, bits, tile_keys, hist.get()), sizeof(u64) * (size_t)n);
}

// the key layout: the fields back out of a key
extern "C" void maskops_key_host(uint64_t unit, int32_t pos, int32_t is_sub, int32_t is_end, int32_t posbits, uint64_t *key, uint64_t *unit_out,
                                 int32_t *pos_out, uint32_t *dadd, uint32_t *dsub)
{
    const u64 k = mo::event_key(unit, pos, is_sub != 0, is_end != 0, posbits);
    *key = k, *unit_out = mo::at_unit(mo::key_at(k), posbits), *pos_out = mo::at_pos(mo::key_at(k), posbits);
    *dadd = mo::delta_add(k), *dsub = mo::delta_sub(k);
}

// the host-side read_united_masks route of tools/dazz_main.cpp (sort and merge per contig), for the rate comparison only
extern "C" int64_t maskops_host_route(const int64_t *const *ptr, const int32_t *const *iv, int32_t nmasks, int32_t ncontigs, int64_t *out_ptr,
                                      int32_t *out_iv)
{
    std::vector<std::pair<int32_t, int32_t>> v;
    int64_t total = 0;
    out_ptr[0] = 0;
    for (int32_t c = 0; c < ncontigs; c++) {
        v.clear();
        for (int32_t k = 0; k < nmasks; k++)
            for (int64_t i = ptr[k][c]; i < ptr[k][c + 1]; i++)
                if (iv[k][2 * i + 1] > iv[k][2 * i]) v.emplace_back(iv[k][2 * i], iv[k][2 * i + 1]);
        std::sort(v.begin(), v.end());
        const int64_t at = total;
        for (const auto &x : v) {
            if (total > at && x.first <= out_iv[2 * total - 1])
                out_iv[2 * total - 1] = std::max(out_iv[2 * total - 1], x.second);
            else
                out_iv[2 * total] = x.first, out_iv[2 * total + 1] = x.second, total++;
        }
        out_ptr[c + 1] = total;
    }
    return total;
}
