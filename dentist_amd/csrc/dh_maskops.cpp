// dh_maskops.cpp -- host side of dh_mask_combine (`dentist merge-masks`, `dentist filter-mask`, the ReferenceRegion operators)
// and dh_la_tandem_mask (TANmask's rule) on the device.  Kernels: dh_maskops.hip; lane code, key layout and the plan:
// dh_maskops.h.
//
// The call: everything is checked on the host threads; then every launch group -- whole contigs, as many as DH_MASKOPS_CHUNK_MB hold --
// uploads its intervals, writes two keys per non-empty interval, sorts them device-wide (rx: as many 8-bit passes as the keys
// have digits in use), sweeps them into runs, closes gaps, drops short runs, and builds the offsets; the runs and offsets come
// back and are appended to the result.  With min_count > 1 the masks are normalised on their own first: the same sort and sweep
// over keys that carry the mask in front of the contig, min_count 1; its runs become the events of the second sweep (one wait
// in between: the number of runs sizes the second sort).  What the device alone knows otherwise (boundaries, runs) stays there.
// DH_TRACE prints a line per call.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "dh_maskops.h"

using mo::u64;

extern "C" void dhk_mo_events(hipStream_t st, int place, const int32_t *iv, const int32_t *segoff, int32_t nseg, int64_t i0, int64_t n, int32_t ncg,
                              int32_t nmasks, int unit_masks, int32_t posbits, uint32_t *idx, const uint32_t *base, u64 *keys);
extern "C" void dhk_mo_events_la(hipStream_t st, int place, const dh_la *las, int64_t n, int32_t first_read, int32_t min_len, int32_t posbits,
                                 uint32_t *idx, u64 *keys);
extern "C" void dhk_mo_events_runs(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t ncg, int32_t posbits, u64 *keys);
extern "C" u64 *dhk_rx_sort(hipStream_t st, u64 *a, u64 *b, int64_t n, int32_t bits, int32_t tile_keys, uint32_t *hist, uint32_t *sums);
extern "C" void dhk_mo_sweep(hipStream_t st, const u64 *keys, int64_t n, int has_sub, int32_t min_count, uint32_t *da, uint32_t *ds, uint32_t *bf,
                             uint32_t *sums, u64 *bat, uint8_t *bkept, u64 *rb, u64 *re, uint32_t *nr);
extern "C" void dhk_mo_close_gaps(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t posbits, int32_t min_gap,
                                  uint32_t *head, uint32_t *sums, u64 *ob, u64 *oe, uint32_t *nout);
extern "C" void dhk_mo_drop_short(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t posbits, int32_t min_interval,
                                  uint32_t *keep, uint32_t *sums, u64 *ob, u64 *oe, uint32_t *nout);
extern "C" void dhk_mo_output(hipStream_t st, const u64 *rb, const u64 *re, const uint32_t *nr, int64_t cap, int32_t ncg, int32_t posbits, uint32_t *ptr,
                              int32_t *iv);

static_assert(sizeof(mo::Opts) == sizeof(dh_mask_opts) && sizeof(u64) == sizeof(uint64_t), "dh_maskops.h states the layouts");

struct dh_mask_set {
    int32_t ncontigs = 0;
    std::vector<int64_t> ptr;  // ncontigs + 1
    std::vector<int32_t> iv;   // (begin, end) pairs
    int64_t events = 0, sort_passes = 0, groups = 0;
};

namespace {

// the device buffers of one launch group, carved from one slot of the arena.  in_bytes: the uploaded input (intervals and
// segment offsets, or alignment records); n_in: its lanes; cap_ev: no sweep of the group sees more events (even)
struct Work {
    char *input;
    uint32_t *idx, *da, *ds, *bf, *hist, *sums, *ctr, *ptr;
    u64 *ka, *kb, *rb[2], *re[2];
    uint8_t *bkept;
    int32_t *iv;
};
int carve(dh_ctx *ctx, size_t in_bytes, int64_t n_in, int64_t cap_ev, int32_t ncg, int32_t tile_keys, Work &w)
{
    const mo::Sizes z(n_in, cap_ev, ncg, tile_keys);
    size_t at = 0;
    auto take = [&](size_t bytes) {
        const size_t here = at;
        at += (bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t o_in = take(in_bytes), o_idx = take(4 * z.idx), o_da = take(4 * z.ev1), o_ds = take(4 * z.ev1), o_bf = take(4 * z.ev1),
                 o_hist = take(4 * z.hist), o_sums = take(4 * z.sums), o_ctr = take(4 * z.ctr), o_ptr = take(4 * z.ptr), o_ka = take(8 * z.keys),
                 o_kb = take(8 * z.keys), o_rb0 = take(8 * z.runs), o_re0 = take(8 * z.runs), o_rb1 = take(8 * z.runs), o_re1 = take(8 * z.runs),
                 o_bk = take(z.bkept), o_iv = take(4 * z.iv);
    char *base;
    if (int rc = dh_scr(ctx, SLOT_MO_WORK, at, &base)) return rc;
    w.input = base + o_in, w.idx = (uint32_t *)(base + o_idx), w.da = (uint32_t *)(base + o_da), w.ds = (uint32_t *)(base + o_ds);
    w.bf = (uint32_t *)(base + o_bf), w.hist = (uint32_t *)(base + o_hist), w.sums = (uint32_t *)(base + o_sums), w.ctr = (uint32_t *)(base + o_ctr);
    w.ptr = (uint32_t *)(base + o_ptr), w.ka = (u64 *)(base + o_ka), w.kb = (u64 *)(base + o_kb), w.rb[0] = (u64 *)(base + o_rb0);
    w.re[0] = (u64 *)(base + o_re0), w.rb[1] = (u64 *)(base + o_rb1), w.re[1] = (u64 *)(base + o_re1), w.bkept = (uint8_t *)(base + o_bk);
    w.iv = (int32_t *)(base + o_iv);
    return DH_OK;
}

struct Knobs {
    int32_t tile_keys;
    int64_t chunk_bytes;
    Knobs()
    {
        tile_keys = (int32_t)dh_env_knob("DH_MASKOPS_TILE_KEYS", RX_TILE_KEYS, RX_TILE_KEYS_MIN, RX_TILE_KEYS) / MO_BLOCK * MO_BLOCK;
        chunk_bytes = mo::chunk_bytes_of(getenv("DH_MASKOPS_CHUNK_MB"));
    }
};

// the stage times of a DH_TRACE line (only when asked for: each lap is a wait; an error of the wait shows at the next call)
enum { T_PLAN = 0, T_EVENTS = 1, T_SORT = 2, T_SWEEP = 3, T_FILTER = 4, T_COUNT = 5 };
struct Laps {
    bool on = getenv("DH_TRACE") != nullptr;
    double ms[T_COUNT] = {0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(hipStream_t st, int k)
    {
        if (!on) return;
        if (st) (void)hipStreamSynchronize(st);
        ms[k] += dh_ms_since(t);
        t = std::chrono::steady_clock::now();
    }
};

// `events` keys of `bits` bits in w.ka -> sorted and swept (the runs in w.rb[0] / w.re[0], their number in w.ctr[0])
void sort_and_sweep(hipStream_t st, Work &w, int64_t events, int32_t bits, int32_t tile_keys, bool has_sub, int32_t min_count, dh_mask_set *res,
                    Laps &laps)
{
    laps.lap(st, T_EVENTS);
    u64 *sorted = dhk_rx_sort(st, w.ka, w.kb, events, bits, tile_keys, w.hist, w.sums);
    res->sort_passes += rx::passes_of_bits(bits);
    laps.lap(st, T_SORT);
    dhk_mo_sweep(st, sorted, events, has_sub, min_count, w.da, w.ds, w.bf, w.sums, sorted == w.ka ? w.kb : w.ka, w.bkept, w.rb[0], w.re[0], w.ctr);
    laps.lap(st, T_SWEEP);
}

// the runs of the group's last sweep -> filtered, with offsets, downloaded and appended to the result as contigs [c0, c0 + ncg)
int finish_group(dh_ctx *ctx, const std::string &name, Work &w, int64_t cap_ev, int32_t c0, int32_t ncg, int32_t posbits, const mo::Opts &o,
                 dh_mask_set *res)
{
    hipStream_t st = ctx->stream;
    const int64_t cap = cap_ev / 2;
    int cur = 0, ctr = 0;
    if (o.min_gap > 0) {
        dhk_mo_close_gaps(st, w.rb[cur], w.re[cur], w.ctr + ctr, cap, posbits, o.min_gap, w.ds, w.sums, w.rb[cur ^ 1], w.re[cur ^ 1], w.ctr + ctr + 1);
        cur ^= 1, ctr++;
    }
    if (o.min_interval > 1) {  // (a run has a base)
        dhk_mo_drop_short(st, w.rb[cur], w.re[cur], w.ctr + ctr, cap, posbits, o.min_interval, w.bf, w.sums, w.rb[cur ^ 1], w.re[cur ^ 1], w.ctr + ctr + 1);
        cur ^= 1, ctr++;
    }
    dhk_mo_output(st, w.rb[cur], w.re[cur], w.ctr + ctr, cap, ncg, posbits, w.ptr, w.iv);
    HIPCHK(hipGetLastError());
    std::vector<uint32_t> h_ptr((size_t)ncg + 1);
    HIPCHK(hipMemcpyAsync(h_ptr.data(), w.ptr, sizeof(uint32_t) * ((size_t)ncg + 1), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    const size_t total = h_ptr[(size_t)ncg];
    if ((int64_t)total > cap) return dh_fail(DH_EOVERFLOW, name + ": more runs than events allow");
    const size_t at = res->iv.size();
    res->iv.resize(at + 2 * total);
    if (total) HIPCHK(hipMemcpyAsync(res->iv.data() + at, w.iv, sizeof(int32_t) * 2 * total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int32_t c = 0; c <= ncg; c++) res->ptr[(size_t)(c0 + c)] = (int64_t)(at / 2) + h_ptr[(size_t)c];
    return DH_OK;
}

}  // namespace

extern "C" void dh_default_mask_opts(dh_mask_opts *o)
{
    if (o) *o = dh_mask_opts{1, 0, 0, 0};
}

extern "C" int dh_mask_combine(dh_ctx *ctx, const int64_t *const *ptr, const int32_t *const *iv, int32_t nmasks, const int64_t *sub_ptr,
                               const int32_t *sub_iv, const int64_t *contig_off, int32_t ncontigs, const dh_mask_opts *opts, dh_mask_set **out)
{
    const std::string name("dh_mask_combine");
    if (!ctx || !ptr || !iv || !contig_off || !opts || !out || nmasks < 1 || ncontigs < 0 || (sub_ptr == nullptr) != (sub_iv == nullptr))
        return dh_fail(DH_EINVAL, name + ": bad argument");
    for (int32_t k = 0; k < nmasks; k++)
        if (!ptr[k] || !iv[k]) return dh_fail(DH_EINVAL, name + ": bad argument");
    const mo::Opts o{opts->min_count, opts->min_gap, opts->min_interval, 0};
    if (const char *w = mo::check_opts(o, nmasks)) return dh_fail(DH_EINVAL, name + ": " + w);
    const auto t_call = std::chrono::steady_clock::now();
    Laps laps;
    std::vector<const int64_t *> mp(ptr, ptr + nmasks);
    std::vector<const int32_t *> mi(iv, iv + nmasks);
    mp.push_back(sub_ptr), mi.push_back(sub_iv);
    mo::Fault f;
    std::vector<int64_t> ne_in, ne_sub;
    mo::check_masks(mp.data(), mi.data(), nmasks, contig_off, ncontigs, dh_plan_runner<DH_PLAN_GRAIN>, ne_in, ne_sub, f);
    if (f.any()) return dh_fail(DH_EINVAL, name + ": " + mo::fault_text(f, nmasks));
    const Knobs knobs;
    mo::Plan pl;
    mo::make_groups(mp.data(), nmasks, contig_off, ncontigs, ne_in, ne_sub, knobs.chunk_bytes, pl);
    if (pl.intervals >= ((int64_t)1 << 30)) return dh_fail(DH_EOVERFLOW, name + ": 2^30 intervals or more");
    std::unique_ptr<dh_mask_set> res(new dh_mask_set);
    res->ncontigs = ncontigs;
    res->ptr.assign((size_t)ncontigs + 1, 0);
    for (const mo::Group &g : pl.groups) res->events += 2 * g.nonempty;
    laps.lap(nullptr, T_PLAN);
    const bool normalise = o.min_count > 1;  // (with min_count 1 a base counts as soon as one interval of any mask has it)
    bool up = false;
    std::vector<int32_t, PinnedAlloc<int32_t>> h_in;
    for (const mo::Group &g : pl.groups) {
        const int32_t ncg = g.c1 - g.c0, nseg = (nmasks + 1) * ncg;
        const int64_t n_all = g.intervals, n_sub = g.sub_intervals, n_in = n_all - n_sub, ne_in = g.nonempty - g.sub_nonempty;
        if (ne_in == 0) {  // nothing to keep
            for (int32_t c = g.c0; c <= g.c1; c++) res->ptr[(size_t)c] = (int64_t)res->iv.size() / 2;
            continue;
        }
        const int32_t posbits = mo::bits_of((u64)g.maxlen);
        const int32_t bits1 = mo::bits_of((u64)nmasks * (u64)ncg - 1) + posbits + 2, bits2 = mo::bits_of((u64)ncg - 1) + posbits + 2;
        if (normalise && bits1 > 64) return dh_fail(DH_EOVERFLOW, name + ": masks times contigs times the longest contig do not fit a key");
        if (!up) {
            HIPCHK(hipSetDevice(ctx->device));
            up = true;
        }
        hipStream_t st = ctx->stream;
        res->groups++;
        // ---- upload: the pairs mask-major (the subtract mask last), behind them the first pair of every (mask, contig)
        HIPCHK(hipStreamSynchronize(st));  // (h_in is read by the copy of the group before)
        h_in.resize((size_t)(2 * n_all + nseg + 1));
        int32_t *segoff = h_in.data() + 2 * n_all;
        int64_t at = 0;
        for (int32_t k = 0; k <= nmasks; k++)
            for (int32_t c = g.c0; c < g.c1; c++) {
                segoff[(size_t)k * ncg + (c - g.c0)] = (int32_t)at;
                if (!mp[(size_t)k]) continue;
                const int64_t i0 = mp[(size_t)k][c], m = mp[(size_t)k][c + 1] - i0;
                if (m) memcpy(h_in.data() + 2 * at, mi[(size_t)k] + 2 * i0, sizeof(int32_t) * 2 * (size_t)m);
                at += m;
            }
        segoff[nseg] = (int32_t)at;
        const int64_t cap_ev = 2 * g.nonempty;
        Work w;
        if (int rc = carve(ctx, sizeof(int32_t) * h_in.size(), n_all, cap_ev, ncg, knobs.tile_keys, w)) return rc;
        HIPCHK(hipMemcpyAsync(w.input, h_in.data(), sizeof(int32_t) * h_in.size(), hipMemcpyHostToDevice, st));
        const int32_t *d_iv = (const int32_t *)w.input, *d_seg = d_iv + 2 * n_all;
        int64_t events;
        if (!normalise) {
            for (int place = 0; place < 2; place++) {
                dhk_mo_events(st, place, d_iv, d_seg, nseg, 0, n_all, ncg, nmasks, 0, posbits, w.idx, nullptr, w.ka);
                if (!place) dhk_scan(st, w.idx, n_all + 1, w.sums);
            }
            events = 2 * g.nonempty;
        } else {
            for (int place = 0; place < 2; place++) {
                dhk_mo_events(st, place, d_iv, d_seg, nseg, 0, n_in, ncg, nmasks, 1, posbits, w.idx, nullptr, w.ka);
                if (!place) dhk_scan(st, w.idx, n_in + 1, w.sums);
            }
            sort_and_sweep(st, w, 2 * ne_in, bits1, knobs.tile_keys, false, 1, res.get(), laps);
            HIPCHK(hipGetLastError());
            uint32_t nruns = 0;
            HIPCHK(hipMemcpyAsync(&nruns, w.ctr, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));
            if ((int64_t)nruns > ne_in) return dh_fail(DH_EOVERFLOW, name + ": more runs than events allow");
            // the runs live in rb[0] / re[0] until the second sweep writes them again, behind its sort: their keys first
            dhk_mo_events_runs(st, w.rb[0], w.re[0], w.ctr, ne_in, ncg, posbits, w.ka);
            if (n_sub > 0) {
                for (int place = 0; place < 2; place++) {
                    dhk_mo_events(st, place, d_iv, d_seg, nseg, n_in, n_sub, ncg, nmasks, 0, posbits, w.idx, w.ctr, w.ka);
                    if (!place) dhk_scan(st, w.idx, n_sub + 1, w.sums);
                }
            }
            events = 2 * ((int64_t)nruns + g.sub_nonempty);
        }
        HIPCHK(hipGetLastError());
        if (events == 0) {
            for (int32_t c = g.c0; c <= g.c1; c++) res->ptr[(size_t)c] = (int64_t)res->iv.size() / 2;
            continue;
        }
        sort_and_sweep(st, w, events, bits2, knobs.tile_keys, g.sub_nonempty > 0, o.min_count, res.get(), laps);
        if (int rc = finish_group(ctx, name, w, cap_ev, g.c0, ncg, posbits, o, res.get())) return rc;
        laps.lap(st, T_FILTER);
    }
    if (laps.on)
        fprintf(stderr,
                "[maskops] %d masks, %lld intervals, %d contigs in %lld groups, %lld events, %lld sort passes, tile %d; checks+plan %.2f, "
                "pack+upload+events %.2f, sort %.2f, sweep %.2f, filter+offsets+download %.2f ms, total %.2f ms; %lld runs\n",
                nmasks, (long long)pl.intervals, ncontigs, (long long)res->groups, (long long)res->events, (long long)res->sort_passes, knobs.tile_keys,
                laps.ms[T_PLAN], laps.ms[T_EVENTS], laps.ms[T_SORT], laps.ms[T_SWEEP], laps.ms[T_FILTER], dh_ms_since(t_call),
                (long long)res->iv.size() / 2);
    *out = res.release();
    return DH_OK;
}

extern "C" int dh_la_tandem_mask(dh_ctx *ctx, const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads, int32_t first_read,
                                 int32_t min_len, dh_mask_set **out)
{
    const std::string name("dh_la_tandem_mask");
    if (!ctx || (n > 0 && !las) || !read_off || !out || n < 0 || nreads < 0) return dh_fail(DH_EINVAL, name + ": bad argument");
    if (n >= ((int64_t)1 << 30)) return dh_fail(DH_EOVERFLOW, name + ": 2^30 records or more");
    int64_t maxlen = 0;
    std::string why;
    const int64_t counted = mo::check_tandem(las, n, read_off, nreads, first_read, min_len, &maxlen, why);
    if (counted < 0) return dh_fail(DH_EINVAL, name + ": " + why);
    std::unique_ptr<dh_mask_set> res(new dh_mask_set);
    res->ncontigs = nreads;
    res->ptr.assign((size_t)nreads + 1, 0);
    if (counted > 0) {
        const Knobs knobs;
        const int32_t posbits = mo::bits_of((u64)maxlen), bits = mo::bits_of((u64)nreads - 1) + posbits + 2;
        HIPCHK(hipSetDevice(ctx->device));
        hipStream_t st = ctx->stream;
        res->groups = 1, res->events = 2 * counted;
        Work w;
        if (int rc = carve(ctx, sizeof(dh_la) * (size_t)n, n, 2 * counted, nreads, knobs.tile_keys, w)) return rc;
        HIPCHK(hipMemcpyAsync(w.input, las, sizeof(dh_la) * (size_t)n, hipMemcpyHostToDevice, st));
        for (int place = 0; place < 2; place++) {
            dhk_mo_events_la(st, place, (const dh_la *)w.input, n, first_read, min_len, posbits, w.idx, w.ka);
            if (!place) dhk_scan(st, w.idx, n + 1, w.sums);
        }
        Laps laps;
        laps.on = false;
        sort_and_sweep(st, w, 2 * counted, bits, knobs.tile_keys, false, 1, res.get(), laps);
        if (int rc = finish_group(ctx, name, w, 2 * counted, 0, nreads, posbits, mo::Opts{1, 0, 0, 0}, res.get())) return rc;
    }
    *out = res.release();
    return DH_OK;
}

extern "C" void dh_mask_set_destroy(dh_mask_set *s) { delete s; }
extern "C" const int64_t *dh_mask_set_ptr(const dh_mask_set *s) { return s->ptr.data(); }
extern "C" const int32_t *dh_mask_set_iv(const dh_mask_set *s) { return s->iv.data(); }
extern "C" int64_t dh_mask_set_count(const dh_mask_set *s) { return (int64_t)s->iv.size() / 2; }
extern "C" int64_t dh_mask_set_events(const dh_mask_set *s) { return s->events; }
extern "C" int64_t dh_mask_set_sort_passes(const dh_mask_set *s) { return s->sort_passes; }
extern "C" int64_t dh_mask_set_groups(const dh_mask_set *s) { return s->groups; }
