// TEST INFRASTRUCTURE -- the lane code and the host plan of dh_la_repeat_mask (dentist_amd/csrc/dh_rmask.h) compiled for the CPU
// and played the way the kernels of dh_rmask.hip run it: 64-lane wavefronts whose ballots and shuffles are loops over the lanes,
// workgroups whose barriers are the ends of loops over the threads.  Every device buffer is a heap block of exactly the size the
// driver (dh_rmask.cpp) gives it, so an access behind a segment, a list or an interval buffer is a sanitizer report.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../dentist_amd/csrc/dh_rmask.h"

using rm::Opts;
using rm::Rec;
using rm::u64;

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

struct Side {
    int32_t lower, upper, carry = 0, nstart = 0, nend = 0;
    bool prev = false;
    int64_t at = 0;
    int32_t *iv = nullptr;
};

// k_rm_cover<PLACE> for contig c
void cover(bool place, const u64 *ev, const int32_t *seg, int32_t c, int32_t len, const Opts &o, uint32_t *cnt_all, uint32_t *cnt_imp,
           int32_t *iv_all, int32_t *iv_imp)
{
    const int32_t s0 = seg[c], size = seg[c + 1] - s0;
    Side side[2];
    side[0].lower = o.lower, side[0].upper = o.upper, side[0].at = place ? cnt_all[c] : 0, side[0].iv = iv_all;
    side[1].lower = o.improper_lower, side[1].upper = o.improper_upper, side[1].at = place && o.with_improper ? cnt_imp[c] : 0, side[1].iv = iv_imp;
    const int nsides = o.with_improper ? 2 : 1;
    const bool head = len > 0 && (size == 0 || rm::key_pos(ev[s0]) > 0);
    for (int a = 0; a < nsides; a++) {
        Side &s = side[a];
        if (head && rm::bad(0, s.lower, s.upper)) {
            if (place) s.iv[2 * s.at] = 0;
            s.nstart = 1, s.prev = true;
        }
    }
    for (int32_t base = 0; base < size; base += 64) {
        u64 k[64], last = 0;
        bool is_last[64];
        int32_t pos[64];
        for (int lane = 0; lane < 64; lane++) {
            const int32_t idx = base + lane;
            k[lane] = idx < size ? ev[s0 + idx] : rm::PAD;
            const u64 nxt = idx + 1 < size ? ev[s0 + idx + 1] : rm::PAD;
            is_last[lane] = idx < size && rm::key_pos(nxt) != rm::key_pos(k[lane]);
            if (is_last[lane]) last |= (u64)1 << lane;
            pos[lane] = (int32_t)rm::key_pos(k[lane]);
        }
        for (int a = 0; a < nsides; a++) {
            Side &s = side[a];
            int32_t incl[64], run = 0;
            u64 badb = 0, sb = 0, eb = 0;
            for (int lane = 0; lane < 64; lane++) {
                run += a == 0 ? rm::delta_all(k[lane]) : rm::delta_improper(k[lane]);
                incl[lane] = run;
                if (is_last[lane] && pos[lane] != len && rm::bad(s.carry + incl[lane], s.lower, s.upper)) badb |= (u64)1 << lane;
            }
            bool st[64], en[64];
            for (int lane = 0; lane < 64; lane++) {
                rm::lane_edges(lane, last, badb, s.prev, &st[lane], &en[lane]);
                if (st[lane]) sb |= (u64)1 << lane;
                if (en[lane]) eb |= (u64)1 << lane;
            }
            if (place)
                for (int lane = 0; lane < 64; lane++) {
                    if (st[lane]) s.iv[2 * (s.at + s.nstart + rm::lanes_below(sb, lane))] = pos[lane];
                    if (en[lane]) s.iv[2 * (s.at + s.nend + rm::lanes_below(eb, lane)) + 1] = pos[lane];
                }
            s.nstart += __builtin_popcountll(sb), s.nend += __builtin_popcountll(eb);
            s.prev = rm::state_behind(last, badb, s.prev);
            s.carry += incl[63];
        }
    }
    for (int a = 0; a < nsides; a++) {
        Side &s = side[a];
        if (s.prev) {
            if (place) s.iv[2 * (s.at + s.nend) + 1] = len;
            s.nend++;
        }
        if (!place) (a == 0 ? cnt_all : cnt_imp)[c] = (uint32_t)s.nstart;
        if (s.nstart != s.nend) abort();  // starts and ends alternate
    }
}

void scan(uint32_t *v, size_t n)
{
    uint32_t run = 0;
    for (size_t i = 0; i < n; i++) {
        const uint32_t x = v[i];
        v[i] = run, run += x;
    }
}

}  // namespace

// opts6: the fields of dh_repeat_opts.  ptr3: 3 * (ncontigs + 1) entries (mask, all, improper); iv3: 3 buffers of iv_cap pairs each,
// one behind the other.  info: units, improper units, contigs of tier 0..3, groups.  Returns 0, -1 for a refusal (msg says why),
// -2 if iv_cap is too small.
extern "C" int64_t rmask_host(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                              const int32_t *opts6, int32_t lds_events, int64_t chunk_bytes, int64_t *ptr3, int32_t *iv3, int64_t iv_cap,
                              int64_t *info, char *msg, int32_t msg_cap)
{
    const Opts o{opts6[0], opts6[1], opts6[2], opts6[3], opts6[4], opts6[5] ? 1 : 0};
    auto refuse = [&](const std::string &s) {
        snprintf(msg, (size_t)msg_cap, "%s", s.c_str());
        return (int64_t)-1;
    };
    if ((n > 0 && !las) || !contig_off || n < 0 || ncontigs < 0 || nreads < 0 || (o.with_improper && !read_off)) return refuse("bad argument");
    if (const char *w = rm::check_opts(o)) return refuse(w);
    Buf<Rec> recs((size_t)n);
    Buf<int32_t> alen((size_t)ncontigs), blen(o.with_improper ? (size_t)nreads : 0);
    rm::Plan pl;
    pl.recs = recs.get(), pl.alen = alen.get(), pl.blen = blen.get();
    rm::Fault f;
    rm::build_plan(las, n, contig_off, ncontigs, read_off, nreads, o, chunk_bytes, serial, pl, f);
    if (f.record >= 0) return refuse("record " + std::to_string(f.record) + ": " + f.what);
    if (f.contig >= 0) return refuse("contig " + std::to_string(f.contig) + ": " + f.what);
    std::vector<int64_t> ptr[3];
    std::vector<int32_t> iv[3];
    for (int k = 0; k < 3; k++) ptr[k].assign((size_t)ncontigs + 1, 0);
    memset(info, 0, 7 * sizeof(int64_t));
    enum { M_MASK = 0, M_ALL = 1, M_IMPROPER = 2 };
    for (const rm::Group &g : n == 0 ? std::vector<rm::Group>() : pl.groups) {
        const int64_t m = g.r1 - g.r0;
        const int32_t nc = g.c1 - g.c0;
        const size_t sm = (size_t)m, snc = (size_t)nc;
        info[6]++;
        const Rec *grecs = pl.recs + g.r0;
        Buf<int32_t> roff(snc + 1), flag(sm), uid(sm + 1), seg(snc + 1);
        for (int32_t c = 0; c <= nc; c++) roff[(size_t)c] = (int32_t)(pl.rec_off[(size_t)(g.c0 + c)] - g.r0);
        // k_cf_start, the scan
        for (int64_t i = 0; i < m; i++) flag[(size_t)i] = uid[(size_t)i] = i == 0 || !cf::continues(grecs[i - 1], grecs[i]) ? 1 : 0;
        uid[sm] = 0;
        scan((uint32_t *)uid.get(), sm + 1);
        const int64_t nunits = uid[sm];
        // k_rm_events (the group's records end at m: a chain never reaches into the next contig)
        Buf<u64> ev(2 * sm);
        int64_t nimproper = 0;
        for (int64_t i = 0; i < m; i++)
            if (flag[(size_t)i]) {
                const int64_t u = uid[(size_t)i];
                nimproper += rm::unit_events(grecs, i, m, pl.alen, pl.blen, o, &ev[(size_t)(2 * u)], &ev[(size_t)(2 * u + 1)]) ? 1 : 0;
            }
        // k_rm_classify
        const size_t cap_l = std::min(snc, 2 * sm / (RM_WAVE_EVENTS + 1)), cap_g = std::min(snc, 2 * sm / ((size_t)lds_events + 1));
        Buf<int32_t> l_wave(snc), l_lds(cap_l), l_glob(cap_g);
        Buf<u64> slab_at(cap_g);
        u64 ctr[rm::C_COUNT] = {0, 0, 0, 0, 0, 0};
        for (int32_t c = nc; c >= 0; c--) {  // (descending: the order of the lists reaches no result)
            seg[(size_t)c] = 2 * uid[(size_t)roff[(size_t)c]];
            if (c == nc) continue;
            const int32_t events = 2 * uid[(size_t)roff[(size_t)c + 1]] - seg[(size_t)c];
            const int tier = rm::tier_of(events, lds_events);
            if (tier == 0) ctr[rm::C_ZERO]++;
            if (tier == 1) l_wave[(size_t)ctr[rm::C_WAVE]++] = c;
            if (tier == 2) l_lds[(size_t)ctr[rm::C_LDS]++] = c;
            if (tier == 3) {
                l_glob[(size_t)ctr[rm::C_GLOBAL]] = c;
                slab_at[(size_t)ctr[rm::C_GLOBAL]++] = ctr[rm::C_SLAB];
                ctr[rm::C_SLAB] += (u64)cf::pow2ceil(events);
            }
        }
        for (int t = 0; t < 4; t++) info[2 + t] += (int64_t)ctr[rm::C_ZERO + t];
        // k_rm_sort_wave
        for (u64 q = 0; q < ctr[rm::C_WAVE]; q++) {
            const int32_t c = l_wave[(size_t)q], s0 = seg[(size_t)c], size = seg[(size_t)c + 1] - s0;
            u64 me[64];
            int32_t rank[64];
            for (int lane = 0; lane < 64; lane++) me[lane] = lane < size ? ev[(size_t)(s0 + lane)] : rm::PAD, rank[lane] = 0;
            for (int32_t z = 0; z < size; z++)
                for (int lane = 0; lane < 64; lane++) rank[lane] += rm::ranks_before(me[z], z, me[lane], lane);
            for (int lane = 0; lane < size; lane++) ev[(size_t)(s0 + rank[lane])] = me[lane];
        }
        // k_rm_sort_block
        for (u64 q = 0; q < ctr[rm::C_LDS]; q++) {
            const int32_t c = l_lds[(size_t)q], s0 = seg[(size_t)c], size = seg[(size_t)c + 1] - s0, P = cf::pow2ceil(size);
            if (P > cf::pow2ceil(lds_events)) abort();  // (the launch's LDS)
            Buf<u64> key((size_t)P);
            for (int32_t t = 0; t < P; t++) key[(size_t)t] = t < size ? ev[(size_t)(s0 + t)] : rm::PAD;
            for (int32_t k = 2; k <= P; k <<= 1)
                for (int32_t j = k >> 1; j > 0; j >>= 1)
                    for (int32_t t = P / 2 - 1; t >= 0; t--) rm::bt_compare(key.get(), t, k, j);
            for (int32_t t = 0; t < size; t++) ev[(size_t)(s0 + t)] = key[(size_t)t];
        }
        // k_rm_sort_big<0>, <1> per step, <2>: the launches of the driver, every contig of the list in each
        Buf<u64> slab((size_t)ctr[rm::C_SLAB]);
        int64_t max_padded = 2;
        for (int32_t c = 0; c < nc; c++) max_padded = std::max<int64_t>(max_padded, cf::pow2ceil(2 * (roff[(size_t)c + 1] - roff[(size_t)c])));
        auto big = [&](int mode, int32_t k, int32_t j) {
            for (u64 q = 0; q < ctr[rm::C_GLOBAL]; q++) {
                const int32_t c = l_glob[(size_t)q], s0 = seg[(size_t)c], size = seg[(size_t)c + 1] - s0, P = cf::pow2ceil(size);
                if (P > max_padded) abort();  // (the launch's grid)
                u64 *key = slab.get() + slab_at[(size_t)q];
                for (int64_t t = (mode == 1 ? max_padded / 2 : max_padded) - 1; t >= 0; t--) {
                    if (mode == 0 && t < P) key[t] = t < size ? ev[(size_t)(s0 + t)] : rm::PAD;
                    if (mode == 1 && t < P / 2 && k <= P) rm::bt_compare(key, (int32_t)t, k, j);
                    if (mode == 2 && t < size) ev[(size_t)(s0 + t)] = key[t];
                }
            }
        };
        if (ctr[rm::C_GLOBAL]) {
            big(0, 0, 0);
            for (int64_t k = 2; k <= max_padded; k <<= 1)
                for (int64_t j = k >> 1; j > 0; j >>= 1) big(1, (int32_t)k, (int32_t)j);
            big(2, 0, 0);
        }
        // k_rm_cover: count, scan, place; k_rm_union: count, scan, place
        const size_t cap_iv = sm + snc;
        Buf<uint32_t> cnt_all(snc + 1), cnt_imp(snc + 1), cnt_mask(snc + 1);
        Buf<int32_t> iv_all(2 * cap_iv), iv_imp(o.with_improper ? 2 * cap_iv : 0), iv_mask(o.with_improper ? 4 * cap_iv : 0);
        for (int place = 0; place < 2; place++) {
            for (int32_t c = 0; c < nc; c++)
                cover(place != 0, ev.get(), seg.get(), c, pl.alen[g.c0 + c], o, cnt_all.get(), cnt_imp.get(), iv_all.get(), iv_imp.get());
            if (!place) scan(cnt_all.get(), snc + 1), scan(cnt_imp.get(), snc + 1);
        }
        if (o.with_improper)
            for (int place = 0; place < 2; place++) {
                for (int32_t c = 0; c < nc; c++) {
                    const int32_t k = rm::merge_union(iv_all.get() + 2 * (int64_t)cnt_all[(size_t)c], (int32_t)(cnt_all[(size_t)c + 1] - cnt_all[(size_t)c]),
                                                      iv_imp.get() + 2 * (int64_t)cnt_imp[(size_t)c], (int32_t)(cnt_imp[(size_t)c + 1] - cnt_imp[(size_t)c]),
                                                      place ? iv_mask.get() + 2 * (int64_t)cnt_mask[(size_t)c] : nullptr);
                    if (!place) cnt_mask[(size_t)c] = (uint32_t)k;
                }
                if (!place) scan(cnt_mask.get(), snc + 1);
            }
        uint32_t *cnts[3] = {cnt_mask.get(), cnt_all.get(), cnt_imp.get()};
        int32_t *ivs[3] = {iv_mask.get(), iv_all.get(), iv_imp.get()};
        for (int k = o.with_improper ? M_MASK : M_ALL; k <= (o.with_improper ? M_IMPROPER : M_ALL); k++) {
            const int64_t at = (int64_t)iv[k].size() / 2;
            for (int32_t c = 0; c <= nc; c++) ptr[k][(size_t)(g.c0 + c)] = at + cnts[k][(size_t)c];
            iv[k].insert(iv[k].end(), ivs[k], ivs[k] + 2 * (size_t)cnts[k][snc]);
        }
        info[0] += nunits, info[1] += nimproper;
    }
    if (o.with_improper && info[1] == 0) ptr[M_IMPROPER].assign((size_t)ncontigs + 1, 0), iv[M_IMPROPER].clear();
    if (!o.with_improper || info[1] == 0) ptr[M_MASK] = ptr[M_ALL], iv[M_MASK] = iv[M_ALL];
    for (int k = 0; k < 3; k++) {
        if ((int64_t)iv[k].size() / 2 > iv_cap) return -2;
        memcpy(ptr3 + (size_t)k * ((size_t)ncontigs + 1), ptr[k].data(), sizeof(int64_t) * ((size_t)ncontigs + 1));
        if (!iv[k].empty()) memcpy(iv3 + 2 * (size_t)k * (size_t)iv_cap, iv[k].data(), sizeof(int32_t) * iv[k].size());
    }
    return 0;
}
