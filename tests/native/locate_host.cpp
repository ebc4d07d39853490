// The lane code of the exact-match locator (dentist_amd/csrc/dh_locate.h: funnel, window, tail_mask, record_of, probe,
// scan_member, verify_word, short_match) and its host planning (pack_words, build_plan, make_units, finish) compiled for
// the CPU.  A wavefront is played lane by lane the way the kernels of dh_locate.hip use these functions: the scan holds a
// word and its successor per lane, rolls the window over the 32 positions, walks a hit group in a wave-uniform loop and
// appends the candidates of a step with one add to the counter; the short kernel is one lane per position; a verify unit
// is 64 lanes, one pattern word each, a ballot per step.  The ranges, the halving on overflow and the unit batches are the
// driver's loop of dh_locate.cpp.  The text and the pattern words live in buffers of exactly the size the driver allocates,
// so that a sanitizer sees every load past them.  tests/test_locate_host.py compares with tests/locate_ref.py.
#include <stdint.h>
#include <string.h>

#include <functional>
#include <utility>
#include <vector>

#include "../../dentist_amd/csrc/dh_locate.h"

namespace {

struct Wave {  // the candidate buffer of a range
    std::vector<LocCand> cands;
    int64_t cap;
    uint64_t counter;
};

// loc_append of dh_locate.hip: the lanes that emit, in lane order, behind one add
void append(Wave &wv, const bool *emit, const int64_t *pos, const uint32_t *pat)
{
    int n = 0;
    for (int l = 0; l < 64; l++) n += emit[l];
    if (!n) return;
    uint64_t at = wv.counter;
    wv.counter += (uint64_t)n;
    for (int l = 0; l < 64; l++)
        if (emit[l]) {
            if ((int64_t)at < wv.cap) wv.cands[(size_t)at] = LocCand{pos[l], pat[l], 1u};
            at++;
        }
}

void scan_range(const uint64_t *text, int64_t nbases, int64_t w0, int64_t w1, const loc::Plan &pl, bool use_bitmap, const int64_t *starts,
                int64_t nref, Wave &wv)
{
    for (int64_t wbase = w0; wbase < w1; wbase += 64) {
        uint64_t lo[64] = {}, hi[64] = {};
        bool live[64];
        for (int l = 0; l < 64; l++) {
            const int64_t t = wbase + l;
            live[l] = t < w1;
            if (live[l]) {
                lo[l] = text[t];
                hi[l] = text[t + 1];
            }
        }
        for (uint32_t j = 0; j < 32; j++) {
            uint32_t first[64] = {}, count[64] = {};
            int64_t pos[64];
            uint32_t most = 0;
            for (int l = 0; l < 64; l++) {
                pos[l] = ((wbase + l) << 5) + j;
                if (live[l] && pos[l] + 32 <= nbases)
                    loc::probe(pl.table.data(), pl.tbits, use_bitmap ? pl.bitmap.data() : (const uint32_t *)nullptr,
                               loc::funnel(lo[l], hi[l], 2u * j), first[l], count[l]);
                most = count[l] > most ? count[l] : most;
            }
            for (uint32_t k = 0; k < most; k++) {
                bool emit[64];
                uint32_t e[64] = {};
                for (int l = 0; l < 64; l++) {
                    emit[l] = false;
                    if (k < count[l]) {
                        e[l] = pl.memb[first[l] + k];
                        emit[l] = loc::scan_member(text, nbases, starts, nref, pl.pw.data(), pl.pats[e[l]], pos[l]);
                    }
                }
                append(wv, emit, pos, e);
            }
        }
    }
}

void short_range(const uint64_t *text, int64_t nbases, int64_t p0, int64_t p1, const loc::Plan &pl, const int64_t *starts, int64_t nref,
                 Wave &wv)
{
    for (int64_t pbase = p0; pbase < p1; pbase += 64) {
        bool live[64];
        uint64_t win[64];
        int64_t pos[64], rec_end[64];
        for (int l = 0; l < 64; l++) {
            pos[l] = pbase + l;
            live[l] = pos[l] < p1 && pos[l] < nbases;
            win[l] = live[l] ? loc::window(text, pos[l]) : 0;
            rec_end[l] = -1;
        }
        for (const LocShort &sp : pl.shorts) {
            bool emit[64];
            uint32_t e[64];
            for (int l = 0; l < 64; l++) {
                e[l] = sp.pat;
                emit[l] = live[l] && pos[l] + (int64_t)sp.len <= nbases && loc::short_match(win[l], sp);
                if (emit[l]) {
                    if (rec_end[l] < 0) rec_end[l] = starts[loc::record_of(starts, nref, pos[l]) + 1];
                    emit[l] = pos[l] + (int64_t)sp.len <= rec_end[l];
                }
            }
            append(wv, emit, pos, e);
        }
    }
}

void verify_unit(const uint64_t *text, int64_t nbases, const loc::Plan &pl, LocCand *cands, int64_t ncands, LocUnit un, int64_t seg)
{
    if ((int64_t)un.cand >= ncands) return;
    const int64_t pos = cands[un.cand].pos;
    const LocPat p = pl.pats[cands[un.cand].pat];
    const int64_t base0 = (int64_t)un.seg * seg;
    if (base0 >= p.len || pos < 0 || pos + p.len > nbases) return;
    const int64_t nb = p.len - base0 < seg ? p.len - base0 : seg, nw = (nb + 31) >> 5;
    for (int64_t wb = 0; wb < nw; wb += 64) {
        bool any = false;
        for (int l = 0; l < 64; l++) {
            const int64_t w = wb + l;
            const uint64_t diff = w < nw ? loc::verify_word(text, pl.pw.data(), p, pos, base0, nb, w) : 0;
            any = any || diff != 0;
        }
        if (any) {
            cands[un.cand].ok = 0u;
            return;
        }
    }
}

}  // namespace

// The whole call.  Returns the number of hits (their first `cap_hits` are written), -1 for a refused input (what
// dh_exact_locate answers with DH_EINVAL).  info[0] = candidates written, info[1] = verify units, info[2] = ranges scanned.
extern "C" int64_t locate_host(const uint8_t *ref, const int64_t *ref_off, int64_t nref, const uint8_t *qry, const int64_t *qry_off,
                               int64_t nqry, int32_t both, int64_t cand_cap, int64_t seg_bases, int32_t use_bitmap, loc::Hit *hits,
                               int64_t cap_hits, int64_t *info)
{
    if (nref < 0 || nqry < 0) return -1;
    for (int64_t i = 0; i < nref; i++)
        if (ref_off[0] < 0 || ref_off[i + 1] < ref_off[i]) return -1;
    for (int64_t i = 0; i < nqry; i++)
        if (qry_off[0] < 0 || qry_off[i + 1] < qry_off[i]) return -1;
    const int64_t nbases = nref > 0 ? ref_off[nref] - ref_off[0] : 0;
    const uint8_t *bytes = nref > 0 ? ref + ref_off[0] : nullptr;
    std::vector<int64_t> starts((size_t)nref + 1, 0);
    int64_t longest = 0;
    for (int64_t i = 0; i < nref; i++) {
        starts[(size_t)i + 1] = ref_off[i + 1] - ref_off[0];
        longest = std::max(longest, ref_off[i + 1] - ref_off[i]);
    }
    loc::Plan pl;
    loc::build_plan(qry, qry_off, nqry, both != 0, longest, [](int64_t n, const std::function<void(int64_t, int64_t)> &fn) { fn(0, n); }, pl);
    if (pl.bad_query >= 0) return -1;
    const int64_t nwords = (nbases + 31) >> 5;
    std::vector<uint64_t> text((size_t)nwords + LOC_TEXT_PAD, 0);
    if (!loc::pack_words(bytes, nbases, 0, nwords, false, text.data())) return -1;
    info[0] = info[1] = info[2] = 0;
    std::vector<loc::Hit> out;
    if (!pl.memb.empty() || !pl.shorts.empty()) {
        const int64_t seg = loc::round_seg(seg_bases);
        Wave wv;
        wv.cap = cand_cap;
        std::vector<LocCand> all;
        std::vector<LocUnit> units;
        std::vector<std::pair<int64_t, int64_t>> todo{{0, nwords}};
        while (!todo.empty()) {
            const std::pair<int64_t, int64_t> r = todo.back();
            todo.pop_back();
            if (r.second <= r.first) continue;
            wv.cands.assign((size_t)wv.cap, LocCand{-1, 0, 0});
            wv.counter = 0;
            if (!pl.memb.empty()) scan_range(text.data(), nbases, r.first, r.second, pl, use_bitmap != 0, starts.data(), nref, wv);
            short_range(text.data(), nbases, 32 * r.first, std::min(nbases, 32 * r.second), pl, starts.data(), nref, wv);
            info[2]++;
            if ((int64_t)wv.counter > wv.cap) {
                if (r.second - r.first > 1) {
                    const int64_t mid = r.first + (r.second - r.first) / 2;
                    todo.push_back({mid, r.second});
                    todo.push_back({r.first, mid});
                } else {
                    wv.cap = (int64_t)wv.counter;
                    todo.push_back(r);
                }
                continue;
            }
            const int64_t count = (int64_t)wv.counter;
            loc::make_units(wv.cands.data(), count, pl, seg, units);
            for (const LocUnit &u : units) verify_unit(text.data(), nbases, pl, wv.cands.data(), count, u, seg);
            for (int64_t c = 0; c < count; c++)
                if (wv.cands[(size_t)c].ok) all.push_back(wv.cands[(size_t)c]);
            info[0] += count;
            info[1] += (int64_t)units.size();
        }
        loc::finish(all, pl, starts.data(), nref, out);
    }
    for (size_t i = 0; i < out.size() && (int64_t)i < cap_hits; i++) hits[i] = out[i];
    return (int64_t)out.size();
}
