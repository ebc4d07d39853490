// A stand-alone run of the chaining's CPU harness (chain_host.cpp) for the sanitizers: `make tests/native/chain_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every case agrees and no report was printed.
// The cases: the hand-worked pairs of tests/chain_cases.py with their chains written out; random pairs of 1..300 enabled
// records (abutting with indels around max_indel, overlapping around 0.3, equal starts, jumps around max_chain_gap, a second
// strand, disabled and shuffled records) chained once per tier -- LDS limit 1536, 128 and 64 with small launch groups -- whose
// results must be the same arrays; the array tiers run in buffers of exactly their size, so an access behind them is a report.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../dentist_amd/csrc/dh_chain.h"

extern "C" int64_t chain_host(const dh_la *las, int64_t n, const chn::Opts *o, int64_t lds_cap, int64_t chunk_words, int64_t *off, int32_t *score,
                              int64_t cap_chains, int64_t *src, uint32_t *flags, int64_t cap_rec, int64_t *info);

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

static dh_la rec(int32_t ab, int32_t ae, int32_t bb, int32_t be, uint32_t flags, int32_t aread, int32_t bread)
{
    dh_la l = {};
    l.abpos = ab, l.aepos = ae, l.bbpos = bb, l.bepos = be, l.flags = flags, l.aread = aread, l.bread = bread;
    return l;
}

static void run_of(std::vector<dh_la> &out, int n, uint32_t comp, int32_t aread, int32_t bread)
{
    int32_t pab = rnd_in(0, 3000), pbb = rnd_in(5000, 9000), la = rnd_in(600, 3000), lb = la + rnd_in(-30, 30);
    int32_t pae = pab + la, pbe = pbb + lb;
    out.push_back(rec(pab, pae, pbb, pbe, comp, aread, bread));
    for (int i = 1; i < n; i++) {
        la = rnd_in(600, 3000), lb = la + rnd_in(-30, 30);
        int32_t ab, bb;
        const uint32_t kind = rnd() % 20;
        if (kind < 9) {
            const int32_t g = rnd_in(0, 200);
            ab = pae + g, bb = std::max(pbb + 1, pbe + g + rnd_in(-1100, 1100));
        } else if (kind < 14) {
            const int32_t pct = rnd_in(5, 50);
            ab = pae - pct * std::min(pae - pab, la) / 100, bb = pbe - pct * std::min(pbe - pbb, lb) / 100;
        } else if (kind < 17)
            ab = pab, bb = pbb;
        else {
            const int32_t g = rnd_in(9000, 14000);
            ab = pae + g, bb = pbe + g + rnd_in(-50, 50);
        }
        pab = ab, pbb = bb, pae = ab + la, pbe = bb + lb;
        out.push_back(rec(pab, pae, pbb, pbe, comp, aread, bread));
    }
}

struct Result {
    int64_t nch = 0;
    std::vector<int64_t> off, src;
    std::vector<int32_t> score;
    std::vector<uint32_t> flags;
    int64_t info[8];
    bool operator==(const Result &r) const { return nch == r.nch && off == r.off && src == r.src && score == r.score && flags == r.flags; }
};

static Result chain(const std::vector<dh_la> &las, const chn::Opts &o, int64_t lds_cap, int64_t chunk_words)
{
    Result r;
    std::vector<dh_la> exact(las);  // an exact-size heap copy: a read behind it is a report
    exact.shrink_to_fit();
    const int64_t cap = 1 << 20;
    std::vector<int64_t> off((size_t)cap + 1), src((size_t)cap);
    std::vector<int32_t> score((size_t)cap);
    std::vector<uint32_t> flags((size_t)cap);
    r.nch = chain_host(exact.data(), (int64_t)exact.size(), &o, lds_cap, chunk_words, off.data(), score.data(), cap, src.data(), flags.data(), cap,
                       r.info);
    if (r.nch < 0) return r;
    r.off.assign(off.begin(), off.begin() + r.nch + 1);
    r.score.assign(score.begin(), score.begin() + r.nch);
    r.src.assign(src.begin(), src.begin() + r.info[0]);
    r.flags.assign(flags.begin(), flags.begin() + r.info[0]);
    return r;
}

int main()
{
    int bad = 0, cases = 0;
    chn::Opts o = {1000, 10000, 100, 0, 0.3, 1.0};
    const uint32_t SB = CH_FLAG_START | CH_FLAG_BEST, S = CH_FLAG_START, N = CH_FLAG_NEXT;
    {  // the hand-worked cases
        std::vector<dh_la> fork{rec(0, 1000, 0, 1000, 0, 3, 5), rec(1100, 2100, 1100, 2100, 0, 3, 5), rec(1105, 2105, 1105, 2105, 0, 3, 5)};
        const Result r = chain(fork, o, 1536, 1 << 20);
        cases++;
        bad += !(r.nch == 2 && r.off == std::vector<int64_t>{0, 2, 4} && r.src == std::vector<int64_t>{0, 1, 0, 2} &&
                 r.flags == std::vector<uint32_t>{SB, N, S, N} && r.score == std::vector<int32_t>{1990, 1990});
        std::vector<dh_la> edge{rec(0, 1000, 0, 1000, 0, 3, 5), rec(700, 1700, 700, 1700, 0, 3, 5), rec(0, 99, 0, 99, 0, 3, 6),
                                rec(0, 3000, 0, 3000, 0, 4, 0), rec(3100, 6100, 4101, 7101, 0, 4, 0)};
        const Result e = chain(edge, o, 1536, 1 << 20);
        cases++;
        bad += !(e.nch == 3 && e.off == std::vector<int64_t>{0, 2, 3, 4} && e.src == std::vector<int64_t>{0, 1, 3, 4} &&
                 e.flags == std::vector<uint32_t>{SB, N, SB, SB} && e.score == std::vector<int32_t>{1970, 3000, 3000});
        std::vector<dh_la> unordered{rec(0, 1000, 0, 1000, 0, 3, 5), rec(0, 1000, 0, 1000, CH_FLAG_DISABLED, 1, 1), rec(0, 1000, 0, 1000, 0, 3, 4)};
        const Result u = chain(unordered, o, 1536, 1 << 20);
        cases++;
        bad += !(u.nch == -1 && u.info[6] == 2);
        const Result none = chain(std::vector<dh_la>(), o, 1536, 1 << 20);
        cases++;
        bad += !(none.nch == 0);
    }
    const int sizes[] = {1, 2, 3, 9, 63, 64, 65, 127, 128, 129, 200, 300};
    const double rels[] = {1.0, 0.5, 0.0, 0.8};
    for (int it = 0; it < 8; it++) {
        std::vector<dh_la> las;
        int pair = 0;
        for (int size : sizes) {
            std::vector<dh_la> p;
            const int ncomp = size / 3;
            run_of(p, size - ncomp, 0, pair / 3, pair % 3);
            if (ncomp) run_of(p, ncomp, CH_FLAG_COMP, pair / 3, pair % 3);
            for (int k = 0; k < size / 20 + 1; k++) {
                dh_la d = p[rnd() % p.size()];
                d.flags |= CH_FLAG_DISABLED;
                p.push_back(d);
            }
            for (size_t i = p.size(); i > 1; i--) std::swap(p[i - 1], p[rnd() % i]);
            las.insert(las.end(), p.begin(), p.end());
            pair++;
        }
        o.min_rel_score = rels[it % 4];
        o.min_score = it % 4 == 3 ? 2500 : 100;
        const Result lds = chain(las, o, 1536, 1 << 20), mid = chain(las, o, 128, 1 << 20), glob = chain(las, o, 64, 3000);
        cases++;
        bad += !(lds.nch > 0 && lds == mid && lds == glob && lds.info[1] == 0 && mid.info[1] == 3 && glob.info[1] == 6 && glob.info[7] > 1);
        // every chain is a run of chainable records that begins with START
        for (int64_t c = 0; c < lds.nch; c++)
            for (int64_t i = lds.off[(size_t)c]; i < lds.off[(size_t)c + 1]; i++) {
                const bool first = i == lds.off[(size_t)c];
                bad += !(((lds.flags[(size_t)i] & CH_FLAG_START) != 0) == first && ((lds.flags[(size_t)i] & CH_FLAG_NEXT) != 0) == !first);
                if (!first) bad += !(las[(size_t)lds.src[(size_t)i - 1]].abpos < las[(size_t)lds.src[(size_t)i]].abpos);
            }
    }
    printf("%d cases, %d disagreements\n", cases, bad);
    return bad ? 1 : 0;
}
