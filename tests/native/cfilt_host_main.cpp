// A stand-alone run of the collect filters' CPU harness (cfilt_host.cpp) for the sanitizers: `make tests/native/cfilt_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every case agrees and no report was printed.
// The cases: random sets of chains of 1..4 members on few contigs and few reads, so that reads have up to a few hundred units
// that nest, repeat and intersect, with random masks (touching and empty intervals included) and a tenth of the records
// disabled on entry; each in the order drawn, grouped by read, and with the LDS cap at 8192 and at 64 -- against the filters
// written out here the way the host function has them: the mask walked interval by interval, Contained as the SEQUENTIAL loop
// (the harness, like the kernels, runs its order-free form).  The harness keeps every device buffer in a heap block of exactly
// its size, so an access behind a read's order, the mask or a tier list is a report.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/dentist_hip.h"

extern "C" int64_t cfilt_host(dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                              const int64_t *rep_ptr, const int32_t *rep_iv, int32_t ppm, int32_t allowance, int32_t min_anchor,
                              int32_t lds_units, int64_t *dropped6, uint8_t *read_used, int64_t *info);

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

struct Case {
    std::vector<dh_la> las;
    std::vector<int64_t> contig_off{0}, read_off{0}, rep_ptr{0};
    std::vector<int32_t> rep_iv;
    int32_t ppm = 300000, allowance = 100, min_anchor = 50;
    bool with_mask = true;
};
struct Result {
    std::vector<uint32_t> flags;
    std::vector<int64_t> dropped;
    std::vector<uint8_t> used;
    bool operator==(const Result &r) const { return flags == r.flags && dropped == r.dropped && used == r.used; }
};

static bool continues(const dh_la &p, const dh_la &c)
{
    return (c.flags & DH_FLAG_NEXT) && !(c.flags & DH_FLAG_START) && c.aread == p.aread && c.bread == p.bread &&
           (c.flags & DH_FLAG_COMP) == (p.flags & DH_FLAG_COMP);
}

// the contract, the plain way
static Result reference(const Case &c)
{
    const int64_t n = (int64_t)c.las.size();
    const int32_t nreads = (int32_t)c.read_off.size() - 1;
    struct U {
        dh_la u;
        int64_t first, end, covered, unmasked;
        bool dis;
        int why;
    };
    std::vector<U> units;
    for (int64_t i = 0; i < n;) {
        int64_t e = i + 1;
        while (e < n && continues(c.las[e - 1], c.las[e])) e++;
        U x{c.las[i], i, e, 0, 0, false, 0};
        x.u.diffs = 0;
        for (int64_t j = i; j < e; j++) {
            x.u.aepos = c.las[j].aepos, x.u.bepos = c.las[j].bepos, x.u.diffs += c.las[j].diffs;
            x.covered += c.las[j].aepos - c.las[j].abpos;
            x.dis = x.dis || (c.las[j].flags & DH_FLAG_DISABLED);
        }
        units.push_back(x);
        i = e;
    }
    const bool trivial = (int64_t)units.size() == n;
    for (U &x : units) {
        int32_t done = -1;
        for (int64_t j = x.first; j < x.end; j++) {
            const dh_la &l = c.las[j];
            const int32_t b0 = trivial ? l.abpos : std::max(l.abpos, done), e0 = l.aepos;
            if (trivial) x.unmasked = e0 - b0;
            if (e0 <= b0) continue;
            int64_t un = e0 - b0;
            if (c.with_mask)
                for (int64_t k = c.rep_ptr[l.aread]; k < c.rep_ptr[l.aread + 1]; k++) {
                    const int32_t b = std::max(c.rep_iv[2 * k], b0), e = std::min(c.rep_iv[2 * k + 1], e0);
                    if (e > b) un -= e - b;
                }
            x.unmasked = trivial ? un : x.unmasked + un;
            done = e0;
        }
    }
    auto alen = [&](const dh_la &l) { return (int32_t)(c.contig_off[l.aread + 1] - c.contig_off[l.aread]); };
    auto blen = [&](const dh_la &l) { return (int32_t)(c.read_off[l.bread + 1] - c.read_off[l.bread]); };
    auto bfb = [&](const dh_la &l) { return (l.flags & DH_FLAG_COMP) ? blen(l) - l.bepos : l.bbpos; };
    auto bfe = [&](const dh_la &l) { return (l.flags & DH_FLAG_COMP) ? blen(l) - l.bbpos : l.bepos; };
    Result r;
    r.dropped.assign(6, 0);
    r.used.assign((size_t)nreads, 1);
    auto drop = [&](U &x, int stage) {
        x.dis = true;
        x.why = stage;
        r.dropped[(size_t)stage]++;
    };
    for (U &x : units) {
        if (x.dis) continue;
        const dh_la &l = x.u;
        const bool begins = l.abpos <= c.allowance || l.bbpos <= c.allowance;
        const bool ends = l.aepos + c.allowance >= alen(l) || l.bepos + c.allowance >= blen(l);
        if ((int64_t)l.diffs * 1000000 > (int64_t)c.ppm * x.covered)
            drop(x, 0);
        else if (!(begins && ends))
            drop(x, 1);
        else if (x.unmasked <= c.min_anchor)
            drop(x, 2);
    }
    for (int32_t rd = 0; rd < nreads; rd++) {
        std::vector<size_t> idx;
        for (size_t k = 0; k < units.size(); k++)
            if (units[k].u.bread == rd) idx.push_back(k);
        std::vector<size_t> ord(idx);
        std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) {
            const dh_la &p = units[x].u, &q = units[y].u;
            if (p.aread != q.aread) return p.aread < q.aread;
            if (p.abpos != q.abpos) return p.abpos < q.abpos;
            if (p.bbpos != q.bbpos) return p.bbpos < q.bbpos;
            if (p.aepos != q.aepos) return p.aepos < q.aepos;
            return p.bepos < q.bepos;
        });
        for (size_t x = 0; x < ord.size(); x++) {
            if (units[ord[x]].dis) continue;
            const dh_la a1 = units[ord[x]].u;
            for (size_t y = x + 1; y < ord.size(); y++) {
                U &u2 = units[ord[y]];
                const dh_la &a2 = u2.u;
                if (a2.aread != a1.aread || !(a1.abpos <= a2.abpos && a2.aepos <= a1.aepos)) break;
                if ((a2.flags & DH_FLAG_COMP) == (a1.flags & DH_FLAG_COMP) && bfb(a1) <= bfb(a2) && bfe(a2) <= bfe(a1) && !u2.dis) drop(u2, 3);
            }
        }
        bool amb = false, red = false;
        for (size_t x = 0; x < idx.size(); x++)
            for (size_t y = x + 1; y < idx.size(); y++) {
                const U &p = units[idx[x]], &q = units[idx[y]];
                if (!p.dis && !q.dis && bfb(p.u) < bfe(q.u) && bfb(q.u) < bfe(p.u)) amb = true;
            }
        if (!amb)
            for (size_t k : idx) {
                const dh_la &p = units[k].u;
                if (!units[k].dis && p.bbpos <= p.abpos && (int64_t)p.aepos + blen(p) - p.bepos < alen(p)) red = true;
            }
        if (amb || red) {
            r.used[(size_t)rd] = 0;
            for (size_t k : idx)
                if (!units[k].dis) drop(units[k], amb ? 4 : 5);
        }
    }
    r.flags.resize((size_t)n);
    for (const U &x : units)
        for (int64_t j = x.first; j < x.end; j++) r.flags[(size_t)j] = c.las[j].flags | (x.dis ? DH_FLAG_DISABLED : 0u);
    return r;
}

static bool run(const Case &c, int32_t lds_units, Result &r, int64_t *info)
{
    std::vector<dh_la> las(c.las);
    las.shrink_to_fit();
    std::vector<int32_t> iv(c.rep_iv);
    iv.shrink_to_fit();
    const int32_t ncontigs = (int32_t)c.contig_off.size() - 1, nreads = (int32_t)c.read_off.size() - 1;
    r.dropped.assign(6, -1);
    r.used.assign((size_t)nreads, 7);
    const int64_t rc = cfilt_host(las.data(), (int64_t)las.size(), c.contig_off.data(), ncontigs, c.read_off.data(), nreads,
                                  c.with_mask ? c.rep_ptr.data() : nullptr, c.with_mask ? iv.data() : nullptr, c.ppm, c.allowance, c.min_anchor,
                                  lds_units, r.dropped.data(), r.used.data(), info);
    r.flags.clear();
    for (const dh_la &l : las) r.flags.push_back(l.flags);
    return rc == 0;
}

static Case random_case(int32_t nchains, int32_t ncontigs, int32_t nreads, bool with_mask)
{
    Case c;
    c.with_mask = with_mask;
    const int32_t clen = 4000, rlen = 3000;
    for (int32_t k = 0; k < ncontigs; k++) c.contig_off.push_back(c.contig_off.back() + clen);
    for (int32_t k = 0; k < nreads; k++) c.read_off.push_back(c.read_off.back() + rlen);
    for (int32_t k = 0; k < ncontigs; k++) {
        int32_t at = rnd_in(0, 300);
        const int32_t m = rnd_in(0, 6);
        for (int32_t j = 0; j < m && at < clen; j++) {
            const int32_t e = std::min(clen, at + rnd_in(0, 400));
            c.rep_iv.push_back(at);
            c.rep_iv.push_back(e);
            at = e + (rnd() % 3 == 0 ? 0 : rnd_in(1, 500));  // touching now and then
        }
        c.rep_ptr.push_back((int64_t)c.rep_iv.size() / 2);
    }
    for (int32_t k = 0; k < nchains; k++) {
        const int32_t a = rnd_in(0, ncontigs - 1), b = rnd_in(0, nreads - 1), members = rnd() % 4 == 0 ? rnd_in(2, 4) : 1;
        const uint32_t comp = rnd() & 1u;
        // a few coordinates only, so that units nest, repeat and tie
        int32_t ab = 200 * rnd_in(0, 6), bb = 200 * rnd_in(0, 4);
        if (rnd() % 3 == 0) ab = 0;
        for (int32_t m = 0; m < members; m++) {
            dh_la l{};
            const int32_t ln = 200 * rnd_in(1, members > 1 ? 4 : 14);
            l.aread = a, l.bread = b, l.abpos = ab, l.aepos = std::min(clen, ab + ln), l.bbpos = bb, l.bepos = std::min(rlen, bb + ln);
            if (rnd() % 3 == 0) l.aepos = clen;
            l.diffs = rnd() % 8 == 0 ? ln / 2 : ln / 20;
            l.flags = comp | (m == 0 ? DH_FLAG_START : DH_FLAG_NEXT) | (rnd() % 10 == 0 ? DH_FLAG_DISABLED : 0u);
            if (members == 1 && (rnd() & 1u)) l.flags &= ~DH_FLAG_START;  // (unchained records come with and without START)
            c.las.push_back(l);
            ab = l.aepos - (rnd() % 4 == 0 ? 30 : 0), bb = l.bepos;  // members overlap now and then
        }
    }
    return c;
}

int main()
{
    int64_t cases = 0, units = 0, tiers[3] = {0, 0, 0}, dropped[6] = {0, 0, 0, 0, 0, 0};
    for (int round = 0; round < 400; round++) {
        const bool big = round % 40 == 0;
        Case c = random_case(big ? rnd_in(300, 700) : rnd_in(0, 60), rnd_in(1, 3), big ? 2 : rnd_in(1, 6), round % 5 != 0);
        c.allowance = round % 7 == 0 ? 100 : 1000000;
        if (round % 3 == 1)  // grouped by read
            std::stable_sort(c.las.begin(), c.las.end(), [](const dh_la &p, const dh_la &q) { return p.bread < q.bread; });
        const Result exp = reference(c);
        for (int32_t cap : {8192, 64}) {
            Result got;
            int64_t info[8];
            if (!run(c, cap, got, info) || !(got == exp)) {
                fprintf(stderr, "round %d, cap %d: the harness and the written-out filters differ\n", round, cap);
                return 1;
            }
            units += info[0];
            for (int k = 0; k < 3; k++) tiers[k] += info[1 + k];
        }
        for (int k = 0; k < 6; k++) dropped[k] += exp.dropped[(size_t)k];
        cases++;
    }
    for (int k = 0; k < 3; k++)
        if (!tiers[k]) {
            fprintf(stderr, "tier %d was never reached\n", k);
            return 1;
        }
    for (int k = 0; k < 6; k++)
        if (!dropped[k]) {
            fprintf(stderr, "stage %d never dropped a chain\n", k);
            return 1;
        }
    printf("cfilt_host_san: %lld cases, %lld chains, reads per tier %lld / %lld / %lld, dropped %lld %lld %lld %lld %lld %lld: all agree\n",
           (long long)cases, (long long)units, (long long)tiers[0], (long long)tiers[1], (long long)tiers[2], (long long)dropped[0],
           (long long)dropped[1], (long long)dropped[2], (long long)dropped[3], (long long)dropped[4], (long long)dropped[5]);
    return 0;
}
