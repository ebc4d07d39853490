// A stand-alone run of the repeat mask's CPU harness (rmask_host.cpp) for the sanitizers: `make tests/native/rmask_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every case agrees and no report was printed.
// The cases: random chains of 1..4 members on a few contigs (some without any, some of length 0 or 1), many units at equal
// positions and at the contigs' ends, proper and improper ones, a few bounds -- each at the LDS cap 8192 and 1024, in one launch
// group and with every contig a group of its own -- against the contract's per-base statement written out here: one counter per
// base.  The harness keeps every device buffer in a heap block of exactly its size.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/dentist_hip.h"

extern "C" int64_t rmask_host(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                              const int32_t *opts6, int32_t lds_events, int64_t chunk_bytes, int64_t *ptr3, int32_t *iv3, int64_t iv_cap,
                              int64_t *info, char *msg, int32_t msg_cap);

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
    std::vector<int64_t> contig_off{0}, read_off{0};
    int32_t opts[6];
};
typedef std::vector<std::vector<int32_t>> Runs;  // per contig: begin, end, begin, end, ...

static bool continues(const dh_la &p, const dh_la &c)
{
    return (c.flags & DH_FLAG_NEXT) && !(c.flags & DH_FLAG_START) && c.aread == p.aread && c.bread == p.bread &&
           (c.flags & DH_FLAG_COMP) == (p.flags & DH_FLAG_COMP);
}

// the contract, the plain way: [0] mask, [1] all, [2] improper
static void reference(const Case &c, Runs out[3])
{
    const int32_t nc = (int32_t)c.contig_off.size() - 1;
    std::vector<std::vector<int32_t>> cov[2];
    int64_t counted[2] = {0, 0};
    for (int a = 0; a < 2; a++)
        for (int32_t k = 0; k < nc; k++) cov[a].push_back(std::vector<int32_t>((size_t)(c.contig_off[k + 1] - c.contig_off[k]), 0));
    const int64_t n = (int64_t)c.las.size();
    for (int64_t i = 0; i < n;) {
        int64_t e = i;
        while (e + 1 < n && continues(c.las[e], c.las[e + 1])) e++;
        const dh_la &f = c.las[i], &l = c.las[e];
        const int64_t alen = c.contig_off[f.aread + 1] - c.contig_off[f.aread], blen = c.read_off[f.bread + 1] - c.read_off[f.bread];
        const int32_t al = c.opts[4];
        const bool proper = (f.abpos <= al || f.bbpos <= al) && ((int64_t)l.aepos + al >= alen || (int64_t)l.bepos + al >= blen);
        for (int a = 0; a < 2; a++) {
            if (a == 1 && (!c.opts[5] || proper)) continue;
            counted[a]++;
            for (int32_t p = f.abpos; p < l.aepos; p++) cov[a][(size_t)f.aread][(size_t)p]++;
        }
        i = e + 1;
    }
    for (int k = 0; k < 3; k++) out[k].assign((size_t)nc, std::vector<int32_t>());
    for (int a = 0; a < 2; a++) {
        if (!counted[a]) continue;
        const int32_t lo = c.opts[2 * a], hi = c.opts[2 * a + 1];
        for (int32_t k = 0; k < nc; k++) {
            bool in = false;
            const std::vector<int32_t> &v = cov[a][(size_t)k];
            for (size_t p = 0; p <= v.size(); p++) {
                const bool bad = p < v.size() && (v[p] < lo || v[p] > hi);
                if (bad != in) out[1 + a][(size_t)k].push_back((int32_t)p), in = bad;
            }
        }
    }
    for (int32_t k = 0; k < nc; k++) {  // the union, per base
        const size_t len = (size_t)(c.contig_off[k + 1] - c.contig_off[k]);
        std::vector<char> m(len + 1, 0);
        // (marked bases: two touching runs are one run of marked bases, as the union merges them)
        for (int a = 1; a <= 2; a++)
            for (size_t j = 0; j + 1 < out[a][(size_t)k].size(); j += 2)
                for (int32_t p = out[a][(size_t)k][j]; p < out[a][(size_t)k][j + 1]; p++) m[(size_t)p] = 1;
        bool in = false;
        for (size_t p = 0; p <= len; p++) {
            const bool bad = p < len && m[p];
            if (bad != in) out[0][(size_t)k].push_back((int32_t)p), in = bad;
        }
    }
}

static bool run(const Case &c, int32_t lds_events, int64_t chunk, Runs got[3], int64_t *info)
{
    std::vector<dh_la> las(c.las);
    las.shrink_to_fit();
    const int32_t nc = (int32_t)c.contig_off.size() - 1, nr = (int32_t)c.read_off.size() - 1;
    const int64_t cap = 2 * ((int64_t)las.size() + nc) + 4;
    std::vector<int64_t> ptr3(3 * ((size_t)nc + 1));
    std::vector<int32_t> iv3((size_t)(6 * cap));
    char msg[256];
    if (rmask_host(las.data(), (int64_t)las.size(), c.contig_off.data(), nc, c.read_off.data(), nr, c.opts, lds_events, chunk, ptr3.data(), iv3.data(),
                   cap, info, msg, 256) != 0) {
        fprintf(stderr, "refused: %s\n", msg);
        return false;
    }
    for (int k = 0; k < 3; k++) {
        got[k].assign((size_t)nc, std::vector<int32_t>());
        const int64_t *ptr = ptr3.data() + (size_t)k * ((size_t)nc + 1);
        for (int32_t ctg = 0; ctg < nc; ctg++)
            for (int64_t j = ptr[ctg]; j < ptr[ctg + 1]; j++)
                for (int h = 0; h < 2; h++) got[k][(size_t)ctg].push_back(iv3[(size_t)(2 * k * cap + 2 * j + h)]);
    }
    return true;
}

static Case random_case(int32_t nunits, int32_t ncontigs, bool improper)
{
    Case c;
    std::vector<int32_t> lens;
    for (int32_t k = 0; k < ncontigs; k++) {
        lens.push_back(rnd() % 7 == 0 ? rnd_in(0, 1) : rnd_in(2, 900));
        c.contig_off.push_back(c.contig_off.back() + lens.back());
    }
    const int32_t rlen = 300;
    std::vector<std::vector<dh_la>> per((size_t)ncontigs);
    int32_t nreads = 0;
    for (int32_t u = 0; u < nunits; u++) {
        const int32_t a = rnd_in(0, ncontigs - 1), len = lens[(size_t)a];
        if (a % 5 == 3) continue;  // (contigs without units)
        const int32_t members = rnd() % 4 == 0 ? rnd_in(2, 4) : 1;
        const uint32_t comp = rnd() & 1u;
        // a few coordinates only, so that positions repeat
        int32_t ab = rnd() % 3 == 0 ? 0 : (len / 8) * rnd_in(0, 8), bb = rnd() % 2 ? 0 : 40;
        ab = std::min(ab, len);
        for (int32_t m = 0; m < members; m++) {
            dh_la l{};
            l.aread = a, l.bread = nreads, l.abpos = ab, l.bbpos = bb;
            l.aepos = rnd() % 3 == 0 ? len : std::min(len, ab + (len / 8) * rnd_in(0, 4) + (int32_t)(rnd() % 2));
            l.bepos = rnd() % 2 ? rlen : std::min(rlen, bb + 50);
            l.flags = comp | (m == 0 ? DH_FLAG_START : DH_FLAG_NEXT);
            per[(size_t)a].push_back(l);
            ab = std::min(len, l.aepos + (int32_t)(rnd() % 30)), bb = l.bepos;
        }
        // (a chain must not end before it begins: every member begins at or behind the end of the one before)
        nreads++;
    }
    for (auto &v : per) c.las.insert(c.las.end(), v.begin(), v.end());
    for (int32_t r = 0; r < std::max(nreads, 1); r++) c.read_off.push_back(c.read_off.back() + rlen);
    const int32_t lo = rnd_in(0, 3), ilo = rnd_in(0, 1);
    const int32_t o[6] = {lo, lo + rnd_in(0, nunits / 4 + 1), ilo, ilo + rnd_in(0, 6), (int32_t)(rnd() % 2) * 20, improper ? 1 : 0};
    std::copy(o, o + 6, c.opts);
    return c;
}

int main()
{
    int64_t cases = 0, units = 0, tiers[4] = {0, 0, 0, 0}, runs[3] = {0, 0, 0};
    for (int round = 0; round < 300; round++) {
        const bool big = round % 30 == 0;
        const Case c = random_case(big ? rnd_in(1500, 5000) : rnd_in(0, 120), big ? 2 : rnd_in(1, 9), round % 3 != 0);
        Runs exp[3];
        reference(c, exp);
        for (int32_t cap : {8192, 1024})
            for (int64_t chunk : {(int64_t)1 << 30, (int64_t)1}) {
                Runs got[3];
                int64_t info[8];
                if (!run(c, cap, chunk, got, info) || got[0] != exp[0] || got[1] != exp[1] || got[2] != exp[2]) {
                    fprintf(stderr, "round %d, cap %d, chunk %lld: the harness and the per-base statement differ\n", round, cap, (long long)chunk);
                    return 1;
                }
                units += info[0];
                for (int k = 0; k < 4; k++) tiers[k] += info[2 + k];
            }
        for (int k = 0; k < 3; k++)
            for (const auto &v : exp[k]) runs[k] += (int64_t)v.size() / 2;
        cases++;
    }
    for (int k = 0; k < 4; k++)
        if (!tiers[k]) {
            fprintf(stderr, "tier %d was never reached\n", k);
            return 1;
        }
    for (int k = 0; k < 3; k++)
        if (!runs[k]) {
            fprintf(stderr, "mask %d never had a run\n", k);
            return 1;
        }
    printf("rmask_host_san: %lld cases, %lld chains, contigs per tier %lld / %lld / %lld / %lld, runs %lld mask, %lld all, %lld improper: all agree\n",
           (long long)cases, (long long)units, (long long)tiers[0], (long long)tiers[1], (long long)tiers[2], (long long)tiers[3], (long long)runs[0],
           (long long)runs[1], (long long)runs[2]);
    return 0;
}
