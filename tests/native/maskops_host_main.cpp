// A stand-alone run of the mask algebra's CPU harness (maskops_host.cpp) for the sanitizers: `make tests/native/maskops_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every case agrees and no report was printed.
// The cases: random intervals (overlapping, nested, touching, empty, at 0 and at the contig's end, unsorted) of 1..4 masks and a
// subtract mask on a few contigs (some without any, some of length 0 or 1), every min_count, a few gaps and sizes; many copies
// of one interval; a contig of 2^31 - 1 bases; 70 001 contigs -- each at the sort tiles 2048 and 256, in one launch group and
// with every contig a group of its own -- against the contract written out here per contig on intervals; the tandem rule; the
// sort alone on key counts around a tile.  The harness keeps every device buffer in a heap block of exactly its size.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <map>
#include <vector>

#include "../../include/dentist_hip.h"

extern "C" int64_t maskops_host(const int64_t *const *ptr, const int32_t *const *iv, int32_t nmasks, const int64_t *sub_ptr, const int32_t *sub_iv,
                                const int64_t *contig_off, int32_t ncontigs, const int32_t *opts4, int32_t tile_keys, int64_t chunk_bytes,
                                int64_t *out_ptr, int32_t *out_iv, int64_t cap, int64_t *info, char *msg, int32_t msg_cap);
extern "C" int64_t maskops_tandem_host(const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads, int32_t first_read, int32_t min_len,
                                       int32_t tile_keys, int64_t *out_ptr, int32_t *out_iv, int64_t cap, int64_t *info, char *msg, int32_t msg_cap);
extern "C" void maskops_rx_sort_host(unsigned long long *keys, int64_t n, int32_t bits, int32_t tile_keys);

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

struct Mask {
    std::vector<int64_t> ptr{0};
    std::vector<int32_t> iv;
};
struct Case {
    std::vector<Mask> masks;  // the last one: the subtract mask when has_sub
    bool has_sub = false;
    std::vector<int64_t> contig_off{0};
    int32_t opts[4] = {1, 0, 0, 0};
};
struct Triple {
    int32_t c, b, e;
    bool operator==(const Triple &o) const { return c == o.c && b == o.b && e == o.e; }
};

static std::vector<std::pair<int32_t, int32_t>> normalized(const Mask &m, int32_t c)
{
    std::vector<std::pair<int32_t, int32_t>> v, out;
    for (int64_t i = m.ptr[(size_t)c]; i < m.ptr[(size_t)c + 1]; i++)
        if (m.iv[(size_t)(2 * i)] < m.iv[(size_t)(2 * i + 1)]) v.emplace_back(m.iv[(size_t)(2 * i)], m.iv[(size_t)(2 * i + 1)]);
    std::sort(v.begin(), v.end());
    for (const auto &x : v) {
        if (!out.empty() && x.first <= out.back().second)
            out.back().second = std::max(out.back().second, x.second);
        else
            out.push_back(x);
    }
    return out;
}

// the contract on intervals: every mask normalised, a walk over the distinct positions, then filterMask.d:124-159
static std::vector<Triple> reference(const Case &c)
{
    const int32_t nc = (int32_t)c.contig_off.size() - 1, nin = (int32_t)c.masks.size() - (c.has_sub ? 1 : 0);
    std::vector<Triple> runs, acc, out;
    for (int32_t k = 0; k < nc; k++) {
        std::map<int32_t, std::pair<int32_t, int32_t>> delta;
        for (int32_t m = 0; m < (int32_t)c.masks.size(); m++)
            for (const auto &x : normalized(c.masks[(size_t)m], k)) {
                if (m < nin)
                    delta[x.first].first++, delta[x.second].first--;
                else
                    delta[x.first].second++, delta[x.second].second--;
            }
        int32_t cov = 0, sub = 0, start = -1;
        for (const auto &d : delta) {
            cov += d.second.first, sub += d.second.second;
            const bool kept = cov >= c.opts[0] && sub == 0;
            if (kept && start < 0) start = d.first;
            if (!kept && start >= 0) runs.push_back(Triple{k, start, d.first}), start = -1;
        }
    }
    for (const Triple &t : runs) {
        if (!acc.empty() && acc.back().c == t.c && (int64_t)acc.back().e + c.opts[1] >= t.b)
            acc.back().e = t.e;
        else
            acc.push_back(t);
    }
    for (const Triple &t : acc)
        if (t.e - t.b >= c.opts[2]) out.push_back(t);
    return out;
}

static int g_failed = 0, g_checked = 0;

static void check(const char *what, const Case &c)
{
    const int32_t nc = (int32_t)c.contig_off.size() - 1, nin = (int32_t)c.masks.size() - (c.has_sub ? 1 : 0);
    const std::vector<Triple> exp = reference(c);
    std::vector<const int64_t *> ptr;
    std::vector<const int32_t *> iv;
    std::vector<std::vector<int32_t>> padded;  // (never an empty array)
    int64_t cap = 1;
    for (const Mask &m : c.masks) {
        padded.push_back(m.iv);
        padded.back().push_back(0);
        cap += (int64_t)m.iv.size() / 2;
    }
    for (size_t m = 0; m < c.masks.size(); m++) ptr.push_back(c.masks[m].ptr.data()), iv.push_back(padded[m].data());
    const int32_t tiles[3] = {2048, 256, 2048};
    const int64_t chunks[3] = {(int64_t)1 << 30, (int64_t)1 << 30, 1};
    for (int s = 0; s < 3; s++) {
        std::vector<int64_t> out_ptr((size_t)nc + 1), info(3);
        std::vector<int32_t> out_iv((size_t)(2 * cap));
        char msg[256] = "";
        const int64_t n = maskops_host(ptr.data(), iv.data(), nin, c.has_sub ? ptr.back() : nullptr, c.has_sub ? iv.back() : nullptr, c.contig_off.data(),
                                       nc, c.opts, tiles[s], chunks[s], out_ptr.data(), out_iv.data(), cap, info.data(), msg, 256);
        std::vector<Triple> got;
        for (int32_t k = 0; n >= 0 && k < nc; k++)
            for (int64_t i = out_ptr[(size_t)k]; i < out_ptr[(size_t)k + 1]; i++) got.push_back(Triple{k, out_iv[(size_t)(2 * i)], out_iv[(size_t)(2 * i + 1)]});
        g_checked++;
        if (n != (int64_t)exp.size() || !(got == exp)) {
            g_failed++;
            fprintf(stderr, "%s (tile %d, chunk %lld): %lld runs, expected %zu %s\n", what, tiles[s], (long long)chunks[s], (long long)n, exp.size(), msg);
        }
    }
}

static Mask random_mask(const std::vector<int64_t> &off, int32_t n)
{
    const int32_t nc = (int32_t)off.size() - 1;
    std::vector<std::vector<int32_t>> per((size_t)nc);
    for (int32_t i = 0; i < n; i++) {
        const int32_t c = rnd_in(0, nc - 1), len = (int32_t)(off[(size_t)c + 1] - off[(size_t)c]);
        int32_t b = rnd_in(0, len), e = std::min(len, b + rnd_in(0, 9));
        if (rnd() % 8 == 0) b = 0;
        if (rnd() % 8 == 0) e = len;
        per[(size_t)c].push_back(b), per[(size_t)c].push_back(e);
    }
    Mask m;
    for (const auto &p : per) {
        m.iv.insert(m.iv.end(), p.begin(), p.end());
        m.ptr.push_back((int64_t)m.iv.size() / 2);
    }
    return m;
}

static Mask one_contig_mask(int32_t nc, int32_t c, const std::vector<int32_t> &iv)
{
    Mask m;
    for (int32_t k = 0; k < nc; k++) {
        if (k == c) m.iv = iv;
        m.ptr.push_back((int64_t)m.iv.size() / 2);
    }
    return m;
}

int main()
{
    for (int round = 0; round < 60; round++) {
        Case c;
        const int32_t nc = rnd_in(1, 9), nin = rnd_in(1, 4);
        for (int32_t k = 0; k < nc; k++) c.contig_off.push_back(c.contig_off.back() + (rnd() % 4 == 0 ? rnd_in(0, 1) : rnd_in(2, 300)));
        for (int32_t m = 0; m < nin; m++) c.masks.push_back(random_mask(c.contig_off, rnd_in(0, round % 3 == 0 ? 900 : 40)));
        c.has_sub = rnd() % 2 == 0;
        if (c.has_sub) c.masks.push_back(random_mask(c.contig_off, rnd_in(0, 30)));
        c.opts[0] = rnd_in(1, nin), c.opts[1] = rnd() % 2 ? rnd_in(0, 6) : 0, c.opts[2] = rnd() % 2 ? rnd_in(0, 8) : 0;
        check("random", c);
    }
    {  // one bucket over many tiles
        Case c;
        c.contig_off = {0, 50, 100};
        std::vector<int32_t> iv;
        for (int i = 0; i < 3000; i++) iv.push_back(7), iv.push_back(19);
        c.masks.push_back(one_contig_mask(2, 1, iv));
        check("all keys equal", c);
        c.masks.push_back(one_contig_mask(2, 1, iv));
        c.opts[0] = 2;
        check("all keys equal, min_count 2", c);
    }
    {  // the top position digit
        Case c;
        const int32_t top = INT32_MAX;
        c.contig_off = {0, 100, 100 + (int64_t)top};
        c.masks.push_back(one_contig_mask(2, 1, {top - 5, top, 0, 3}));
        c.masks.push_back(one_contig_mask(2, 1, {2, top - 3}));
        check("longest contig", c);
        c.opts[0] = 2;
        check("longest contig, min_count 2", c);
    }
    {  // a third contig digit, many contigs without anything
        Case c;
        const int32_t nc = 70001;
        for (int32_t k = 0; k < nc; k++) c.contig_off.push_back(c.contig_off.back() + 50);
        Mask a, b;
        for (int32_t k = 0; k < nc; k++) {
            if (k == 0 || k == nc - 1 || rnd() % 35 == 0) {
                a.iv.push_back(k % 30), a.iv.push_back(k % 30 + 1 + k % 20);
                if (k % 3 == 0) b.iv.push_back(5), b.iv.push_back(45);
            }
            a.ptr.push_back((int64_t)a.iv.size() / 2), b.ptr.push_back((int64_t)b.iv.size() / 2);
        }
        c.masks = {a, b};
        check("many contigs", c);
        c.opts[0] = 2, c.opts[1] = 3;
        check("many contigs, min_count 2", c);
    }
    {  // the tandem rule
        const int32_t rows[8][7] = {{5, 5, 100, 600, 150, 700, 0},    {5, 6, 0, 900, 0, 900, 0},       {5, 5, 0, 900, 0, 900, 1},
                                    {7, 7, 50, 500, 100, 550, 0},     {7, 7, 1000, 1400, 1001, 1499, 0}, {7, 7, 550, 1000, 600, 1100, 0},
                                    {5, 5, 650, 1300, 600, 1200, 0}, {8, 8, 0, 2000, 5, 1990, 0}};
        std::vector<dh_la> las(8);
        for (int i = 0; i < 8; i++) {
            las[(size_t)i] = dh_la{};
            las[(size_t)i].aread = rows[i][0], las[(size_t)i].bread = rows[i][1], las[(size_t)i].abpos = rows[i][2], las[(size_t)i].aepos = rows[i][3];
            las[(size_t)i].bbpos = rows[i][4], las[(size_t)i].bepos = rows[i][5], las[(size_t)i].flags = (uint32_t)rows[i][6];
        }
        const int64_t read_off[5] = {0, 1500, 1600, 3200, 5200};
        const int32_t exp[6] = {100, 1300, 50, 1100, 0, 2000};
        const int64_t exp_ptr[5] = {0, 1, 1, 2, 3};
        for (int32_t tile : {2048, 256}) {
            int64_t out_ptr[5], info[3];
            int32_t out_iv[18];
            char msg[256] = "";
            const int64_t n = maskops_tandem_host(las.data(), 8, read_off, 4, 5, 500, tile, out_ptr, out_iv, 9, info, msg, 256);
            g_checked++;
            if (n != 3 || !std::equal(exp, exp + 6, out_iv) || !std::equal(exp_ptr, exp_ptr + 5, out_ptr)) g_failed++, fprintf(stderr, "tandem: %lld %s\n", (long long)n, msg);
        }
    }
    // the sort alone: counts around a tile, the input place above the digits in use
    for (int32_t tile : {256, 2048})
        for (int64_t n : {(int64_t)1, (int64_t)tile - 1, (int64_t)tile, (int64_t)tile + 1, (int64_t)3 * tile + 5})
            for (int32_t bits : {8, 13, 24, 40}) {
                const int32_t top = 8 * ((bits + 7) / 8);
                std::vector<unsigned long long> keys((size_t)n), exp;
                for (int64_t i = 0; i < n; i++)
                    keys[(size_t)i] = ((((unsigned long long)rnd() << 20) ^ rnd()) % (bits == 13 ? 2 : 1ull << bits)) | ((unsigned long long)(n - i) << top);
                exp = keys;
                const unsigned long long low = (1ull << top) - 1;
                std::stable_sort(exp.begin(), exp.end(), [&](unsigned long long x, unsigned long long y) { return (x & low) < (y & low); });
                maskops_rx_sort_host(keys.data(), n, bits, tile);
                g_checked++;
                if (keys != exp) g_failed++, fprintf(stderr, "sort: %lld keys of %d bits, tile %d\n", (long long)n, bits, tile);
            }
    printf("%d checks, %d failed\n", g_checked, g_failed);
    return g_failed ? 1 : 0;
}
