// A stand-alone run of the locator's CPU harness (locate_host.cpp) for the sanitizers: `make tests/native/locate_host_san`
// builds both with -fsanitize=address,undefined, the program exits 0 when every case equals a naive search and no report was
// printed.  The cases sit where the lane code reads closest to the end of its buffers: texts that end at every length mod 32
// around a word boundary, matches that end at the last base of the text, patterns of every length around the word and the
// wave step, small candidate buffers and short segments.
#include <stdint.h>
#include <stdio.h>

#include <tuple>
#include <vector>

#include "../../dentist_amd/csrc/dh_locate.h"

extern "C" int64_t locate_host(const uint8_t *ref, const int64_t *ref_off, int64_t nref, const uint8_t *qry, const int64_t *qry_off,
                               int64_t nqry, int32_t both, int64_t cand_cap, int64_t seg_bases, int32_t use_bitmap, loc::Hit *hits,
                               int64_t cap_hits, int64_t *info);

typedef std::vector<uint8_t> Seq;
typedef std::tuple<int32_t, int32_t, int64_t, int64_t, int32_t> T5;

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}
static Seq rnd_seq(size_t n, int ncodes = 4)
{
    Seq s(n);
    for (uint8_t &c : s) c = (uint8_t)(rnd() % (uint32_t)ncodes);
    return s;
}
static Seq rc(const Seq &q)
{
    Seq r(q.rbegin(), q.rend());
    for (uint8_t &c : r) c = (uint8_t)(3 - c);
    return r;
}

static std::vector<T5> naive(const std::vector<Seq> &refs, const std::vector<Seq> &qs)
{
    std::vector<T5> out;
    for (size_t q = 0; q < qs.size(); q++) {
        if (qs[q].empty()) continue;
        for (int comp = 0; comp < 2; comp++) {
            const Seq pat = comp ? rc(qs[q]) : qs[q];
            for (size_t r = 0; r < refs.size(); r++)
                for (size_t p = 0; p + pat.size() <= refs[r].size(); p++)
                    if (std::equal(pat.begin(), pat.end(), refs[r].begin() + (long)p))
                        out.push_back(T5((int32_t)q, (int32_t)r, (int64_t)p, (int64_t)(p + pat.size()), comp));
        }
    }
    return out;
}

static int check(const std::vector<Seq> &refs, const std::vector<Seq> &qs, int64_t cap, int64_t seg, int bitmap)
{
    // exact-size heap copies: a read past either array is a report
    std::vector<int64_t> roff{0}, qoff{0};
    Seq r, q;
    for (const Seq &s : refs) {
        r.insert(r.end(), s.begin(), s.end());
        roff.push_back((int64_t)r.size());
    }
    for (const Seq &s : qs) {
        q.insert(q.end(), s.begin(), s.end());
        qoff.push_back((int64_t)q.size());
    }
    r.shrink_to_fit();
    q.shrink_to_fit();
    std::vector<loc::Hit> hits(1 << 16);
    int64_t info[3];
    const int64_t n = locate_host(r.data(), roff.data(), (int64_t)refs.size(), q.data(), qoff.data(), (int64_t)qs.size(), 1, cap, seg, bitmap,
                                  hits.data(), (int64_t)hits.size(), info);
    const std::vector<T5> exp = naive(refs, qs);
    if (n != (int64_t)exp.size()) return 1;
    for (int64_t i = 0; i < n; i++)
        if (T5(hits[(size_t)i].query, hits[(size_t)i].ref, hits[(size_t)i].begin, hits[(size_t)i].end, hits[(size_t)i].complement) != exp[(size_t)i])
            return 1;
    return 0;
}

int main()
{
    int bad = 0, cases = 0;
    for (size_t n = 1; n <= 200; n += (n < 70 ? 1 : 13)) {  // one record that ends the text
        const Seq rec = rnd_seq(n, n % 3 ? 4 : 2);
        std::vector<Seq> qs{rec, rc(rec), Seq(rec.end() - (long)std::min<size_t>(n, 33), rec.end()), Seq(rec.end() - (long)std::min<size_t>(n, 5), rec.end()),
                            Seq(rec.begin(), rec.begin() + (long)std::min<size_t>(n, 32)), Seq()};
        for (int bm = 0; bm < 2; bm++, cases++) bad += check({rec}, qs, 1 << 20, 1 << 20, bm);
        cases++;
        bad += check({rnd_seq(n % 7), rec, Seq(), rec}, qs, 3, 32, 0);
    }
    for (int it = 0; it < 40; it++) {  // many records, patterns around the word and the wave step
        std::vector<Seq> refs, qs;
        const int nr = 1 + (int)(rnd() % 6);
        for (int i = 0; i < nr; i++) refs.push_back(rnd_seq(rnd() % 3000, it % 4 ? 4 : 2));
        const size_t lens[] = {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 288, 289, 2047, 2048, 2049};
        for (size_t len : lens) {
            const Seq &src = refs[rnd() % refs.size()];
            if (src.size() < len) continue;
            const size_t at = it % 2 ? src.size() - len : rnd() % (src.size() - len + 1);  // odd rounds: ending at the record's last base
            Seq s(src.begin() + (long)at, src.begin() + (long)(at + len));
            qs.push_back(s);
            if (len > 40) {
                s[len - 1] ^= 1;
                qs.push_back(s);
            }
        }
        cases++;
        bad += check(refs, qs, it % 3 ? 1 << 20 : 16, it % 2 ? 1 << 20 : 64, it % 2);
    }
    printf("%d cases, %d differ from the naive search\n", cases, bad);
    return bad ? 1 : 0;
}
