// A stand-alone run of the mask propagation's CPU harness (pmask_host.cpp) for the sanitizers: `make tests/native/pmask_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every case agrees and no report was printed.
// The cases: the worked example of the header with its intervals written out; random records of 1..700 tiles on both strands
// with 0..200 intersecting mask intervals (first and last cut at or beginning at the record's ends, tiles without b-bases),
// into reads of 1..65 and of thousands of bases, propagated with one destination range and one launch group, and again with a
// range per few words and small launch groups -- against a sort-and-merge union computed here.  The harness keeps every device
// buffer in a heap block of exactly its size, so an access behind the bitmap's edge words or a trace's last chunk is a report.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/dentist_hip.h"

extern "C" int64_t pmask_host(const dh_la *las, int64_t n, const uint16_t *trace, int64_t trace_len, int32_t tspace, const int64_t *mask_ptr,
                              const int32_t *mask_iv, int32_t ncontigs, const int64_t *read_off, int32_t nreads, int64_t cap_bits,
                              int64_t group_raw, int64_t *out_ptr, int32_t *out_iv, int64_t cap, int64_t *info);

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
    std::vector<uint16_t> trace;
    std::vector<int64_t> mask_ptr{0}, read_off;
    std::vector<int32_t> mask_iv;
    int32_t ts = 100;
};
struct Result {
    int64_t m = 0;
    std::vector<int64_t> ptr;
    std::vector<int32_t> iv;
    int64_t info[8];
    bool operator==(const Result &r) const { return m == r.m && ptr == r.ptr && iv == r.iv; }
};

static Result run(const Case &c, int64_t cap_bits, int64_t group_raw)
{
    Result r;
    const int64_t cap = 1 << 18;
    const int32_t nreads = (int32_t)c.read_off.size() - 1;
    std::vector<int32_t> iv((size_t)(2 * cap));
    std::vector<int32_t> miv(c.mask_iv);
    miv.shrink_to_fit();
    r.ptr.assign((size_t)nreads + 1, -1);
    r.m = pmask_host(c.las.data(), (int64_t)c.las.size(), c.trace.data(), (int64_t)c.trace.size(), c.ts, c.mask_ptr.data(), miv.data(),
                     (int32_t)c.mask_ptr.size() - 1, c.read_off.data(), nreads, cap_bits, group_raw, r.ptr.data(), iv.data(), cap, r.info);
    if (r.m > 0) r.iv.assign(iv.begin(), iv.begin() + 2 * r.m);
    return r;
}

// the contract by sorting: trace-point indices by walking the trace points one by one
static Result reference(const Case &c)
{
    struct Iv {
        int32_t rd, b, e;
    };
    std::vector<Iv> all;
    const int32_t ts = c.ts;
    for (const dh_la &l : c.las) {
        const int32_t blen = (int32_t)(c.read_off[(size_t)l.bread + 1] - c.read_off[(size_t)l.bread]);
        for (int64_t j = c.mask_ptr[(size_t)l.aread]; j < c.mask_ptr[(size_t)l.aread + 1]; j++) {
            const int32_t mb = c.mask_iv[(size_t)(2 * j)], me = c.mask_iv[(size_t)(2 * j + 1)];
            if (me <= l.abpos || mb >= l.aepos) continue;
            const int32_t ib = std::max(mb, l.abpos), ie = std::min(me, l.aepos);
            // trace points on A: abpos, the multiples of ts inside, aepos
            int32_t a = l.abpos, b = l.bbpos, b0 = l.bbpos, b1 = -1;
            if (ie == l.abpos) b1 = l.bbpos;
            for (int32_t t = 0; t < l.tlen / 2; t++) {
                const int32_t na = std::min(l.aepos, a / ts * ts + ts);
                b += c.trace[(size_t)(l.toff + 2 * t + 1)];
                a = na;
                if (a <= ib) b0 = b;                  // the last trace point at or before ib
                if (b1 < 0 && a >= ie) b1 = b;        // the first trace point at or behind ie
            }
            if (l.flags & DH_FLAG_COMP) {
                const int32_t x0 = blen - b1, x1 = blen - b0;
                b0 = x0, b1 = x1;
            }
            if (b1 > b0) all.push_back(Iv{l.bread, b0, b1});
        }
    }
    std::sort(all.begin(), all.end(), [](const Iv &x, const Iv &y) { return x.rd != y.rd ? x.rd < y.rd : (x.b != y.b ? x.b < y.b : x.e < y.e); });
    Result r;
    const int32_t nreads = (int32_t)c.read_off.size() - 1;
    size_t at = 0;
    for (int32_t rd = 0; rd < nreads; rd++) {
        r.ptr.push_back(r.m);
        while (at < all.size() && all[at].rd == rd) {
            int32_t b = all[at].b, e = all[at].e;
            for (at++; at < all.size() && all[at].rd == rd && all[at].b <= e; at++) e = std::max(e, all[at].e);
            r.iv.push_back(b);
            r.iv.push_back(e);
            r.m++;
        }
    }
    r.ptr.push_back(r.m);
    return r;
}

static void add_record(Case &c, int32_t aread, int32_t bread, int32_t abpos, int32_t aepos, int32_t bbpos, const std::vector<int32_t> &bb,
                       uint32_t flags)
{
    dh_la l = {};
    l.aread = aread, l.bread = bread, l.abpos = abpos, l.aepos = aepos, l.bbpos = bbpos, l.flags = flags;
    l.tlen = 2 * (int32_t)bb.size(), l.toff = (int64_t)c.trace.size();
    int32_t be = bbpos;
    for (int32_t b : bb) {
        c.trace.push_back(0);
        c.trace.push_back((uint16_t)b);
        be += b;
    }
    l.bepos = be;
    c.las.push_back(l);
}

// short reads: a record per read whose single tile covers the read, the mask picks a part of the tile or all of it
static Case small_reads()
{
    Case c;
    const int32_t lens[] = {1, 31, 32, 33, 63, 64, 65, 1, 64, 64, 32, 32, 300};
    int32_t contig = 0;
    c.read_off.push_back(0);
    for (int32_t len : lens) {
        const int32_t rd = (int32_t)c.read_off.size() - 1;
        c.read_off.push_back(c.read_off.back() + len);
        // tiles that end inside the read at random cuts
        std::vector<int32_t> cuts{0, len};
        for (int k = 0; k < 3 && len > 2; k++) cuts.push_back(rnd_in(1, len - 1));
        std::sort(cuts.begin(), cuts.end());
        cuts.erase(std::unique(cuts.begin(), cuts.end()), cuts.end());
        std::vector<int32_t> bb;
        for (size_t k = 0; k + 1 < cuts.size(); k++) bb.push_back(cuts[k + 1] - cuts[k]);
        add_record(c, contig, rd, 0, 100 * (int32_t)bb.size(), 0, bb, rd % 3 == 0 ? DH_FLAG_COMP : 0u);
        if (rd % 4 == 3)  // the whole read
            c.mask_iv.insert(c.mask_iv.end(), {0, 100 * (int32_t)bb.size()});
        else
            for (size_t k = 0; k < bb.size(); k += 2) c.mask_iv.insert(c.mask_iv.end(), {100 * (int32_t)k + 10, 100 * (int32_t)k + 20});
        c.mask_ptr.push_back((int64_t)c.mask_iv.size() / 2);
        contig++;
    }
    return c;
}

static Case random_case(int32_t ts)
{
    Case c;
    c.ts = ts;
    const int tiles[] = {1, 2, 63, 64, 65, 129, 700}, counts[] = {0, 1, 2, 63, 64, 65, 200};
    const int32_t nreads = 9;
    std::vector<int64_t> len((size_t)nreads, 0);
    int32_t contig = 0;
    for (int t : tiles)
        for (int k : counts) {
            const int32_t abpos = 2 * ts + ((contig & 1) ? 0 : 37), aepos = (2 + t) * ts - ((contig & 1) ? 0 : 11);
            const int32_t kk = std::min(k, (aepos - abpos) / 2);
            std::vector<int32_t> bb;
            for (int x = 0; x < t; x++) bb.push_back(rnd() % 10 == 0 ? 0 : rnd_in(ts - 12, ts + 12));
            const int32_t rd = rnd_in(0, nreads - 2), bbpos = rnd_in(0, 2000);
            add_record(c, contig, rd, abpos, aepos, bbpos, bb, (contig & 2) ? DH_FLAG_COMP : 0u);
            len[(size_t)rd] = std::max<int64_t>(len[(size_t)rd], c.las.back().bepos + rnd_in(0, 30));
            // kk intervals: cut points drawn from [abpos, aepos], sorted, made distinct
            std::vector<int32_t> pts;
            while ((int32_t)pts.size() < 2 * kk) {
                pts.push_back(rnd_in(abpos, aepos));
                std::sort(pts.begin(), pts.end());
                pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
            }
            if (kk) {
                if (contig & 4)
                    pts.front() = abpos - 5, pts.back() = aepos + 5;
                else
                    pts.front() = abpos, pts.back() = aepos;
            }
            c.mask_iv.insert(c.mask_iv.end(), pts.begin(), pts.end());
            c.mask_ptr.push_back((int64_t)c.mask_iv.size() / 2);
            contig++;
        }
    c.read_off.push_back(0);
    for (int64_t x : len) c.read_off.push_back(c.read_off.back() + x);
    return c;
}

int main()
{
    int bad = 0, cases = 0;
    {  // the worked example of the header, forward and complement
        Case c;
        add_record(c, 0, 0, 150, 420, 1000, {48, 103, 97, 21}, 0u);
        c.mask_iv = {0, 160, 250, 260, 405, 500};
        c.mask_ptr = {0, 3};
        c.read_off = {0, 2000};
        const Result r = run(c, (int64_t)1 << 35, (int64_t)1 << 31);
        cases++;
        bad += !(r.m == 2 && r.ptr == std::vector<int64_t>{0, 2} && r.iv == std::vector<int32_t>{1000, 1151, 1248, 1269} && r == reference(c));
        c.las[0].flags = DH_FLAG_COMP;
        const Result q = run(c, (int64_t)1 << 35, (int64_t)1 << 31);
        cases++;
        bad += !(q.m == 2 && q.iv == std::vector<int32_t>{731, 752, 849, 1000} && q == reference(c));
        c.trace[7] = 60000;  // the b-bases run past the read
        const Result p = run(c, (int64_t)1 << 35, (int64_t)1 << 31);
        cases++;
        bad += !(p.m == -1 && p.info[6] == 0);
    }
    {
        const Case c = small_reads();
        const Result ref = reference(c);
        for (int64_t cap_bits : {(int64_t)1 << 35, (int64_t)512, (int64_t)1}) {
            const Result r = run(c, cap_bits, (int64_t)1 << 31);
            cases++;
            bad += !(r == ref && r.m > 0);
        }
    }
    for (int it = 0; it < 6; it++) {
        const Case c = random_case(it % 2 ? 126 : 100);
        const Result ref = reference(c), one = run(c, (int64_t)1 << 35, (int64_t)1 << 31), cut = run(c, 2048, 150);
        cases++;
        bad += !(one == ref && cut == ref && ref.m > 0 && one.info[0] > ref.m && one.info[2] == 1 && cut.info[2] > 2 && cut.info[3] > 2);
    }
    printf("%d cases, %d disagreements\n", cases, bad);
    return bad ? 1 : 0;
}
