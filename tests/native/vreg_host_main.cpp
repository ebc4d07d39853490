// A stand-alone run of the region validation's CPU harness (vreg_host.cpp) for the sanitizers: `make tests/native/vreg_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every case agrees and no report was printed.
// The cases: the hand-worked region of the header's contract; random records around random regions that nest, repeat and reach
// over the ends of their contigs, with windows of 1 base to more than a region, validated with the LDS tier, with the global
// tier for every region of more than one window and with a launch group per region that needs scratch -- against the
// per-region loop written out here.  The harness keeps every device buffer in a heap block of exactly its size, so an access
// behind a difference array or a list is a report.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../include/dentist_hip.h"

extern "C" int64_t vreg_host(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const dh_region *regions,
                             int32_t nregions, int32_t region_context, int32_t window, int32_t min_cov, int32_t min_span,
                             int64_t lds_windows, int64_t budget, dh_region_report *reports, int32_t *weak, int64_t weak_cap,
                             int64_t *span_off, int32_t *span_ids, int64_t span_cap, int64_t *mask_ptr, int32_t *mask_iv, int64_t mask_cap,
                             int64_t *info);

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
    std::vector<int64_t> contig_off{0};
    std::vector<dh_region> regions;
    int32_t context = 10, window = 5, min_cov = 1, min_span = 1;
};
struct Result {
    int64_t m = 0;
    std::vector<int32_t> rep, weak, ids;  // rep: 5 per region
    std::vector<int64_t> off;
    int64_t info[8];
    bool operator==(const Result &r) const { return m == r.m && rep == r.rep && weak == r.weak && ids == r.ids && off == r.off; }
};

static Result run(const Case &c, int64_t lds_windows, int64_t budget)
{
    Result r;
    const int64_t cap = 1 << 16;
    const int32_t nreg = (int32_t)c.regions.size(), ncontigs = (int32_t)c.contig_off.size() - 1;
    std::vector<dh_region_report> rep((size_t)nreg);
    std::vector<int32_t> weak((size_t)(3 * cap)), ids((size_t)cap), miv((size_t)(2 * cap));
    std::vector<int64_t> mptr((size_t)ncontigs + 1);
    std::vector<dh_la> las(c.las);
    las.shrink_to_fit();
    r.off.assign((size_t)nreg + 1, -1);
    r.m = vreg_host(las.data(), (int64_t)las.size(), c.contig_off.data(), ncontigs, c.regions.data(), nreg, c.context, c.window, c.min_cov,
                    c.min_span, lds_windows, budget, rep.data(), weak.data(), cap, r.off.data(), ids.data(), cap, mptr.data(), miv.data(), cap,
                    r.info);
    if (r.m < 0) return r;
    for (const dh_region_report &x : rep) r.rep.insert(r.rep.end(), {x.num_spanning_reads, x.weak_bp, x.is_valid, x.ctx_begin, x.ctx_end});
    r.weak.assign(weak.begin(), weak.begin() + 3 * r.m);
    r.ids.assign(ids.begin(), ids.begin() + r.off[(size_t)nreg]);
    return r;
}

// the contract region by region and window by window
static Result reference(const Case &c)
{
    Result r;
    r.off.push_back(0);
    for (const dh_region &rg : c.regions) {
        const int32_t clen = (int32_t)(c.contig_off[(size_t)rg.contig + 1] - c.contig_off[(size_t)rg.contig]);
        const int32_t cb = rg.begin > c.context ? rg.begin - c.context : 0, ce = std::min(rg.end + c.context, clen);
        int32_t span = 0, bp = 0;
        bool any = false;
        for (const dh_la &l : c.las) {
            if (l.aread != rg.contig) continue;
            if (l.abpos < cb && ce < l.aepos) span++, r.ids.push_back(l.bread);
            any = any || (l.abpos < ce && cb < l.aepos);
        }
        const int32_t wlen = std::min(c.window, ce - cb);
        std::vector<int32_t> wk;
        for (int32_t w = cb; any && wlen > 0 && w + wlen <= ce; w++) {
            int32_t cov = 0;
            for (const dh_la &l : c.las) cov += l.aread == rg.contig && l.abpos <= w && w + wlen <= l.aepos ? 1 : 0;
            if (cov >= c.min_cov) continue;
            if (wk.empty() || wk.back() < w) {
                wk.push_back(w);
                wk.push_back(w + wlen);
            } else
                wk.back() = w + wlen;
        }
        for (size_t x = 0; x + 1 < wk.size(); x += 2) {
            bp += wk[x + 1] - wk[x];
            r.weak.insert(r.weak.end(), {rg.contig, wk[x], wk[x + 1]});
            r.m++;
        }
        r.rep.insert(r.rep.end(), {span, bp, span >= c.min_span && bp == 0 ? 1 : 0, cb, ce});
        r.off.push_back((int64_t)r.ids.size());
    }
    return r;
}

static void add_record(Case &c, int32_t aread, int32_t abpos, int32_t aepos, int32_t bread)
{
    dh_la l = {};
    l.aread = aread, l.abpos = abpos, l.aepos = aepos, l.bread = bread;
    c.las.push_back(l);
}

static Case random_case(int32_t window, int32_t context)
{
    Case c;
    c.window = window, c.context = context, c.min_cov = rnd_in(1, 4), c.min_span = rnd_in(0, 3);
    const int32_t lens[] = {1, 700, 64, 1500, 300};
    for (int32_t len : lens) c.contig_off.push_back(c.contig_off.back() + len);
    for (int32_t a = 0; a < 5; a++) {
        if (a == 2) continue;  // a contig without records
        for (int k = 0; k < (lens[a] > 100 ? 70 : 3); k++) {
            const int32_t b = rnd_in(0, lens[a] - 1);
            add_record(c, a, b, std::min(lens[a], b + rnd_in(0, lens[a] / 2 + 1)), rnd_in(0, 999));
        }
    }
    for (int k = 0; k < 24; k++) {
        const int32_t a = rnd_in(0, 4), b = rnd_in(0, lens[a] + 20);
        c.regions.push_back(dh_region{a, b, b + rnd_in(0, 300)});
        if (k % 5 == 0) c.regions.push_back(c.regions.back());
    }
    return c;
}

int main()
{
    int bad = 0, cases = 0;
    {  // cb = 30, ce = 60, window 5: [35, 52) leaves [30, 39) and [48, 60) weak; [29, 61) spans
        Case c;
        c.contig_off = {0, 100};
        c.regions = {dh_region{0, 40, 50}};
        add_record(c, 0, 35, 52, 1);
        const Result r = run(c, 8192, (int64_t)1 << 30);
        cases++;
        bad += !(r.m == 2 && r.weak == std::vector<int32_t>{0, 30, 39, 0, 48, 60} && r.rep == std::vector<int32_t>{0, 21, 0, 30, 60} && r == reference(c));
        add_record(c, 0, 29, 61, 3);
        const Result q = run(c, 8192, (int64_t)1 << 30);
        cases++;
        bad += !(q.m == 0 && q.ids == std::vector<int32_t>{3} && q.rep == std::vector<int32_t>{1, 0, 1, 30, 60} && q == reference(c));
        c.las[0].aepos = 101;  // behind the contig
        const Result p = run(c, 8192, (int64_t)1 << 30);
        cases++;
        bad += !(p.m == -1 && p.info[4] == 0);
    }
    const int32_t windows[] = {1, 5, 64, 500}, contexts[] = {0, 10, 100};
    for (int32_t w : windows)
        for (int32_t x : contexts) {
            const Case c = random_case(w, x);
            const Result ref = reference(c), lds = run(c, 8192, (int64_t)1 << 30), slab = run(c, 2, (int64_t)1 << 30), cut = run(c, 100, 0);
            cases++;
            bad += !(lds == ref && slab == ref && cut == ref && lds.info[1] == 0 && (w == 500 || slab.info[1] > 0) && cut.info[2] > 10);
        }
    printf("%d cases, %d disagreements\n", cases, bad);
    return bad ? 1 : 0;
}
