// dh_scaffold_views.cpp -- the pile-ups read off a finished scaffold (dh_scaffold_spanning, dh_scaffold_gap_pileups,
// dh_scaffold_all_pileups): one per-join function that turns a join's read alignments into (read, LA on flank 0, LA on
// flank 1) triples, one parallel loop over the joins, one pass that concatenates them.  The three calls differ in which
// joins they take, whether they keep read alignments of one LA, and how the pile-ups are handed over.
#include <array>

#include "dh_scaffold.h"
#include "dh_parallel.h"

using namespace dh_scaffold_detail;

namespace {
struct View {
    bool adjacent;  // the gap joins (c, end) -- (c + 1, begin) only; else by `only`
    int32_t only;   // & 1: gap joins of any two contig ends, & 2: extension joins
    bool one_la;    // keep the extension-type read alignments, (read, LA, -1) / (read, -1, LA)
};
typedef std::array<int32_t, 3> Triple;
typedef std::array<int32_t, 4> Nodes;  // (contig0, seed0, contig1 or -1, seed1) as dh_pileups_create_joins takes them

// The triples of join j sorted stably by read (empty: the view does not take the join, or none of its entries), and its
// nodes.  An LA belongs to the flank whose contig and seed it has (flank_of); a read alignment of two LAs needs one on
// each flank and complement flags that fit the join (parallel: equal, anti-parallel: different).  A scaffold of the
// builder derives an edge's nodes from its entries (read_joins; the JoinRec nodes of the blob path), so the flank test
// holds for every entry there and all three views use it.  (The loop waits on cache misses into `las`: the two-LA case
// states the test as four comparisons on the two records, which measured 0.2 ms less per plan than two flank_of calls.)
void join_triples(const dh_scaffold *s, const dh_la *las, int64_t n, const dh_join &j, const View &v, Nodes &node, std::vector<Triple> &t)
{
    const bool gap = real_part(j.part0) && real_part(j.part1) && j.contig0 != j.contig1;
    const bool fext = j.contig0 == j.contig1 && j.part0 == PRE && j.part1 == BEGIN;
    const bool bext = j.contig0 == j.contig1 && j.part0 == END && j.part1 == POST;
    if (v.adjacent ? !(j.type == 1 && j.part0 == END && j.part1 == BEGIN && j.contig1 == j.contig0 + 1)
                   : !((gap && (v.only & 1)) || ((fext || bext) && (v.only & 2))))
        return;
    const int32_t c0 = j.contig0, c1 = gap ? j.contig1 : -1;
    const int32_t s0 = gap ? (j.part0 == BEGIN ? FRONT : BACK) : (fext ? FRONT : BACK), s1 = gap ? (j.part1 == BEGIN ? FRONT : BACK) : 0;
    node = {c0, s0 == FRONT ? DH_SEED_FRONT : DH_SEED_BACK, c1, gap && s1 == BACK ? DH_SEED_BACK : DH_SEED_FRONT};
    t.reserve((size_t)j.count);
    auto flank_of = [&](int32_t la, int32_t seed) {
        if (las[la].aread == c0 && seed == s0) return 0;
        if (gap && las[la].aread == c1 && seed == s1) return 1;
        return -1;
    };
    for (int64_t x = j.first; x < j.first + j.count; x++) {
        const dh_read_alignment &ra = s->entries[(size_t)x];
        if (ra.la0 < 0 || ra.la0 >= n) continue;
        if (ra.n == 2) {
            if (ra.la1 < 0 || ra.la1 >= n || !gap) continue;
            const dh_la &a = las[ra.la0], &b = las[ra.la1];
            // (one LA on each flank: as the builder orders them, la0 on flank 0, or the other way round)
            const bool fwd = a.aread == c0 && ra.seed0 == s0 && b.aread == c1 && ra.seed1 == s1;
            if (!fwd && !(b.aread == c0 && ra.seed1 == s0 && a.aread == c1 && ra.seed0 == s1)) continue;
            if (((a.flags & DH_FLAG_COMP) == (b.flags & DH_FLAG_COMP)) != (s0 != s1)) continue;
            t.push_back({ra.read, fwd ? ra.la0 : ra.la1, fwd ? ra.la1 : ra.la0});
        } else if (v.one_la) {
            const int f0 = flank_of(ra.la0, ra.seed0);
            if (f0 >= 0) t.push_back(f0 == 0 ? Triple{ra.read, ra.la0, -1} : Triple{ra.read, -1, ra.la0});
        }
    }
    std::stable_sort(t.begin(), t.end(), [](const Triple &a, const Triple &b) { return a[0] < b[0]; });
}

// the pile-ups of view v: by contig_left (dh_pileups_create) or, with_nodes, with their nodes in node order
// (dh_pileups_create_joins); *skipped = joins that yield no pile-up
int view_pileups(const dh_scaffold *s, const dh_la *las, int64_t n, const View &v, bool with_nodes, dh_pileups **out, int32_t *skipped)
{
    // joins are independent: host threads fill one triple list per join, the lists are concatenated in join order
    const int64_t nj = (int64_t)s->joins.size();
    std::vector<std::vector<Triple>> per((size_t)nj);
    std::vector<Nodes> node((size_t)nj);
    dh_parallel_for(nj, 16, [&](int64_t lo, int64_t hi) {
        for (int64_t ji = lo; ji < hi; ji++) join_triples(s, las, n, s->joins[(size_t)ji], v, node[(size_t)ji], per[(size_t)ji]);
    });
    std::vector<int64_t> order;
    size_t total = 0;
    for (int64_t ji = 0; ji < nj; ji++)
        if (!per[(size_t)ji].empty()) {
            order.push_back(ji);
            total += per[(size_t)ji].size();
        }
    if (skipped) *skipped = (int32_t)(nj - (int64_t)order.size());
    if (with_nodes) {
        // dh_pileups_create_joins wants the pile-ups in node order: (contig0, seed0, contig1 or "none" last, seed1)
        auto key = [&](int64_t ji) {
            const Nodes &q = node[(size_t)ji];
            return std::array<int64_t, 4>{q[0], q[1], q[2] < 0 ? INT32_MAX : q[2], q[3]};
        };
        std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return key(a) < key(b); });
    }
    std::vector<int32_t> nd, cl, cnt, tri;
    tri.reserve(3 * total);
    for (int64_t ji : order) {
        nd.insert(nd.end(), node[(size_t)ji].begin(), node[(size_t)ji].end());
        cl.push_back(node[(size_t)ji][0]);
        cnt.push_back((int32_t)per[(size_t)ji].size());
        for (const Triple &x : per[(size_t)ji]) tri.insert(tri.end(), x.begin(), x.end());
    }
    return with_nodes ? dh_pileups_create_joins(nd.data(), cnt.data(), (int32_t)cnt.size(), tri.data(), out)
                      : dh_pileups_create(cl.data(), cnt.data(), (int32_t)cl.size(), tri.data(), out);
}
}  // namespace

// The gap pile-ups the process path handles: joins (c, end) -- (c + 1, begin) whose spanning reads see both contigs in the
// same orientation; of every such pile-up the spanning read alignments (left LA seeded at the back, right LA at the front)
// become (read, left LA, right LA) triples ordered by read.  Everything else (extension pile-ups, joins between other
// contig ends, extension reads merged into a gap) is counted in *skipped.
extern "C" int dh_scaffold_spanning(const dh_scaffold *s, const dh_la *las, int64_t n, dh_pileups **out, int32_t *skipped)
{
    if (!s || !out || (n > 0 && !las)) return dh_fail(DH_EINVAL, "dh_scaffold_spanning: bad argument");
    return view_pileups(s, las, n, View{true, 0, false}, false, out, skipped);
}

// The pile-ups of the gap joins (c, end)--(c + 1, begin) with EVERY read alignment the builder put into them: reads
// spanning the gap as (read, left LA, right LA) and the extension-type read alignments that mergeExtensionsWithGaps
// (scaffold.d:789-816) moved into the gap -- (read, LA, -1) for a back extension of the left contig, (read, -1, LA) for a
// front extension of the right one -- which the reference crops and aligns like any other member of the pile-up
// (cropper.d:113-175, 339-361).  Entries are ordered by read, then by their position in the builder's list.  *skipped =
// pile-ups of any other kind.
extern "C" int dh_scaffold_gap_pileups(const dh_scaffold *s, const dh_la *las, int64_t n, dh_pileups **out, int32_t *skipped)
{
    if (!s || !out || (n > 0 && !las)) return dh_fail(DH_EINVAL, "dh_scaffold_gap_pileups: bad argument");
    return view_pileups(s, las, n, View{true, 0, true}, false, out, skipped);
}

// Every pile-up of the scaffold the process stage can take (`dentist process` is handed all of them; `--only` of
// `dentist output`, commandline.d:2230-2250, decides later which insertions are used): only & 1 = the gap joins of
// any two contig ends -- same orientation, anti-parallel ((c, end) -> (d, end), (c, begin) -> (d, begin)), contig-
// skipping --, only & 2 = the extension joins ((c, pre) -> (c, begin), (c, end) -> (c, post)).  Pile-ups come with
// their nodes (dh_pileups_create_joins); entries are (read, LA on flank 0, LA on flank 1), extension-type read
// alignments merged into a gap have one of the two.  A read alignment whose two complement flags do not fit the
// join (parallel: equal, anti-parallel: different) is left out, as dh_scaffold_gap_pileups does.  *skipped = joins
// without entries, joins of a contig with itself.
extern "C" int dh_scaffold_all_pileups(const dh_scaffold *s, const dh_la *las, int64_t n, int32_t only, dh_pileups **out, int32_t *skipped)
{
    if (!s || !out || (n > 0 && !las) || (only & ~3) || !only) return dh_fail(DH_EINVAL, "dh_scaffold_all_pileups: bad argument");
    return view_pileups(s, las, n, View{false, only, true}, true, out, skipped);
}
