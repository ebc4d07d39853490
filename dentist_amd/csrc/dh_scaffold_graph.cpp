// dh_scaffold_graph.cpp -- the graph pipeline of the scaffold-graph pile-up builder (collectPileUps/pileups.d:173-208
// build), one function per step of the reference under the names of oracle/scaffold.py: the scaffold graph with its four
// nodes per contig (scaffold.d:75-115, 237-244), multi-edges merged (pileups.d:626-636), forks resolved by read support
// (pileups.d:1592-1657, 1754-1804), min-spanning-reads (pileups.d:1807-1838), input-gap marks removed
// (pileups.d:1840-1852), extensions merged into their gap (scaffold.d:789-816) and the pile-ups read off the edges in
// edge order (pileups.d:435-444).
//
// Host code: the graph itself has 4 nodes per contig and is handled serially.  Where the reference merges equal edges
// after an unstable sort, the order here is the stable one (read id, then position on the read).
#include "dh_scaffold.h"
#include "dh_parallel.h"

namespace dh_scaffold_detail {
int check_input_gaps(const char *who, const int32_t *input_gaps, int32_t ngaps, int32_t ncontigs)
{
    for (int32_t g = 0; g < ngaps; g++)
        if (input_gaps[2 * g] < 0 || input_gaps[2 * g] >= ncontigs || input_gaps[2 * g + 1] < 0 || input_gaps[2 * g + 1] >= ncontigs)
            return dh_fail(DH_EINVAL, std::string(who) + ": input gap names a contig out of range");
    return DH_OK;
}

void remove_none_joins(std::vector<Edge> &g)
{
    g.erase(std::remove_if(g.begin(), g.end(), [](const Edge &x) { return !x.is_default() && x.empty_payload(); }), g.end());
}

// raw joins [i0, i1) sorted stably by edge, every run of equal keys as one edge appended to `out`: its read alignments
// in input order, its array allocated once, at its size
void edges_of_equal_keys(const RawJoin **i0, const RawJoin **i1, std::vector<Edge> &out)
{
    std::stable_sort(i0, i1, [](const RawJoin *a, const RawJoin *b) { return a->s == b->s ? a->e < b->e : a->s < b->s; });
    for (const RawJoin **i = i0; i < i1;) {
        const RawJoin **j = i + 1;
        while (j < i1 && (*j)->s == (*i)->s && (*j)->e == (*i)->e) j++;
        Edge m;
        m.s = (*i)->s;
        m.e = (*i)->e;
        m.types = T_PILEUP;
        m.ras.reserve((size_t)(j - i));
        for (const RawJoin **x = i; x < j; x++) m.ras.push_back((*x)->ra);
        out.push_back(std::move(m));
        i = j;
    }
}

// sort stably and merge equal edges: types OR-ed, read alignments concatenated (bulkAdd!mergeJoins)
void merge_multi_edges(std::vector<Edge> &g)
{
    std::stable_sort(g.begin(), g.end(), key_less);
    std::vector<Edge> out;
    for (size_t i = 0; i < g.size();) {
        size_t j = i + 1;
        while (j < g.size() && key_eq(g[i], g[j])) j++;
        Edge m = std::move(g[i]);
        if (j - i > 1) {
            size_t tot = m.ras.size();
            for (size_t x = i + 1; x < j; x++) tot += g[x].ras.size();
            m.ras.reserve(tot);
            for (size_t x = i + 1; x < j; x++) {
                m.types |= g[x].types;
                m.ras.insert(m.ras.end(), g[x].ras.begin(), g[x].ras.end());
            }
        }
        out.push_back(std::move(m));
        i = j;
    }
    g.swap(out);
}

Incidence incidence(const std::vector<Edge> &g, int32_t ncontigs)
{
    Incidence inc;
    inc.off.assign((size_t)ncontigs * 4 + 1, 0);
    for (const Edge &x : g) {
        inc.off[(size_t)x.s.contig * 4 + x.s.part + 1]++;
        if (!(x.e == x.s)) inc.off[(size_t)x.e.contig * 4 + x.e.part + 1]++;
    }
    for (size_t v = 0; v + 1 < inc.off.size(); v++) inc.off[v + 1] += inc.off[v];
    inc.idx.resize((size_t)inc.off.back());
    std::vector<int32_t> cur(inc.off.begin(), inc.off.end() - 1);
    for (size_t i = 0; i < g.size(); i++) {
        inc.idx[(size_t)cur[(size_t)g[i].s.contig * 4 + g[i].s.part]++] = (int32_t)i;
        if (!(g[i].e == g[i].s)) inc.idx[(size_t)cur[(size_t)g[i].e.contig * 4 + g[i].e.part]++] = (int32_t)i;
    }
    return inc;
}

namespace {
// the runs' raw joins (their concatenation is in read order) become edges by ONE stable sort by edge, spread over the
// host threads: the key space is cut into buckets by the start contig, every run counts and then scatters its joins
// into the buckets' slices (bucket-major, run order inside: the concatenation's order), every bucket is sorted stably
// by edge on its own and yields its edges with their read alignments in read order -- an edge's array is allocated
// once, at its size.  (Edges per run first, then a merge of the runs' edge lists: reads lie anywhere, so a run of
// 4 096 joins of configs[2] held 2 500 edges of 1.6 read alignments -- 100 000 small arrays allocated, merged and freed,
// 3.3 of the plan's 8 ms at N = 8; before that one serial stable sort over all edges: 7.7 of the collect stage's 14 ms.)
void edges_from_runs(const std::vector<std::vector<RawJoin>> &found, int32_t ncontigs, std::vector<Edge> &g)
{
    const int32_t nbuck = (int32_t)std::max<int64_t>(1, std::min<int64_t>(256, ncontigs / 4));
    const int64_t nruns = (int64_t)found.size();
    auto bucket_of = [&](int32_t contig) {  // (monotone in the contig; ids are checked by the callers, the clamp keeps a stray one inside)
        const int64_t b = (int64_t)contig * nbuck / std::max(ncontigs, 1);
        return (int32_t)std::min<int64_t>(std::max<int64_t>(b, 0), nbuck - 1);
    };
    std::vector<int64_t> at((size_t)nruns * (size_t)nbuck + 1, 0);  // [bucket][run] -> first slot
    dh_parallel_for(nruns, 1, [&](int64_t lo, int64_t hi) {
        for (int64_t run = lo; run < hi; run++)
            for (const RawJoin &r : found[(size_t)run]) at[(size_t)bucket_of(r.s.contig) * (size_t)nruns + (size_t)run]++;
    });
    int64_t total = 0;
    for (size_t i = 0; i < (size_t)nruns * (size_t)nbuck; i++) {
        const int64_t c = at[i];
        at[i] = total;
        total += c;
    }
    at[(size_t)nruns * (size_t)nbuck] = total;
    std::vector<const RawJoin *> item((size_t)total);
    dh_parallel_for(nruns, 1, [&](int64_t lo, int64_t hi) {
        std::vector<int64_t> cur((size_t)nbuck);
        for (int64_t run = lo; run < hi; run++) {
            for (int32_t bk = 0; bk < nbuck; bk++) cur[(size_t)bk] = at[(size_t)bk * (size_t)nruns + (size_t)run];
            for (const RawJoin &r : found[(size_t)run]) item[(size_t)cur[(size_t)bucket_of(r.s.contig)]++] = &r;
        }
    });
    std::vector<std::vector<Edge>> merged((size_t)nbuck);
    dh_parallel_for(nbuck, 1, [&](int64_t blo, int64_t bhi) {
        for (int64_t bk = blo; bk < bhi; bk++)
            edges_of_equal_keys(item.data() + at[(size_t)bk * (size_t)nruns], item.data() + at[(size_t)(bk + 1) * (size_t)nruns], merged[(size_t)bk]);
    });
    for (auto &v : merged)
        for (auto &e : v) g.push_back(std::move(e));
}

void add_input_gaps(std::vector<Edge> &g, const int32_t *input_gaps, int32_t ngaps)
{
    for (int32_t x = 0; x < ngaps; x++) {
        Edge e = make_edge(Node{input_gaps[2 * x], END}, Node{input_gaps[2 * x + 1], BEGIN});
        e.types = T_INPUTGAP;
        g.push_back(std::move(e));
    }
}

// findCorrectGapJoin (pileups.d:1754-1804): the best-supported join wins if it beats the runner-up by the margin; joins
// of the input assembly get a bonus.  Returns its index in gj (>= 2 joins), gj.size() if none wins
size_t find_correct_gap_join(const std::vector<Edge> &g, const std::vector<int32_t> &gj, const dh_scaffold_opts &o)
{
    std::vector<std::pair<double, size_t>> val;
    for (size_t x = 0; x < gj.size(); x++) {
        const Edge &e = g[(size_t)gj[x]];
        val.emplace_back((double)e.ras.size() * ((e.types & T_INPUTGAP) ? o.existing_gap_bonus : 1.0), x);
    }
    std::stable_sort(val.begin(), val.end(), [](const auto &p, const auto &q) { return p.first > q.first; });
    return val[1].first * o.best_pile_up_margin < val[0].first ? val[0].second : gj.size();
}

// discardAmbiguousJoins (pileups.d:1592-1657)
void discard_ambiguous_joins(std::vector<Edge> &g, int32_t ncontigs, const dh_scaffold_opts &o)
{
    const auto inc = incidence(g, ncontigs);
    std::vector<char> drop(g.size(), 0);
    for (int32_t ct = 0; ct < ncontigs; ct++)
        for (int32_t part : {BEGIN, END}) {
            const auto in = inc[(size_t)ct * 4 + part];
            if (in.size() <= 2) continue;
            std::vector<int32_t> gj;
            for (int32_t ei : in)
                if (g[(size_t)ei].is_gap() && (g[(size_t)ei].types & T_PILEUP)) gj.push_back(ei);
            if (gj.size() <= 1) continue;
            const size_t keep = find_correct_gap_join(g, gj, o);
            for (size_t x = 0; x < gj.size(); x++)
                if (x != keep) drop[(size_t)gj[x]] = 1;
        }
    for (size_t i = 0; i < g.size(); i++)
        if (drop[i]) g[i].drop_pile_up();
    remove_none_joins(g);
}

// enforceMinSpanningReads (pileups.d:1807-1838)
void enforce_min_spanning_reads(std::vector<Edge> &g, int64_t min_spanning_reads)
{
    for (Edge &e : g)
        if ((e.types & T_PILEUP) && e.is_gap() && (int64_t)e.ras.size() < min_spanning_reads) e.drop_pile_up();
    remove_none_joins(g);
}

// removeInputGaps (pileups.d:1840-1852)
void remove_input_gaps(std::vector<Edge> &g)
{
    for (Edge &e : g) e.types &= ~(uint32_t)T_INPUTGAP;
    remove_none_joins(g);
}

// mergeExtensionsWithGaps (scaffold.d:789-816): emptied edges stay until the end
int merge_extensions_with_gaps(std::vector<Edge> &g, int32_t ncontigs)
{
    const auto inc = incidence(g, ncontigs);
    for (int32_t ct = 0; ct < ncontigs; ct++)
        for (int32_t part : {BEGIN, END}) {
            const auto in = inc[(size_t)ct * 4 + part];
            if (in.size() > 3) return dh_fail(DH_EINVAL, "dh_scaffold_pileups: node degree must be <= 3");
            if (in.size() != 3) continue;
            int32_t nd[2], k = 0;
            for (int32_t ei : in)
                if (!g[(size_t)ei].is_default() && k < 2) nd[k++] = ei;
            if (k != 2) continue;
            const Node me{ct, part};
            auto other = [&](const Edge &e) { return e.s == me ? e.e : e.s; };
            const int gi = real_part(other(g[(size_t)nd[0]]).part) ? 0 : 1;
            Edge &gap = g[(size_t)nd[gi]], &ext = g[(size_t)nd[1 - gi]];
            gap.types |= ext.types;
            gap.ras.insert(gap.ras.end(), ext.ras.begin(), ext.ras.end());
            ext.types = 0;
            ext.ras.clear();
        }
    remove_none_joins(g);
    return DH_OK;
}

// collectPileUps (pileups.d:435-444): valid pile-ups in edge order
dh_scaffold *collect_pile_ups(const std::vector<Edge> &g)
{
    dh_scaffold *res = new dh_scaffold();
    for (const Edge &e : g) {
        if (!(e.types & T_PILEUP) || e.ras.empty()) continue;
        bool any_gap = false, all_front = true, all_back = true;
        for (const dh_read_alignment &ra : e.ras) {
            any_gap = any_gap || ra.n == 2;
            all_front = all_front && ra.n == 1 && ra.seed0 == FRONT;
            all_back = all_back && ra.n == 1 && ra.seed0 == BACK;
        }
        const bool is_ext = all_front || all_back;
        if (is_ext == any_gap) continue;  // PileUp.isValid, base.d:2755-2790
        const int32_t type = any_gap ? 1 : (all_front ? 0 : 2);  // ReadAlignmentType: front, gap, back
        res->joins.push_back(dh_join{e.s.contig, e.s.part, e.e.contig, e.e.part, type, (int32_t)e.ras.size(), (int64_t)res->entries.size()});
        res->entries.insert(res->entries.end(), e.ras.begin(), e.ras.end());
    }
    return res;
}
}  // namespace

// build() (pileups.d:173-208) on the raw joins of all reads, which it consumes; rs: resolveBubbles runs between the raw
// scaffold and discardAmbiguousJoins (pileups.d:186), without it the forks of a bubble go through the read-support rule
// like any other fork
int scaffold_from_runs(std::vector<std::vector<RawJoin>> &found, int32_t ncontigs, const int32_t *input_gaps, int32_t ngaps,
                       const dh_scaffold_opts *opts, dh_scaffold **out, Resolver *rs)
{
    dh_lap_timer lap{"[scaffold]", 24};
    // ---- the scaffold: default edges, read joins, input gaps (buildScaffold, scaffold.d:237-244)
    std::vector<Edge> g;
    for (int32_t ct = 0; ct < ncontigs; ct++) g.push_back(make_edge(Node{ct, BEGIN}, Node{ct, END}));
    edges_from_runs(found, ncontigs, g);
    found.clear();
    add_input_gaps(g, input_gaps, ngaps);
    merge_multi_edges(g);
    remove_none_joins(g);
    lap("graph merge");
    if (rs) {
        if (int rc = resolve_bubbles(g, ncontigs, *rs)) return rc;
        lap("resolve bubbles");
    }
    discard_ambiguous_joins(g, ncontigs, *opts);
    lap("discard ambiguous");
    enforce_min_spanning_reads(g, opts->min_spanning_reads);
    remove_input_gaps(g);
    if (opts->merge_extensions)
        if (int rc = merge_extensions_with_gaps(g, ncontigs)) return rc;
    lap("min reads, extensions");
    *out = collect_pile_ups(g);
    lap("collect pile-ups");
    return DH_OK;
}
}  // namespace dh_scaffold_detail
