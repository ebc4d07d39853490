// dh_scaffold_bubbles.cpp -- resolveBubbles (pileups.d:1100-1590) of the scaffold-graph pile-up builder: Paton's cycle
// base as util/math.d:2380-2480 walks it, simple bubbles, skipped path, collectFixedSimpleBubbles, graph surgery.  A
// bubble: a cycle of at most max_bubble_size nodes with exactly two nodes of degree >= 3 (extension joins not counted)
// that are joined by an edge carrying a pile-up -- the reads of that pile-up SKIP the contigs on the other side of the
// cycle (their alignments there were masked or filtered away).  The skipping reads are mapped onto the intermediate
// contigs once more, without any mask (remap = getReadAlignmentsOnContigs, :1316-1385: dh_remap_skipping_reads on the
// device, dh_scaffold_pileups_resolved, or the caller's, dh_scaffold_pileups_cb), their read alignments are collected again
// from the old and the new alignments together, kept iff they walk the skipped path in order
// (collectFixedSimpleBubbles :1414-1491), and replace the pile-up of the skipping edge.
#include "dh_scaffold.h"

namespace dh_scaffold_detail {
namespace {
inline Node node_of(int32_t v) { return Node{v / 4, v % 4}; }
inline int32_t index_of(Node n) { return n.contig * 4 + n.part; }

Edge *find_edge(std::vector<Edge> &g, Node a, Node b)  // g sorted by key (merge_multi_edges)
{
    const Edge key = make_edge(a, b);
    auto it = std::lower_bound(g.begin(), g.end(), key, key_less);
    return it != g.end() && key_eq(*it, key) ? &*it : nullptr;
}

// Paton's cycle base exactly as util/math.d:2380-2480 walks it (roots in node order, LIFO, incident edges in edge order)
std::vector<std::vector<int32_t>> cycle_base(const std::vector<Edge> &g, const Incidence &inc)
{
    const size_t nn = inc.size();
    std::vector<std::vector<int32_t>> used(nn), cycles;
    std::vector<int32_t> parent(nn, -1), stack;
    auto has = [&](int32_t node, int32_t x) { return std::find(used[(size_t)node].begin(), used[(size_t)node].end(), x) != used[(size_t)node].end(); };
    for (int32_t root = 0; root < (int32_t)nn; root++) {
        if (parent[(size_t)root] >= 0 || inc[(size_t)root].empty()) continue;  // (isolated nodes yield nothing)
        parent[(size_t)root] = root;
        used[(size_t)root].push_back(root);
        stack.push_back(root);
        while (!stack.empty()) {
            const int32_t cur = stack.back();
            stack.pop_back();
            const Node me{cur / 4, cur % 4};
            for (int32_t ei : inc[(size_t)cur]) {
                const Edge &e = g[(size_t)ei];
                const Node o = e.s == me ? e.e : e.s;
                const int32_t nb = o.contig * 4 + o.part;
                if (used[(size_t)nb].empty()) {
                    parent[(size_t)nb] = cur;
                    used[(size_t)nb].push_back(cur);
                    stack.push_back(nb);
                } else if (nb == cur)
                    cycles.push_back({cur});
                else if (!has(cur, nb)) {
                    std::vector<int32_t> cyc{nb, cur};
                    int32_t p = parent[(size_t)cur];
                    for (; !has(nb, p); p = parent[(size_t)p]) cyc.push_back(p);
                    cyc.push_back(p);
                    cycles.push_back(std::move(cyc));
                    used[(size_t)nb].push_back(cur);
                }
            }
        }
    }
    return cycles;
}

// the edge of a cycle that skips the rest of it: the one between the cycle's two nodes of degree >= 3, if it carries a
// pile-up (nullptr: none, or resolved through another bubble of this iteration)
Edge *skipping_edge(std::vector<Edge> &g, const std::vector<int32_t> &cyc, const std::vector<int32_t> &deg)
{
    int32_t esc[2], ne = 0;
    for (int32_t v : cyc)
        if (deg[(size_t)v] >= 3 && ne < 2) esc[ne++] = v;
    Edge *sk = ne == 2 ? find_edge(g, node_of(esc[0]), node_of(esc[1])) : nullptr;
    return sk && (sk->types & T_PILEUP) ? sk : nullptr;
}

// the simple bubbles of the graph: degrees without the extension joins (out: deg), the cycles of the base that are small
// enough, have exactly two nodes of degree >= 3 and none below 2, and a skipping edge
std::vector<std::vector<int32_t>> find_bubbles(std::vector<Edge> &g, const Incidence &inc, int32_t max_bubble_size, std::vector<int32_t> &deg)
{
    deg.assign(inc.size(), 0);
    for (size_t v = 0; v < inc.size(); v++)
        for (int32_t ei : inc[v]) deg[v] += g[(size_t)ei].is_ext() ? 0 : 1;
    std::vector<std::vector<int32_t>> bubbles;
    for (auto &cyc : cycle_base(g, inc)) {
        if ((int32_t)cyc.size() > max_bubble_size) continue;
        const auto forks = std::count_if(cyc.begin(), cyc.end(), [&](int32_t v) { return deg[(size_t)v] >= 3; });
        const bool ends = std::any_of(cyc.begin(), cyc.end(), [&](int32_t v) { return deg[(size_t)v] < 2; });
        if (!ends && forks == 2 && skipping_edge(g, cyc, deg)) bubbles.push_back(cyc);
    }
    return bubbles;
}

// the skipped path: from the skipping edge's start around the cycle to its end (the long way)
std::vector<Node> skipped_path(const std::vector<int32_t> &cyc, const Edge &sk)
{
    const int32_t L = (int32_t)cyc.size();
    const int32_t i0 = (int32_t)(std::find(cyc.begin(), cyc.end(), index_of(sk.s)) - cyc.begin()),
                  i1 = (int32_t)(std::find(cyc.begin(), cyc.end(), index_of(sk.e)) - cyc.begin());
    auto walk = [&](int32_t a, int32_t b) {
        std::vector<Node> p;
        for (int32_t x = 0; x <= ((b - a) % L + L) % L; x++) p.push_back(node_of(cyc[(size_t)((a + x) % L)]));
        return p;
    };
    std::vector<Node> path = walk(i0, i1);
    if (path.size() == 2) path = walk(i1, i0);
    return path;
}

// collectFixedSimpleBubbles: the seeded alignments of one read (read order) must walk the skipped path
bool walks_path(const Ctx &c, const std::vector<SA> &sa, const std::vector<Node> &path)
{
    auto matches = [&](const Node &nd, const SA &x) {
        return nd.contig == c.L(x.la).aread && ((nd.part == BEGIN && x.seed == FRONT) || (nd.part == END && x.seed == BACK));
    };
    const bool rev = path[0].contig != c.L(sa[0].la).aread;
    auto pnode = [&](size_t x) { return rev ? path[path.size() - 1 - x] : path[x]; };
    size_t at = 0;
    while (at < sa.size() && !matches(pnode(0), sa[at])) at++;
    if (at == sa.size() || path.size() > sa.size() - at) return false;
    bool good = true;
    for (size_t x = 0; good && x < path.size(); x++) good = matches(pnode(x), sa[at + x]);
    return good;
}

// one bubble: the skipping reads are mapped onto the contigs they skip, their read alignments are collected again and
// those that walk the skipped path replace the pile-up of the skipping edge `sk`
int resolve_bubble(std::vector<Edge> &g, const std::vector<int32_t> &cyc, const std::vector<int32_t> &deg, Edge *sk, Resolver &rs)
{
    // the skipping reads and the contigs they skip
    std::vector<int32_t> inter, rids;
    for (int32_t v : cyc)
        if (deg[(size_t)v] == 2) inter.push_back(v / 4);
    for (const dh_read_alignment &ra : sk->ras) rids.push_back(ra.read);
    for (std::vector<int32_t> *ids : {&inter, &rids}) {  // ascending, distinct
        std::sort(ids->begin(), ids->end());
        ids->erase(std::unique(ids->begin(), ids->end()), ids->end());
    }
    std::vector<dh_la> fresh;
    if (int rc = rs.remap(inter, rids, fresh)) return rc;
    const int64_t first_new = rs.c.n + (int64_t)rs.extra->size();
    rs.extra->insert(rs.extra->end(), fresh.begin(), fresh.end());
    const std::vector<Node> path = skipped_path(cyc, *sk);
    if (path.size() <= 2) return dh_fail(DH_EINVAL, "resolveBubbles: skipped path is too short");
    // old and new alignments of every skipping read, in that order (pileups.d:1262-1266), enabled ones only
    std::vector<std::pair<int32_t, int64_t>> al;  // (read, LA)
    for (const dh_read_alignment &ra : sk->ras) {
        al.emplace_back(ra.read, (int64_t)ra.la0);
        if (ra.n == 2) al.emplace_back(ra.read, (int64_t)ra.la1);
    }
    for (size_t x = 0; x < fresh.size(); x++)
        if (!(fresh[x].flags & DH_FLAG_DISABLED)) al.emplace_back(fresh[x].bread, first_new + (int64_t)x);
    std::stable_sort(al.begin(), al.end(), [](const auto &p, const auto &q) { return p.first < q.first; });
    std::vector<RawJoin> raw;
    std::vector<SA> sa;
    std::vector<std::pair<size_t, size_t>> sl;
    for (size_t i = 0; i < al.size();) {
        size_t j = i;
        std::vector<int64_t> idx;
        while (j < al.size() && al[j].first == al[i].first) idx.push_back(al[j++].second);
        const size_t r0 = raw.size();
        read_joins(rs.c, idx.data(), (int64_t)idx.size(), raw, sa, sl);
        if (raw.size() > r0 && !walks_path(rs.c, sa, path)) raw.resize(r0);
        i = j;
    }
    sk->drop_pile_up();
    // the new joins as edges, merged into the graph by the stable multi-edge merge (bulkAdd!mergeJoins): an edge that
    // exists keeps its read alignments first, the new ones follow in raw order
    std::vector<const RawJoin *> item(raw.size());
    for (size_t x = 0; x < raw.size(); x++) item[x] = &raw[x];
    edges_of_equal_keys(item.data(), item.data() + item.size(), g);
    merge_multi_edges(g);
    rs.resolved++;
    return DH_OK;
}
}  // namespace

int resolve_bubbles(std::vector<Edge> &g, int32_t ncontigs, Resolver &rs)
{
    for (int32_t iter = 0; iter < rs.max_iterations; iter++) {
        std::vector<int32_t> deg;
        const auto bubbles = find_bubbles(g, incidence(g, ncontigs), rs.max_bubble_size, deg);
        if (bubbles.empty()) break;
        for (const auto &cyc : bubbles)
            if (Edge *sk = skipping_edge(g, cyc, deg))  // (nullptr: resolved through another bubble of this iteration)
                if (int rc = resolve_bubble(g, cyc, deg, sk, rs)) return rc;
        remove_none_joins(g);
    }
    return DH_OK;
}
}  // namespace dh_scaffold_detail
