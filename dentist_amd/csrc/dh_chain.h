// dh_chain.h -- chaining of local alignments (dh_la_chain; chainLocalAlignments, common/alignments/chaining.d:122-334):
// the layouts, the lane code shared by the kernels of dh_chain.hip and the CPU harness of tests/native/chain_host.cpp, and the
// host-side plan (grouping of the records into pairs, the order check, the tiers).  Driver: dh_chain.cpp.
//
// One wavefront chains one pair.  The nodes of a pair are its enabled records in the order (abpos, bbpos, input index), a
// topological order of areChainable.  Three representations of the same computation:
//   * registers (2..64 nodes): lane v owns node v; the kernel broadcasts node u and lane v > u relaxes its own node with
//     relax_edge().  Only the per-edge functions of this header are shared with that kernel.
//   * arrays in LDS or in a slab of global memory (more nodes): the arr_* phases below, each written for one lane of 64 and
//     separated by barriers in the kernel (the harness plays the 64 lanes of a phase one after the other).
//   * the emission (every tier): emit_keys / emit_write read the per-node State a tier left in global memory.
// What a tier leaves per node (at its position in the node order) is a State; per pair it leaves the number of output records
// and of chains.  After an exclusive scan of those the emission writes src_index, flags, off and score in contract order.
#ifndef DH_CHAIN_H
#define DH_CHAIN_H

#include <stdint.h>

#if defined(__HIPCC__)
#define CH_HD __host__ __device__ __forceinline__
#else
#define CH_HD inline
#endif

#define CH_WAVE_NODES 64    // the register tier's limit: one node per lane
#define CH_LDS_NODES 1536   // the LDS tier's limit: CH_ARRAYS int32 arrays of that many nodes are 61 440 bytes of static LDS
#define CH_ARRAYS 10
#define CH_FLAG_COMP 0x1u
#define CH_FLAG_START 0x4u
#define CH_FLAG_NEXT 0x8u
#define CH_FLAG_BEST 0x10u
#define CH_FLAG_DISABLED 0x20u
// bits of State.depth above the depth itself
#define CH_TAKEN 0x80000000u  // the node lies on a taken chain (selection)
#define CH_END 0x40000000u    // the node ends a chain: selected (within a tier), accepted (in the State a tier leaves)
#define CH_ALT 0x20000000u    // ... an alternate chain
#define CH_DEPTH 0x1FFFFFFFu
#define CH_IDX 0x7FFFFFFF     // State.idx: the node's index among the pair's enabled records; bit 31: the COMP flag

namespace chn {

struct Node {  // what is uploaded per enabled record (20 bytes)
    int32_t abpos, aepos, bbpos, bepos;
    uint32_t flags;  // the input's flags without START, NEXT and BEST
};
struct Opts {  // = dh_chain_opts
    int32_t max_indel, max_gap, min_score, pad_;
    double max_rel_overlap, min_rel_score;
};
struct State {  // per node, at its position in the node order
    int32_t idx, pred;
    uint32_t depth;  // nodes on the path that ends here | CH_END | CH_ALT
    int32_t dist;
};
struct Key {  // sort key of the chain that ends at a node: first.abpos, first.bbpos, last.aepos, last.bepos
    int32_t ab, bb, ae, be;
};

CH_HD int32_t iabs(int32_t x) { return x < 0 ? -x : x; }
CH_HD int32_t imax(int32_t x, int32_t y) { return x > y ? x : y; }
CH_HD int32_t imin(int32_t x, int32_t y) { return x < y ? x : y; }
// alignmentScore (chaining.d:455-461)
CH_HD int32_t score(int32_t ab, int32_t ae, int32_t bb, int32_t be) { return ((ae - ab) + (be - bb)) / 2; }
// the node order
CH_HD bool precedes(int32_t xab, int32_t xbb, int32_t xi, int32_t yab, int32_t ybb, int32_t yi)
{
    return xab != yab ? xab < yab : (xbb != ybb ? xbb < ybb : xi < yi);
}
// areChainable (:434-451): x before y
CH_HD bool chainable(int32_t xab, int32_t xae, int32_t xbb, int32_t xbe, uint32_t xcomp, int32_t yab, int32_t yae, int32_t ybb,
                     int32_t ybe, uint32_t ycomp, const Opts &o)
{
    if (xcomp != ycomp) return false;
    const int32_t ga = yab - xae, gb = ybb - xbe;
    if (!(xab < yab && xbb < ybb)) return false;
    if (iabs(ga - gb) > o.max_indel || imax(iabs(ga), iabs(gb)) > o.max_gap) return false;
    const int32_t mla = imin(xae - xab, yae - yab), mlb = imin(xbe - xbb, ybe - ybb);
    const double la = o.max_rel_overlap * (double)mla, lb = o.max_rel_overlap * (double)mlb;
    return (double)imax(0, -ga) <= la && (double)imax(0, -gb) <= lb;
}
// chainScore (:467-475): the weight of the edge x -> y
CH_HD int32_t chain_score(int32_t xae, int32_t xbe, int32_t yab, int32_t yae, int32_t ybb, int32_t ybe)
{
    const int32_t ga = yab - xae, gb = ybb - xbe;
    return iabs(ga - gb) + imax(iabs(ga), iabs(gb)) / 10 - score(yab, yae, ybb, ybe);
}
// (int32_t) max((double) min_score, min_relative_score * best)
CH_HD int32_t threshold(int32_t min_score, double min_rel, int32_t best)
{
    const double a = (double)min_score, b = min_rel * (double)best;
    return (int32_t)(a < b ? b : a);
}
// the whole of a pair with one enabled record
CH_HD State single_state(const Node &x, const Opts &o)
{
    const int32_t sc = score(x.abpos, x.aepos, x.bbpos, x.bepos);
    const bool acc = sc >= threshold(o.min_score, o.min_rel_score, sc);
    return State{(int32_t)((x.flags & CH_FLAG_COMP) << 31), -1, 1u | (acc ? CH_END : 0u), -sc};
}
// node u (final) against node v > u of the node order: true when the edge exists; relaxes v
CH_HD bool relax_edge(int32_t uab, int32_t uae, int32_t ubb, int32_t ube, uint32_t ucomp, int32_t udist, uint32_t udepth, int32_t u,
                      int32_t vab, int32_t vae, int32_t vbb, int32_t vbe, uint32_t vcomp, const Opts &o, int32_t &dist, int32_t &pred,
                      uint32_t &depth)
{
    if (!chainable(uab, uae, ubb, ube, ucomp, vab, vae, vbb, vbe, vcomp, o)) return false;
    const int32_t d = udist + chain_score(uae, ube, vab, vae, vbb, vbe);
    if (dist > d) {
        dist = d;
        pred = u;
        depth = (udepth & CH_DEPTH) + 1u;
    }
    return true;
}

// ------------------------------------------------------------------------------------ nodes in arrays (LDS, global memory)
struct Arrays {
    int32_t *ab, *ae, *bb, *be, *idx, *dist, *pred;
    uint32_t *depth;
    int32_t *uf;   // union-find parents during the relaxation, then the nodes in selection order
    int32_t *aux;  // the component label of every node
};
CH_HD Arrays carve(int32_t *base, int64_t n)
{
    Arrays a;
    a.ab = base, a.ae = base + n, a.bb = base + 2 * n, a.be = base + 3 * n, a.idx = base + 4 * n, a.dist = base + 5 * n;
    a.pred = base + 6 * n, a.depth = (uint32_t *)(base + 7 * n), a.uf = base + 8 * n, a.aux = base + 9 * n;
    return a;
}

// Mem: how the parents of the union-find are read and lowered (the kernels: atomics; the harness: plain, its lanes run one
// after the other)
struct PlainMem {
    static inline int32_t load(const int32_t *p) { return *p; }
    static inline int32_t atomic_min(int32_t *p, int32_t v)
    {
        const int32_t old = *p;
        if (v < old) *p = v;
        return old;
    }
};

template <class Mem>
CH_HD int32_t uf_find(int32_t *parent, int32_t x)
{
    for (;;) {
        const int32_t p = Mem::load(parent + x);
        if (p == x) return x;
        x = p;  // parents only ever decrease
    }
}
// the larger root goes under the smaller one; a hook that lost a race is retried from what the atomic returned
template <class Mem>
CH_HD void uf_unite(int32_t *parent, int32_t a, int32_t b)
{
    for (;;) {
        a = uf_find<Mem>(parent, a);
        b = uf_find<Mem>(parent, b);
        if (a == b) return;
        if (a > b) {
            const int32_t t = a;
            a = b;
            b = t;
        }
        const int32_t old = Mem::atomic_min(parent + b, a);
        if (old == b) return;  // b was a root and hangs under a now
        b = old;               // parent[b] is min(old, a): what it pointed to still has to meet a
    }
}

// phase 1: the rank sort into the node order, and the start values
CH_HD void arr_load(const Node *nodes, int32_t n, const Arrays &a, int32_t lane)
{
    for (int32_t v = lane; v < n; v += 64) {
        const Node x = nodes[v];
        int32_t r = 0;
        for (int32_t w = 0; w < n; w++) r += precedes(nodes[w].abpos, nodes[w].bbpos, w, x.abpos, x.bbpos, v) ? 1 : 0;
        a.ab[r] = x.abpos, a.ae[r] = x.aepos, a.bb[r] = x.bbpos, a.be[r] = x.bepos;
        a.idx[r] = (int32_t)((uint32_t)v | ((x.flags & CH_FLAG_COMP) << 31));
        a.dist[r] = -score(x.abpos, x.aepos, x.bbpos, x.bepos);
        a.pred[r] = -1;
        a.depth[r] = 1u;
        a.uf[r] = r;
    }
}
// phase 2, once per u ascending, a barrier behind every step: the lanes stride over v in (u, hi(u)), hi(u) the first v with
// abpos[v] - aepos[u] > max_chain_gap (abpos ascends: nothing behind it is chainable)
template <class Mem>
CH_HD void arr_relax(const Arrays &a, int32_t n, int32_t u, const Opts &o, int32_t lane)
{
    const int32_t uab = a.ab[u], uae = a.ae[u], ubb = a.bb[u], ube = a.be[u], ud = a.dist[u];
    const uint32_t ucomp = (uint32_t)a.idx[u] >> 31, udepth = a.depth[u];
    for (int32_t v = u + 1 + lane; v < n; v += 64) {
        const int32_t vab = a.ab[v];
        if (vab - uae > o.max_gap) break;
        int32_t dist = a.dist[v], pred = a.pred[v];
        uint32_t depth = a.depth[v];
        const int32_t before = dist;
        if (!relax_edge(uab, uae, ubb, ube, ucomp, ud, udepth, u, vab, a.ae[v], a.bb[v], a.be[v], (uint32_t)a.idx[v] >> 31, o, dist, pred,
                        depth))
            continue;
        if (dist != before) a.dist[v] = dist, a.pred[v] = pred, a.depth[v] = depth;
        uf_unite<Mem>(a.uf, u, v);
    }
}
// phase 3: the label of a component is its smallest node position
template <class Mem>
CH_HD void arr_label(const Arrays &a, int32_t n, int32_t lane)
{
    for (int32_t v = lane; v < n; v += 64) a.aux[v] = uf_find<Mem>(a.uf, v);
}
// phase 4: the rank sort by (component, dist, position) into a.uf
CH_HD void arr_rank(const Arrays &a, int32_t n, int32_t lane)
{
    for (int32_t v = lane; v < n; v += 64) {
        const int32_t lv = a.aux[v], dv = a.dist[v];
        int32_t r = 0;
        for (int32_t w = 0; w < n; w++) {
            const int32_t lw = a.aux[w], dw = a.dist[w];
            r += (lw != lv ? lw < lv : (dw != dv ? dw < dv : w < v)) ? 1 : 0;
        }
        a.uf[r] = v;
    }
}
// phase 5: one lane per component takes its end nodes best first.  A walk stops at the first taken node: every ancestor of
// a taken node is taken.  Components share no nodes.
CH_HD void arr_select(const Arrays &a, int32_t n, const Opts &o, int32_t lane)
{
    for (int32_t r = lane; r < n; r += 64) {
        const int32_t e0 = a.uf[r], c = a.aux[e0];
        if (r > 0 && a.aux[a.uf[r - 1]] == c) continue;  // not the first of its component
        const int32_t cthr = threshold(o.min_score, o.min_rel_score, -a.dist[e0]);
        for (int32_t k = r; k < n; k++) {
            const int32_t e = a.uf[k];
            if (a.aux[e] != c) break;
            if (a.depth[e] & CH_TAKEN) continue;
            if (-a.dist[e] < cthr) break;  // (ascending dist: the rest scores less)
            bool alt = false;
            for (int32_t v = e; v >= 0; v = a.pred[v]) {
                if (a.depth[v] & CH_TAKEN) {
                    alt = true;
                    break;
                }
                a.depth[v] |= CH_TAKEN;
            }
            a.depth[e] |= CH_END | (alt ? CH_ALT : 0u);
        }
    }
}
// phase 6a: a lane's share of the pair's best score (the kernel reduces the 64 values)
CH_HD int32_t arr_best(const Arrays &a, int32_t n, int32_t lane)
{
    int32_t best = INT32_MIN;
    for (int32_t v = lane; v < n; v += 64) best = imax(best, -a.dist[v]);
    return best;
}
// phase 6b: the State of every node; a lane's share of the pair's output records and chains
CH_HD void arr_finish(const Arrays &a, int32_t n, int32_t thr, State *state, int32_t lane, uint64_t &nrec, uint32_t &nch)
{
    for (int32_t v = lane; v < n; v += 64) {
        const uint32_t d = a.depth[v];
        const bool acc = (d & CH_END) && -a.dist[v] >= thr;
        state[v] = State{a.idx[v], a.pred[v], (d & CH_DEPTH) | (acc ? CH_END | (d & CH_ALT) : 0u), a.dist[v]};
        if (acc) nrec += d & CH_DEPTH, nch++;
    }
}
// what a tier stores as a pair's number of output records (the scan is 32 bits wide; its 64-bit total finds the overflow)
CH_HD uint32_t clamp_records(uint64_t nrec) { return nrec > 0x80000000ull ? 0x80000000u : (uint32_t)nrec; }

// ------------------------------------------------------------------------------------ emission (every tier)
// phase 1: the sort key of every accepted chain
CH_HD void emit_keys(const Node *nodes, const State *state, int32_t n, Key *key, int32_t lane)
{
    for (int32_t v = lane; v < n; v += 64) {
        if (!(state[v].depth & CH_END)) continue;
        int32_t r = v;
        while (state[r].pred >= 0) r = state[r].pred;
        const Node &f = nodes[state[r].idx & CH_IDX], &l = nodes[state[v].idx & CH_IDX];
        key[v] = Key{f.abpos, f.bbpos, l.aepos, l.bepos};
    }
}
CH_HD bool key_less(const Key &x, int32_t xi, const Key &y, int32_t yi)
{
    if (x.ab != y.ab) return x.ab < y.ab;
    if (x.bb != y.bb) return x.bb < y.bb;
    if (x.ae != y.ae) return x.ae < y.ae;
    if (x.be != y.be) return x.be < y.be;
    return xi < yi;
}
// phase 2: a chain's place among the pair's chains, then its records back to front.  node0: the number of the pair's first
// node among all nodes (src_index receives node numbers; the driver turns them into record indices)
CH_HD void emit_write(const Node *nodes, const State *state, int32_t n, const Key *key, int64_t node0, int64_t rec0, int64_t chain0,
                      int64_t *off, int32_t *sc, int64_t *src, uint32_t *flags, int32_t lane)
{
    for (int32_t v = lane; v < n; v += 64) {
        const State sv = state[v];
        if (!(sv.depth & CH_END)) continue;
        const Key kv = key[v];
        int64_t rank = 0, at = 0;
        for (int32_t w = 0; w < n; w++) {
            const uint32_t dw = state[w].depth;
            if (!(dw & CH_END) || w == v) continue;
            if (key_less(key[w], w, kv, v)) rank++, at += dw & CH_DEPTH;
        }
        off[chain0 + rank] = rec0 + at;
        sc[chain0 + rank] = -sv.dist;
        const int32_t depth = (int32_t)(sv.depth & CH_DEPTH);
        int32_t x = v;
        for (int32_t k = depth - 1; k >= 0; k--) {
            const State sx = state[x];
            const int32_t i = sx.idx & CH_IDX;
            src[rec0 + at + k] = node0 + i;
            flags[rec0 + at + k] = nodes[i].flags | (k ? CH_FLAG_NEXT : CH_FLAG_START | ((sv.depth & CH_ALT) ? 0u : CH_FLAG_BEST));
            x = sx.pred;
        }
    }
}

}  // namespace chn

// ------------------------------------------------------------------------------------ the plan (host)
#include <algorithm>
#include <functional>
#include <vector>

#include "../../include/dentist_hip.h"

namespace chn {

enum { TIER_SINGLE = 0, TIER_WAVE = 1, TIER_LDS = 2, TIER_GLOBAL = 3, TIER_COUNT = 4 };

struct Plan {
    std::vector<Node> nodes;        // the enabled records in input order
    std::vector<int64_t> node_src;  // their indices in las
    std::vector<int64_t> pair_off;  // pairs + 1: pair p = nodes [pair_off[p], pair_off[p + 1])
    std::vector<int32_t> list;      // the pairs tier by tier: [tier_at[t], tier_at[t + 1])
    int64_t tier_at[TIER_COUNT + 1] = {0, 0, 0, 0, 0};
    int64_t bad = -1;               // first enabled record that precedes the enabled record before it in (aread, bread)
    bool too_many = false;          // more than 2^31 - 1 enabled records
};

CH_HD int tier_of(int64_t n, int64_t lds_cap) { return n <= 1 ? TIER_SINGLE : (n <= CH_WAVE_NODES ? TIER_WAVE : (n <= lds_cap ? TIER_LDS : TIER_GLOBAL)); }

// par(n, fn): fn(lo, hi) over disjoint parts of [0, n), possibly on several threads
typedef std::function<void(int64_t, const std::function<void(int64_t, int64_t)> &)> Par;

inline void build_plan(const dh_la *las, int64_t n, int64_t lds_cap, const Par &par, Plan &pl)
{
    const int64_t grain = 1 << 15, nchunks = (n + grain - 1) / grain;
    struct Chunk {
        int64_t count = 0, bad = -1, first = -1, pairs = 0, node0 = 0, pair0 = 0;
        int64_t first_key = 0, last_key = 0, prev_key = -1;
    };
    std::vector<Chunk> ch((size_t)nchunks);
    auto key_of = [&](int64_t i) { return (int64_t)(((uint64_t)(uint32_t)las[i].aread << 32) | (uint32_t)las[i].bread); };
    auto enabled = [&](int64_t i) { return !(las[i].flags & CH_FLAG_DISABLED); };
    // the enabled records of every chunk, their order inside it
    par(nchunks, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; c++) {
            Chunk &k = ch[(size_t)c];
            const int64_t i1 = std::min(n, (c + 1) * grain);
            for (int64_t i = c * grain; i < i1; i++) {
                if (!enabled(i)) continue;
                const int64_t key = key_of(i);
                if (k.count == 0)
                    k.first = i, k.first_key = key;
                else if (key < k.last_key && k.bad < 0)
                    k.bad = i;
                k.last_key = key;
                k.count++;
            }
        }
    });
    int64_t total = 0, prev = -1;
    for (Chunk &k : ch) {
        k.node0 = total;
        k.prev_key = prev;
        if (k.count) {
            if (k.first_key < prev && (pl.bad < 0 || k.first < pl.bad)) pl.bad = k.first;
            prev = k.last_key;
        }
        if (k.bad >= 0 && (pl.bad < 0 || k.bad < pl.bad)) pl.bad = k.bad;
        total += k.count;
    }
    if (pl.bad >= 0) return;
    if (total > INT32_MAX) {
        pl.too_many = true;
        return;
    }
    pl.nodes.resize((size_t)total);
    pl.node_src.resize((size_t)total);
    std::vector<uint8_t> start((size_t)total);
    par(nchunks, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; c++) {
            Chunk &k = ch[(size_t)c];
            const int64_t i1 = std::min(n, (c + 1) * grain);
            int64_t at = k.node0, last = k.prev_key;
            for (int64_t i = c * grain; i < i1; i++) {
                if (!enabled(i)) continue;
                const dh_la &l = las[i];
                pl.nodes[(size_t)at] = Node{l.abpos, l.aepos, l.bbpos, l.bepos, l.flags & ~(CH_FLAG_START | CH_FLAG_NEXT | CH_FLAG_BEST)};
                pl.node_src[(size_t)at] = i;
                const int64_t key = key_of(i);
                start[(size_t)at] = key != last;
                k.pairs += key != last;
                last = key;
                at++;
            }
        }
    });
    int64_t npairs = 0;
    for (Chunk &k : ch) {
        k.pair0 = npairs;
        npairs += k.pairs;
    }
    pl.pair_off.resize((size_t)npairs + 1);
    par(nchunks, [&](int64_t c0, int64_t c1) {
        for (int64_t c = c0; c < c1; c++) {
            const Chunk &k = ch[(size_t)c];
            int64_t p = k.pair0;
            for (int64_t at = k.node0; at < k.node0 + k.count; at++)
                if (start[(size_t)at]) pl.pair_off[(size_t)p++] = at;
        }
    });
    pl.pair_off[(size_t)npairs] = total;
    int64_t cnt[TIER_COUNT] = {0, 0, 0, 0};
    for (int64_t p = 0; p < npairs; p++) cnt[tier_of(pl.pair_off[(size_t)p + 1] - pl.pair_off[(size_t)p], lds_cap)]++;
    for (int t = 0; t < TIER_COUNT; t++) pl.tier_at[t + 1] = pl.tier_at[t] + cnt[t];
    pl.list.resize((size_t)npairs);
    int64_t cur[TIER_COUNT];
    for (int t = 0; t < TIER_COUNT; t++) cur[t] = pl.tier_at[t];
    for (int64_t p = 0; p < npairs; p++)
        pl.list[(size_t)cur[tier_of(pl.pair_off[(size_t)p + 1] - pl.pair_off[(size_t)p], lds_cap)]++] = (int32_t)p;
}

// the pairs of the global tier in launch groups whose slabs stay under `limit` int32 words (one pair always fits):
// group g = pairs [gat[g], gat[g + 1]) of the tier's list; woff[i]: where pair i's arrays begin in its group's slab
inline void plan_groups(const Plan &pl, int64_t limit_words, std::vector<int64_t> &gat, std::vector<int64_t> &woff, int64_t &max_words)
{
    const int64_t b0 = pl.tier_at[TIER_GLOBAL], b1 = pl.tier_at[TIER_GLOBAL + 1];
    gat.assign(1, 0);
    woff.assign((size_t)(b1 - b0), 0);
    max_words = 0;
    int64_t used = 0;
    for (int64_t i = b0; i < b1; i++) {
        const int32_t p = pl.list[(size_t)i];
        const int64_t w = CH_ARRAYS * (pl.pair_off[(size_t)p + 1] - pl.pair_off[(size_t)p]);
        if (used > 0 && used + w > limit_words) {
            gat.push_back(i - b0);
            used = 0;
        }
        woff[(size_t)(i - b0)] = used;
        used += w;
        max_words = std::max(max_words, used);
    }
    gat.push_back(b1 - b0);
}

}  // namespace chn

#endif
