// dh_scaffold.h -- internals shared by the sources of the scaffold-graph pile-up builder of `dentist collect`
// (dh_scaffold*.cpp: joins per read, graph pipeline, bubbles, join blobs, views, entry points)
#ifndef DH_SCAFFOLD_H
#define DH_SCAFFOLD_H

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <functional>

#include "dh_internal.h"

struct dh_scaffold {
    std::vector<dh_join> joins;
    std::vector<dh_read_alignment> entries;
};

// the laps DH_TRACE=1 prints to stderr: "<prefix> <what, left-aligned in `width`> <ms since the last lap> ms"
struct dh_lap_timer {
    const char *prefix;
    int width;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    void operator()(const char *what)
    {
        if (!getenv("DH_TRACE")) return;
        const auto t = std::chrono::steady_clock::now();
        fprintf(stderr, "%s %-*s %.2f ms\n", prefix, width, what, std::chrono::duration<double, std::milli>(t - t0).count());
        t0 = t;
    }
};

// dh_scaffold_blob.cpp: the gathered join blobs -> the scaffold every rank derives; glas = the LA records of the joins
// (the chains of both flanks of every join), which the entries of the scaffold index
int dh_scaffold_from_join_blobs(const uint8_t *const *blobs, const int64_t *sizes, int32_t world, int32_t ncontigs, const int32_t *input_gaps,
                                int32_t ngaps, const struct dh_scaffold_opts *opts, dh_la_vec &glas, dh_scaffold **out);

namespace dh_scaffold_detail {
enum { FRONT = 0, BACK = 1 };
enum { PRE = 0, BEGIN = 1, END = 2, POST = 3 };
enum { T_PILEUP = 1, T_INPUTGAP = 2 };

struct Node {
    int32_t contig, part;
    bool operator<(const Node &o) const { return contig != o.contig ? contig < o.contig : part < o.part; }
    bool operator==(const Node &o) const { return contig == o.contig && part == o.part; }
};
inline bool real_part(int32_t p) { return p == BEGIN || p == END; }

struct Edge {
    Node s, e;
    uint32_t types = 0;
    std::vector<dh_read_alignment> ras;
    bool is_default() const { return s.part == BEGIN && e.part == END && s.contig == e.contig; }
    bool is_gap() const { return s.contig != e.contig && real_part(s.part) && real_part(e.part); }
    bool is_ext() const { return s.contig == e.contig && ((s.part == PRE && e.part == BEGIN) || (s.part == END && e.part == POST)); }
    bool empty_payload() const { return types == 0 && ras.empty(); }
    void drop_pile_up() { types &= ~(uint32_t)T_PILEUP; ras.clear(); }
};
inline bool key_less(const Edge &a, const Edge &b) { return a.s == b.s ? a.e < b.e : a.s < b.s; }
inline bool key_eq(const Edge &a, const Edge &b) { return a.s == b.s && a.e == b.e; }
inline Edge make_edge(Node a, Node b)
{
    Edge x;
    x.s = b < a ? b : a;  // undirected: start <= end (math.d:385-398)
    x.e = b < a ? a : b;
    return x;
}

struct SA {
    int64_t la;
    int32_t seed, b, e, srel;
};

struct Ctx {
    const dh_la *las;
    const int64_t *coff, *roff;
    // the bubble resolver adds alignments: LA i >= n is (*extra)[i - n]
    int64_t n = INT64_MAX;
    const std::vector<dh_la> *extra = nullptr;
    const dh_la &L(int64_t i) const { return i < n ? las[i] : (*extra)[(size_t)(i - n)]; }
    int32_t alen(const dh_la &l) const { return (int32_t)(coff[l.aread + 1] - coff[l.aread]); }
    int32_t blen(const dh_la &l) const { return (int32_t)(roff[l.bread + 1] - roff[l.bread]); }
};

// one read alignment with the edge it contributes to: plain data, so that a run of reads yields one flat array
// (no allocation per join); runs are turned into edges by edges_from_runs
struct RawJoin {
    Node s, e;
    dh_read_alignment ra;
};

// edges incident to every node: inc[4 * contig + part] = edge indices in edge order (two flat arrays: a vector per node
// was 4 000 small allocations per call, half a millisecond of the plan every rank of a sharded run derives)
struct Incidence {
    std::vector<int32_t> off, idx;
    struct Span {
        const int32_t *b, *e;
        const int32_t *begin() const { return b; }
        const int32_t *end() const { return e; }
        size_t size() const { return (size_t)(e - b); }
        bool empty() const { return b == e; }
    };
    Span operator[](size_t node) const { return Span{idx.data() + off[node], idx.data() + off[node + 1]}; }
    size_t size() const { return off.size() - 1; }  // nodes
};

// resolveBubbles (dh_scaffold_bubbles.cpp) with the re-mapping of the skipping reads as a callback
struct Resolver {
    Ctx c;                       // LA access incl. the alignments added so far
    std::vector<dh_la> *extra;   // the added alignments (LA index n + i)
    // contig ids, read ids (ascending, distinct) -> alignments with ids of the full DBs, DISABLED unless they cover their contig
    std::function<int(const std::vector<int32_t> &, const std::vector<int32_t> &, std::vector<dh_la> &)> remap;
    int32_t max_bubble_size = 8, max_iterations = 4;  // commandline.d:1826-1837
    int32_t resolved = 0;
};

// ---- dh_scaffold_joins.cpp
void read_joins(const Ctx &c, const int64_t *idx, int64_t cnt, std::vector<RawJoin> &out, std::vector<SA> &sa, std::vector<std::pair<size_t, size_t>> &sl);
int collect_raw_joins(const char *who, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                      const int64_t *read_off, int32_t read_first, int32_t nreads, std::vector<std::vector<RawJoin>> *raws);
// ---- dh_scaffold_graph.cpp
int check_input_gaps(const char *who, const int32_t *input_gaps, int32_t ngaps, int32_t ncontigs);
void edges_of_equal_keys(const RawJoin **i0, const RawJoin **i1, std::vector<Edge> &out);
void merge_multi_edges(std::vector<Edge> &g);
void remove_none_joins(std::vector<Edge> &g);
Incidence incidence(const std::vector<Edge> &g, int32_t ncontigs);
int scaffold_from_runs(std::vector<std::vector<RawJoin>> &runs, int32_t ncontigs, const int32_t *input_gaps, int32_t ngaps,
                       const dh_scaffold_opts *opts, dh_scaffold **out, Resolver *rs = nullptr);
// ---- dh_scaffold_bubbles.cpp
int resolve_bubbles(std::vector<Edge> &g, int32_t ncontigs, Resolver &rs);
}  // namespace dh_scaffold_detail

#endif
