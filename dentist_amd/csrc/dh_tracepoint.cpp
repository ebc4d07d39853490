// dh_tracepoint.cpp -- arithmetic on records and their trace points, host only: the regions and the common trace point of
// the cropper (cropper.d:446-550), Trace.translateTracePoint, isValidPileUpAlignment, chainLocalAlignments for one pair
// (chain_pair), the two C entry points dh_common_trace_point / dh_translate_trace_point, and the host dh_propagate_mask,
// which is translate_trace_point over a mask.
#include <atomic>

#include "dh_process.h"
#include "dh_parallel.h"

namespace dhp {

// ------------------------------------------------------------------------------------ trace maths

static int32_t ceil_to(int32_t x, int32_t m) { return (x + m - 1) / m * m; }

static int64_t chain_end(const dh_la *las, int64_t n, int64_t i)
{
    int64_t j = i + 1;
    while (j < n && dh_continues_chain(las[j - 1], las[j])) j++;
    return j;
}
void intersect_chain(Region &reg, const dh_la *las, int64_t n, int64_t i)
{
    const int64_t j = chain_end(las, n, i);
    Region mine;
    for (int64_t x = i; x < j; x++) mine.emplace_back(las[x].abpos, las[x].aepos);
    if (j - i > 1) {
        std::sort(mine.begin(), mine.end());
        Region m2;
        for (const auto &iv : mine)
            if (!m2.empty() && iv.first <= m2.back().second)
                m2.back().second = std::max(m2.back().second, iv.second);
            else
                m2.push_back(iv);
        mine.swap(m2);
    }
    Region out;
    for (const auto &a : reg)
        for (const auto &b : mine) {
            const int32_t lo = std::max(a.first, b.first), hi = std::min(a.second, b.second);
            if (lo < hi) out.emplace_back(lo, hi);
        }
    reg.swap(out);
}
// the first member of the chain at record i that covers apos (AlignmentChain.translateTracePoint, base.d:866-880)
int64_t covering_member(const dh_la *las, int64_t n, int64_t i, int32_t apos)
{
    const int64_t j = chain_end(las, n, i);
    for (int64_t x = i; x < j; x++)
        if (las[x].abpos <= apos && apos <= las[x].aepos) return x;
    return -1;
}

// getCommonTracePoint, cropper.d:446-500: candidates are the trace points of the region (plus the contig end),
// innermost first for `front` seeds; the common A region minus the repeat mask is tried first, then the region itself.
static int32_t common_trace_point_in(const Region &reg, int32_t contig_len, int32_t ts, bool seed_front)
{
    if (reg.empty()) return -1;
    const int32_t lo = reg.front().first, hi = reg.back().second;
    const int32_t tp_min = ceil_to(lo, ts), tp_sup = ceil_to(hi, ts);
    std::vector<int32_t> cands;
    for (int32_t c = tp_min; c < tp_sup; c += ts) cands.push_back(c);
    if (tp_sup > contig_len) cands.push_back(contig_len);
    if (seed_front) std::reverse(cands.begin(), cands.end());
    for (int32_t c : cands) {
        bool in = c == hi;
        for (size_t x = 0; x < reg.size() && !in; x++) in = reg[x].first <= c && c < reg[x].second;
        if (in) return c;
    }
    return -1;
}
// mask: sorted disjoint (begin, end) pairs of this contig, nmask of them (may be 0 / NULL)
int32_t common_trace_point(const Region &reg, int32_t contig_len, int32_t ts, bool seed_front, const int32_t *mask, int64_t nmask)
{
    if (nmask > 0 && !reg.empty()) {
        Region un;  // reg - mask
        for (const auto &iv : reg) {
            int32_t b = iv.first;
            for (int64_t m = 0; m < nmask && b < iv.second; m++) {
                const int32_t mb = mask[2 * m], me = mask[2 * m + 1];
                if (me <= b) continue;
                if (mb >= iv.second) break;
                if (mb > b) un.emplace_back(b, mb);
                b = std::max(b, me);
            }
            if (b < iv.second) un.emplace_back(b, iv.second);
        }
        const int32_t c = common_trace_point_in(un, contig_len, ts, seed_front);
        if (c >= 0) return c;
    }
    return common_trace_point_in(reg, contig_len, ts, seed_front);
}

static int32_t trace_points_up_to_a(const dh_la &la, int32_t ts, int32_t apos, int32_t mode)
{
    const int32_t ntp = la.tlen / 2;
    const int32_t second = la.abpos / ts * ts + ts;
    if (mode == 0) {
        if (apos < second) return 0;
        if (apos < la.aepos) return 1 + (apos - second) / ts;
        return ntp;
    }
    const int32_t second_from_last = (la.aepos - 1) / ts * ts;
    if (apos == la.abpos) return 0;
    if (apos <= second) return 1;
    if (apos <= second_from_last) return 1 + (apos - second + ts - 1) / ts;
    return ntp;
}

// Trace.translateTracePoint!"contigA"(pos, mode), base.d:185-203: the position is assigned to a trace
// point of the LA; returns its coordinates on A and on B
void translate_trace_point(const dh_la &la, const uint16_t *tr, int32_t ts, int32_t apos, int32_t mode,
                                  int32_t *outa, int32_t *outb)
{
    const int32_t ntp = la.tlen / 2;
    const int32_t idx = trace_points_up_to_a(la, ts, apos, mode);
    int32_t b = la.bbpos;
    for (int32_t i = 0; i < idx; i++) b += tr[2 * i + 1];
    *outb = b;
    *outa = idx == 0 ? la.abpos : (idx < ntp ? la.abpos / ts * ts + idx * ts : la.aepos);
}

int32_t translate_floor_b(const dh_la &la, const uint16_t *tr, int32_t ts, int32_t apos)
{
    int32_t a, b;
    translate_trace_point(la, tr, ts, apos, 0, &a, &b);
    return b;
}


// isValidPileUpAlignment (flat), dazzler.d:4126-4141
bool valid_pileup_alignment(const dh_la &la, bool same, int32_t alen, int32_t blen, int32_t allow)
{
    const bool ab = la.abpos <= allow, bb = la.bbpos <= allow;
    const bool ae = la.aepos + allow >= alen, be = la.bepos + allow >= blen;
    return !same && (((ab && bb) && (ae || be)) || ((ae && be) && (ab || bb)));
}

// chainLocalAlignments / buildAlignmentChains (common/alignments/chaining.d:122-334) with the
// defaults of commandline.d:1819, 1982, 2014, 2165-2173 and minRelativeScore = min_rel (--min-relative-score, :2141-2153).
// `la` is grouped by (aread, bread) [first, last):
//  * the pair's enabled LAs are split into the connected components of the undirected chainability relation (:182);
//  * a shortest-path problem rates the chains (:227-233; relaxations over the LAs ordered by (abpos, bbpos, index), a
//    topological order -- no edge joins two components, so one pass serves all of them);
//  * per component the end nodes within effectiveMinScore of the component's best chain are taken best first (:236-266):
//    a node already on a taken chain is no end node, a chain that runs into nodes of a better chain is an ALTERNATE chain
//    and is composed of its whole path (:269-285) -- the LAs it shares are written once per chain: their further
//    occurrences go to `dups` (record index, flags) and are inserted behind the first one by the caller;
//  * the chains scoring >= max(minScore, minRelativeScore * best of the pair) are accepted (:305-312).
// First LA of a chain: START (+ BEST unless alternate, dazzler.d:2063-2068), the others NEXT; every other enabled LA of the
// pair gets DISABLED.  Ties: the lower position in the (abpos, bbpos, index) order first (oracle/pile.c:chain_pair).
void chain_pair(LaVec &la, size_t first, size_t last, int32_t min_score, double min_rel_score, std::vector<ChainDup> &dups)
{
    const int32_t max_indel = 1000, max_gap = 10000;
    const double max_rel_overlap = 0.3;
    const uint32_t cmask = DH_FLAG_START | DH_FLAG_NEXT | DH_FLAG_BEST;
    // fast path (the common case): a single enabled LA is its own best chain
    size_t nen = 0, only = first;
    for (size_t i = first; i < last; i++)
        if (!(la[i].flags & DH_FLAG_DISABLED)) {
            nen++;
            only = i;
        }
    if (nen == 0) return;
    if (nen == 1) {
        dh_la &l = la[only];
        const int32_t sc = ((l.aepos - l.abpos) + (l.bepos - l.bbpos)) / 2;
        if (sc < (int32_t)std::max<double>(min_score, min_rel_score * sc))
            l.flags |= DH_FLAG_DISABLED;
        else
            l.flags = (l.flags & ~cmask) | DH_FLAG_START | DH_FLAG_BEST;
        return;
    }
    std::vector<size_t> order;
    for (size_t i = first; i < last; i++)
        if (!(la[i].flags & DH_FLAG_DISABLED)) order.push_back(i);
    const size_t n = order.size();
    std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) {
        if (la[x].abpos != la[y].abpos) return la[x].abpos < la[y].abpos;
        if (la[x].bbpos != la[y].bbpos) return la[x].bbpos < la[y].bbpos;
        return x < y;
    });
    auto score = [&](const dh_la &x) { return ((x.aepos - x.abpos) + (x.bepos - x.bbpos)) / 2; };
    auto chainable = [&](const dh_la &x, const dh_la &y) {
        if ((x.flags & DH_FLAG_COMP) != (y.flags & DH_FLAG_COMP)) return false;
        const int32_t ga = y.abpos - x.aepos, gb = y.bbpos - x.bepos;
        if (!(x.abpos < y.abpos && x.bbpos < y.bbpos)) return false;
        if (std::abs(ga - gb) > max_indel || std::max(std::abs(ga), std::abs(gb)) > max_gap) return false;
        const int32_t mla = std::min(x.aepos - x.abpos, y.aepos - y.abpos);
        const int32_t mlb = std::min(x.bepos - x.bbpos, y.bepos - y.bbpos);
        return std::max(0, -ga) <= max_rel_overlap * mla && std::max(0, -gb) <= max_rel_overlap * mlb;
    };
    auto chain_score = [&](const dh_la &x, const dh_la &y) {
        const int32_t ga = y.abpos - x.aepos, gb = y.bbpos - x.bepos;
        return std::abs(ga - gb) + std::max(std::abs(ga), std::abs(gb)) / 10 - score(y);
    };
    std::vector<int32_t> dist(n), pred(n, -1), comp(n);
    for (size_t v = 0; v < n; v++) {
        dist[v] = -score(la[order[v]]);
        comp[v] = (int32_t)v;
    }
    for (size_t u = 0; u < n; u++)
        for (size_t v = u + 1; v < n; v++)
            if (chainable(la[order[u]], la[order[v]])) {
                const int32_t d = dist[u] + chain_score(la[order[u]], la[order[v]]);
                if (dist[v] > d) {
                    dist[v] = d;
                    pred[v] = (int32_t)u;
                }
                const int32_t cu = comp[u], cv = comp[v];
                if (cu != cv)
                    for (size_t w = 0; w < n; w++)
                        if (comp[w] == cv) comp[w] = cu;
            }
    // components in the order of their smallest record index (util/graphalgo.d:43-66)
    std::vector<size_t> cmin(n, SIZE_MAX), cord;
    for (size_t v = 0; v < n; v++) cmin[(size_t)comp[v]] = std::min(cmin[(size_t)comp[v]], order[v]);
    for (size_t v = 0; v < n; v++)
        if (cmin[v] != SIZE_MAX) cord.push_back(v);
    std::sort(cord.begin(), cord.end(), [&](size_t x, size_t y) { return cmin[x] < cmin[y]; });
    struct Sel {
        size_t end;
        bool alt;
        int32_t score;
    };
    std::vector<Sel> sel;
    std::vector<uint8_t> forbidden(n, 0);
    std::vector<size_t> ends;
    for (size_t c : cord) {
        ends.clear();
        for (size_t v = 0; v < n; v++)
            if ((size_t)comp[v] == c) ends.push_back(v);
        std::stable_sort(ends.begin(), ends.end(), [&](size_t x, size_t y) { return dist[x] < dist[y]; });
        const int32_t cbest = -dist[ends[0]];
        const int32_t cthr = (int32_t)std::max<double>(min_score, min_rel_score * cbest);
        for (size_t e : ends) {
            if (forbidden[e] || -dist[e] < cthr) continue;
            bool alt = false;
            for (int32_t v = (int32_t)e; v >= 0; v = pred[(size_t)v]) {
                alt = alt || forbidden[(size_t)v];
                forbidden[(size_t)v] = 1;
            }
            sel.push_back({e, alt, -dist[e]});
        }
    }
    int32_t best = 0;
    for (size_t x = 0; x < sel.size(); x++)
        if (x == 0 || sel[x].score > best) best = sel[x].score;
    const int32_t thr = (int32_t)std::max<double>(min_score, min_rel_score * best);
    std::vector<uint8_t> occ(n, 0);
    std::vector<size_t> path;
    for (const Sel &c : sel) {
        if (c.score < thr) continue;
        path.clear();
        for (int32_t v = (int32_t)c.end; v >= 0; v = pred[(size_t)v]) path.push_back((size_t)v);
        std::reverse(path.begin(), path.end());
        for (size_t k = 0; k < path.size(); k++) {
            const size_t v = path[k];
            dh_la &l = la[order[v]];
            const uint32_t f = k == 0 ? (DH_FLAG_START | (c.alt ? 0u : DH_FLAG_BEST)) : DH_FLAG_NEXT;
            if (!occ[v]) {
                occ[v] = 1;
                l.flags = (l.flags & ~cmask) | f;
            } else
                dups.push_back({order[v], (l.flags & ~cmask) | f});
        }
    }
    for (size_t v = 0; v < n; v++)
        if (!occ[v]) la[order[v]].flags |= DH_FLAG_DISABLED;
}

}  // namespace dhp

using namespace dhp;

// the cropper's common trace point as an entry of its own: first[] names the first record of each alignment chain of
// one flank (all on the same contig, all with the same seed)
extern "C" int dh_common_trace_point(const dh_la *las, int64_t n, const int32_t *first, int32_t count, int32_t contig_len,
                                     int32_t tspace, int32_t seed_front, const int32_t *mask_iv, int64_t nmask, int32_t *out)
{
    if (!out || count < 0 || (count > 0 && (!las || !first)) || tspace < 1 || nmask < 0 || (nmask > 0 && !mask_iv))
        return dh_fail(DH_EINVAL, "dh_common_trace_point: bad argument");
    Region reg{{0, INT32_MAX}};
    for (int32_t x = 0; x < count; x++) {
        if (first[x] < 0 || first[x] >= n) return dh_fail(DH_EINVAL, "dh_common_trace_point: record index out of range");
        intersect_chain(reg, las, n, first[x]);
    }
    *out = count > 0 ? common_trace_point(reg, contig_len, tspace, seed_front != 0, mask_iv, nmask) : -1;
    return DH_OK;
}

// the same through the C ABI (the cropper of `dentist process` is built on it: cropper.d:503-550)
extern "C" int dh_translate_trace_point(const dh_la *la, const uint16_t *trace, int32_t tspace, int32_t apos,
                                        int32_t mode, int32_t *out_a, int32_t *out_b)
{
    if (!la || !trace || !out_a || !out_b || tspace < 1 || (mode != 0 && mode != 1) || la->tlen < 0 || la->tlen % 2)
        return dh_fail(DH_EINVAL, "dh_translate_trace_point: bad argument");
    if (apos < la->abpos || apos > la->aepos)  // the reference asserts contigA.begin <= pos <= contigA.end
        return dh_fail(DH_EINVAL, "dh_translate_trace_point: position outside the local alignment");
    if (la->tlen / 2 != (la->aepos + tspace - 1) / tspace - la->abpos / tspace)
        return dh_fail(DH_EINVAL, "dh_translate_trace_point: trace length does not fit the A interval");
    translate_trace_point(*la, trace + la->toff, tspace, apos, mode, out_a, out_b);
    return DH_OK;
}

// ------------------------------------------------------------------------------------ propagate-mask
// `dentist propagate-mask` (commands/propagateMask.d:136-305): every interval of the contig mask is cut
// to the local alignments it intersects (:214-262) and carried over to the read through the trace
// points -- begin rounded down, end rounded up (:264-293, translateTracePoint base.d:185-203) -- and
// mirrored for complement alignments (:295-300); the union per read is the result (:307-313, Region
// normalisation util/region.d:776-816: sorted, intersecting or touching intervals merged, empty ones
// dropped).  Alignments are independent of each other, so they are spread over the host threads.
// out_ptr gets nreads + 1 entries; out_iv may be NULL to size; returns the number of intervals.
extern "C" int64_t dh_propagate_mask(const dh_la *las, int64_t n, const uint16_t *trace, int32_t tspace,
                                     const int64_t *mask_ptr, const int32_t *mask_iv, int32_t ncontigs,
                                     const int64_t *read_off, int32_t nreads, int64_t *out_ptr, int32_t *out_iv,
                                     int64_t cap)
{
    if ((n > 0 && (!las || !trace)) || n < 0 || !mask_ptr || !read_off || !out_ptr || tspace < 1 || ncontigs < 0 || nreads < 0)
        return dh_fail(DH_EINVAL, "dh_propagate_mask: bad argument");
    struct Iv {
        int32_t rd, b, e;
    };
    const int64_t grain = 4096, nchunks = (n + grain - 1) / grain;
    std::vector<std::vector<Iv>> found((size_t)std::max<int64_t>(nchunks, 1));
    std::atomic<int> bad{0};
    dh_parallel_for(nchunks, 1, [&](int64_t clo, int64_t chi) {
        for (int64_t c = clo; c < chi; c++) {
            std::vector<Iv> &out = found[(size_t)c];
            const int64_t i1 = std::min(n, (c + 1) * grain);
            for (int64_t i = c * grain; i < i1; i++) {
                const dh_la &l = las[i];
                if (l.aread < 0 || l.aread >= ncontigs || l.bread < 0 || l.bread >= nreads || l.tlen < 0 || l.tlen % 2 ||
                    l.tlen / 2 != (l.aepos + tspace - 1) / tspace - l.abpos / tspace) {
                    bad = 1;
                    continue;
                }
                const int64_t m0 = mask_ptr[l.aread], m1 = mask_ptr[l.aread + 1];
                if (m1 <= m0) continue;
                // first mask interval that ends after the alignment begins
                int64_t lo = m0, hi = m1;
                while (lo < hi) {
                    const int64_t mid = (lo + hi) >> 1;
                    if (mask_iv[2 * mid + 1] <= l.abpos)
                        lo = mid + 1;
                    else
                        hi = mid;
                }
                const int32_t blen = (int32_t)(read_off[l.bread + 1] - read_off[l.bread]);
                for (int64_t j = lo; j < m1 && mask_iv[2 * j] < l.aepos; j++) {
                    const int32_t ib = std::max(mask_iv[2 * j], l.abpos), ie = std::min(mask_iv[2 * j + 1], l.aepos);
                    int32_t ta, b0, b1;
                    translate_trace_point(l, trace + l.toff, tspace, ib, 0, &ta, &b0);
                    translate_trace_point(l, trace + l.toff, tspace, ie, 1, &ta, &b1);
                    if (l.flags & DH_FLAG_COMP) {
                        const int32_t x0 = blen - b1, x1 = blen - b0;
                        b0 = x0;
                        b1 = x1;
                    }
                    if (b1 > b0) out.push_back(Iv{l.bread, b0, b1});
                }
            }
        }
    });
    if (bad) return dh_fail(DH_EINVAL, "dh_propagate_mask: id out of range or trace length does not fit the A interval");
    std::vector<Iv> all;
    for (auto &v : found) all.insert(all.end(), v.begin(), v.end());
    std::sort(all.begin(), all.end(), [](const Iv &x, const Iv &y) {
        return x.rd != y.rd ? x.rd < y.rd : (x.b != y.b ? x.b < y.b : x.e < y.e);
    });
    int64_t m = 0;
    size_t at = 0;
    for (int32_t r = 0; r < nreads; r++) {
        out_ptr[r] = m;
        while (at < all.size() && all[at].rd == r) {
            int32_t b = all[at].b, e = all[at].e;
            at++;
            while (at < all.size() && all[at].rd == r && all[at].b <= e) {  // intersecting or touching
                e = std::max(e, all[at].e);
                at++;
            }
            if (out_iv && m < cap) {
                out_iv[2 * m] = b;
                out_iv[2 * m + 1] = e;
            }
            m++;
        }
    }
    out_ptr[nreads] = m;
    return m;
}
