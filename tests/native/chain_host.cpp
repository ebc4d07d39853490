// The lane code and the host plan of the chaining (dentist_amd/csrc/dh_chain.h: the per-edge functions, the arr_* and emit_*
// phases, build_plan, plan_groups) compiled for the CPU.  A wavefront is played the way the kernels of dh_chain.hip use these
// functions: the register tier keeps one value per lane in arrays of 64, a shuffle is an index and a ballot a loop; an array
// tier runs the 64 lanes of a phase one after the other where the kernel has a barrier, with its arrays in a buffer of the
// LDS tier's size or in a slab cut into launch groups; the emission reads the States the tiers left.  The scans and the
// translation of node numbers into record indices are the driver's (dh_chain.cpp).
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../dentist_amd/csrc/dh_chain.h"

using chn::Key;
using chn::Node;
using chn::Opts;
using chn::State;

namespace {

// k_chain_wave
void play_wave(const Node *nodes, int32_t n, const Opts &o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    Node x[64];
    int32_t rank[64], from[64], ab[64], ae[64], bb[64], be[64], dist[64], pred[64], label[64], srank[64];
    uint32_t comp[64], depth[64];
    uint64_t nbr[64], reach[64];
    for (int l = 0; l < 64; l++) x[l] = l < n ? nodes[l] : Node{0, 0, 0, 0, 0u};
    for (int l = 0; l < 64; l++) {
        rank[l] = 0;
        for (int w = 0; w < n; w++) rank[l] += chn::precedes(x[w].abpos, x[w].bbpos, w, x[l].abpos, x[l].bbpos, l) ? 1 : 0;
    }
    for (int l = 0; l < 64; l++) {
        from[l] = l;
        for (int w = 0; w < n; w++)
            if (rank[w] == l && l < n) from[l] = w;
    }
    for (int l = 0; l < 64; l++) {
        const Node &s = x[from[l]];
        ab[l] = s.abpos, ae[l] = s.aepos, bb[l] = s.bbpos, be[l] = s.bepos, comp[l] = s.flags & CH_FLAG_COMP;
        dist[l] = -chn::score(ab[l], ae[l], bb[l], be[l]), pred[l] = -1, depth[l] = 1u, nbr[l] = 0;
    }
    for (int u = 0; u < n; u++) {
        uint64_t m = 0;
        const int32_t ud = dist[u];
        const uint32_t udepth = depth[u];
        for (int l = u + 1; l < n; l++)
            if (chn::relax_edge(ab[u], ae[u], bb[u], be[u], comp[u], ud, udepth, u, ab[l], ae[l], bb[l], be[l], comp[l], o, dist[l], pred[l],
                                depth[l])) {
                m |= 1ull << l;
                nbr[l] |= 1ull << u;
            }
        nbr[u] |= m;
    }
    for (int l = 0; l < 64; l++) reach[l] = nbr[l] | (1ull << l);
    for (int w = 0; w < n; w++) {
        const uint64_t rw = reach[w];
        for (int l = 0; l < 64; l++)
            if ((reach[l] >> w) & 1ull) reach[l] |= rw;
    }
    for (int l = 0; l < 64; l++) label[l] = __builtin_ffsll((long long)reach[l]) - 1;
    for (int l = 0; l < 64; l++) {
        srank[l] = 0;
        for (int w = 0; w < n; w++)
            srank[l] += (label[w] != label[l] ? label[w] < label[l] : (dist[w] != dist[l] ? dist[w] < dist[l] : w < l)) ? 1 : 0;
    }
    uint64_t taken = 0, ends = 0, alts = 0;
    int32_t cur = -1, cthr = 0;
    for (int k = 0; k < n; k++) {
        int e = -1;
        for (int l = 0; l < n && e < 0; l++)
            if (srank[l] == k) e = l;
        if (label[e] != cur) {
            cur = label[e];
            cthr = chn::threshold(o.min_score, o.min_rel_score, -dist[e]);
        }
        if (((taken >> e) & 1ull) || -dist[e] < cthr) continue;
        bool alt = false;
        for (int v = e; v >= 0; v = pred[v]) {
            if ((taken >> v) & 1ull) {
                alt = true;
                break;
            }
            taken |= 1ull << v;
        }
        ends |= 1ull << e;
        if (alt) alts |= 1ull << e;
    }
    int32_t best = INT32_MIN;
    for (int l = 0; l < n; l++) best = chn::imax(best, -dist[l]);
    const int32_t thr = chn::threshold(o.min_score, o.min_rel_score, best);
    uint64_t nrec = 0;
    uint32_t nch = 0;
    for (int l = 0; l < n; l++) {
        const bool acc = ((ends >> l) & 1ull) && -dist[l] >= thr;
        state[l] = State{(int32_t)((uint32_t)from[l] | (comp[l] << 31)), pred[l], depth[l] | (acc ? CH_END | (((alts >> l) & 1ull) ? CH_ALT : 0u) : 0u),
                         dist[l]};
        if (acc) nrec += depth[l], nch++;
    }
    *cnt_rec = (uint32_t)nrec;
    *cnt_ch = nch;
}

// chain_arrays of dh_chain.hip: a loop over the lanes where the kernel has a barrier
void play_arrays(const Node *nodes, int32_t n, int32_t *words, const Opts &o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch)
{
    const chn::Arrays a = chn::carve(words, n);
    for (int l = 0; l < 64; l++) chn::arr_load(nodes, n, a, l);
    for (int32_t u = 0; u < n; u++)
        for (int l = 0; l < 64; l++) chn::arr_relax<chn::PlainMem>(a, n, u, o, l);
    for (int l = 0; l < 64; l++) chn::arr_label<chn::PlainMem>(a, n, l);
    for (int l = 0; l < 64; l++) chn::arr_rank(a, n, l);
    for (int l = 0; l < 64; l++) chn::arr_select(a, n, o, l);
    int32_t best = INT32_MIN;
    for (int l = 0; l < 64; l++) best = chn::imax(best, chn::arr_best(a, n, l));
    const int32_t thr = chn::threshold(o.min_score, o.min_rel_score, best);
    uint64_t nrec = 0;
    uint32_t nch = 0;
    for (int l = 0; l < 64; l++) chn::arr_finish(a, n, thr, state, l, nrec, nch);
    *cnt_rec = chn::clamp_records(nrec);
    *cnt_ch = nch;
}

}  // namespace

// Returns the number of chains; -1: unordered input (info[6] = the record), -2: a result array is too small, -3: overflow.
// info: [0] output records, [1] pairs of the global tier, [2..5] pairs per tier, [6] offending record, [7] launch groups
extern "C" int64_t chain_host(const dh_la *las, int64_t n, const Opts *o, int64_t lds_cap, int64_t chunk_words, int64_t *off, int32_t *score,
                              int64_t cap_chains, int64_t *src, uint32_t *flags, int64_t cap_rec, int64_t *info)
{
    memset(info, 0, 8 * sizeof(int64_t));
    info[6] = -1;
    if (lds_cap > CH_LDS_NODES) lds_cap = CH_LDS_NODES;
    chn::Plan pl;
    chn::build_plan(las, n, lds_cap, [](int64_t m, const std::function<void(int64_t, int64_t)> &fn) {
        for (int64_t i = 0; i < m; i++) fn(i, i + 1);  // a part at a time: the chunks meet as they do under the pool
    }, pl);
    if (pl.bad >= 0) {
        info[6] = pl.bad;
        return -1;
    }
    if (pl.too_many) return -3;
    const int64_t nnodes = (int64_t)pl.nodes.size(), npairs = (int64_t)pl.pair_off.size() - 1;
    for (int t = 0; t < chn::TIER_COUNT; t++) info[2 + t] = pl.tier_at[t + 1] - pl.tier_at[t];
    info[1] = info[2 + chn::TIER_GLOBAL];
    off[0] = 0;
    if (nnodes == 0) return 0;
    std::vector<State> state((size_t)nnodes);
    std::vector<Key> key((size_t)nnodes);
    std::vector<uint32_t> cnt_rec((size_t)npairs + 1, 0), cnt_ch((size_t)npairs + 1, 0);
    const Node *nodes = pl.nodes.data();
    auto pair_n = [&](int32_t p) { return (int32_t)(pl.pair_off[(size_t)p + 1] - pl.pair_off[(size_t)p]); };
    for (int64_t i = pl.tier_at[0]; i < pl.tier_at[1]; i++) {  // k_chain_single
        const int32_t p = pl.list[(size_t)i];
        const int64_t at = pl.pair_off[(size_t)p];
        state[(size_t)at] = chn::single_state(nodes[at], *o);
        cnt_rec[(size_t)p] = cnt_ch[(size_t)p] = (state[(size_t)at].depth & CH_END) ? 1u : 0u;
    }
    for (int64_t i = pl.tier_at[1]; i < pl.tier_at[2]; i++) {
        const int32_t p = pl.list[(size_t)i];
        const int64_t at = pl.pair_off[(size_t)p];
        play_wave(nodes + at, pair_n(p), *o, state.data() + at, &cnt_rec[(size_t)p], &cnt_ch[(size_t)p]);
    }
    {  // k_chain_lds: a buffer of exactly the pair's arrays (the sanitizers see an access behind them)
        for (int64_t i = pl.tier_at[2]; i < pl.tier_at[3]; i++) {
            const int32_t p = pl.list[(size_t)i];
            const int64_t at = pl.pair_off[(size_t)p];
            if (pair_n(p) > CH_LDS_NODES) return -3;
            std::vector<int32_t> lds((size_t)CH_ARRAYS * (size_t)pair_n(p));
            play_arrays(nodes + at, pair_n(p), lds.data(), *o, state.data() + at, &cnt_rec[(size_t)p], &cnt_ch[(size_t)p]);
        }
    }
    {  // k_chain_global in launch groups
        std::vector<int64_t> gat, woff;
        int64_t slab_words = 0;
        chn::plan_groups(pl, chunk_words, gat, woff, slab_words);
        info[7] = (int64_t)gat.size() - 1;
        std::vector<int32_t> slab((size_t)slab_words);
        for (size_t g = 0; g + 1 < gat.size(); g++)
            for (int64_t j = gat[g]; j < gat[g + 1]; j++) {
                const int32_t p = pl.list[(size_t)(pl.tier_at[3] + j)];
                const int64_t at = pl.pair_off[(size_t)p];
                play_arrays(nodes + at, pair_n(p), slab.data() + woff[(size_t)j], *o, state.data() + at, &cnt_rec[(size_t)p], &cnt_ch[(size_t)p]);
            }
    }
    // the exclusive scans
    uint64_t nrec = 0, nch = 0;
    for (int64_t p = 0; p <= npairs; p++) {
        const uint32_t r = cnt_rec[(size_t)p], c = cnt_ch[(size_t)p];
        cnt_rec[(size_t)p] = (uint32_t)nrec, cnt_ch[(size_t)p] = (uint32_t)nch;
        nrec += r, nch += c;
    }
    if (nrec > (uint64_t)INT32_MAX) return -3;
    if ((int64_t)nch > cap_chains || (int64_t)nrec > cap_rec) return -2;
    // the emission
    for (int64_t i = 0; i < npairs; i++) {
        const int32_t p = pl.list[(size_t)i];
        if (cnt_ch[(size_t)p + 1] == cnt_ch[(size_t)p]) continue;
        const int64_t at = pl.pair_off[(size_t)p];
        if (i < pl.tier_at[1]) {  // k_chain_emit_single
            off[cnt_ch[(size_t)p]] = cnt_rec[(size_t)p];
            score[cnt_ch[(size_t)p]] = -state[(size_t)at].dist;
            src[cnt_rec[(size_t)p]] = at;
            flags[cnt_rec[(size_t)p]] = nodes[at].flags | CH_FLAG_START | CH_FLAG_BEST;
            continue;
        }
        for (int l = 0; l < 64; l++) chn::emit_keys(nodes + at, state.data() + at, pair_n(p), key.data() + at, l);
        for (int l = 0; l < 64; l++)
            chn::emit_write(nodes + at, state.data() + at, pair_n(p), key.data() + at, at, (int64_t)cnt_rec[(size_t)p], (int64_t)cnt_ch[(size_t)p], off,
                            score, src, flags, l);
    }
    off[nch] = (int64_t)nrec;
    for (uint64_t i = 0; i < nrec; i++) src[i] = pl.node_src[(size_t)src[i]];
    info[0] = (int64_t)nrec;
    return (int64_t)nch;
}
