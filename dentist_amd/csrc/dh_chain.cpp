// dh_chain.cpp -- host side of dh_la_chain: chainLocalAlignments (common/alignments/chaining.d:122-334) on batches of pairs,
// what `dentist chain-local-alignments` writes and `dentist check-results` runs on its daligner output
// (commands/checkResults.d:617-624).  Kernels: dh_chain.hip; lane code, layouts and the plan: dh_chain.h.
//
// The call: the options are checked; the host threads group the enabled records into pairs and check their order (all of it
// before the first launch); the compact nodes, the pair offsets and the tier lists are uploaded; every tier's kernel leaves a
// State per node and the pair's record and chain counts; two exclusive scans place the pairs; the emission writes the result
// arrays, which come back in one copy each.  src_index arrives as node numbers and is turned into record indices here.
#include "dh_host.h"

#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "dh_chain.h"

using chn::Key;
using chn::Node;
using chn::State;

extern "C" void dhk_chain_single(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, int64_t npairs,
                                 const void *o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch);
extern "C" void dhk_chain_wave(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, int64_t npairs,
                               const void *o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch);
extern "C" void dhk_chain_lds(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, int64_t npairs, const void *o,
                              State *state, uint32_t *cnt_rec, uint32_t *cnt_ch);
extern "C" void dhk_chain_global(hipStream_t st, const Node *nodes, const int64_t *pair_off, const int32_t *list, const int64_t *woff,
                                 int64_t npairs, int32_t *slab, const void *o, State *state, uint32_t *cnt_rec, uint32_t *cnt_ch);
extern "C" void dhk_chain_emit(hipStream_t st, const Node *nodes, const State *state, const int64_t *pair_off, const int32_t *list,
                               int64_t nsingle, int64_t nmulti, const uint32_t *rec_at, const uint32_t *ch_at, Key *key, int64_t *off,
                               int32_t *sc, int64_t *src, uint32_t *flags);

struct dh_la_chains {
    std::vector<int64_t> off{0}, src;
    std::vector<int32_t> score;
    std::vector<uint32_t> flags;
    int64_t big_pairs = 0;
};
static_assert(sizeof(dh_chain_opts) == 32 && sizeof(chn::Opts) == 32 && sizeof(Node) == 20 && sizeof(State) == 16,
              "the header states the layouts");

extern "C" void dh_default_chain_opts(dh_chain_opts *o, int32_t tspace)
{
    if (!o) return;
    o->max_indel = 1000;
    o->max_chain_gap = 10000;
    o->min_score = tspace;
    o->pad_ = 0;
    o->max_relative_overlap = 0.3;
    o->min_relative_score = 1.0;
}

extern "C" int dh_la_chain(dh_ctx *ctx, const dh_la *las, int64_t n, const dh_chain_opts *o, dh_la_chains **out)
{
    if (!ctx || !out || !o || n < 0 || (n > 0 && !las)) return dh_fail(DH_EINVAL, "dh_la_chain: bad argument");
    *out = nullptr;
    if (!(o->max_relative_overlap > 0.0 && o->max_relative_overlap < 1.0))
        return dh_fail(DH_EINVAL, "dh_la_chain: max_relative_overlap outside (0, 1)");
    if (!(o->min_relative_score >= 0.0 && o->min_relative_score <= 1.0))
        return dh_fail(DH_EINVAL, "dh_la_chain: min_relative_score outside [0, 1]");
    if (o->min_score <= 0) return dh_fail(DH_EINVAL, "dh_la_chain: min_score must be positive");
    if (o->max_indel < 0 || o->max_chain_gap < 0) return dh_fail(DH_EINVAL, "dh_la_chain: negative max_indel or max_chain_gap");
    const auto t_call = std::chrono::steady_clock::now();
    const bool trace = getenv("DH_TRACE") != nullptr;
    const int64_t lds_cap = dh_env_knob("DH_CHAIN_LDS_NODES", CH_LDS_NODES, CH_WAVE_NODES, CH_LDS_NODES);
    const int64_t chunk_kb = dh_env_knob("DH_CHAIN_CHUNK_KB", (int64_t)1 << 20, 1, (int64_t)1 << 26);
    // ---- the plan, before anything is launched
    chn::Plan pl;
    chn::build_plan(las, n, lds_cap, dh_plan_runner<1>, pl);  // (the plan runs one index per chunk of records)
    if (pl.bad >= 0) {
        char msg[200];
        snprintf(msg, sizeof(msg), "dh_la_chain: record %lld (aread %d, bread %d) precedes the enabled record before it: the input must be "
                 "sorted by (aread, bread)", (long long)pl.bad, las[pl.bad].aread, las[pl.bad].bread);
        return dh_fail(DH_EINVAL, msg);
    }
    if (pl.too_many) return dh_fail(DH_EOVERFLOW, "dh_la_chain: more than 2^31 - 1 enabled records");
    std::unique_ptr<dh_la_chains> res(new dh_la_chains);
    const int64_t nnodes = (int64_t)pl.nodes.size(), npairs = (int64_t)pl.pair_off.size() - 1;
    if (nnodes == 0) {
        *out = res.release();
        return DH_OK;
    }
    const double ms_plan = dh_ms_since(t_call);
    const int64_t *tat = pl.tier_at;
    res->big_pairs = tat[chn::TIER_GLOBAL + 1] - tat[chn::TIER_GLOBAL];
    std::vector<int64_t> gat, woff;
    int64_t slab_words = 0;
    chn::plan_groups(pl, chunk_kb * 256, gat, woff, slab_words);
    // ---- upload
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Node *d_nodes;
    int64_t *d_pair_off, *d_woff;
    int32_t *d_list, *d_slab;
    State *d_state;
    Key *d_key;
    uint32_t *d_cnt_rec, *d_cnt_ch, *d_sums;
    unsigned long long *d_total;
    if (int rc = dh_upload(ctx, SLOT_CH_NODES, pl.nodes, &d_nodes)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CH_PAIR_OFF, pl.pair_off, &d_pair_off)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CH_LIST, pl.list, &d_list)) return rc;
    if (int rc = dh_upload(ctx, SLOT_CH_WOFF, woff, &d_woff)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_SLAB, (size_t)slab_words, &d_slab)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_STATE, (size_t)nnodes, &d_state)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_KEY, (size_t)nnodes, &d_key)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_CNT_REC, (size_t)npairs + 1, &d_cnt_rec)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_CNT_CH, (size_t)npairs + 1, &d_cnt_ch)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_SUMS, (size_t)(npairs + 1) / 2048 + 1, &d_sums)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_TOTAL, 2, &d_total)) return rc;
    HIPCHK(hipMemsetAsync(d_cnt_rec + npairs, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(d_cnt_ch + npairs, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(d_total, 0, 2 * sizeof(unsigned long long), st));
    double ms_tier[chn::TIER_COUNT] = {0, 0, 0, 0};
    auto tier_done = [&](int t, std::chrono::steady_clock::time_point t0) -> int {  // (a traced call times every tier on its own)
        HIPCHK(hipGetLastError());
        if (trace) {
            HIPCHK(hipStreamSynchronize(st));
            ms_tier[t] = dh_ms_since(t0);
        }
        return DH_OK;
    };
    if (trace) HIPCHK(hipStreamSynchronize(st));
    const double ms_upload = dh_ms_since(t_call) - ms_plan;
    // ---- the tiers
    auto t0 = std::chrono::steady_clock::now();
    dhk_chain_single(st, d_nodes, d_pair_off, d_list + tat[0], tat[1] - tat[0], o, d_state, d_cnt_rec, d_cnt_ch);
    if (int rc = tier_done(chn::TIER_SINGLE, t0)) return rc;
    t0 = std::chrono::steady_clock::now();
    dhk_chain_wave(st, d_nodes, d_pair_off, d_list + tat[1], tat[2] - tat[1], o, d_state, d_cnt_rec, d_cnt_ch);
    if (int rc = tier_done(chn::TIER_WAVE, t0)) return rc;
    t0 = std::chrono::steady_clock::now();
    dhk_chain_lds(st, d_nodes, d_pair_off, d_list + tat[2], tat[3] - tat[2], o, d_state, d_cnt_rec, d_cnt_ch);
    if (int rc = tier_done(chn::TIER_LDS, t0)) return rc;
    t0 = std::chrono::steady_clock::now();
    for (size_t g = 0; g + 1 < gat.size(); g++)  // (launches of one stream: a group's slab is free when the next one starts)
        dhk_chain_global(st, d_nodes, d_pair_off, d_list + tat[3] + gat[g], d_woff + gat[g], gat[g + 1] - gat[g], d_slab, o, d_state,
                         d_cnt_rec, d_cnt_ch);
    if (int rc = tier_done(chn::TIER_GLOBAL, t0)) return rc;
    // ---- where every pair's records and chains go
    t0 = std::chrono::steady_clock::now();
    dhk_scan_total(st, d_cnt_rec, npairs + 1, d_sums, d_total);
    dhk_scan_total(st, d_cnt_ch, npairs + 1, d_sums, d_total + 1);
    HIPCHK(hipGetLastError());
    unsigned long long total[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(total, d_total, sizeof(total), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (total[0] > (unsigned long long)INT32_MAX) return dh_fail(DH_EOVERFLOW, "dh_la_chain: more than 2^31 - 1 output records");
    const int64_t nrec = (int64_t)total[0], nch = (int64_t)total[1];
    // ---- emission
    int64_t *d_off, *d_src;
    int32_t *d_score;
    uint32_t *d_flags;
    if (int rc = dh_scr(ctx, SLOT_CH_OUT_OFF, (size_t)nch, &d_off)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_OUT_SCORE, (size_t)nch, &d_score)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_OUT_SRC, (size_t)nrec, &d_src)) return rc;
    if (int rc = dh_scr(ctx, SLOT_CH_OUT_FLAGS, (size_t)nrec, &d_flags)) return rc;
    dhk_chain_emit(st, d_nodes, d_state, d_pair_off, d_list, tat[1], npairs - tat[1], d_cnt_rec, d_cnt_ch, d_key, d_off, d_score, d_src, d_flags);
    HIPCHK(hipGetLastError());
    res->off.resize((size_t)nch + 1);
    res->score.resize((size_t)nch);
    res->src.resize((size_t)nrec);
    res->flags.resize((size_t)nrec);
    if (nch > 0) {
        HIPCHK(hipMemcpyAsync(res->off.data(), d_off, sizeof(int64_t) * (size_t)nch, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(res->score.data(), d_score, sizeof(int32_t) * (size_t)nch, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(res->src.data(), d_src, sizeof(int64_t) * (size_t)nrec, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(res->flags.data(), d_flags, sizeof(uint32_t) * (size_t)nrec, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    res->off[(size_t)nch] = nrec;
    const double ms_emit = dh_ms_since(t0);
    int64_t *src = res->src.data();
    const int64_t *node_src = pl.node_src.data();
    dh_parallel_for(nrec, 1 << 16, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) src[i] = node_src[src[i]];  // node number -> record index
    });
    if (trace)
        fprintf(stderr,
                "[chain] %lld records, %lld enabled in %lld pairs: tiers single %lld, wave %lld, lds %lld (cap %lld), global %lld (%zu "
                "launches); plan %.2f ms, upload %.2f ms, kernels %.2f / %.2f / %.2f / %.2f ms, scan+emit+download %.2f ms, total %.2f ms; "
                "%lld chains, %lld output records\n",
                (long long)n, (long long)nnodes, (long long)npairs, (long long)(tat[1] - tat[0]), (long long)(tat[2] - tat[1]),
                (long long)(tat[3] - tat[2]), (long long)lds_cap, (long long)(tat[4] - tat[3]), gat.size() - 1, ms_plan, ms_upload, ms_tier[0],
                ms_tier[1], ms_tier[2], ms_tier[3], ms_emit, dh_ms_since(t_call), (long long)nch, (long long)nrec);
    *out = res.release();
    return DH_OK;
}

extern "C" int dh_la_set_chain(dh_ctx *ctx, const dh_la_set *set, const dh_chain_opts *o, dh_la_chains **out)
{
    const dh_la *las;
    int64_t n;
    if (int rc = dh_set_host_records("dh_la_set_chain", true, set, &las, &n)) return rc;  // (dh_la_chain checks the others)
    return dh_la_chain(ctx, las, n, o, out);
}

extern "C" void dh_la_chains_destroy(dh_la_chains *c) { delete c; }
extern "C" int64_t dh_la_chains_count(const dh_la_chains *c) { return c ? (int64_t)c->score.size() : 0; }
extern "C" int64_t dh_la_chains_records(const dh_la_chains *c) { return c ? (int64_t)c->src.size() : 0; }
extern "C" const int64_t *dh_la_chains_off(const dh_la_chains *c) { return c ? c->off.data() : nullptr; }
extern "C" const int32_t *dh_la_chains_score(const dh_la_chains *c) { return c ? c->score.data() : nullptr; }
extern "C" const int64_t *dh_la_chains_src_index(const dh_la_chains *c) { return c ? c->src.data() : nullptr; }
extern "C" const uint32_t *dh_la_chains_flags(const dh_la_chains *c) { return c ? c->flags.data() : nullptr; }
extern "C" int64_t dh_la_chains_big_pairs(const dh_la_chains *c) { return c ? c->big_pairs : 0; }

extern "C" int dh_la_chains_to_set(const dh_la_chains *c, const dh_la *las, int64_t n, const uint16_t *trace, int32_t tspace,
                                   dh_la_set **out)
{
    if (!c || !out || n < 0 || (n > 0 && !las)) return dh_fail(DH_EINVAL, "dh_la_chains_to_set: bad argument");
    *out = nullptr;
    const int64_t nrec = (int64_t)c->src.size();
    int64_t tlen = 0;
    for (int64_t i = 0; i < nrec; i++) {
        const int64_t s = c->src[(size_t)i];
        if (s < 0 || s >= n) return dh_fail(DH_EINVAL, "dh_la_chains_to_set: the chains were not made from these records");
        if (las[s].tlen < 0) return dh_fail(DH_EINVAL, "dh_la_chains_to_set: negative tlen");
        tlen += las[s].tlen;
    }
    std::unique_ptr<dh_la_set> set(new dh_la_set);
    set->tspace = tspace;
    set->la.resize((size_t)nrec);
    if (trace) set->trace.resize((size_t)tlen);
    int64_t at = 0;
    for (int64_t i = 0; i < nrec; i++) {
        dh_la l = las[c->src[(size_t)i]];
        l.flags = c->flags[(size_t)i];
        if (trace) {
            std::copy(trace + l.toff, trace + l.toff + l.tlen, set->trace.data() + at);
            l.toff = at;
            at += l.tlen;
        } else
            l.toff = 0;
        set->la[(size_t)i] = l;
    }
    *out = set.release();
    return DH_OK;
}
