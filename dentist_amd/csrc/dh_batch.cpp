// dh_batch.cpp -- the batch drivers of the process stage: dh_process_pileups* crop a batch of pile-ups and run
// dh_process_cropped on it, in concurrent parts (each on a context and a host thread of its own) when the batch is
// large enough; dh_process_pileups_set first fetches the trace values the cropper reads from a mapping result that left
// them on the device.
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <string>
#include <thread>

#include "dh_process.h"
#include "dh_parallel.h"

using namespace dhp;

extern "C" {
void dhk_gather_ranges16(hipStream_t st, const uint16_t *src, const int64_t *desc, int32_t n, uint16_t *dst);
}

// ------------------------------------------------------------------------------------ trace values left on the device
namespace {

// ---- 1. the records of the needed reads (all of them: chain members follow their first record), found by the host
// threads: desc gets (offset in the set's trace, offset in the gathered array, length) per record, total the gathered length
int select_trace_ranges(const dh_db *reads, const dh_la_set *set, const dh_pileups *piles, std::vector<int64_t> &desc, int64_t &total)
{
    const int64_t n = (int64_t)set->la.size();
    std::vector<uint8_t> need((size_t)reads->n, 0);
    for (const auto &t : piles->triples)
        for (size_t x = 0; x + 2 < t.size(); x += 3) {
            if (t[x] < 0 || t[x] >= reads->n) return dh_fail(DH_EINVAL, "dh_process_pileups_set: read id out of range");
            need[(size_t)t[x]] = 1;
        }
    const dh_la *la = set->la.data();
    const int64_t grain = 1 << 15, nch = (n + grain - 1) / grain;
    std::vector<std::vector<int64_t>> part((size_t)std::max<int64_t>(nch, 1));
    std::atomic<int> bad{0};
    dh_parallel_for(nch, 1, [&](int64_t clo, int64_t chi) {
        for (int64_t c = clo; c < chi; c++) {
            auto &v = part[(size_t)c];
            for (int64_t i = c * grain; i < std::min(n, (c + 1) * grain); i++) {
                if (la[i].bread < 0 || la[i].bread >= reads->n) continue;
                if (!need[(size_t)la[i].bread] || la[i].tlen <= 0) continue;
                if (la[i].toff < 0 || la[i].toff + la[i].tlen > set->d_trace_own_len) bad = 1;
                v.push_back(i);
            }
        }
    });
    if (bad.load()) return dh_fail(DH_EINVAL, "dh_process_pileups_set: a record's trace lies outside the set's trace");
    for (const auto &v : part)
        for (int64_t i : v) {
            desc.push_back(la[i].toff);
            desc.push_back(total);
            desc.push_back(la[i].tlen);
            total += la[i].tlen;
        }
    return DH_OK;
}

// ---- 2. those ranges gathered on the device (k_gather_ranges16), brought over in one copy and laid out at their offsets
// in `sparse`, nothing else of which is touched
int gather_sparse_trace(hipStream_t st, const dh_la_set *set, const std::vector<int64_t> &desc, int64_t total, uint16_t *sparse)
{
    const int64_t nsel = (int64_t)desc.size() / 3;
    if (nsel > 0) {
        if (nsel > INT32_MAX) return dh_fail(DH_EOVERFLOW, "dh_process_pileups_set: too many records");
        DevBuf<int64_t> d_desc;
        DevBuf<uint16_t> d_tt;
        HIPCHK(d_desc.alloc(desc.size()));
        HIPCHK(d_tt.alloc((size_t)total));
        TraceVec tmp((size_t)total);
        HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), sizeof(int64_t) * desc.size(), hipMemcpyHostToDevice, st));
        dhk_gather_ranges16(st, set->d_trace_own, d_desc.p, (int32_t)nsel, d_tt.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tmp.data(), d_tt.p, sizeof(uint16_t) * (size_t)total, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        const int64_t *dp = desc.data();
        const uint16_t *tp = tmp.data();
        dh_parallel_for(nsel, 4096, [&](int64_t lo, int64_t hi) {
            for (int64_t r = lo; r < hi; r++) memcpy(sparse + dp[3 * r], tp + dp[3 * r + 1], sizeof(uint16_t) * (size_t)dp[3 * r + 2]);
        });
    }
    return DH_OK;
}

}  // namespace

extern "C" int dh_process_pileups(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const dh_la *las, int64_t n,
                                  const uint16_t *trace, const dh_pileups *piles,
                                  const dh_process_opts *opts, dh_insertions **out)
{
    return dh_process_pileups_masked(ctx, contigs, reads, las, n, trace, piles, nullptr, nullptr, opts, out);
}

// The same on a mapping result whose trace values were left on the device (dh_map_reads, want_sorted & 8): the cropper reads
// the trace of the pile-up reads' records only -- one record in ten at configs[2] --, so those ranges are gathered on the
// device (k_gather_ranges16), brought over in one copy and laid out at their offsets in a host array nothing else of
// which is touched; 330 MB of trace values per step of configs[2] no longer cross PCIe.  rep_ptr / rep_iv may be NULL.
extern "C" int dh_process_pileups_set(dh_ctx *ctx, dh_db *contigs, dh_db *reads, dh_la_set *set, const dh_pileups *piles,
                                      const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                                      dh_insertions **out)
{
    if (!ctx || !reads || !set || !piles || !out) return dh_fail(DH_EINVAL, "dh_process_pileups_set: NULL argument");
    const int64_t n = (int64_t)set->la.size();
    if (!(set->trace.empty() && set->d_trace_own_len > 0))
        return dh_process_pileups_masked(ctx, contigs, reads, set->la.data(), n, set->trace.data(), piles, rep_ptr, rep_iv, opts, out);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<int64_t> desc;
    int64_t total = 0;
    if (int rc = select_trace_ranges(reads, set, piles, desc, total)) return rc;
    // (from the pool of page-locked result buffers, as the whole trace would have been: no page is faulted in here -- a
    // malloc'd array cost 30 ms of first-touch faults per call -- and nothing but the gathered ranges is written)
    TraceVec sparse_v((size_t)std::max<int64_t>(set->d_trace_own_len, 1));
    if (int rc = gather_sparse_trace(ctx->stream, set, desc, total, sparse_v.data())) return rc;
    return dh_process_pileups_masked(ctx, contigs, reads, set->la.data(), n, sparse_v.data(), piles, rep_ptr, rep_iv, opts, out);
}

// ------------------------------------------------------------------------------------ the batch in concurrent parts
// dh_process_pileups_masked is the stages below, called in the order they stand in.
//
// Parts of the batch run concurrently, each on its own context (streams, scratch) and host thread: between its
// kernels a part has host work -- device-to-host copies of 3.5 M overlap records, LAsort, filters and chains, the
// per-tile descriptors of the consensus rounds -- during which the device served nobody (configs[2]: one call 188 ms,
// two concurrent halves 160 ms).  Pile-ups are independent and keep their order; the parts balance n^2.
namespace {

// what every part of a batch is cropped and processed with
struct BatchRun {
    dh_db *contigs, *reads;
    const dh_la *las;
    int64_t n;
    const uint16_t *trace;
    const int64_t *rep_ptr;
    const int32_t *rep_iv;
    const dh_process_opts *opts;
    int32_t batch_most;  // largest pile-up of the whole batch (dh_cropped::batch_most)
    int one(dh_ctx *cx, const dh_pileups *pl, dh_insertions **res) const
    {
        dh_cropped *c = nullptr;
        if (int rc = dh_crop_pileups_masked(cx, contigs, reads, 0, las, n, trace, pl, rep_ptr, rep_iv, opts, &c)) return rc;
        c->batch_most = batch_most;
        const int rc = dh_process_cropped(cx, contigs, c, opts, res);
        dh_cropped_destroy(c);
        return rc;
    }
};

// what one part leaves: its result, its return code and message, the ProcStats of the thread that ran it
struct PartOut {
    dh_insertions *res = nullptr;
    int rc = DH_OK;
    std::string msg;
    ProcStats st;
};

// the number of parts of a batch of np pile-ups: one below 64 pile-ups or with DH_PROCESS_SERIAL, else three
// (DH_PROCESS_PARTS: 1 to 4) of at least 16 pile-ups each
// (three parts: with two, both tend to sit in their host phases at the same time -- measured at configs[2] on one
// MI355X, two runs each: 2 parts 116.9 / 127.3 ms, 3 parts 109.3 / 110.9 ms, 4 parts 112.1 ms of process wall)
int32_t plan_part_count(size_t np)
{
    if (np < 64 || getenv("DH_PROCESS_SERIAL")) return 1;
    int32_t nparts = 3;
    if (const char *e = getenv("DH_PROCESS_PARTS")) nparts = std::max(1, std::min(4, atoi(e)));
    return (int32_t)std::min<size_t>((size_t)nparts, np / 16);
}

// ---- 1. the cuts: part k is the pile-ups [cut[k], cut[k + 1]) -- contiguous runs of about total / nparts of the cost
// n^2 each, none empty (tests/helpers.py: process_part_cuts restates this arithmetic)
std::vector<size_t> plan_part_cuts(const dh_pileups *piles, int32_t nparts)
{
    const size_t np = piles->contig_left.size();
    std::vector<double> cost(np);
    double total = 0;
    for (size_t p = 0; p < np; p++) {
        const double e = (double)piles->triples[p].size() / 3.0;
        cost[p] = e * e;
        total += cost[p];
    }
    // cumulative shares of the parts (equal unless DH_PROCESS_SPLIT = "w0,w1,..." says otherwise: development)
    std::vector<double> wcum((size_t)nparts + 1, 0.0);
    {
        std::vector<double> wt((size_t)nparts, 1.0);
        if (const char *e = getenv("DH_PROCESS_SPLIT")) {
            const char *q = e;
            for (int32_t k = 0; k < nparts && *q; k++) {
                wt[(size_t)k] = std::max(0.01, atof(q));
                while (*q && *q != ',') q++;
                if (*q == ',') q++;
            }
        }
        double sum = 0;
        for (double x : wt) sum += x;
        for (int32_t k = 0; k < nparts; k++) wcum[(size_t)k + 1] = wcum[(size_t)k] + wt[(size_t)k] / sum;
    }
    std::vector<size_t> cut((size_t)nparts + 1, np);
    cut[0] = 0;
    {
        size_t p = 0;
        double acc = 0;
        for (int32_t k = 1; k < nparts; k++) {
            while (p < np && acc + cost[p] <= total * wcum[(size_t)k]) acc += cost[p++];
            while (p < cut[(size_t)k - 1] + 1) acc += cost[p++];
            p = std::min(p, np - (size_t)(nparts - k));
            cut[(size_t)k] = p;
        }
    }
    return cut;
}

// ---- 2. the pile-ups of every part, copied
std::vector<dh_pileups> split_pileups(const dh_pileups *piles, const std::vector<size_t> &cut)
{
    const int32_t nparts = (int32_t)cut.size() - 1;
    std::vector<dh_pileups> part((size_t)nparts);
    for (int32_t k = 0; k < nparts; k++)
        for (size_t p = cut[(size_t)k]; p < cut[(size_t)k + 1]; p++) {
            part[(size_t)k].contig_left.push_back(piles->contig_left[p]);
            part[(size_t)k].triples.push_back(piles->triples[p]);
            if (!piles->join.empty()) part[(size_t)k].join.push_back(piles->join[p]);
        }
    return part;
}

// ---- 3. part 0 on this thread and the context of the call, part k on a thread and a sub-context of its own (created on
// first use); every part's code, message and statistics are kept, no exception leaves its thread
int run_parts(dh_ctx *ctx, const BatchRun &run, const std::vector<dh_pileups> &part, std::vector<PartOut> &po)
{
    const int32_t nparts = (int32_t)part.size();
    for (int32_t k = 1; k < nparts; k++)
        if (!ctx->sub[k - 1])
            if (int rc = dh_ctx_create(ctx->device, nullptr, &ctx->sub[k - 1])) return rc;
    std::vector<std::thread> workers;
    for (int32_t k = 1; k < nparts; k++)
        workers.emplace_back([&, k] {
            PartOut &o = po[(size_t)k];
            try {
                o.rc = run.one(ctx->sub[k - 1], &part[(size_t)k], &o.res);
                if (o.rc) o.msg = dh_last_error();
            } catch (const std::exception &e) {  // (an exception leaving a thread would end the process)
                o.rc = DH_EINVAL;
                o.msg = std::string("dh_process_pileups: a concurrent part of the batch failed: ") + e.what();
            }
            o.st = dh_proc_stats();
        });
    try {
        po[0].rc = run.one(ctx, &part[0], &po[0].res);
    } catch (const std::exception &e) {  // (the workers must be joined whatever happens here; no exception crosses the C ABI)
        po[0].rc = dh_fail(DH_EINVAL, std::string("dh_process_pileups: the first part of the batch failed: ") + e.what());
    }
    for (std::thread &w : workers) w.join();
    return DH_OK;
}

// ---- 4. the counters the sub-contexts gathered belong to this call: folded into the parent, zeroed in the children
void fold_part_counters(dh_ctx *ctx, int32_t nparts)
{
    // the other contexts' alignment statistics belong to this call (the streams' event times overlap: their sum
    // overstates the kernel time of the step, never understates it)
    for (int32_t k = 1; k < nparts; k++) {
        dh_cum_stats &a = ctx->cum, &b = ctx->sub[k - 1]->cum;
        a.ms_index += b.ms_index; a.ms_seed += b.ms_seed; a.ms_wave += b.ms_wave; a.ms_gather += b.ms_gather;
        a.wave_launches += b.wave_launches; a.wave_cells += b.wave_cells; a.alignments += b.alignments; a.las += b.las;
        a.aligned_bp += b.aligned_bp; a.trace_values += b.trace_values; a.hits += b.hits; a.b_bases += b.b_bases;
        b = dh_cum_stats();
        // ... and so do their pile-up joins (dh_get_join_counts: hits and first capacity of the call are sums over its parts)
        dh_ctx *sc = ctx->sub[k - 1];
        ctx->join_launches += sc->join_launches;
        ctx->join_reruns += sc->join_reruns;
        ctx->join_last_hits += sc->join_last_hits;
        ctx->join_first_cap += sc->join_first_cap;
        sc->join_launches = sc->join_reruns = sc->join_last_hits = sc->join_first_cap = 0;
        // ... and the table joins of their re-alignment rounds (dh_get_tjoin_counts)
        ctx->tj_calls += sc->tj_calls;
        ctx->tj_fallbacks += sc->tj_fallbacks;
        ctx->tj_last_hits += sc->tj_last_hits;
        ctx->tj_reruns += sc->tj_reruns;
        sc->tj_calls = sc->tj_fallbacks = sc->tj_last_hits = sc->tj_reruns = 0;
        // ... and the middle seed tier of those rounds (dh_get_seed_tier_counts)
        ctx->seed_mid_chunks += sc->seed_mid_chunks;
        ctx->seed_mid_redone += sc->seed_mid_redone;
        sc->seed_mid_chunks = sc->seed_mid_redone = 0;
    }
}

// ---- 5. the statistics of the call in this thread's ProcStats (where part 0 left its own): times side by side, counts summed
void fold_part_stats(const std::vector<PartOut> &po)
{
    ProcStats &ps = dh_proc_stats();
    for (size_t k = 1; k < po.size(); k++) {
        for (int i = 0; i < 7; i++) ps.ms[i] = std::max(ps.ms[i], po[k].st.ms[i]);  // side by side
        for (int i = 0; i < 3; i++) ps.counters[i] += po[k].st.counters[i];
        for (int i = 0; i < 4; i++) ps.work[i] += po[k].st.work[i];
    }
}

// ---- 6. later parts appended to the first (and destroyed): offsets into the bases, the flank overlaps, their trace and
// the read ids shifted by what the result holds already
dh_insertions *append_insertions(std::vector<PartOut> &po)
{
    dh_insertions *r0 = po[0].res;
    for (size_t k = 1; k < po.size(); k++) {
        dh_insertions *r1 = po[k].res;
        const int64_t b0 = (int64_t)r0->bases.size();
        const int32_t f0 = (int32_t)r0->flank.size(), i0 = r0->ids_off.empty() ? 0 : r0->ids_off.back();
        const int64_t t0 = (int64_t)r0->flank_tr.size();
        for (dh_insertion x : r1->rec) {
            x.cons_off += b0;
            r0->rec.push_back(x);
        }
        r0->bases.insert(r0->bases.end(), r1->bases.begin(), r1->bases.end());
        for (dh_la f : r1->flank) {
            f.toff += t0;
            r0->flank.push_back(f);
        }
        r0->flank_tr.insert(r0->flank_tr.end(), r1->flank_tr.begin(), r1->flank_tr.end());
        for (int32_t v : r1->flank_of) r0->flank_of.push_back(v < 0 ? v : v + f0);
        if (!r1->ids_off.empty()) {
            if (r0->ids_off.empty()) r0->ids_off.push_back(0);
            for (size_t j = 1; j < r1->ids_off.size(); j++) r0->ids_off.push_back(r1->ids_off[j] + i0);
            r0->ids.insert(r0->ids.end(), r1->ids.begin(), r1->ids.end());
        }
        dh_insertions_destroy(r1);
    }
    return r0;
}

}  // namespace

// with the repeat mask of the contigs (--mask of `dentist process`: the cropper keeps its trace points out of it)
extern "C" int dh_process_pileups_masked(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const dh_la *las, int64_t n,
                                         const uint16_t *trace, const dh_pileups *piles, const int64_t *rep_ptr,
                                         const int32_t *rep_iv, const dh_process_opts *opts, dh_insertions **out)
{
    if (!ctx || !contigs || !reads || !piles || !opts || !out || (n > 0 && (!las || !trace)))
        return dh_fail(DH_EINVAL, "dh_process_pileups: NULL argument");
    int32_t batch_most = 0;
    for (const auto &t : piles->triples) batch_most = std::max(batch_most, (int32_t)(t.size() / 3));
    const BatchRun run{contigs, reads, las, n, trace, rep_ptr, rep_iv, opts, batch_most};
    const int32_t nparts = plan_part_count(piles->contig_left.size());
    if (nparts < 2) return run.one(ctx, piles, out);
    const std::vector<size_t> cut = plan_part_cuts(piles, nparts);
    const std::vector<dh_pileups> part = split_pileups(piles, cut);
    std::vector<PartOut> po((size_t)nparts);
    if (int rc = run_parts(ctx, run, part, po)) return rc;
    fold_part_counters(ctx, nparts);
    for (int32_t k = 0; k < nparts; k++)
        if (po[(size_t)k].rc) {
            for (PartOut &o : po) dh_insertions_destroy(o.res);
            if (k == 0) return po[0].rc;  // (its message is this thread's last error)
            return dh_fail(po[(size_t)k].rc, po[(size_t)k].msg.empty() ? "dh_process_pileups: a concurrent part of the batch failed" : po[(size_t)k].msg);
        }
    fold_part_stats(po);
    *out = append_insertions(po);
    return DH_OK;
}
