// dh_align_extend.cpp -- what follows a chunk's seeds: the extension of its candidates (extend_chunk) and the gather of its
// records into the result (gather_chunk, with the transposed records and the items whose records did not fit).
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "dh_align.h"

#define fail dh_fail

// the extension of the chunk's candidates: k_tile (DH-2), k_wave2 (two or four alignments per wavefront) or k_wave;
// symmetric launches first lay out their work units and record slots
int extend_chunk(AlignRun &r, AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    const dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    const int64_t item0 = c.item0;
    const int32_t ni = c.ni;
    const int32_t trmax = r.trmax;
    HIPCHK(hipEventRecord(ctx->ev[3], st));
    HIPCHK(hipMemsetAsync(r.d_queue, 0, sizeof(uint32_t), st));
    // symmetric mode claims slots with atomics: every counter starts at zero
    HIPCHK(hipMemsetAsync(r.d_nla, 0, sizeof(uint32_t) * (size_t)(o.skip_self == 2 ? ni + 1 : 0), st));
    HIPCHK(hipMemsetAsync(r.d_ntr, 0, sizeof(uint32_t) * (size_t)(o.skip_self == 2 ? ni + 1 : 0), st));
    HIPCHK(hipMemsetAsync(r.d_nla + ni, 0, sizeof(uint32_t), st));
    HIPCHK(hipMemsetAsync(r.d_ntr + ni, 0, sizeof(uint32_t), st));
    // symmetric all-vs-all: one work unit per (item, A read) group of candidates instead of per
    // item (k_units); d_queue[3] counts them
    if (r.sym_tiled) {
        // candidate slots: exclusive prefix sums of the items' candidate counts; two record slots per candidate
        SCR(SLOT_CANDOFF, c.d_candoff, (size_t)ni + 1)
        dhk_cand_counts(st, r.d_ncand, ni, c.d_candoff);
        dhk_scan(st, c.d_candoff, (int64_t)ni + 1, r.d_sums);
        uint32_t ncand_total = 0;
        HIPCHK(hipMemcpyAsync(&ncand_total, c.d_candoff + ni, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        c.nrec_slots = 2 * (int64_t)ncand_total;
        if (c.nrec_slots >= INT32_MAX) return fail(DH_EOVERFLOW, "symmetric alignment: more than 2^30 candidates in one call");
        SCR(SLOT_LA, r.d_la, (size_t)c.nrec_slots)
        SCR(SLOT_TRSLOTS, r.d_trslots, (size_t)c.nrec_slots * trmax)
        SCR(SLOT_RECLIST, c.d_reclist, (size_t)c.nrec_slots)
        HIPCHK(dhk_memset(st, r.d_la, 0, sizeof(DhLa) * (size_t)std::max<int64_t>(c.nrec_slots, 1)));
    }
    if (o.skip_self == 2 && ni > 1) {
        if (r.tiled) {
            dhtile::Unit *d_u;
            SCR(SLOT_UNITS, d_u, (size_t)ni * (size_t)o.max_cand)  // at most one unit per candidate
            c.d_units = d_u;
            dhk_tile_units(st, c.candbase, c.ncandbase, (const int32_t *)c.d_candoff - item0, (int32_t)item0, ni, o.max_cand, A->d_off,
                           B->d_off, d_u, r.d_queue + 3);
        } else {
            int4 *d_u;
            SCR(SLOT_UNITS, d_u, (size_t)ni * (size_t)o.max_cand)
            c.d_units = d_u;
            dhk_units(st, c.candbase, c.ncandbase, (int32_t)item0, ni, o.max_cand, c.d_units, r.d_queue + 3);
        }
        HIPCHK(hipGetLastError());
    }
    HIPCHK(dhk_memset(st, r.d_ovf, 0, sizeof(int32_t) * (size_t)ni));
    WaveScratch ws{r.d_pool, r.d_cdj, r.d_queue, (const int4 *)c.d_units, r.d_queue + 3, r.poolcap, r.nbmax, r.d_ovf - item0};
    const ChunkCopies &cc = c.cc;
    const bool packed = c.packed;
    if (r.tiled) {
        dhtile::Params tp = {};
        tp.aoff = A->d_off;
        tp.boff = B->d_off;
        tp.apk = (const uint32_t *)A->d_pk;
        tp.arcpk = (const uint32_t *)A->d_rcpk;
        tp.bpp = (const dhtile::PlanePair *)cc.pk;
        tp.brcpp = (const dhtile::PlanePair *)cc.rcpk;
        // transposed pairs: a symmetric launch (A == B) reads the same copies in both roles
        tp.apk1 = tp.apk;
        tp.arcpk1 = tp.arcpk;
        tp.bpp1 = tp.bpp;
        tp.brcpp1 = tp.brcpp;
        tp.out_la2 = nullptr;
        tp.out_trace2 = nullptr;
        tp.out_nla2 = tp.out_ntr2 = nullptr;
        if (r.res2) {
            tp.apk1 = (const uint32_t *)(c.d_bpk2 + PK_PAD + (cc.pk - cc.pk_w0));
            tp.arcpk1 = (const uint32_t *)(c.d_brcpk2 + PK_PAD + (cc.rcpk - cc.rcpk_w0));
            tp.bpp1 = (const dhtile::PlanePair *)(r.d_app + PK_PAD);
            tp.brcpp1 = (const dhtile::PlanePair *)(r.d_arcpp + PK_PAD);
            tp.out_la2 = r.d_la2 - item0 * o.max_la;
            tp.out_trace2 = r.d_trslots2 - item0 * (int64_t)o.max_la * trmax;
            tp.out_nla2 = (int32_t *)r.d_nla2 - item0;
            tp.out_ntr2 = (int32_t *)r.d_ntr2 - item0;
            HIPCHK(hipMemsetAsync(r.d_nla2, 0, sizeof(uint32_t) * (size_t)(ni + 1), st));
            HIPCHK(hipMemsetAsync(r.d_ntr2, 0, sizeof(uint32_t) * (size_t)(ni + 1), st));
        }
        tp.o = r.dopt;
        tp.item0 = (int32_t)item0;
        tp.nitems = ni;
        tp.cand = c.candbase;
        tp.ncand = c.ncandbase;
        tp.queue = r.d_queue;
        tp.units = (const dhtile::Unit *)c.d_units;
        tp.nunits = r.d_queue + 3;
        tp.candoff = r.sym_tiled ? (const int32_t *)c.d_candoff - item0 : nullptr;
        tp.book_min = 1;
        if (const char *e = getenv("DH_TILE_BOOK_MIN")) tp.book_min = std::max(1, std::min(64, atoi(e)));
        tp.qbatch = 64;
        if (const char *e = getenv("DH_TILE_QBATCH")) tp.qbatch = std::max(1, std::min(4096, atoi(e)));  // development
        tp.regs = r.d_regs;
        tp.cold = r.d_cold;
        tp.nbmax = r.nbmax;
        tp.trmax = trmax;
        tp.out_la = r.sym_tiled ? r.d_la : c.labase;
        tp.out_trace = r.sym_tiled ? r.d_trslots : c.trbase;
        tp.out_nla = c.nlabase;
        tp.out_ntr = c.ntrbase;
        tp.counters = r.d_counters;
        tp.status = r.d_status;
        tp.pflags = o.skip_self == 2 ? B->d_pflags : nullptr;
        tp.tandem = o.skip_self == 3 ? 1 : 0;
        dhk_tile(st, r.tile_waves, &tp);
    } else if (r.dual)
        dhk_wave2(st, r.nslots / r.per_wave, r.av, r.bv, A->d_rc, cc.rc, packed ? A->d_pk : nullptr,
                  packed ? A->d_rcpk : nullptr, packed ? cc.pk : nullptr, packed ? cc.rcpk : nullptr, r.dopt,
                  (int32_t)item0, ni, c.candbase, c.ncandbase, ws, c.labase, c.trbase, trmax, c.nlabase, c.ntrbase, r.d_counters,
                  r.d_status);
    else
        dhk_wave(st, r.nslots, r.av, r.bv, cc.rc, packed ? A->d_pk : nullptr, packed ? cc.pk : nullptr,
                 packed ? cc.rcpk : nullptr, r.dopt, (int32_t)item0, ni, c.candbase, c.ncandbase, ws, c.labase, c.trbase,
                 trmax, c.nlabase, c.ntrbase, r.d_counters, r.d_status);
    HIPCHK(hipGetLastError());
    r.stats.wave_launches++;
    HIPCHK(hipEventRecord(ctx->ev[4], st));
    return DH_OK;
}

// items whose records did not fit (DH-1: > max_la slots; DH-2: > 512 per read and strand)
static int read_ovf(AlignRun &r, const AlignChunk &c)
{
    std::vector<int32_t> h_ovf((size_t)c.ni);
    HIPCHK(hipMemcpy(h_ovf.data(), r.d_ovf, sizeof(int32_t) * (size_t)c.ni, hipMemcpyDeviceToHost));
    for (int32_t it = 0; it < c.ni; it++)
        if (h_ovf[(size_t)it]) {
            r.stats.overflow_items++;
            r.res->ovf_reads.push_back((int32_t)((c.item0 + it) >> 1));
        }
    return DH_OK;
}

// the transposed records of the chunk: same compaction, copied on this stream (not the benched path)
static int gather_transposed(AlignRun &r, const AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = r.st;
    dh_la_set *res2 = r.res2.get();
    const int32_t ni = c.ni;
    dhk_scan(st, r.d_nla2, (int64_t)ni + 1, r.d_sums);
    dhk_scan(st, r.d_ntr2, (int64_t)ni + 1, r.d_sums);
    uint32_t tot2[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(&tot2[0], r.d_nla2 + ni, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&tot2[1], r.d_ntr2 + ni, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (tot2[0] > 0) {
        SCR(SLOT_LAOUT2, r.d_laout2, tot2[0])
        SCR(SLOT_TROUT2, r.d_trout2, tot2[1])
        const size_t l2 = res2->la.size(), t2 = res2->trace.size();
        dhk_compact(st, r.d_la2, r.d_trslots2, r.trmax, r.o.max_la, 0, ni, r.d_nla2, r.d_ntr2, (int64_t)t2, r.d_laout2, r.d_trout2);
        HIPCHK(hipGetLastError());
        res2->la.resize(l2 + tot2[0]);
        res2->trace.resize(t2 + tot2[1]);
        HIPCHK(hipMemcpyAsync(res2->la.data() + l2, r.d_laout2, sizeof(dh_la) * (size_t)tot2[0], hipMemcpyDeviceToHost, st));
        if (tot2[1] > 0)
            HIPCHK(hipMemcpyAsync(res2->trace.data() + t2, r.d_trout2, sizeof(uint16_t) * (size_t)tot2[1],
                                  hipMemcpyDeviceToHost, st));
    }
    return DH_OK;
}

// The chunk's records: compaction on the device, the result grown, the device-to-host copy on the copy stream and the
// chunk hook (both deferred to the next chunk when they may be, see the chunk loop), the transposed records
int gather_chunk(AlignRun &r, AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    dh_la_set *res = r.res.get();
    const ChunkHook *hook = r.hook;
    const int64_t item0 = c.item0, nitems_total = r.nitems_total;
    const int32_t ni = c.ni;
    const bool keep_dev = r.keep_dev, sym_tiled = r.sym_tiled;
    // compaction on the device: exclusive scans of the per-item counts, then one copy kernel
    if (sym_tiled) dhk_rec_count(st, r.d_la, c.nrec_slots, (int32_t)item0, r.d_nla, r.d_ntr);  // records per A-read item
    dhk_scan(st, r.d_nla, (int64_t)ni + 1, r.d_sums);
    dhk_scan(st, r.d_ntr, (int64_t)ni + 1, r.d_sums);
    uint32_t totals[2] = {0, 0};
    int32_t status = 0;
    HIPCHK(hipMemcpyAsync(&totals[0], r.d_nla + ni, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&totals[1], r.d_ntr + ni, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&status, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    unsigned long long sm2[4] = {0, 0, 0, 0};
    dhk_seed_summary(st, r.d_ncand, r.d_nhits, ni, r.d_summary);
    HIPCHK(hipMemcpyAsync(sm2, r.d_summary, sizeof(sm2), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    r.lap(2);
    if (status & DH_ST_POOL_OVERFLOW)
        return fail(DH_EOVERFLOW, "wave: trace-tree pool or boundary capacity exceeded");
    r.stats.hits += (int64_t)sm2[0];
    r.stats.cands += (int64_t)sm2[1];
    if (sm2[3] > 0) {  // the seed filter gave up on some items (> 256 candidate band pairs): which reads
        HIPCHK(hipMemcpy(r.h_ncand.data(), r.d_ncand, sizeof(int32_t) * (size_t)ni, hipMemcpyDeviceToHost));
        for (int32_t it = 0; it < ni; it++)
            if (r.h_ncand[(size_t)it] == -2) {
                r.stats.overflow_items++;
                res->ovf_reads.push_back((int32_t)((item0 + it) >> 1));
            }
    }
    if (o.skip_self == 2 && !sym_tiled)
        if (int rc = read_ovf(r, c)) return rc;
    r.lap(3);
    hipEvent_t copied = nullptr;
    std::function<int()> enqueue_copy;
    bool defer_copy = false;
    if (totals[0] > 0) {
        // the compacted buffers are reused: the previous chunk's copies must have left them
        HIPCHK(hipStreamSynchronize(ctx->cstream));
        SCR(SLOT_LAOUT, r.d_laout, totals[0])
        const size_t l0 = res->la.size(), t0 = keep_dev ? (size_t)res->d_trace_own_len : res->trace.size();
        if (keep_dev) {
            // the chunk's trace values are compacted straight into the set's own device buffer (grown by copy when
            // the first chunk's yield was a bad guess for the call)
            const int64_t need = (int64_t)t0 + totals[1];
            if (need > res->d_trace_own_cap) {
                const double f = 1.15 * (double)nitems_total / std::max<double>(1.0, (double)(item0 - r.item_first + ni));
                const int64_t cap = std::max<int64_t>(need + 65536, (int64_t)(f * (double)need) + 65536);
                uint16_t *nb = nullptr;
                HIPCHK(dh_dev_alloc((void **)&nb, sizeof(uint16_t) * (size_t)cap));
                if (res->d_trace_own) {
                    HIPCHK(hipMemcpyAsync(nb, res->d_trace_own, sizeof(uint16_t) * t0, hipMemcpyDeviceToDevice, st));
                    HIPCHK(hipStreamSynchronize(st));
                    dh_dev_free(res->d_trace_own);
                }
                res->d_trace_own = nb;
                res->d_trace_own_cap = cap;
                res->device = ctx->device;
            }
            r.d_trout = res->d_trace_own + t0;
        } else
            SCR(SLOT_TROUT, r.d_trout, totals[1])
        DhLa *const d_laout = r.d_laout;
        uint16_t *const d_trout = r.d_trout;
        if (sym_tiled) {
            uint32_t *d_cur;
            SCR(SLOT_RECCUR, d_cur, (size_t)ni)
            HIPCHK(dhk_memset(st, d_cur, 0, sizeof(uint32_t) * (size_t)ni));
            dhk_rec_scatter(st, r.d_la, c.nrec_slots, (int32_t)item0, r.d_nla, d_cur, c.d_reclist);
            dhk_compact_sym(st, r.d_la, r.d_trslots, r.trmax, c.d_reclist, ni, r.d_nla, r.d_ntr, (int64_t)t0, d_laout, d_trout, r.d_ovf);
        } else
            dhk_compact(st, r.d_la, r.d_trslots, r.trmax, o.max_la, o.skip_self == 2 ? 1 : 0, ni, r.d_nla, r.d_ntr, (int64_t)t0,
                        d_laout, d_trout);
        HIPCHK(hipGetLastError());
        if (l0 == 0 && ni < nitems_total) {
            // first of several chunks: reserve for the whole call (this chunk's yield + 15 %) so that
            // the result never moves while it grows
            const double f = 1.15 * (double)nitems_total / ni;
            res->la.reserve((size_t)(f * totals[0]) + 1024);
            if (!keep_dev) res->trace.reserve((size_t)(f * totals[1]) + 65536);
        }
        if (l0 + totals[0] > res->la.capacity() || (!keep_dev && t0 + totals[1] > res->trace.capacity()))
            r.tasks.join();  // the records are about to move: copies and hooks in flight finish first
        const bool whole = item0 == r.item_first && ni == nitems_total;  // the call is this one chunk
        const bool dev_only = (r.want_sorted & 2) && t0 == 0 && whole;
        const bool rec_dev = dev_only && (r.want_sorted & 4) && sym_tiled && l0 == 0 && !hook;
        if (!rec_dev) res->la.resize(l0 + totals[0]);
        if (keep_dev)
            res->d_trace_own_len = (int64_t)t0 + totals[1];
        else if (!dev_only)
            res->trace.resize(t0 + totals[1]);
        r.lap(4);
        // device-to-host on the copy stream: it overlaps the next chunk's kernels
        hipEvent_t compacted = ctx->cev[r.nchunk_done & 1];
        copied = ctx->cev[2 + (r.nchunk_done & 1)];
        HIPCHK(hipEventRecord(compacted, st));
        res->d_trace = (t0 == 0 && whole) ? d_trout : nullptr;
        if (totals[1] > 0 && dev_only) res->d_trace_len = (int64_t)totals[1];
        const hipEvent_t copied_ev = copied;
        const uint32_t nla_c = totals[0], ntr_c = totals[1];
        hipStream_t cst = ctx->cstream;
        enqueue_copy = [res, l0, t0, nla_c, ntr_c, dev_only, keep_dev, compacted, copied_ev, cst, d_laout, d_trout]() -> int {
            HIPCHK(hipStreamWaitEvent(cst, compacted, 0));
            HIPCHK(hipMemcpyAsync(res->la.data() + l0, d_laout, sizeof(dh_la) * (size_t)nla_c, hipMemcpyDeviceToHost, cst));
            // the chunk's hook (chain flags, filters, candidates) reads the records only: it starts when they have
            // arrived, while the trace values -- ten times the bytes -- are still on their way (Tasks::join waits
            // for the stream before anybody sees the result)
            HIPCHK(hipEventRecord(copied_ev, cst));
            // (want_sorted & 2: the caller reads the trace from the device copy -- the pile-up all-vs-all, whose host
            // side needs 1 / n of the values: the overlaps of the reference reads -- so the 2 x 160 MB of configs[2] stay)
            if (ntr_c > 0 && !dev_only && !keep_dev)
                HIPCHK(hipMemcpyAsync(res->trace.data() + t0, d_trout, sizeof(uint16_t) * (size_t)ntr_c, hipMemcpyDeviceToHost, cst));
            return DH_OK;
        };
        defer_copy = hook && r.tiled && !r.db_copies && !r.res2 && !sym_tiled && item0 + r.cn < r.item_end && !getenv("DH_NO_DEFER_COPY");
        if (rec_dev) {  // the caller works on the device copy of the records (dh_process_cropped's funnel)
            res->d_la = d_laout;
            res->d_la_n = (int64_t)totals[0];
            res->d_item_off = r.d_nla;
            HIPCHK(hipEventRecord(copied_ev, cst));
        } else if (!defer_copy)
            if (int rc = enqueue_copy()) return rc;
    }
    if (r.res2)
        if (int rc = gather_transposed(r, c)) return rc;
    HIPCHK(hipEventRecord(ctx->ev[5], st));
    HIPCHK(hipStreamSynchronize(st));
    if (sym_tiled && totals[0] > 0)  // (set by the compaction)
        if (int rc = read_ovf(r, c)) return rc;
    r.lap(5);
    r.nchunk_done++;
    if (hook && totals[0] > 0) {
        dh_la *p = res->la.data() + (res->la.size() - totals[0]);
        const int64_t cnt = (int64_t)totals[0];
        const ChunkHook h = *hook;
        const int dev = ctx->device;
        const int64_t l0h = (int64_t)(res->la.size() - totals[0]), chunk_no = r.nchunk_done - 1;
        const bool best = r.want_best != 0;
        const hipEvent_t copied_h = copied;
        const int32_t near_ppm = r.near_ppm;
        Tasks *tasks = &r.tasks;
        auto make_hook = [tasks, h, p, cnt, copied_h, dev, l0h, chunk_no, best, near_ppm]() {
            tasks->v.emplace_back([h, p, cnt, copied_h, dev, l0h, chunk_no, best, near_ppm] {
                (void)hipSetDevice(dev);
                const auto t0 = std::chrono::steady_clock::now();
                (void)hipEventSynchronize(copied_h);  // the records of this chunk have arrived
                const auto t1 = std::chrono::steady_clock::now();
                if (best) dh_select_best_range(p, (size_t)cnt, near_ppm);  // chain flags: a per-read decision too
                const auto t2 = std::chrono::steady_clock::now();
                h(p, cnt, l0h, chunk_no);
                if (getenv("DH_TRACE"))
                    fprintf(stderr, "[chunk hook %lld] %lld records: wait %.2f chains %.2f filters + candidates %.2f ms\n",
                            (long long)chunk_no, (long long)cnt, std::chrono::duration<double, std::milli>(t1 - t0).count(),
                            std::chrono::duration<double, std::milli>(t2 - t1).count(),
                            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t2).count());
            });
        };
        if (defer_copy)  // (the event the hook waits for is recorded when the copy is issued: both wait for the next chunk)
            r.deferred = [enqueue_copy, make_hook]() -> int {
                if (int rc = enqueue_copy()) return rc;
                make_hook();
                return DH_OK;
            };
        else
            make_hook();
    } else if (defer_copy)
        r.deferred = enqueue_copy;
    float t;
    HIPCHK(hipEventElapsedTime(&t, ctx->ev[2], ctx->ev[3]));
    r.ms_seed += t;
    HIPCHK(hipEventElapsedTime(&t, ctx->ev[3], ctx->ev[4]));
    r.ms_wave += t;
    HIPCHK(hipEventElapsedTime(&t, ctx->ev[4], ctx->ev[5]));
    r.ms_gather += t;
    return DH_OK;
}
