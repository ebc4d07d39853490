// dh_align.cpp -- the alignment pipeline: dh_align_db*, dh_map_reads and align_range, which runs the reads of B against
// A chunk by chunk through the stages plan_join ... finish_align.  Sequences launches on the context's stream and times
// the stages with HIP events on that stream; device buffers are slots of the context's scratch arena (DhSlot).  The
// stages themselves: dh_align_prepare.cpp (copies and scratch), dh_align_join.cpp (the pile-up join), dh_align_seed.cpp
// (the seeds), dh_align_extend.cpp (extension and gather); dh_align.h is what they share.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "dh_align.h"
#include "dh_parallel.h"

#define fail dh_fail

#ifdef DH_SEED_PROF
extern "C" void dhk_seed_prof_dump();
extern "C" void dhk_join_prof_dump();
extern "C" void dhk_tile_prof_dump();
#endif
// ------------------------------------------------------------------------------------ align


extern "C" int dh_align_db(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts,
                           int32_t want_best, dh_la_set **out)
{
    return dh_align_db_ex(ctx, A, B, opts, want_best, 1, out);
}

static int align_range(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t first, int32_t count, const dh_align_opts *opts,
                       int32_t want_best, int32_t want_sorted, dh_la_set **out, const ChunkHook *hook = nullptr,
                       dh_la_set **out_tr = nullptr, const SeedDump *dump = nullptr, const CandPlant *plant = nullptr);

// `damapper <ref> <reads>.<block>` (snakemake/Snakefile:1143-1170): the reads [first, first + count)
// of B against all of A; read ids in the records are those of the whole DB, as in a block's .las
extern "C" int dh_align_db_block(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t first, int32_t count,
                                 const dh_align_opts *opts, int32_t want_best, dh_la_set **out)
{
    if (!B || first < 0 || count < 0 || (int64_t)first + count > B->n)
        return fail(DH_EINVAL, "dh_align_db_block: block outside the DB");
    return align_range(ctx, A, B, first, count, opts, want_best, 1, out);
}

// The mapping pass with the alignment filters of `dentist collect` applied on the way
// (damapper per read block, Snakefile:1143-1170, + collectPileUps/filter.d:122-356): all six filters
// decide per read, so the records of a finished chunk of reads are filtered on a host thread while the
// device maps the next chunk.  Same records and flags as dh_align_db_block(want_best = 1) followed by
// dh_collect_filter.  rep_ptr / rep_iv: repeat mask of the contigs for WeaklyAnchored (may be NULL).
extern "C" int dh_map_reads(dh_ctx *ctx, dh_db *contigs, dh_db *reads, int32_t first, int32_t count,
                            const dh_align_opts *opts, const dh_process_opts *popts, const int64_t *rep_ptr,
                            const int32_t *rep_iv, int32_t want_sorted, int64_t *dropped6, dh_la_set **out,
                            dh_pileups **cands)
{
    if (!contigs || !reads || !popts || first < 0 || count < 0 || (int64_t)first + count > reads->n)
        return fail(DH_EINVAL, "dh_map_reads: bad argument");
    if (cands && (want_sorted & 1))
        return fail(DH_EINVAL, "dh_map_reads: candidates index the records in mapping order (want_sorted bit 0 clear)");
    want_sorted &= 1 | 8;  // (bit 0: LAsort order; bit 3: the trace values stay on the device, dh_la_set_trace fetches them on demand)
    if (cands) *cands = nullptr;
    std::mutex mu;
    int64_t dropped[6] = {0, 0, 0, 0, 0, 0};
    int hook_rc = DH_OK;
    std::string hook_msg;  // dh_last_error() is per thread: the hook thread's message travels with its code
    std::vector<dh_pileups *> per_chunk;  // spanning-read candidates of every chunk, LA indices of the result
    struct CandGuard {
        std::vector<dh_pileups *> &v;
        ~CandGuard()
        {
            for (dh_pileups *p : v) dh_pileups_destroy(p);
        }
    } cguard{per_chunk};
    const ChunkHook hook = [&](dh_la *las, int64_t n, int64_t l0, int64_t chunk_no) {
        int64_t d[6] = {0, 0, 0, 0, 0, 0};
        int rc = dh_collect_filter(las, n, contigs->h_off.data(), contigs->n, reads->h_off.data(), reads->n, rep_ptr,
                                   rep_iv, popts, d, nullptr);
        dh_pileups *pc = nullptr;
        if (rc == DH_OK && cands) rc = dh_collect_candidates(las, n, contigs->h_off.data(), contigs->n, popts, &pc);
        if (pc && l0 != 0) dh_pileups_shift(pc, (int32_t)l0);
        std::lock_guard<std::mutex> lk(mu);
        if (rc != DH_OK && hook_rc == DH_OK) {
            hook_rc = rc;
            hook_msg = dh_last_error();
        }
        for (int k = 0; k < 6; k++) dropped[k] += d[k];
        if ((size_t)chunk_no >= per_chunk.size()) per_chunk.resize((size_t)chunk_no + 1, nullptr);
        per_chunk[(size_t)chunk_no] = pc;
    };
    const int rc = align_range(ctx, contigs, reads, first, count, opts, 1, want_sorted, out, &hook);
    if (rc != DH_OK) return rc;
    if (hook_rc != DH_OK) {
        dh_la_set_destroy(*out);
        *out = nullptr;
        return fail(hook_rc, hook_msg.empty() ? "dh_map_reads: a chunk's filters failed" : hook_msg);
    }
    if (cands) {  // chunks hold ascending read ranges: concatenating per gap keeps every gap ordered by read
        if (int rc2 = dh_pileups_concat(per_chunk.data(), (int32_t)per_chunk.size(), cands)) {
            dh_la_set_destroy(*out);
            *out = nullptr;
            return rc2;
        }
    }
    if (dropped6) memcpy(dropped6, dropped, sizeof(dropped));
    return DH_OK;
}

int dh_align_db_ex(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, int32_t want_best,
                   int32_t want_sorted, dh_la_set **out)
{
    if (!B) return fail(DH_EINVAL, "dh_align_db: NULL argument");
    return align_range(ctx, A, B, 0, B->n, opts, want_best, want_sorted, out);
}

static_assert(sizeof(dh_seed_cand) == sizeof(DhCand), "dh_seed_cand is DhCand");
// the seed stage of dh_align_db(ctx, A, B, opts) alone: align_range up to seed_chunk, every chunk's candidates copied out
extern "C" int dh_seed_candidates(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, dh_seed_cand *cand,
                                  int32_t *ncand, int32_t *nhits)
{
    if (!B || !cand || !ncand || !nhits) return fail(DH_EINVAL, "dh_seed_candidates: NULL argument");
    const SeedDump dump{cand, ncand, nhits};
    dh_la_set *none = nullptr;
    return align_range(ctx, A, B, 0, B->n, opts, 0, 1, &none, nullptr, nullptr, &dump);
}

// the extension stage of dh_align_db(ctx, A, B, opts) alone: align_range with the caller's candidates in seed_chunk's place
extern "C" int dh_extend_candidates(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, const dh_seed_cand *cand,
                                    const int32_t *ncand, int32_t want_sorted, dh_la_set **out, dh_la_set **out_transposed)
{
    if (!B || !cand || !ncand) return fail(DH_EINVAL, "dh_extend_candidates: NULL argument");
    const CandPlant plant{cand, ncand};
    return align_range(ctx, A, B, 0, B->n, opts, 0, want_sorted ? 1 : 0, out, nullptr, out_transposed, nullptr, &plant);
}

// ---- align_range: the reads [first, first + count) of B against A, chunk by chunk.  Every chunk runs the same stages on
// ctx->stream -- the plan of its mapping join, its derived copies, the seeds, the extension, the gather -- and AlignRun
// holds what crosses them for one call.

static int check_align_args(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, dh_la_set **out,
                            const ChunkHook *hook, dh_la_set **out_tr)
{
    if (!ctx || !A || !B || !opts || !out) return fail(DH_EINVAL, "dh_align_db: NULL argument");
    if (A->ctx != ctx || B->ctx != ctx) return fail(DH_EINVAL, "dh_align_db: DB of another context");
    const dh_align_opts &o = *opts;
    if (o.k < 8 || o.k > 28) return fail(DH_EINVAL, "k must be in [8, 28]");
    if (o.algo != 0 && o.algo != 1) return fail(DH_EINVAL, "algo must be 0 (DH-1, wave) or 1 (DH-2, tiled band)");
    if (o.algo == 1) {
        if (o.width != 64 && o.width != 32) return fail(DH_EINVAL, "algo 1 (DH-2): width is the band, it must be 64 or 32");
        if (o.tspace > dhtile::TS_MAX) return fail(DH_EINVAL, "algo 1 (DH-2): tspace must be <= 128");
    } else if (o.width < 1 || o.width > 62)
        return fail(DH_EINVAL, "width must be in [1, 62]");
    if (o.tspace < 16 || o.tspace > 32767) return fail(DH_EINVAL, "tspace out of range");
    if (o.max_cand < 1 || o.max_cand > 256) return fail(DH_EINVAL, "max_cand must be in [1, 256]");
    if (o.max_la < 1 || o.max_la > 256) return fail(DH_EINVAL, "max_la must be in [1, 256]");
    if (o.pen < 2) return fail(DH_EINVAL, "pen must be >= 2");
    if (o.band_shift < 1 || o.band_shift > 12) return fail(DH_EINVAL, "band_shift out of range");
    if (o.skip_self && A != B) return fail(DH_EINVAL, "skip_self needs A == B");
    if (out_tr && (o.algo != 1 || A == B || hook))
        return fail(DH_EINVAL, "the transposed file is defined for DH-2 (algo 1) mappings of one DB onto another");
    if (o.skip_self < 0 || o.skip_self > 3) return fail(DH_EINVAL, "skip_self must be 0, 1, 2 or 3");
    if (o.skip_self == 3 && (o.algo != 1 || o.strands != 1 || hook || out_tr))
        return fail(DH_EINVAL, "skip_self 3 (a read against itself, datander) is defined for DH-2 (algo 1) on the forward strand (strands 1)");
    if (o.kmer_mod < 1 || o.kmer_mod > 64) return fail(DH_EINVAL, "kmer_mod must be in [1, 64]");
    return DH_OK;
}

// dh_extend_candidates: nothing a planted candidate says may take a kernel outside its sequences, or outside what the seed
// stage could have said under the same options (all items of the call, on the host, before anything is launched)
static int check_plant(const dh_db *A, const dh_db *B, const dh_align_opts &o, const CandPlant &p)
{
    for (int64_t it = 0; it < 2ll * B->n; it++) {
        const int32_t n = p.ncand[it], read = (int32_t)(it >> 1);
        if (n < 0 || n > o.max_cand) return fail(DH_EINVAL, "dh_extend_candidates: ncand outside [0, max_cand]");
        if (n > 0 && !(o.strands & (1 << (it & 1)))) return fail(DH_EINVAL, "dh_extend_candidates: candidates on a strand that opts->strands leaves out");
        const int64_t blen = B->h_off[(size_t)read + 1] - B->h_off[(size_t)read];
        const dh_seed_cand *row = p.cand + it * o.max_cand;
        for (int32_t c = 0; c < n; c++) {
            const dh_seed_cand &q = row[c];
            if (q.aseq < 0 || q.aseq >= A->n) return fail(DH_EINVAL, "dh_extend_candidates: aseq outside A");
            const int64_t alen = A->h_off[(size_t)q.aseq + 1] - A->h_off[(size_t)q.aseq];
            if (q.apos < 0 || q.apos > alen) return fail(DH_EINVAL, "dh_extend_candidates: apos outside its sequence");
            if (q.bpos < 0 || q.bpos > blen) return fail(DH_EINVAL, "dh_extend_candidates: bpos outside its read");
            if ((o.skip_self == 1 || o.skip_self == 2) && q.aseq == read)
                return fail(DH_EINVAL, "dh_extend_candidates: skip_self 1 and 2 take no candidate of a read on itself");
            if (o.skip_self == 3 && (q.aseq != read || q.apos <= q.bpos))
                return fail(DH_EINVAL, "dh_extend_candidates: skip_self 3 takes candidates of a read on itself with apos > bpos");
        }
    }
    return DH_OK;
}

// after the last chunk: counters, chain flags, sort order, the statistics of the call and of the context
static int finish_align(AlignRun &r, double wall0)
{
    dh_ctx *ctx = r.ctx;
    const dh_db *A = r.A, *B = r.B;
    dh_la_set *res = r.res.get(), *res2 = r.res2.get();
    dh_align_stats &stats = r.stats;
    const int32_t near_ppm = r.near_ppm;
    const double w_a = now_ms();
    unsigned long long counters[2] = {0, 0};
    HIPCHK(hipMemcpy(counters, r.d_counters, sizeof(counters), hipMemcpyDeviceToHost));
    stats.wave_cells = (int64_t)counters[0];
    stats.alignments = (int64_t)counters[1];

    r.tasks.join();
    const double tail_hooks = r.tasks.ms_hooks, tail_copies = r.tasks.ms_copies;
    if (r.want_best && !r.hook) dh_select_best_range(res->la.data(), res->la.size(), near_ppm);
    if (r.want_sorted & 1) dh_lasort(res, A->n);
    if (res2) dh_finish_transposed_set(res2, r.want_best != 0, near_ppm);  // (grouped by read already: items are (read, strand) in order)
    r.w_post = now_ms() - w_a;
    stats.las = res->d_la_n > 0 ? res->d_la_n : (int64_t)res->la.size();
    float t;
    HIPCHK(hipEventElapsedTime(&t, ctx->ev[0], ctx->ev[1]));
    stats.ms_index = t;
    stats.ms_seed = r.ms_seed + r.ms_join;  // the k-mer join is seeding work
    stats.ms_wave = r.ms_wave;
    stats.ms_gather = r.ms_gather;
    stats.ms_total = stats.ms_index + r.ms_seed + r.ms_wave + r.ms_gather;
    ctx->stats = stats;
    {
        dh_cum_stats &c = ctx->cum;
        c.ms_index += stats.ms_index;
        c.ms_seed += stats.ms_seed;
        c.ms_wave += stats.ms_wave;
        c.ms_gather += stats.ms_gather;
        c.wave_launches += stats.wave_launches;
        c.wave_cells += stats.wave_cells;
        c.alignments += stats.alignments;
        c.las += stats.las;
        c.hits += stats.hits;
        c.b_bases += stats.b_bases;
        c.trace_values += res->d_trace_len > 0 ? res->d_trace_len : (res->d_trace_own_len > 0 ? res->d_trace_own_len : (int64_t)res->trace.size());
        std::atomic<int64_t> abp{0};
        const dh_la *lp = res->la.data();
        dh_parallel_for((int64_t)res->la.size(), 1 << 16, [&](int64_t lo, int64_t hi) {
            int64_t sum = 0;
            for (int64_t i = lo; i < hi; i++) sum += lp[i].aepos - lp[i].abpos;
            abp += sum;
        });
        c.aligned_bp += abp.load();
    }
#ifdef DH_SEED_PROF
    if (getenv("DH_TRACE")) {
        dhk_seed_prof_dump();
        dhk_join_prof_dump();
        dhk_tile_prof_dump();
    }
#endif
    const double *w_g = r.w_g;
    if (getenv("DH_TRACE"))
        fprintf(stderr,
                "[dh_align_db] A=%d seqs/%lld bp B=%d seqs/%lld bp hits=%lld cands=%lld aln=%lld las=%lld cells=%lld | "
                "index %.2f seed %.2f (join %.2f: %lld hits) wave %.2f gather %.2f ms, wall %.2f ms (host: index %.2f loop %.2f post %.2f; "
                "loop: copies %.2f seed %.2f wave %.2f stats %.2f resize %.2f d2h %.2f; tail: hooks %.2f copies %.2f)\n",
                A->n, (long long)A->total, B->n, (long long)B->total, (long long)stats.hits, (long long)stats.cands,
                (long long)stats.alignments, (long long)stats.las, (long long)stats.wave_cells, stats.ms_index,
                stats.ms_seed, r.ms_join, (long long)r.join_hits, stats.ms_wave, stats.ms_gather,
                ((double)std::chrono::duration_cast<std::chrono::microseconds>(
                     std::chrono::steady_clock::now().time_since_epoch()).count() - wall0) / 1e3,
                r.w_index, r.w_loop, r.w_post, w_g[0], w_g[1], w_g[2], w_g[3], w_g[4], w_g[5], tail_hooks, tail_copies);
    return DH_OK;
}

// dh_seed_candidates: the seeds of the chunk as they stand in the scratch arena, into the caller's rows of its items
static int dump_seeds(AlignRun &r, const AlignChunk &c, const SeedDump &d)
{
    const size_t at = (size_t)(c.item0 - r.item_first), ni = (size_t)c.ni;
    HIPCHK(hipMemcpyAsync(d.cand + at * r.o.max_cand, r.d_cand, sizeof(DhCand) * ni * r.o.max_cand, hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipMemcpyAsync(d.ncand + at, r.d_ncand, sizeof(int32_t) * ni, hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipMemcpyAsync(d.nhits + at, r.d_nhits, sizeof(int32_t) * ni, hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    return DH_OK;
}

static int align_range(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t first, int32_t count, const dh_align_opts *opts,
                       int32_t want_best, int32_t want_sorted, dh_la_set **out, const ChunkHook *hook, dh_la_set **out_tr,
                       const SeedDump *dump, const CandPlant *plant)
{
    const double wall0 = now_ms() * 1e3;
    double w_a = now_ms();
    if (int rc = check_align_args(ctx, A, B, opts, out, hook, out_tr)) return rc;
    if (plant)
        if (int rc = check_plant(A, B, *opts, *plant)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    AlignRun r(ctx, A, B, *opts, first, count, want_best, want_sorted, hook);
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    r.stats.b_bases = B->h_off[(size_t)first + (size_t)count] - B->h_off[(size_t)first];
    r.res.reset(new dh_la_set());
    r.res->tspace = o.tspace;
    *out = nullptr;
    if (out_tr) {
        r.res2.reset(new dh_la_set());
        r.res2->tspace = o.tspace;
        *out_tr = nullptr;
    }

    HIPCHK(hipEventRecord(ctx->ev[0], st));
    // A sequences start at multiples of 4096 on the virtual axis and sepv is one too, so the
    // position of a hit inside its diagonal band (2^band_shift <= 4096 wide) depends only on the
    // pair (A sequence, B read) -- never on which other sequences share the DB or the launch
    r.sepv = (B->max_len + 64 + 4095) & ~4095;
    JoinPlan jp;
    plan_join(r, jp);
    if (int rc = dh_build_index(A, o.k, r.sepv, o.kmer_mod, r.use_join)) return rc;
    if (int rc = prepare_dbs(r)) return rc;
    HIPCHK(hipEventRecord(ctx->ev[1], st));
    r.w_index = now_ms() - w_a;
    w_a = now_ms();

    memcpy(&r.dopt, &o, sizeof(r.dopt));
    r.iv = index_view(A);
    r.av = A->view();
    r.bv = B->view();
    if (int rc = alloc_scratch(r)) return rc;
    if (r.use_join)
        if (int rc = build_join(r, jp)) return rc;
    if (int rc = plan_seeds(r)) return rc;
    r.h_ncand.resize((size_t)r.cn);
    r.h_nhits.resize((size_t)r.cn);

    // The device-to-host copy of a chunk's records runs as a copy kernel here; beside it the streaming kernels that make
    // the next chunk's derived copies (pack, reverse complement, planes) ran 2-5 x slower (12 ms between two chunks of
    // configs[2] for 6.5 ms of work).  The copy -- and the hook that waits for it -- of chunk c is therefore issued after
    // chunk c + 1's copies have been made: it overlaps that chunk's seed kernel instead.
    for (int64_t item0 = r.item_first; item0 < r.item_end;) {
        AlignChunk c;
        c.item0 = item0;
        c.ni = (int32_t)std::min<int64_t>(r.cn, r.item_end - item0);
        r.w_c = now_ms();
        if (!plant)  // (planted candidates: no join of the chunk is planned, no k-mer is looked up)
            if (int rc = plan_mj_chunk(r, c)) return rc;
        if (int rc = copy_chunk(r, c)) return rc;
        SeedRedo redo = SEED_DONE;
        if (int rc = plant ? plant_chunk(r, c, *plant) : seed_chunk(r, c, &redo)) return rc;
        if (redo != SEED_DONE) continue;  // the same chunk again (SeedRedo says why)
        r.lap(1);
        if (dump) {  // dh_seed_candidates: the chunk ends here
            if (int rc = dump_seeds(r, c, *dump)) return rc;
            item0 += r.cn;
            continue;
        }
        if (int rc = extend_chunk(r, c)) return rc;
        if (int rc = gather_chunk(r, c)) return rc;
        item0 += r.cn;
    }
    r.w_loop = now_ms() - w_a;
    if (dump) {  // the statistics of the seed stage alone (hits, cands, overflow_items, big_items, b_bases); no cumulative ones
        for (int64_t it = 0; it < r.nitems_total; it++) {
            r.stats.hits += dump->nhits[it];
            r.stats.cands += std::max(dump->ncand[it], 0);
            r.stats.overflow_items += dump->ncand[it] == -2;
        }
        ctx->stats = r.stats;
        return DH_OK;
    }
    if (int rc = finish_align(r, wall0)) return rc;
    *out = r.res.release();
    if (out_tr) *out_tr = r.res2.release();
    return DH_OK;
}

// `damapper -C <ref> <reads>`: the mapping and, as a second set, the records of the transposed pairs (read, contig) --
// for every accepted local alignment the tiled alignment (DH-2) of A'' = the read on its forward strand against B'' = the
// contig (complemented for a reverse-strand mapping) through the same seed, accepted on its own; one pass over the reads
// (the reference's tools write <reads>.<ref>.las from the same alignments: source/dentist/dazzler.d:6158-6170,
// getLasFile :4339-4354).  opts->algo must be 1.
extern "C" int dh_align_db_transposed(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, int32_t want_best,
                                      dh_la_set **out, dh_la_set **out_transposed)
{
    if (!B || !out_transposed) return fail(DH_EINVAL, "dh_align_db_transposed: NULL argument");
    return align_range(ctx, A, B, 0, B->n, opts, want_best, 1, out, nullptr, out_transposed);
}
