// dh_align.cpp -- the alignment pipeline: dh_align_db*, dh_map_reads and align_range, which runs the reads of B against
// A chunk by chunk through the stages plan_join ... finish_align.  Sequences launches on the context's stream and times
// the stages with HIP events on that stream; device buffers are slots of the context's scratch arena (DhSlot).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>

#include "dh_internal.h"
#include "dh_join.h"
#include "dh_mjoin.h"
#include "dh_tjoin.h"
#include "dh_tile.h"
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

// per-chunk hook: called on a host thread of its own with the records of a finished chunk (B-major,
// whole reads) while the device works on the next chunk; the records may be modified in place
// (records of the chunk, their number, their offset in the result, number of the chunk)
typedef std::function<void(dh_la *, int64_t, int64_t, int64_t)> ChunkHook;
// dh_seed_candidates: the caller's arrays (item 0 = the first item of the call); with it a chunk ends behind its seeds
struct SeedDump {
    dh_seed_cand *cand;
    int32_t *ncand, *nhits;
};
static int align_range(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t first, int32_t count, const dh_align_opts *opts,
                       int32_t want_best, int32_t want_sorted, dh_la_set **out, const ChunkHook *hook = nullptr,
                       dh_la_set **out_tr = nullptr, const SeedDump *dump = nullptr);

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

// derived copies (reverse complement, 2-bit packed forward / reverse) of the reads [r0, r1) of B in
// the context's scratch arena; the returned pointers are shifted so that absolute base offsets of
// the DB index them, exactly like the DB-owned whole copies
struct ChunkCopies {
    const uint8_t *rc = nullptr, *pk = nullptr, *rcpk = nullptr;
    bool has_n = false;
    // the packed words of the chunk themselves (unshifted) -- k_tile turns them into plane words in place
    uint8_t *pk_w0 = nullptr, *rcpk_w0 = nullptr;
    int64_t pk_words = 0;
    bool planes = false;  // the copies are plane-packed already (made so straight from the bytes)
};
// planes: plane-packed copies for k_tile instead of the 2-bit packed ones (a DH-2 mapping that does not keep the packed
// words for the transposed pairs): the conversion passes over both copies -- 8 of the 24 GB a chunk of configs[2] moves
// for its copies -- fall away
static int chunk_copies(dh_ctx *ctx, dh_db *B, int32_t r0, int32_t r1, bool want_packed, bool need_bytes,
                        ChunkCopies *out, bool planes = false)
{
    hipStream_t st = ctx->stream;
    const int64_t o0 = B->h_off[(size_t)r0], o1 = B->h_off[(size_t)r1];
    const int64_t a0 = o0 & ~31ll;  // packed words hold 32 bases: start the chunk on a word boundary
    uint8_t *d_rc, *d_pk, *d_rcpk;
    int32_t *d_flag;
    out->has_n = false;
    auto rc_bytes = [&]() -> int {
        // reverse complement as bytes (only the wave kernels' byte path reads it): every read mirrored
        // inside its own [off, off + len) range
        if (int rc = dh_scratch(ctx, SLOT_CHUNK_RC, (size_t)(o1 - a0) + 2 * DB_PAD, (void **)&d_rc)) return rc;
        HIPCHK(dhk_memset(st, d_rc, 4, (size_t)(o1 - a0) + 2 * DB_PAD));
        uint8_t *rc_shift = d_rc + DB_PAD - a0;
        dhk_revcomp(st, B->d_bases, rc_shift, B->d_off + r0, r1 - r0, B->max_len);
        HIPCHK(hipGetLastError());
        out->rc = rc_shift;
        return DH_OK;
    };
    if (!want_packed) return rc_bytes();
    // 2-bit packed forward copy and, straight from the forward bytes, the packed reverse complements
    const size_t pbytes = (size_t)((o1 - a0 + 31) / 32) * 8 + 2 * PK_PAD;
    if (int rc = dh_scratch(ctx, SLOT_CHUNK_PK, pbytes, (void **)&d_pk)) return rc;
    if (int rc = dh_scratch(ctx, SLOT_CHUNK_RCPK, pbytes, (void **)&d_rcpk)) return rc;
    if (int rc = dh_scratch(ctx, SLOT_STATUS, DH_STW_COUNT * sizeof(int32_t), (void **)&d_flag)) return rc;
    HIPCHK(hipMemsetAsync(d_flag + DH_STW_PACK, 0, 2 * sizeof(int32_t), st));  // DH_STW_PACK and DH_STW_PACK_RC
    // k_pack2_rc stores the words inside a read whole and ORs into the words reads share: only those (and the padding on
    // both sides) are zeroed -- the memset of the whole buffer was 2 GB per chunk of the mapping
    HIPCHK(hipMemsetAsync(d_rcpk, 0, PK_PAD + 8, st));
    HIPCHK(hipMemsetAsync(d_rcpk + pbytes - PK_PAD - 8, 0, PK_PAD + 8, st));
    if (planes) {
        dhk_pack2_planes(st, B->d_bases + a0, o1 - a0, d_pk + PK_PAD, d_flag + DH_STW_PACK);
        // (the reverse-complement planes from the forward planes: the chunk's bytes are read once, not twice)
        dhk_planes_rc(st, d_pk + PK_PAD, B->d_off + r0, r1 - r0, B->max_len, a0, d_rcpk + PK_PAD);
    } else {
        dhk_pack2_rc_bounds(st, B->d_off + r0, r1 - r0, a0, d_rcpk + PK_PAD);
        dhk_pack2(st, B->d_bases + a0, o1 - a0, d_pk + PK_PAD, d_flag + DH_STW_PACK);
        dhk_pack2_rc(st, B->d_bases, B->d_off + r0, r1 - r0, B->max_len, a0, d_rcpk + PK_PAD);
    }
    out->planes = planes;
    HIPCHK(hipGetLastError());
    int32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag + DH_STW_PACK, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out->has_n = flag != 0;
    out->pk = d_pk + PK_PAD - (a0 >> 2);
    out->rcpk = d_rcpk + PK_PAD - (a0 >> 2);
    out->pk_words = (o1 - a0 + 31) / 32;
    out->pk_w0 = d_pk + PK_PAD;
    out->rcpk_w0 = d_rcpk + PK_PAD;
    // codes outside 0..3 (here or in A): the wave kernels slide over the byte arrays
    if (out->has_n || need_bytes) return rc_bytes();
    return DH_OK;
}

// ---- align_range: the reads [first, first + count) of B against A, chunk by chunk.  Every chunk runs the same stages on
// ctx->stream -- the plan of its mapping join, its derived copies, the seeds, the extension, the gather -- and AlignRun
// holds what crosses them for one call.

static double now_ms()
{
    return (double)std::chrono::duration_cast<std::chrono::microseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count() / 1e3;
}

// hook tasks in flight; joined before the result can move or is handed out (also on error paths)
struct Tasks {
    hipStream_t cs;
    std::vector<std::thread> v;
    double ms_hooks = 0, ms_copies = 0;  // of the last join: waiting for the hook threads, then for the copy stream
    void join()
    {
        const auto t0 = std::chrono::steady_clock::now();
        for (auto &t : v)
            if (t.joinable()) t.join();
        v.clear();
        const auto t1 = std::chrono::steady_clock::now();
        (void)hipStreamSynchronize(cs);  // copies in flight have landed
        const auto t2 = std::chrono::steady_clock::now();
        ms_hooks = std::chrono::duration<double, std::milli>(t1 - t0).count();
        ms_copies = std::chrono::duration<double, std::milli>(t2 - t1).count();
    }
    ~Tasks() { join(); }
};

// the state of one align_range call that crosses its stages
struct AlignRun {
    dh_ctx *ctx;
    dh_db *A, *B;
    const dh_align_opts &o;
    int32_t first, count, want_best, want_sorted;
    const ChunkHook *hook;
    hipStream_t st;
    int32_t near_ppm;
    // the result and the transposed file of a mapping (`damapper -C`: records (read, contig) of the transposed pairs);
    // declared ahead of `tasks`, whose hook threads write into the records: they are joined first
    std::unique_ptr<dh_la_set> res, res2;
    Tasks tasks;
    dh_align_stats stats = {};
    // derived flags
    bool tiled, use_join = false, use_mj = false, use_tj = false, db_copies = false, want_packed = false, dual = false, sym_tiled = false,
         keep_dev = false;
    // geometry: items of the call, per chunk (cn), capacities of the extension
    int64_t nitems_total, item_first, item_end;
    int32_t sepv = 0, chunk = 0, cn = 0, nbmax = 0, trmax = 0, per_wave = 0, poolcap = 0, nslots = 0, tile_waves = 0;
    int cap = 0;       // LDS hit capacity of the directory path's seed filter (doubled when many reads overflow it)
    double dens = 0;   // chance matches of a sampled k-mer per strand
    int64_t mj_min_bases = 0;
    DhOpts dopt;
    IndexView iv;
    DbView av, bv;
    // the pile-up join (its build: ms_join, join_hits; jhist: reads with more than 2048 / 4096 / 8192 hits, the largest count)
    JoinView jv = {};
    int64_t join_hits = 0;
    float ms_join = 0;
    unsigned int jhist[4] = {0, 0, 0, 0};
    // scratch of the call (slots and sizes: alloc_scratch)
    DhCand *d_cand = nullptr;
    int32_t *d_ncand = nullptr, *d_nhits = nullptr, *d_status = nullptr, *d_cdj = nullptr, *d_ovf = nullptr, *d_regs = nullptr;
    uint32_t *d_nla = nullptr, *d_ntr = nullptr, *d_queue = nullptr, *d_sums = nullptr;
    DhNode *d_pool = nullptr;
    DhLa *d_la = nullptr, *d_laout = nullptr;
    uint16_t *d_trslots = nullptr, *d_trout = nullptr;
    unsigned long long *d_counters = nullptr, *d_summary = nullptr;
    dhtile::Cold *d_cold = nullptr;
    DhLa *d_la2 = nullptr, *d_laout2 = nullptr;
    uint16_t *d_trslots2 = nullptr, *d_trout2 = nullptr;
    uint32_t *d_nla2 = nullptr, *d_ntr2 = nullptr;
    uint8_t *d_app = nullptr, *d_arcpp = nullptr;  // plane-packed copies of A (B'' of the transposed pairs)
    // the mapping join across chunks
    bool mj_skip_chunk = false;  // the chunk at hand overflowed a capacity of the join: directory path for it
    uint32_t *d_mjctr_last = nullptr;
    int64_t mj_exp_ent_last = 0, mj_npages_last = 0;
    std::vector<int32_t> h_ncand, h_nhits;
    int64_t nchunk_done = 0;
    std::function<int()> deferred;  // the previous chunk's device-to-host copy and hook, see the chunk loop
    // device time of the stages, host wall of the call (w_g: the chunk loop's phases; DH_TRACE)
    float ms_seed = 0, ms_wave = 0, ms_gather = 0;
    double w_index = 0, w_loop = 0, w_post = 0, w_c = 0;
    double w_g[6] = {0, 0, 0, 0, 0, 0};

    AlignRun(dh_ctx *ctx_, dh_db *A_, dh_db *B_, const dh_align_opts &o_, int32_t first_, int32_t count_, int32_t want_best_,
             int32_t want_sorted_, const ChunkHook *hook_)
        : ctx(ctx_), A(A_), B(B_), o(o_), first(first_), count(count_), want_best(want_best_), want_sorted(want_sorted_),
          hook(hook_), st(ctx_->stream), near_ppm(dh_ctx_near_best_ppm(ctx_)),
          tasks{ctx_->cstream, {}}, tiled(o_.algo == 1), nitems_total(2ll * count_), item_first(2ll * first_),
          item_end(2ll * first_ + 2ll * count_)
    {
    }
    void lap(int i)
    {
        const double t = now_ms();
        w_g[i] += t - w_c;
        w_c = t;
    }
};

// one chunk of items [item0, item0 + ni)
struct AlignChunk {
    int64_t item0;
    int32_t ni;
    MjView mv = {};
    bool mj_planned = false;
    ChunkCopies cc;
    uint8_t *d_bpk2 = nullptr, *d_brcpk2 = nullptr;  // the chunk's 2-bit copies, kept for the transposed pairs
    bool packed = false;
    // per-chunk arrays are indexed by absolute item inside the kernels: the bases shifted
    DhCand *candbase = nullptr;
    DhLa *labase = nullptr;
    uint16_t *trbase = nullptr;
    int32_t *ncandbase = nullptr, *nhitsbase = nullptr, *nlabase = nullptr, *ntrbase = nullptr;
    // symmetric all-vs-all: work units, candidate slots, record slots
    void *d_units = nullptr;
    uint32_t *d_candoff = nullptr;
    int32_t *d_reclist = nullptr;
    int64_t nrec_slots = 0;
};

static IndexView index_view(const dh_db *A)
{
    return IndexView{A->ix.d_fat, A->ix.d_ent, A->ix.d_goff, A->ix.d_page_seq, A->ix.n,
                     A->ix.na,    A->ix.sepv,   A->ix.shift,  A->ix.pbits};
}

#define SCR(id, ptr, count)                                                                      \
    if (int rc_ = dh_scratch(ctx, id, sizeof(*ptr) * std::max<size_t>((size_t)(count), 1), (void **)&ptr)) return rc_;

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

// ---- a grouped DB against itself (the pile-up all-vs-all): the seeds come from the per-pile-up k-mer join
// (dh_join.hip) -- no k-mer directory is built, no line of HBM is looked up at random; bit-identical hits.
// Plan: slices per group (about JOIN_FILL entries each), part blocks (JP_THREADS chunks of one group each), the
// rows of the two tables.  DH_NO_JOIN=1 forces the directory path (tests compare the two).
struct JoinPlan {
    std::vector<int32_t> gfirst, gns, pfirst;
    std::vector<int2> pblk, jblk;
    std::vector<int64_t> psubrow, segrow;
    int64_t npsub = 0, nseg = 0;
};
static void plan_join(AlignRun &r, JoinPlan &jp)
{
    const dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    bool use_join = A == B && A->d_group && A->ngroups >= 1 && o.k <= 16 && B->max_len < JOIN_MAX_LEN && r.first == 0 &&
                    r.count == B->n && B->n > 0 && !getenv("DH_NO_JOIN");
    if (use_join) {
        const int32_t ng = A->ngroups;
        jp.gfirst.assign((size_t)ng + 1, 0);
        for (int32_t s2 = 0; s2 < A->n && use_join; s2++) {
            if (s2 > 0 && A->h_group[(size_t)s2] < A->h_group[(size_t)s2 - 1]) use_join = false;  // groups must be contiguous
            jp.gfirst[(size_t)A->h_group[(size_t)s2] + 1]++;
        }
        for (int32_t g2 = 0; g2 < ng; g2++) jp.gfirst[(size_t)g2 + 1] += jp.gfirst[(size_t)g2];
        jp.gns.assign((size_t)ng, 1);
        jp.pfirst.assign((size_t)ng + 1, 0);
        jp.segrow.assign((size_t)A->n, 0);
        for (int32_t g2 = 0; g2 < ng && use_join; g2++) {
            const int32_t r0 = jp.gfirst[(size_t)g2], r1 = jp.gfirst[(size_t)g2 + 1];
            if (r1 - r0 > JOIN_MAX_READS) use_join = false;
            int64_t nkm = 0, nch = 0;
            for (int32_t r = r0; r < r1; r++) {
                const int64_t np_ = A->h_off[(size_t)r + 1] - A->h_off[(size_t)r] - o.k + 1;
                if (np_ > 0) {
                    nkm += np_;
                    nch += (np_ + JP_PER - 1) / JP_PER;
                }
            }
            const int64_t ns = std::max<int64_t>(1, (nkm / std::max(1, o.kmer_mod) + JOIN_FILL - 1) / JOIN_FILL);
            if (ns > JOIN_MAX_SLICES) use_join = false;
            jp.gns[(size_t)g2] = (int32_t)ns;
            for (int64_t c0 = 0; c0 < nch; c0 += JP_THREADS) {
                jp.pblk.push_back(int2{g2, (int32_t)c0});
                jp.psubrow.push_back(jp.npsub);
                jp.npsub += ns;
            }
            jp.pfirst[(size_t)g2 + 1] = (int32_t)jp.pblk.size();
            if (nch > 0)
                for (int32_t s2 = 0; s2 < (int32_t)ns; s2++) jp.jblk.push_back(int2{g2, s2});
            for (int32_t r = r0; r < r1; r++) {
                jp.segrow[(size_t)r] = jp.nseg;
                jp.nseg += ns;
            }
        }
        if (jp.pblk.size() > (size_t)INT32_MAX / 2 || jp.jblk.size() > (size_t)INT32_MAX / 2) use_join = false;
    }
    r.use_join = use_join;
}

// the chunk size and the copies of A and B that live with the DBs
static int prepare_dbs(AlignRun &r)
{
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    // B's derived copies (reverse complement, 2-bit packed) live with the DB when the whole DB is
    // one chunk of this call (pile-up and template DBs are re-aligned several times); a block of a
    // larger DB gets them chunk by chunk in the scratch arena, so the resident footprint of a reads
    // DB stays at one byte per base however large it is
    // items per launch.  k_tile runs one alignment per lane: a launch needs several alignments per
    // resident lane (262 144 of them) to keep the wavefronts full until the queue drains -- measured on
    // configs[2]: 2^18 items per launch 70 ms of k_tile per step, 2^20 37 ms (the host filters of a chunk
    // still overlap the next chunk's kernels)
    int32_t chunk = o.algo == 1 ? 1 << 20 : 1 << 18;
    if (const char *e = getenv("DH_ALIGN_CHUNK")) chunk = std::max(2, atoi(e)) & ~1;
    // symmetric mode writes records into the slots of other items: everything is one chunk
    if (o.skip_self == 2) {
        if (r.first != 0 || r.count != B->n) return fail(DH_EINVAL, "symmetric mode needs the whole DB");
        chunk = (int32_t)std::min<int64_t>(std::max<int64_t>(r.nitems_total, 2), INT32_MAX - 1);
    }
    r.chunk = chunk;
    // (DH-2 reads B from plane-packed copies made chunk by chunk in the scratch arena)
    r.db_copies = !r.tiled && (A == B || (r.first == 0 && r.count == B->n && r.nitems_total <= chunk));
    r.want_packed = !getenv("DH_WAVE_BYTES");
    // the wave kernel slides over 2-bit packed copies unless a DB holds codes outside 0..3
    if (int rc = dh_ensure_packed(A, false)) return rc;
    if (r.db_copies) {
        if (int rc = dh_ensure_rc(B)) return rc;
        if (int rc = dh_ensure_packed(B, true)) return rc;
    }
    // up to 30 live diagonals fit a 32-lane half: two alignments per wavefront (k_wave2); its
    // reverse extensions run forward over the reverse complements, so A needs one as well
    r.dual = r.tiled || (o.width <= 30 && !getenv("DH_WAVE_SINGLE"));
    if (r.dual) {
        if (int rc = dh_ensure_rc(A)) return rc;
        if (A->has_n == 0)
            if (int rc = dh_ensure_packed(A, true)) return rc;
    }
    if (r.tiled && (A->has_n != 0 || !A->d_pk || !A->d_rcpk))
        return fail(DH_EINVAL, "algo 1 (DH-2) needs sequences of a, c, g, t only (2-bit copies), A holds other codes");
    return DH_OK;
}

// capacity planning and the scratch buffers of the call
static int alloc_scratch(AlignRun &r)
{
    dh_ctx *ctx = r.ctx;
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    const int64_t nitems_total = r.nitems_total;
    const int64_t maxext =
        std::min<int64_t>(A->max_len, (int64_t)B->max_len + (2ll * B->max_len + o.xdrop) / (o.pen - 1) + 1);
    r.nbmax = (int32_t)(maxext / o.tspace + 3);
    r.trmax = 2 * (2 * r.nbmax + 2);
    const int32_t nbmax = r.nbmax, trmax = r.trmax;
    // resident alignment slots: one per wavefront of k_wave (<= 64 VGPRs -> 8 waves/SIMD), one per
    // 32-lane half of k_wave2 (two per wavefront, 6 waves/SIMD)
    // alignments per wavefront of k_wave2: 2 (32 lanes each, width <= 30) or 4 (16 lanes, width <= 14)
    r.per_wave = (o.width <= 14 && !getenv("DH_WAVE_G32")) ? 4 : 2;
    int32_t slots_per_cu = 32;
    // k_wave2: 80 VGPRs -> 6 waves/SIMD = 24 wavefronts per CU (two per wavefront); 96 VGPRs -> 5 waves/SIMD = 20 (four)
    if (o.width <= 30) slots_per_cu = r.per_wave == 4 ? 20 * 4 : 24 * 2;
    if (const char *e = getenv("DH_WAVE_SLOTS_PER_CU")) slots_per_cu = std::max(4, atoi(e)) & ~3;
    // trace-node pool of one alignment slot.  k_wave2: every lane of the group owns a stretch (a lane
    // crosses each boundary of either grid at most once per diagonal it serves; twice that is the
    // capacity, an overflow is reported); k_wave: one shared pool
    r.poolcap = r.dual ? (64 / r.per_wave) * (4 * nbmax + 8) : 96 * nbmax;
    r.nslots = r.tiled ? 4 : (int32_t)std::min<int64_t>((int64_t)ctx->ncu * slots_per_cu,
                                                        (std::max<int64_t>(nitems_total, 4) + 3) & ~3ll);
    // DH-2: one alignment per lane; wavefronts resident = CUs x waves per CU, no more than the items need
    if (r.tiled) {
        // symmetric launches spend most of a wavefront's time waiting on the records and scratch of short alignments:
        // all 16 wavefronts the registers allow (configs[2]: pile-up launch -2.5 ms against 12; mapping +1 ms with 16)
        int32_t per_cu = o.skip_self == 2 ? 16 : dhk_tile_waves_per_cu();
        if (const char *e = getenv("DH_TILE_WAVES_PER_CU")) per_cu = std::max(1, atoi(e));
        if (o.skip_self == 2)
            if (const char *e = getenv("DH_TILE_SYM_WAVES_PER_CU")) per_cu = std::max(1, atoi(e));  // development
        // (symmetric mode: the work units are groups of candidates, many per item -- a pile-up read meets every other
        // read of its pile-up -- so the items do not bound the lanes that find work)
        const int64_t lanes_wanted = o.skip_self == 2 ? nitems_total * (int64_t)o.max_cand : nitems_total;
        r.tile_waves = (int32_t)std::min<int64_t>((int64_t)ctx->ncu * per_cu, (std::max<int64_t>(lanes_wanted, 1) + 63) / 64);
    }
    r.cn = (int32_t)std::min<int64_t>(r.chunk, std::max<int64_t>(nitems_total, 2));
    const int32_t cn = r.cn;
    SCR(SLOT_CAND, r.d_cand, (size_t)cn * o.max_cand)
    SCR(SLOT_NCAND, r.d_ncand, cn)
    SCR(SLOT_NHITS, r.d_nhits, cn)
    SCR(SLOT_STATUS, r.d_status, DH_STW_COUNT)
    r.d_status += DH_STW_STATUS;  // the call's own word of the slot; the packers use the others
    SCR(SLOT_NLA, r.d_nla, cn + 1)
    SCR(SLOT_NTR, r.d_ntr, cn + 1)
    SCR(SLOT_POOL, r.d_pool, (size_t)r.nslots * r.poolcap)
    SCR(SLOT_CDJ, r.d_cdj, (size_t)r.nslots * 8 * nbmax)
    SCR(SLOT_QUEUE, r.d_queue, 4)
    // (symmetric DH-2 launches keep their records in candidate-indexed slots, sized once the candidates are counted)
    r.sym_tiled = r.tiled && o.skip_self == 2;
    // want_sorted & 8 (dh_map_reads): the trace values of every chunk stay on the device in a buffer the result owns
    r.keep_dev = (r.want_sorted & 8) && r.hook && r.tiled && !r.res2 && !r.sym_tiled;
    if (!r.sym_tiled) {
        SCR(SLOT_LA, r.d_la, (size_t)cn * o.max_la)
        SCR(SLOT_TRSLOTS, r.d_trslots, (size_t)cn * o.max_la * trmax)
    }
    SCR(SLOT_COUNTERS, r.d_counters, 2)
    SCR(SLOT_SUMS, r.d_sums, (size_t)cn / 2048 + 4)
    SCR(SLOT_SUMMARY, r.d_summary, 4)
    SCR(SLOT_OVF, r.d_ovf, cn)
    if (r.tiled) SCR(SLOT_REGS, r.d_regs, (size_t)r.tile_waves * 64 * dhtile::MAXREG * dhtile::REGF)
    if (r.tiled) SCR(SLOT_COLD, r.d_cold, (size_t)r.tile_waves * 64)
    if (r.res2) {
        SCR(SLOT_LA2, r.d_la2, (size_t)cn * o.max_la)
        SCR(SLOT_TRSLOTS2, r.d_trslots2, (size_t)cn * o.max_la * trmax)
        SCR(SLOT_NLA2, r.d_nla2, cn + 1)
        SCR(SLOT_NTR2, r.d_ntr2, cn + 1)
        const size_t awords = (size_t)((A->total + 31) / 32), abytes = awords * 8 + 2 * PK_PAD;
        SCR(SLOT_A_PLANES, r.d_app, abytes)
        SCR(SLOT_A_RC_PLANES, r.d_arcpp, abytes)
        HIPCHK(hipMemcpyAsync(r.d_app, A->d_pk_alloc, abytes, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(r.d_arcpp, A->d_rcpk_alloc, abytes, hipMemcpyDeviceToDevice, st));
        dhk_pk2planes(st, r.d_app + PK_PAD, (int64_t)awords);
        dhk_pk2planes(st, r.d_arcpp + PK_PAD, (int64_t)awords);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(r.d_status, 0, sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(r.d_counters, 0, 2 * sizeof(unsigned long long), st));
    return DH_OK;
}

// the capacity (hits) of the first attempt of the pile-up join: rate x margin x sum over groups of bases x reads (see
// DH_JOIN_HIT_RATE0, dh_internal.h), twice that when both directions of a pair are hits (skip_self other than 2); never
// below what every call got before depth was looked at -- max(2^20, 1.25 x bases): a call that fitted then fits now --
// and, that floor apart, never above DH_JOIN_HIT_MEM_FRACTION of the free device memory
extern "C" int64_t dh_join_hit_capacity(const int64_t *bases, const int32_t *reads, int32_t ngroups, int32_t skip_self,
                                        double rate, int64_t free_bytes)
{
    if (!(rate > 0)) rate = DH_JOIN_HIT_RATE0;
    int64_t total = 0;
    double depth_bases = 0;
    for (int32_t g = 0; bases && reads && g < ngroups; g++)
        if (bases[g] > 0 && reads[g] > 0) {
            total += bases[g];
            depth_bases += (double)bases[g] * (double)reads[g];
        }
    const int64_t floor_cap = std::max<int64_t>(1 << 20, (int64_t)(1.25 * (double)total));
    // (a first hit has 40 bits in a segtab word)
    const double want = std::min(rate * depth_bases * (skip_self == 2 ? 1.0 : 2.0) * DH_JOIN_HIT_MARGIN, (double)(1ll << 39));
    int64_t cap = std::max(floor_cap, (int64_t)want);
    if (free_bytes >= 0)
        cap = std::min(cap, std::max(floor_cap, (int64_t)(DH_JOIN_HIT_MEM_FRACTION * (double)free_bytes) / (int64_t)sizeof(uint64_t)));
    return cap;
}

// the pile-up join: one upload of the plan tables, k_join_part, then k_join until its hits fit (r.jv); a slice that
// overflows its LDS table sends the whole call to the directory path (r.use_join = false, the index rebuilt)
static int build_join(AlignRun &r, const JoinPlan &jp)
{
    dh_ctx *ctx = r.ctx;
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    JoinView &jv = r.jv;
    // one upload of the plan tables; device buffers from the scratch arena
    const size_t ng = (size_t)A->ngroups;
    size_t blob_bytes = 0;
    auto place = [&](size_t bytes) {
        const size_t at = blob_bytes;
        blob_bytes += (bytes + 15) & ~(size_t)15;
        return at;
    };
    const size_t o_gfirst = place(sizeof(int32_t) * (ng + 1)), o_gns = place(sizeof(int32_t) * ng),
                 o_pfirst = place(sizeof(int32_t) * (ng + 1)), o_pblk = place(sizeof(int2) * jp.pblk.size()),
                 o_psubrow = place(sizeof(int64_t) * jp.psubrow.size()), o_jblk = place(sizeof(int2) * jp.jblk.size()),
                 o_segrow = place(sizeof(int64_t) * jp.segrow.size());
    std::vector<uint8_t, PinnedAlloc<uint8_t>> blob(blob_bytes);
    memcpy(blob.data() + o_gfirst, jp.gfirst.data(), sizeof(int32_t) * (ng + 1));
    memcpy(blob.data() + o_gns, jp.gns.data(), sizeof(int32_t) * ng);
    memcpy(blob.data() + o_pfirst, jp.pfirst.data(), sizeof(int32_t) * (ng + 1));
    if (!jp.pblk.empty()) memcpy(blob.data() + o_pblk, jp.pblk.data(), sizeof(int2) * jp.pblk.size());
    if (!jp.psubrow.empty()) memcpy(blob.data() + o_psubrow, jp.psubrow.data(), sizeof(int64_t) * jp.psubrow.size());
    if (!jp.jblk.empty()) memcpy(blob.data() + o_jblk, jp.jblk.data(), sizeof(int2) * jp.jblk.size());
    memcpy(blob.data() + o_segrow, jp.segrow.data(), sizeof(int64_t) * jp.segrow.size());
    uint8_t *d_blob;
    uint32_t *d_psub;
    uint64_t *d_entries, *d_segtab, *d_hits;
    unsigned long long *d_cursor;
    SCR(SLOT_JOIN_BLOB, d_blob, blob_bytes)
    SCR(SLOT_JOIN_PSUB, d_psub, (size_t)jp.npsub)
    SCR(SLOT_JOIN_ENTRIES, d_entries, jp.pblk.size() * (size_t)JP_POS)
    SCR(SLOT_JOIN_SEGTAB, d_segtab, (size_t)jp.nseg)
    SCR(SLOT_JOIN_CURSOR, d_cursor, 4)  // [0] the hit cursor; [1..2] = four 32-bit counters of k_join_hist
    HIPCHK(hipMemcpyAsync(d_blob, blob.data(), blob_bytes, hipMemcpyHostToDevice, st));
    jv.gfirst = (const int32_t *)(d_blob + o_gfirst);
    jv.gns = (const int32_t *)(d_blob + o_gns);
    jv.pfirst = (const int32_t *)(d_blob + o_pfirst);
    jv.pblk = (const int2 *)(d_blob + o_pblk);
    jv.psubrow = (const int64_t *)(d_blob + o_psubrow);
    jv.jblk = (const int2 *)(d_blob + o_jblk);
    jv.segrow = (const int64_t *)(d_blob + o_segrow);
    jv.psub = d_psub;
    jv.entries = d_entries;
    jv.segtab = d_segtab;
    jv.cursor = d_cursor;
    jv.status = r.d_status;
    jv.npart = (int32_t)jp.pblk.size();
    jv.njoin = (int32_t)jp.jblk.size();
    // reads of groups without k-mers have no join block: their rows read as "no hits"
    HIPCHK(dhk_memset(st, d_segtab, 0, sizeof(uint64_t) * (size_t)std::max<int64_t>(jp.nseg, 1)));
    HIPCHK(hipEventRecord(ctx->ev[6], st));
    dhk_join_part(st, jv, r.bv, o.k, o.kmer_mod);
    HIPCHK(hipGetLastError());
    // hit buffer: sized by pile-up depth with the rate this context has learned (dh_join_hit_capacity); a join whose hits
    // do not fit leaves the size it needs in the cursor and is rerun with exactly that
    std::vector<int64_t> gbases(ng);
    std::vector<int32_t> greads(ng);
    double depth_bases = 0;
    for (size_t g = 0; g < ng; g++) {
        const int32_t r0 = jp.gfirst[g], r1 = jp.gfirst[g + 1];
        gbases[g] = A->h_off[(size_t)r1] - A->h_off[(size_t)r0];
        greads[g] = r1 - r0;
        depth_bases += (double)gbases[g] * (double)greads[g];
    }
    if (o.skip_self != 2) depth_bases *= 2.0;  // both directions of a pair are hits
    int64_t hcap = dh_join_hit_capacity(gbases.data(), greads.data(), (int32_t)ng, o.skip_self, ctx->join_hit_rate, -1);
    const size_t have = ctx->arena[SLOT_JOIN_HITS].cap / sizeof(uint64_t);
    if ((size_t)hcap > have) {  // the buffer has to grow: no more than its share of the memory that is free now
        size_t free_b = 0, total_b = 0;
        HIPCHK(hipMemGetInfo(&free_b, &total_b));
        const int64_t clamped = dh_join_hit_capacity(gbases.data(), greads.data(), (int32_t)ng, o.skip_self, ctx->join_hit_rate,
                                                     (int64_t)free_b);
        hcap = std::max(clamped, std::min(hcap, (int64_t)have));
    }
    if (const char *e = getenv("DH_JOIN_HITCAP")) hcap = std::max<int64_t>(1, atoll(e));  // development / tests
    ctx->join_first_cap = hcap;
    int attempt = 0;
    for (;; attempt++) {
        SCR(SLOT_JOIN_HITS, d_hits, (size_t)hcap)
        jv.hits = d_hits;
        jv.hits_cap = hcap;
        HIPCHK(hipMemsetAsync(d_cursor, 0, sizeof(unsigned long long), st));
        dhk_join(st, jv, r.bv, r.dopt, A->ix.d_goff, r.sepv);
        HIPCHK(hipGetLastError());
        ctx->join_launches++;
        if (attempt > 0) ctx->join_reruns++;
        // the histogram reads segtab only, which k_join fills whether the hits fitted or not: it goes right behind, and
        // cursor, histogram and status come back in one wait (a join that is rerun or abandoned discards the histogram)
        dhk_join_hist(st, jv, B->d_group, B->n, (unsigned int *)(d_cursor + 1));
        HIPCHK(hipGetLastError());
        struct {
            unsigned long long cur;
            unsigned int hist[4];
        } back = {0, {0, 0, 0, 0}};
        static_assert(sizeof(back) == 3 * sizeof(unsigned long long), "cursor and histogram words are one copy");
        int32_t jstatus = 0;
        HIPCHK(hipMemcpyAsync(&back, d_cursor, sizeof(back), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&jstatus, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipEventRecord(ctx->ev[7], st));
        HIPCHK(hipStreamSynchronize(st));
        r.join_hits = (int64_t)back.cur;
        if (jstatus & DH_ST_JOIN_OVERFLOW) {  // a slice did not fit its LDS table: directory path for this call
            r.use_join = false;
            break;
        }
        ctx->join_last_hits = (int64_t)back.cur;
        if (depth_bases > 0) ctx->join_hit_rate = std::max(ctx->join_hit_rate, (double)back.cur / depth_bases);
        if (!(jstatus & DH_ST_JOIN_HITCAP)) {
            memcpy(r.jhist, back.hist, sizeof(r.jhist));
            break;
        }
        if (attempt >= 2) return fail(DH_EOVERFLOW, "k-mer join: hit buffer capacity exceeded twice");
        hcap = (int64_t)back.cur + 1024;
        HIPCHK(hipMemsetAsync(r.d_status, 0, sizeof(int32_t), st));
    }
    HIPCHK(hipEventElapsedTime(&r.ms_join, ctx->ev[6], ctx->ev[7]));
    if (getenv("DH_TRACE"))
        fprintf(stderr, "[join] hit buffer %lld (%.1f MB), %lld hits, %d attempt(s); %.4f hits per base per read of depth from now on\n",
                (long long)ctx->join_first_cap, (double)ctx->join_first_cap * sizeof(uint64_t) / 1048576.0, (long long)r.join_hits,
                attempt + 1, ctx->join_hit_rate);
    if (!r.use_join) {
        if (getenv("DH_TRACE")) fprintf(stderr, "[join] a slice overflowed its table: falling back to the k-mer directory\n");
        HIPCHK(hipMemsetAsync(r.d_status, 0, sizeof(int32_t), st));
        if (int rc = dh_build_index(A, o.k, r.sepv, o.kmer_mod, false)) return rc;
        r.iv = index_view(A);
    }
    return DH_OK;
}

// the LDS hit capacity of the seed filter; whether the mapping goes by the partitioned join (and its presence bitmap)
static void ctx_count_tj_fallback(dh_ctx *ctx)
{
    ctx->tj_fallbacks++;
    if (getenv("DH_TRACE")) fprintf(stderr, "[tjoin] a limit of the table join is not met: this call keeps the k-mer directory\n");
}
static int plan_seeds(AlignRun &r)
{
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    // expected hits per read (both strands share the LDS buffer): random matches + true seeds (measured
    // 0.075 per sampled k-mer for 15 % error reads at k = 20; reads that need more are redone with their
    // hits in HBM, and a chunk with many of them restarts with the next capacity); pick the LDS hit capacity
    // (ix.n = indexed k-mers; a sampled k-mer of B meets ix.n / (4^k / kmer_mod) of them by chance)
    r.dens = (double)A->ix.n * std::max(1, o.kmer_mod) / std::pow(4.0, o.k) / std::max(1, A->ngroups);
    const double exp_hits = (double)B->max_len / std::max(1, o.kmer_mod) * (2.0 * r.dens + 0.1);
    int cap = 1024;
    while (cap < 16384 && exp_hits * 1.5 >= cap) cap *= 2;
    if (A == B) {
        // all-vs-all inside pile-ups: a read shares k-mers with every other read of its group; measured
        // ~0.5 hits per base, and the 2048-entry variant (8 blocks per CU) with a few items redone from
        // HBM beats the 8192-entry one by 40 %
        cap = 1024;
        while (cap < 8192 && 0.6 * B->max_len > cap) cap *= 2;
    }
    if (r.use_join) {
        // the hits are counted already (a whole second pass with the next size cost 9.5 ms at configs[2] when the guess
        // was one size short)
        // (tiers: reads above the first capacity are redone by the 8192-entry variant, reads above that from HBM -- so
        // the first tier is the smallest one that serves at least 70 % of the reads)
        const unsigned int tol = (unsigned int)(0.3 * B->n);
        cap = r.jhist[0] <= tol ? 2048 : (r.jhist[1] <= tol ? 4096 : (r.jhist[2] <= tol ? 8192 : 16384));
    }
    if (const char *e = getenv("DH_SEED_CAP")) cap = atoi(e);  // development: 1024 .. 16384, power of two
    r.cap = cap;
    // ---- a mapping pass (A != B, ungrouped): the seeds of a chunk of reads come from the radix-partitioned k-mer join
    // (dh_mjoin.h) -- the reads' k-mers binned by directory slice, every slice joined on chip -- instead of one random
    // directory line per k-mer; bit-identical hits.  Small chunks keep the directory path (the join's fixed costs: 1 024
    // partitions, a page per wavefront); DH_NO_MJOIN=1 forces it, DH_MJOIN_MIN sets the threshold (bases of a chunk).
    r.use_mj = !r.use_join && A != B && !A->d_group && A->ngroups == 1 && !B->d_group && o.k >= MJ_MINK && o.k <= MJ_MAXK &&
               o.skip_self == 0 && r.want_packed && A->ix.n > 0 && A->ix.n < (1ll << 28) && !getenv("DH_NO_MJOIN");
    r.mj_min_bases = 64ll << 20;
    if (const char *e = getenv("DH_MJOIN_MIN")) r.mj_min_bases = atoll(e);
    if (r.use_mj && !A->ix.d_bitmap) {
        // about 16 buckets per indexed k-mer (7 % of the looked-up k-mers then pass the filter without being in A)
        int32_t nbbits = std::min(MJ_MAXBITS, std::min(2 * o.k, std::max(MJ_PBITS + 5, dh_ceil_log2((uint64_t)A->ix.n) + 4)));
        const size_t words = (size_t)1 << (nbbits - 5);
        HIPCHK(dh_dev_alloc(&A->ix.d_bitmap, sizeof(uint32_t) * words));
        HIPCHK(dhk_memset(r.st, A->ix.d_bitmap, 0, sizeof(uint32_t) * words));
        dhk_mj_bitmap(r.st, A->ix.d_ent, A->ix.n, o.k, nbbits, A->ix.d_bitmap);
        HIPCHK(hipGetLastError());
        A->ix.nbbits = nbbits;
    }
    // ---- a grouped A against a grouped B (the consensus re-alignment: templates against the reads of their pile-ups): a
    // read only meets the index entries of its own group, which k_tjoin (dh_tjoin.h) holds in LDS -- bit-identical hits.
    // A call that does not meet the limits keeps the directory and is counted; DH_NO_TJOIN=1 forces the directory,
    // DH_TJOIN_CAP lowers the entries per group the table is planned for (tests: the fall-back).
    if (!r.use_join && A != B && A->d_group && !getenv("DH_NO_TJOIN")) {
        int64_t tcap_ent = TJ_CAP;
        if (const char *e = getenv("DH_TJOIN_CAP")) tcap_ent = std::max<int64_t>(0, std::min<int64_t>(TJ_CAP, atoll(e)));
        // (a group of B without sequences in A, beyond A's last group included, is an empty table to k_tjoin: its reads
        // get no hits, which is what "no template in the pile-up" means; the group ids themselves are the callers' and
        // are the same numbering on both sides)
        r.use_tj = B->d_group && o.k <= TJ_MAXK && o.skip_self == 0 && A->ix.d_gent &&
                   A->ix.max_gent <= tcap_ent && A->ix.n < (1ll << 31) && B->max_len < (1 << 24);
        if (!r.use_tj) ctx_count_tj_fallback(r.ctx);
        if (r.use_tj) {
            r.ctx->tj_calls++;
            r.ctx->tj_last_hits = 0;
        }
    }
    return DH_OK;
}

// the partitioned join of a chunk is planned ahead of the chunk's derived copies and of the previous chunk's
// device-to-host copy: its first kernel (k_mj_tile_reads, a binary search per tile) then runs before the copy kernels
// take the device (beside them it took 4 ms instead of 10 us).  c.mj_planned: the chunk goes by the join.
static int plan_mj_chunk(AlignRun &r, AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    const dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    MjView &mv = c.mv;
    const int32_t cr0 = (int32_t)(c.item0 >> 1), cr1 = (int32_t)((c.item0 + c.ni) >> 1);
    const int64_t cb0 = B->h_off[(size_t)cr0], cb1 = B->h_off[(size_t)cr1];
    if (!r.use_mj || r.mj_skip_chunk || cb1 - cb0 < r.mj_min_bases || cb1 - cb0 >= (1ll << 40)) return DH_OK;
    mv.c0 = cb0;
    mv.c1 = cb1;
    mv.r0 = cr0;
    mv.r1 = cr1;
    mv.k = o.k;
    mv.kmer_mod = std::max(1, o.kmer_mod);
    mv.nbbits = A->ix.nbbits;
    // bases per tile: 13/16 of the tile's capacity expected (modimer sampling is a hash), every
    // lane of the block rolls the same number of positions, positions fit MJ_POSBITS
    // (a wavefront stages its eighth of the tile's entries in its own 1 024 slots: 832 expected, 7 sigma of slack)
    int64_t tb = (int64_t)(MJ_CAP / 16 * 13) * mv.kmer_mod;
    if (mv.kmer_mod == 1) tb = MJ_CAP;
    tb = std::min<int64_t>(tb, (1 << MJ_POSBITS) - 64);
    tb = std::max<int64_t>(MJ_THREADS * 8, tb / (MJ_THREADS * 8) * (MJ_THREADS * 8));
    mv.tb = (int32_t)tb;
    const int64_t ntiles = (cb1 - cb0 + tb - 1) / tb;
    mv.ntiles = (int32_t)ntiles;
    mv.ntiles_pad = (int32_t)((ntiles + MJ_BATCH - 1) / MJ_BATCH * MJ_BATCH);
    mv.ngroups = mv.ntiles_pad / MJ_GROUP;
    const int64_t tbg = tb * MJ_GROUP;
    mv.nseg = (int32_t)((B->max_len + tbg - 1) / tbg + 1);
    // hit pool: 20 % of the sampled k-mers hit (measured 6 % at 13 % error and k = 20; raised when a pool ran out: low-error
    // reads) plus the chance matches, a page per wavefront
    // of the probe kernel on top; the same number of hits regrouped by read
    // (dens: chance matches of a sampled k-mer per strand, as for the LDS capacity above)
    const int64_t exp_ent = (cb1 - cb0) / mv.kmer_mod;
    // (a page is left when less than a quarter of it is free: a third more pages than hits)
    // (the pool holds the SURVIVORS of the filter: the hits' k-mers and a few per cent of the others)
    int64_t npages = (int64_t)(1.34 * (ctx->mj_hit_frac + 0.06 + 2.5 * r.dens) * (double)exp_ent) / MJ_PAGE + (int64_t)ctx->ncu * (MJ_PROBE_THREADS / 64) + 64;
    if (const char *e = getenv("DH_MJOIN_PAGES")) npages = std::max<int64_t>(1, atoll(e));  // development / tests: force the fall-back
    if (ntiles >= (1ll << 30) / MJ_P || npages >= (1ll << 31) / 2 || mv.nseg > 512) return DH_OK;
    mv.npages = (int32_t)npages;
    mv.rcap = npages * MJ_PAGE;
    uint32_t *d_mjctr;
    SCR(SLOT_MJ_ENT, mv.ent, (size_t)ntiles * MJ_CAP)
    SCR(SLOT_MJ_SEGOFF, mv.segoff, (size_t)ntiles * MJ_P)
    SCR(SLOT_MJ_TILE_N, mv.tile_n, (size_t)ntiles)
    SCR(SLOT_MJ_TILE_R, mv.tile_r, (size_t)ntiles)
    SCR(SLOT_MJ_SEG, mv.seg, (size_t)MJ_P * mv.ntiles_pad)
    SCR(SLOT_MJ_HSEG, mv.hseg, (size_t)mv.ngroups * MJ_P)
    SCR(SLOT_MJ_HITS, mv.hits, (size_t)npages * MJ_PAGE)
    SCR(SLOT_MJ_RHITS, mv.rhits, (size_t)mv.rcap)
    SCR(SLOT_MJ_SEGTAB, mv.segtab, (size_t)(cr1 - cr0) * mv.nseg)
    SCR(SLOT_MJ_CTR, d_mjctr, 16)
    mv.ctr = d_mjctr;
    r.d_mjctr_last = d_mjctr;
    r.mj_exp_ent_last = exp_ent;
    r.mj_npages_last = npages;
    mv.bitmap = A->ix.d_bitmap;
    mv.status = r.d_status;
    dhk_mj_tile_reads(r.st, r.bv, mv);
    HIPCHK(hipGetLastError());
    c.mj_planned = true;
    return DH_OK;
}

// the chunk's derived copies of B (plane-packed for DH-2), then the previous chunk's deferred copy and hook
static int copy_chunk(AlignRun &r, AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    dh_db *A = r.A, *B = r.B;
    hipStream_t st = r.st;
    ChunkCopies &cc = c.cc;
    if (r.db_copies) {
        cc.rc = B->d_rc;
        cc.pk = B->d_pk;
        cc.rcpk = B->d_rcpk;
        cc.has_n = B->has_n != 0;
    } else if (int rc = chunk_copies(ctx, B, (int32_t)(c.item0 >> 1), (int32_t)((c.item0 + c.ni) >> 1), r.want_packed, A->has_n != 0,
                                     &cc, r.tiled && r.want_packed && !r.res2 && !getenv("DH_PLANES_BY_PASS")))
        return rc;
    c.packed = r.want_packed && A->has_n == 0 && !cc.has_n && cc.pk && cc.rcpk;
    if (r.tiled) {
        if (!c.packed) return fail(DH_EINVAL, "algo 1 (DH-2) needs sequences of a, c, g, t only (2-bit copies), B holds other codes");
        if (r.res2) {
            // the transposed pairs read this chunk of B as their A'': keep its 2-bit copies
            const size_t pbytes = (size_t)cc.pk_words * 8 + 2 * PK_PAD;
            SCR(SLOT_B_PK2, c.d_bpk2, pbytes)
            SCR(SLOT_B_RC_PK2, c.d_brcpk2, pbytes)
            HIPCHK(hipMemcpyAsync(c.d_bpk2, cc.pk_w0 - PK_PAD, pbytes, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(c.d_brcpk2, cc.rcpk_w0 - PK_PAD, pbytes, hipMemcpyDeviceToDevice, st));
        }
        if (!cc.planes) {
            dhk_pk2planes(st, cc.pk_w0, cc.pk_words);
            dhk_pk2planes(st, cc.rcpk_w0, cc.pk_words);
        }
        HIPCHK(hipGetLastError());
    }
    if (r.deferred) {
        HIPCHK(hipEventRecord(ctx->ev[6], st));
        HIPCHK(hipStreamWaitEvent(ctx->cstream, ctx->ev[6], 0));
        const int rc = r.deferred();
        r.deferred = nullptr;
        if (rc) return rc;
    }
    return DH_OK;
}

// The seeds of a chunk: the first tier of the seed filter (fed by the mapping join, the pile-up join or the directory),
// then the reads that overflowed it -- further tiers of the join path, the rest staged in HBM.  *redo: the chunk has to
// run again (the join's hit pool ran out, a capacity of the join was exceeded, or the directory path doubled its cap).
static int seed_chunk(AlignRun &r, AlignChunk &c, bool *redo)
{
    dh_ctx *ctx = r.ctx;
    const dh_db *B = r.B;
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    const int64_t item0 = c.item0;
    const int32_t ni = c.ni;
    *redo = false;
    // per-chunk arrays are indexed by absolute item inside the kernels: shift the bases
    c.candbase = r.d_cand - item0 * o.max_cand;
    c.labase = r.d_la ? r.d_la - item0 * o.max_la : nullptr;
    c.trbase = r.d_trslots ? r.d_trslots - item0 * (int64_t)o.max_la * r.trmax : nullptr;
    c.ncandbase = r.d_ncand - item0;
    c.nhitsbase = r.d_nhits - item0;
    c.nlabase = (int32_t *)r.d_nla - item0;
    c.ntrbase = (int32_t *)r.d_ntr - item0;
    r.lap(0);
    HIPCHK(hipEventRecord(ctx->ev[2], st));
    HIPCHK(hipMemsetAsync(r.d_queue, 0, 4 * sizeof(uint32_t), st));
    uint64_t *d_fscr = nullptr;
    if (r.cap > 4096 && r.cap <= 8192)
        SCR(SLOT_FSCR, d_fscr, (size_t)ctx->ncu * DH_SEED_FSCR_BLOCKS_PER_CU * DH_SEED_FSCR_WORDS)
    JoinView jv_mj = {};
    bool mj_chunk = false;
    if (c.mj_planned && !c.cc.has_n) {
        const MjView &mv = c.mv;
        HIPCHK(dhk_memset(st, mv.segtab, 0, sizeof(unsigned long long) * (size_t)(mv.r1 - mv.r0) * mv.nseg));
        dhk_mj_run(st, r.bv, r.iv, r.dopt, mv, ctx->ncu);
        HIPCHK(hipGetLastError());
        jv_mj.segtab = (uint64_t *)mv.segtab;
        jv_mj.hits = mv.rhits;
        jv_mj.status = r.d_status;
        jv_mj.ns_fixed = mv.nseg;
        jv_mj.read0 = mv.r0;
        mj_chunk = true;
    }
    // the per-group table join: units (group, run of consecutive reads), count + reserve + write; a hit buffer that was
    // too small is sized by what the cursor counted and the kernel runs again
    JoinView jv_tj = {};
    bool tj_chunk = false;
    unsigned long long tj_hits = 0;
    if (r.use_tj) {
        const int32_t cr0 = (int32_t)(item0 >> 1), cr1 = (int32_t)((item0 + ni) >> 1);
        std::vector<int4> units;
        for (int32_t rd = cr0; rd < cr1;) {
            const int32_t g = B->h_group[(size_t)rd];
            int32_t e = rd + 1;
            while (e < cr1 && e - rd < TJ_RUN && B->h_group[(size_t)e] == g) e++;
            units.push_back(int4{g, rd, e, 0});
            rd = e;
        }
        const int64_t cbases = B->h_off[(size_t)cr1] - B->h_off[(size_t)cr0];
        // first attempt: the hits per base the context has seen (plus a quarter), exact from the cursor after that
        int64_t hcap = (int64_t)(1.25 * ctx->tj_hit_rate * (double)cbases) + 4096;
        if (const char *e = getenv("DH_TJOIN_HITCAP")) hcap = std::max<int64_t>(1, atoll(e));  // development / tests: force the rerun
        TjView tv = {};
        int4 *d_units;
        uint32_t *d_tjctr;
        SCR(SLOT_TJ_UNITS, d_units, units.size())
        SCR(SLOT_TJ_SEGTAB, tv.segtab, (size_t)(cr1 - cr0))
        SCR(SLOT_TJ_CTR, d_tjctr, 4)
        HIPCHK(hipMemcpyAsync(d_units, units.data(), sizeof(int4) * units.size(), hipMemcpyHostToDevice, st));
        tv.gent = r.A->ix.d_gent;
        tv.ngroups = r.A->ngroups;
        tv.units = d_units;
        tv.nunits = (int32_t)units.size();
        tv.read0 = cr0;
        tv.cursor = (unsigned long long *)d_tjctr;
        tv.queue = d_tjctr + 2;
        tv.status = r.d_status;
        int32_t tst = 0;
        for (int attempt = 0;; attempt++) {
            SCR(SLOT_TJ_HITS, tv.hits, (size_t)hcap)
            tv.hits_cap = hcap;
            HIPCHK(hipMemsetAsync(d_tjctr, 0, 4 * sizeof(uint32_t), st));
            dhk_tjoin(st, r.bv, r.iv, r.dopt, tv, ctx->ncu);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(&tj_hits, tv.cursor, sizeof(tj_hits), hipMemcpyDeviceToHost, st));
            HIPCHK(hipMemcpyAsync(&tst, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
            HIPCHK(hipStreamSynchronize(st));  // (units goes out of scope behind this)
            if (!(tst & DH_ST_TJ_HITCAP)) break;
            if (attempt > 0) return fail(DH_EOVERFLOW, "table join: the hit buffer sized by the count pass was too small");
            tst &= ~DH_ST_TJ_HITCAP;
            HIPCHK(hipMemcpyAsync(r.d_status, &tst, sizeof(int32_t), hipMemcpyHostToDevice, st));
            if (getenv("DH_TRACE")) fprintf(stderr, "[tjoin] hit buffer of %lld too small for %llu hits: run again\n", (long long)hcap, tj_hits);
            hcap = (int64_t)tj_hits;
            ctx->tj_reruns++;
        }
        // the next first attempt goes by what this call produced, never below the starting figure: one low-error call
        // (0.87 hits per base at 1 %) does not make every later buffer of the context six times larger at 8 bytes per
        // hit -- a call after it that needs more than it left pays one rerun
        if (cbases > 0) ctx->tj_hit_rate = std::max(DH_TJ_HIT_RATE0, (double)tj_hits / (double)cbases);
        if (tst & DH_ST_TJ_OVERFLOW) {
            // (a read with 2^24 hits or more: nothing the segment word can describe) the whole call by the directory
            tst &= ~DH_ST_TJ_OVERFLOW;
            HIPCHK(hipMemcpyAsync(r.d_status, &tst, sizeof(int32_t), hipMemcpyHostToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
            r.use_tj = false;
            ctx->tj_calls--;
            ctx_count_tj_fallback(ctx);
            *redo = true;
            return DH_OK;
        }
        jv_tj.segtab = tv.segtab;
        jv_tj.hits = tv.hits;
        jv_tj.status = r.d_status;
        jv_tj.ns_fixed = 1;
        jv_tj.read0 = cr0;
        tj_chunk = true;
    }
    const bool jn = r.use_join || mj_chunk || tj_chunk;  // the back end gathers its hits from segments
    const JoinView &jvx = mj_chunk ? jv_mj : (tj_chunk ? jv_tj : r.jv);
    // (the back end fed from segments exists with 2048, 4096 and 8192 entries of LDS; the 8192-entry one scans in a slab)
    const int tier_max = getenv("DH_SEED_NO16K") ? 8192 : 16384;  // development / tests: without the 16384-entry tier
    // (a mapping chunk through the partitioned join starts with the wavefront-per-read tier: 512 hits, 32 candidate band
    // pairs -- 140 hits per read at 1/8 sampling; a block of 512 threads per read kept 3 reads per CU in flight and spent
    // its time in barriers -- then 2048, 8192, 16384 for what overflows; DH_SEED_NO_WAVE_TIER=1: from 2048 as before)
    // The first tier of a mapping chunk goes by the MEAN hits per read -- 0.075 true seeds per sampled k-mer at 13 % error
    // plus the random matches -- with half as much again of room (`cap` above goes by the longest read of the DB: right for
    // the directory path, whose overflowing reads are staged in HBM, two sizes too large here, where the next tiers take
    // them from a list: the unsampled mapping of configs[2] ran all reads through the 4096-entry variant for 1 100 hits per
    // read).  The wavefront-per-read tier is switched off for the context once a quarter of a chunk's reads overflowed it.
    const double kmers_per_read = (double)(B->h_off[(size_t)((item0 + ni) >> 1)] - B->h_off[(size_t)(item0 >> 1)]) /
                                  std::max(1, ni / 2) / std::max(1, o.kmer_mod);
    // (the table join has counted its hits: the mean is known)
    const double mean_hits = tj_chunk ? (double)tj_hits / std::max(1, ni / 2) : kmers_per_read * (2.0 * r.dens + 0.075);
    const bool wave_tier = (mj_chunk || tj_chunk) && ctx->seed_wave_tier && 1.5 * mean_hits <= 512.0 && !getenv("DH_SEED_NO_WAVE_TIER");
    int capj = std::min(std::max(r.cap, 2048), tier_max);
    if (mj_chunk || tj_chunk) {
        capj = 2048;
        while (capj < tier_max && 1.5 * mean_hits > capj) capj *= 2;
        if (wave_tier) capj = 512;
    }
    // (an unsampled mapping -- 925 hits per 15 kb read, 1.5 x the mean above 512 -- takes the middle tier: 2048 hits, four
    // wavefronts per read and 64 candidate band pairs, five blocks per CU where the 512-thread block keeps three.  A read
    // with more hits or more band pairs is marked like an overflow of the wavefront tier and redone from the list by the
    // 512-thread tiers; the context stops using the tier once a quarter of a chunk's reads were.  A block gathers one
    // segment per thread.  DH_SEED_NO_MID_TIER=1: the 512-thread block as before)
    const bool mid_tier = (mj_chunk || tj_chunk) && !wave_tier && capj == 2048 && ctx->seed_mid_tier &&
                          (!mj_chunk || c.mv.nseg <= 256) && !getenv("DH_SEED_NO_MID_TIER");
    if (jn && capj > 4096) SCR(SLOT_FSCR, d_fscr, (size_t)ctx->ncu * DH_SEED_FSCR_BLOCKS_PER_CU * (capj > 8192 ? DH_SEED_FSCR_WORDS16 : DH_SEED_FSCR_WORDS))
    if (jn)
        dhk_seed_join(st, capj, r.bv, r.iv, r.dopt, jvx, (int32_t)item0, ni, c.candbase, c.ncandbase, c.nhitsbase, r.d_status,
                      r.d_queue + 1, ctx->ncu, d_fscr, nullptr, 0, mid_tier ? 1 : 0);
    else
        dhk_seed(st, r.cap, r.bv, r.iv, r.dopt, (int32_t)item0, ni, c.candbase, c.ncandbase, c.nhitsbase, r.d_status,
                 r.d_queue + 1, ctx->ncu, d_fscr);
    HIPCHK(hipGetLastError());
    // items whose hits did not fit the LDS buffer (ncand == -1) are redone with their hits
    // staged in HBM: same kernel code, capacity = the item's own hit count
    int32_t status = 0;
    unsigned long long sm[4] = {0, 0, 0, 0};
    dhk_seed_summary(st, r.d_ncand, r.d_nhits, ni, r.d_summary);
    HIPCHK(hipMemcpyAsync(&status, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(sm, r.d_summary, sizeof(sm), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (mj_chunk && (status & DH_ST_MJ_POOL) && !(status & DH_ST_MJ_OVERFLOW) && !getenv("DH_MJOIN_PAGES")) {
        // the hit pool ran out (more hits per k-mer than planned: low-error reads, short k-mers): sized by the pages
        // the probe kernel asked for, the chunk runs through the join again -- and the later ones start with that rate
        unsigned long long cnt2[2] = {0, 0};  // hits counted for rhits, survivors that found no page
        HIPCHK(hipMemcpyAsync(cnt2, r.d_mjctr_last + 10, sizeof(cnt2), hipMemcpyDeviceToHost, st));
        status &= ~DH_ST_MJ_POOL;
        HIPCHK(hipMemcpyAsync(r.d_status, &status, sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        const double have = (double)r.mj_npages_last * MJ_PAGE / 1.34;
        const double need = 1.2 * std::max(have + (double)cnt2[1], (double)cnt2[0]) / std::max<double>(1.0, (double)r.mj_exp_ent_last);
        ctx->mj_hit_frac = std::max(ctx->mj_hit_frac * 1.5, need);
        if (getenv("DH_TRACE")) fprintf(stderr, "[mjoin] pool too small (%llu survivors without a page, %llu hits): %.2f per k-mer planned from now on\n", cnt2[1], cnt2[0], ctx->mj_hit_frac);
        if (ctx->mj_hit_frac <= 64.0) {
            *redo = true;
            return DH_OK;
        }
        status |= DH_ST_MJ_OVERFLOW;
    }
    if (mj_chunk && (status & (DH_ST_MJ_OVERFLOW | DH_ST_MJ_POOL))) {
        // a capacity of the partitioned join was exceeded (repeat-rich reads): this chunk again, by the directory
        if (getenv("DH_TRACE")) fprintf(stderr, "[mjoin] a capacity was exceeded: chunk at item %lld redone by the directory path\n", (long long)item0);
        status &= ~(DH_ST_MJ_OVERFLOW | DH_ST_MJ_POOL);
        HIPCHK(hipMemcpyAsync(r.d_status, &status, sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        r.mj_skip_chunk = true;
        ctx->mj_fallbacks++;
        *redo = true;
        return DH_OK;
    }
    std::vector<int32_t> big;
    int32_t gcap = 0;
    if (sm[2] > 0) {  // the per-item arrays travel only when some item overflowed its LDS buffer
        HIPCHK(hipMemcpyAsync(r.h_ncand.data(), r.d_ncand, sizeof(int32_t) * (size_t)ni, hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(r.h_nhits.data(), r.d_nhits, sizeof(int32_t) * (size_t)ni, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int32_t it = 0; it + 1 < ni; it += 2)  // a read overflows with both of its strands
            if (r.h_ncand[(size_t)it] == -1) {
                big.push_back((int32_t)((item0 + it) >> 1));
                gcap = std::max(gcap, r.h_nhits[(size_t)it] + r.h_nhits[(size_t)it + 1]);
            }
    }
    if (wave_tier && big.size() * 4 > (size_t)(ni / 2)) {
        ctx->seed_wave_tier = 0;
        if (getenv("DH_TRACE"))
            fprintf(stderr, "[seeds] %zu of %d reads overflow the wavefront-per-read tier: not used by this context any more\n", big.size(), ni / 2);
    }
    // many items overflow the LDS buffer: the next size is cheaper than HBM staging -- up to 8192; the 16384-entry
    // variant keeps one block per CU resident and pays off only when most items need it
    size_t redo_all = (size_t)ni / 50 + 8;
    if (r.cap >= 8192) redo_all = (size_t)ni / 4;
    if (const char *e = getenv("DH_SEED_BIG_PCT")) redo_all = (size_t)((double)ni * atof(e) / 200.0);  // development (reads = ni / 2)
    if (getenv("DH_TRACE") && !big.empty())
        fprintf(stderr, "[seeds] cap %d: %zu of %d reads overflow (whole chunk again above %zu)\n", r.cap, big.size(), ni / 2, redo_all);
    if (!jn && big.size() > redo_all && r.cap < 16384) {
        r.cap *= 2;
        *redo = true;
        return DH_OK;
    }
    if (mj_chunk) ctx->mj_chunks++;
    if (tj_chunk) ctx->tj_last_hits += (int64_t)tj_hits;
    r.mj_skip_chunk = false;  // (the next chunk tries the join again)
    if (mid_tier) {
        ctx->seed_mid_chunks++;
        ctx->seed_mid_redone += (int64_t)big.size();
        if (big.size() * 4 > (size_t)(ni / 2)) ctx->seed_mid_tier = 0;
        if (getenv("DH_TRACE"))
            fprintf(stderr, "[seeds] middle tier (256 threads, 2048 hits, 64 band pairs): %d reads, %zu redone by the 512-thread tiers%s\n",
                    ni / 2, big.size(), ctx->seed_mid_tier ? "" : ": not used by this context any more");
    }
    // (the middle tier's reads with too many band pairs have at most 2048 hits: the tiers below start at 2048 again)
    const int held = mid_tier ? 0 : capj;
    if (jn && held < tier_max && !big.empty()) {
        // further tiers of the join path: the reads above the first capacity that fit the 8192-entry variant, then the
        // 16384-entry one (uncapped pile-ups: ~10 000 hits per read); what is left is staged in HBM
        std::vector<int32_t> huge;
        int32_t gcap2 = 0;
        for (int tier = held < 2048 ? 2048 : 8192; tier <= tier_max; tier = tier < 8192 ? 8192 : tier * 2) {
            if (tier <= held) continue;
            std::vector<int32_t> mid;
            huge.clear();
            gcap2 = 0;
            for (int32_t rd : big) {
                const size_t it = (size_t)(2 * (int64_t)rd - item0);
                const int32_t nh = r.h_nhits[it] + r.h_nhits[it + 1];
                if (nh <= tier)
                    mid.push_back(rd);
                else {
                    huge.push_back(rd);
                    gcap2 = std::max(gcap2, nh);
                }
            }
            if (!mid.empty()) {
                int32_t *d_mid;
                uint64_t *d_fscr2;
                SCR(SLOT_MID_LIST, d_mid, mid.size())
                SCR(SLOT_FSCR, d_fscr2, (size_t)ctx->ncu * DH_SEED_FSCR_BLOCKS_PER_CU * (tier > 8192 ? DH_SEED_FSCR_WORDS16 : DH_SEED_FSCR_WORDS))
                HIPCHK(hipMemcpyAsync(d_mid, mid.data(), sizeof(int32_t) * mid.size(), hipMemcpyHostToDevice, st));
                HIPCHK(hipMemsetAsync(r.d_queue + 1, 0, sizeof(uint32_t), st));
                dhk_seed_join(st, tier, r.bv, r.iv, r.dopt, jvx, (int32_t)item0, ni, c.candbase, c.ncandbase, c.nhitsbase, r.d_status,
                              r.d_queue + 1, ctx->ncu, d_fscr2, d_mid, (int32_t)mid.size(), 0);
                HIPCHK(hipGetLastError());
                HIPCHK(hipStreamSynchronize(st));  // mid goes out of scope
            }
            if (getenv("DH_TRACE"))
                fprintf(stderr, "[seeds] join tiers: %zu reads redone with %d entries, %zu left\n", mid.size(), tier, huge.size());
            big = huge;
        }
        gcap = gcap2;
    }
    if (!big.empty()) {
        if (gcap > (1 << 22)) return fail(DH_EOVERFLOW, "seed filter: more than 4M k-mer hits for one sequence; lower -t");
        int32_t pow2 = 1;
        while (pow2 < gcap) pow2 <<= 1;  // the bitonic sort pads to a power of two
        // per block: pow2 hits, pow2 64-bit prefix sums, pow2 32-bit band-head positions (k_seed<0>)
        const size_t slab_words = 2 * (size_t)pow2 + ((size_t)pow2 + 1) / 2;
        const size_t per_launch = std::max<size_t>(1, (size_t)(2ull << 30) / (slab_words * 8));
        int32_t *d_list;
        uint64_t *d_gbuf;
        SCR(SLOT_BIG_LIST, d_list, big.size())
        SCR(SLOT_BIG_HITS, d_gbuf, std::min(per_launch, big.size()) * slab_words)
        HIPCHK(hipMemcpyAsync(d_list, big.data(), sizeof(int32_t) * big.size(), hipMemcpyHostToDevice, st));
        for (size_t b0 = 0; b0 < big.size(); b0 += per_launch) {
            const int32_t cnt = (int32_t)std::min(per_launch, big.size() - b0);
            HIPCHK(hipMemsetAsync(r.d_queue + 2, 0, sizeof(uint32_t), st));
            if (jn)
                dhk_seed_big_join(st, r.bv, r.iv, r.dopt, jvx, d_list + b0, cnt, d_gbuf, pow2, c.candbase, c.ncandbase,
                                  c.nhitsbase, r.d_status, r.d_queue + 2, ctx->ncu);
            else
                dhk_seed_big(st, r.bv, r.iv, r.dopt, d_list + b0, cnt, d_gbuf, pow2, c.candbase, c.ncandbase,
                             c.nhitsbase, r.d_status, r.d_queue + 2, ctx->ncu);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(&status, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        if (status & DH_ST_HIT_OVERFLOW)
            return fail(DH_EOVERFLOW, "seed filter: capacity exceeded in the HBM-staged pass");
        r.stats.big_items += 2 * (int64_t)big.size();
    }
    return DH_OK;
}

// the extension of the chunk's candidates: k_tile (DH-2), k_wave2 (two or four alignments per wavefront) or k_wave;
// symmetric launches first lay out their work units and record slots
static int extend_chunk(AlignRun &r, AlignChunk &c)
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
static int gather_chunk(AlignRun &r, AlignChunk &c)
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
                       const SeedDump *dump)
{
    const double wall0 = now_ms() * 1e3;
    double w_a = now_ms();
    if (int rc = check_align_args(ctx, A, B, opts, out, hook, out_tr)) return rc;
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
        if (int rc = plan_mj_chunk(r, c)) return rc;
        if (int rc = copy_chunk(r, c)) return rc;
        bool redo = false;
        if (int rc = seed_chunk(r, c, &redo)) return rc;
        if (redo) continue;  // the same chunk again (seed_chunk says why)
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
#undef SCR

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
