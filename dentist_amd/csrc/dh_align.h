// dh_align.h -- what the host files of the alignment pipeline share (dh_align.cpp, dh_align_prepare.cpp, dh_align_join.cpp,
// dh_align_seed.cpp, dh_align_extend.cpp): the state of a call and of a chunk, and the stages align_range runs.  Lives:
// ChunkHook, SeedDump and CandPlant are the caller's, for one call; AlignRun and JoinPlan are made by align_range and live for that
// call; Tasks is a member of AlignRun and is joined before the result is handed out or can move; AlignChunk and its
// ChunkCopies are made anew for every pass of the chunk loop (a chunk that runs again starts from an empty one).  What one
// file alone uses stays in that file.
#ifndef DH_ALIGN_H
#define DH_ALIGN_H

#include <chrono>
#include <functional>
#include <memory>
#include <thread>

#include "dh_internal.h"
#include "dh_join.h"
#include "dh_mjoin.h"
#include "dh_tile.h"
#include "dh_seed_plan.h"

// per-chunk hook: called on a host thread of its own with the records of a finished chunk (B-major,
// whole reads) while the device works on the next chunk; the records may be modified in place
// (records of the chunk, their number, their offset in the result, number of the chunk)
typedef std::function<void(dh_la *, int64_t, int64_t, int64_t)> ChunkHook;
// dh_seed_candidates: the caller's arrays (item 0 = the first item of the call); with it a chunk ends behind its seeds
struct SeedDump {
    dh_seed_cand *cand;
    int32_t *ncand, *nhits;
};

// dh_extend_candidates: the caller's candidates (row 0 = the first item of the call); with it a chunk gets its seeds from
// these rows and seed_chunk does not run
struct CandPlant {
    const dh_seed_cand *cand;
    const int32_t *ncand;
};

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

static inline double now_ms()
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
    seedplan::SeedKnobs knobs;  // the development switches of the seed stage, as plan_seeds found them
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

// why seed_chunk wants the chunk loop to run the chunk again
enum SeedRedo {
    SEED_DONE = 0,           // it does not: the chunk has its seeds
    SEED_POOL_REGROWN,       // the mapping join's hit pool ran out and is planned larger from now on
    SEED_BY_DIRECTORY,       // a capacity of the mapping join was exceeded: this chunk by the directory path
    SEED_CAP_DOUBLED,        // many reads overflowed the directory path's LDS capacity: the next one
    SEED_WITHOUT_TJOIN,      // a read's hits do not fit a segment word of the table join: the call goes on by the directory
};

#define SCR(id, ptr, count)                                                                      \
    if (int rc_ = dh_scratch(ctx, id, sizeof(*ptr) * std::max<size_t>((size_t)(count), 1), (void **)&ptr)) return rc_;

// ---- the stages, in the order align_range runs them (they were one file's static functions: the library exports none)
#pragma GCC visibility push(hidden)
// dh_align_join.cpp
void plan_join(AlignRun &r, JoinPlan &jp);
int build_join(AlignRun &r, const JoinPlan &jp);
// dh_align_prepare.cpp
IndexView index_view(const dh_db *A);
int prepare_dbs(AlignRun &r);
int alloc_scratch(AlignRun &r);
int copy_chunk(AlignRun &r, AlignChunk &c);
// dh_align_seed.cpp
int plan_seeds(AlignRun &r);
int plan_mj_chunk(AlignRun &r, AlignChunk &c);
int seed_chunk(AlignRun &r, AlignChunk &c, SeedRedo *redo);
int plant_chunk(AlignRun &r, AlignChunk &c, const CandPlant &plant);
// dh_align_extend.cpp
int extend_chunk(AlignRun &r, AlignChunk &c);
int gather_chunk(AlignRun &r, AlignChunk &c);
#pragma GCC visibility pop

#endif
