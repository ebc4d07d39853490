// dh_align_seed.cpp -- the seeds of an alignment call: what the call decides once (plan_seeds), the plan of a chunk's mapping
// join (plan_mj_chunk) and the seed stage of a chunk (seed_chunk: hits from the chunk's source, the first tier of the seed
// filter, the tiers and the HBM pass for what overflowed).  Every decision is a function of dh_seed_plan.h; this file
// reads the switches, asks for the slots and sequences the launches.
#include <cstdio>
#include <cstdlib>

#include "dh_align.h"
#include "dh_tjoin.h"

#define fail dh_fail

using namespace seedplan;

static const SeedConsts CONSTS = {MJ_P,   MJ_CAP, MJ_THREADS,      MJ_POSBITS,         MJ_GROUP,             MJ_BATCH,
                                  MJ_PAGE, MJ_PROBE_THREADS, TJ_CAP, TJ_RUN, DH_TJ_HIT_RATE0, DH_SEED_FSCR_WORDS,
                                  DH_SEED_FSCR_WORDS16, DH_SEED_FSCR_BLOCKS_PER_CU};

// the development switches of the seed stage as the environment has them now (tests set them between calls)
static SeedKnobs read_seed_knobs()
{
    SeedKnobs kn;
    if (const char *e = getenv("DH_SEED_CAP")) kn.has_seed_cap = true, kn.seed_cap = atoi(e);
    kn.no16k = getenv("DH_SEED_NO16K") != nullptr;
    kn.no_wave_tier = getenv("DH_SEED_NO_WAVE_TIER") != nullptr;
    kn.no_mid_tier = getenv("DH_SEED_NO_MID_TIER") != nullptr;
    if (const char *e = getenv("DH_SEED_BIG_PCT")) kn.has_big_pct = true, kn.big_pct = atof(e);
    if (const char *e = getenv("DH_MJOIN_MIN")) kn.has_mjoin_min = true, kn.mjoin_min = atoll(e);
    if (const char *e = getenv("DH_MJOIN_PAGES")) kn.has_mjoin_pages = true, kn.mjoin_pages = atoll(e);
    kn.no_mjoin = getenv("DH_NO_MJOIN") != nullptr;
    kn.no_tjoin = getenv("DH_NO_TJOIN") != nullptr;
    if (const char *e = getenv("DH_TJOIN_CAP")) kn.has_tjoin_cap = true, kn.tjoin_cap = atoll(e);
    if (const char *e = getenv("DH_TJOIN_HITCAP")) kn.has_tjoin_hitcap = true, kn.tjoin_hitcap = atoll(e);
    return kn;
}

static void ctx_count_tj_fallback(dh_ctx *ctx)
{
    ctx->tj_fallbacks++;
    if (getenv("DH_TRACE")) fprintf(stderr, "[tjoin] a limit of the table join is not met: this call keeps the k-mer directory\n");
}

// the LDS hit capacity of the seed filter; whether the mapping goes by the partitioned join (and its presence bitmap)
int plan_seeds(AlignRun &r)
{
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    r.knobs = read_seed_knobs();
    const SeedKnobs &kn = r.knobs;
    r.dens = chance_density(A->ix.n, o.kmer_mod, o.k, A->ngroups);
    r.cap = first_cap(B->max_len, o.kmer_mod, r.dens, A == B, r.use_join, r.jhist, B->n, kn);
    // ---- a mapping pass (A != B, ungrouped): the seeds of a chunk of reads come from the radix-partitioned k-mer join
    // (dh_mjoin.h) -- the reads' k-mers binned by directory slice, every slice joined on chip -- instead of one random
    // directory line per k-mer; bit-identical hits.  Small chunks keep the directory path (the join's fixed costs: 1 024
    // partitions, a page per wavefront); DH_NO_MJOIN=1 forces it, DH_MJOIN_MIN sets the threshold (bases of a chunk).
    r.use_mj = !r.use_join && A != B && !A->d_group && A->ngroups == 1 && !B->d_group && o.k >= MJ_MINK && o.k <= MJ_MAXK &&
               o.skip_self == 0 && r.want_packed && A->ix.n > 0 && A->ix.n < (1ll << 28) && !kn.no_mjoin;
    r.mj_min_bases = mj_min_bases(kn);
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
    if (!r.use_join && A != B && A->d_group && !kn.no_tjoin) {
        // (a group of B without sequences in A, beyond A's last group included, is an empty table to k_tjoin: its reads
        // get no hits, which is what "no template in the pile-up" means; the group ids themselves are the callers' and
        // are the same numbering on both sides)
        r.use_tj = B->d_group && o.k <= TJ_MAXK && o.skip_self == 0 && A->ix.d_gent &&
                   A->ix.max_gent <= tj_cap_entries(kn, CONSTS) && A->ix.n < (1ll << 31) && B->max_len < (1 << 24);
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
int plan_mj_chunk(AlignRun &r, AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    const dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    MjView &mv = c.mv;
    const int32_t cr0 = (int32_t)(c.item0 >> 1), cr1 = (int32_t)((c.item0 + c.ni) >> 1);
    const int64_t cb0 = B->h_off[(size_t)cr0], cb1 = B->h_off[(size_t)cr1];
    if (!r.use_mj || r.mj_skip_chunk || !mj_chunk_size_ok(cb1 - cb0, r.mj_min_bases)) return DH_OK;
    const MjGeom g = mj_geometry(cb1 - cb0, B->max_len, o.kmer_mod, ctx->mj_hit_frac, r.dens, ctx->ncu, r.knobs, CONSTS);
    mv.c0 = cb0;
    mv.c1 = cb1;
    mv.r0 = cr0;
    mv.r1 = cr1;
    mv.k = o.k;
    mv.kmer_mod = std::max(1, o.kmer_mod);
    mv.nbbits = A->ix.nbbits;
    mv.tb = (int32_t)g.tb;
    mv.ntiles = (int32_t)g.ntiles;
    mv.ntiles_pad = (int32_t)g.ntiles_pad;
    mv.ngroups = (int32_t)g.ngroups;
    mv.nseg = (int32_t)g.nseg;
    if (!g.fits) return DH_OK;
    mv.npages = (int32_t)g.npages;
    mv.rcap = g.npages * MJ_PAGE;
    uint32_t *d_mjctr;
    SCR(SLOT_MJ_ENT, mv.ent, (size_t)g.ntiles * MJ_CAP)
    SCR(SLOT_MJ_SEGOFF, mv.segoff, (size_t)g.ntiles * MJ_P)
    SCR(SLOT_MJ_TILE_N, mv.tile_n, (size_t)g.ntiles)
    SCR(SLOT_MJ_TILE_R, mv.tile_r, (size_t)g.ntiles)
    SCR(SLOT_MJ_SEG, mv.seg, (size_t)MJ_P * mv.ntiles_pad)
    SCR(SLOT_MJ_HSEG, mv.hseg, (size_t)mv.ngroups * MJ_P)
    SCR(SLOT_MJ_HITS, mv.hits, (size_t)g.npages * MJ_PAGE)
    SCR(SLOT_MJ_RHITS, mv.rhits, (size_t)mv.rcap)
    SCR(SLOT_MJ_SEGTAB, mv.segtab, (size_t)(cr1 - cr0) * mv.nseg)
    SCR(SLOT_MJ_CTR, d_mjctr, 16)
    mv.ctr = d_mjctr;
    r.d_mjctr_last = d_mjctr;
    r.mj_exp_ent_last = g.exp_ent;
    r.mj_npages_last = g.npages;
    mv.bitmap = A->ix.d_bitmap;
    mv.status = r.d_status;
    dhk_mj_tile_reads(r.st, r.bv, mv);
    HIPCHK(hipGetLastError());
    c.mj_planned = true;
    return DH_OK;
}

// ---- seed_chunk and its parts

// where the hits of the chunk at hand come from: the segments of a join (jv) or, for SRC_DIRECTORY, the k-mer directory;
// mean_hits: hits per read the first tier is chosen by; tj_hits: what the table join counted
struct SeedSource {
    SourceKind kind = SRC_DIRECTORY;
    JoinView jv = {};
    double mean_hits = 0;
    unsigned long long tj_hits = 0;
};

// slab scratch of a seed launch (8192 entries and above): per_block words for every resident block, a null pointer for none
static int fscr_scratch(AlignRun &r, size_t per_block, uint64_t **out)
{
    dh_ctx *ctx = r.ctx;
    *out = nullptr;
    if (per_block > 0) SCR(SLOT_FSCR, (*out), fscr_total_words(per_block, ctx->ncu, CONSTS))
    return DH_OK;
}

// per-chunk arrays are indexed by absolute item inside the kernels: shift the bases; the seed stage's clock starts
static int shift_bases(AlignRun &r, AlignChunk &c)
{
    const dh_align_opts &o = r.o;
    const int64_t item0 = c.item0;
    c.candbase = r.d_cand - item0 * o.max_cand;
    c.labase = r.d_la ? r.d_la - item0 * o.max_la : nullptr;
    c.trbase = r.d_trslots ? r.d_trslots - item0 * (int64_t)o.max_la * r.trmax : nullptr;
    c.ncandbase = r.d_ncand - item0;
    c.nhitsbase = r.d_nhits - item0;
    c.nlabase = (int32_t *)r.d_nla - item0;
    c.ntrbase = (int32_t *)r.d_ntr - item0;
    r.lap(0);
    HIPCHK(hipEventRecord(r.ctx->ev[2], r.st));
    HIPCHK(hipMemsetAsync(r.d_queue, 0, 4 * sizeof(uint32_t), r.st));
    return DH_OK;
}

// the mapping join of a planned chunk: its hits regrouped by read
static int run_mapping_join(AlignRun &r, AlignChunk &c, SeedSource &src)
{
    const MjView &mv = c.mv;
    HIPCHK(dhk_memset(r.st, mv.segtab, 0, sizeof(unsigned long long) * (size_t)(mv.r1 - mv.r0) * mv.nseg));
    dhk_mj_run(r.st, r.bv, r.iv, r.dopt, mv, r.ctx->ncu);
    HIPCHK(hipGetLastError());
    src.jv.segtab = (uint64_t *)mv.segtab;
    src.jv.hits = mv.rhits;
    src.jv.status = r.d_status;
    src.jv.ns_fixed = mv.nseg;
    src.jv.read0 = mv.r0;
    return DH_OK;
}

// the per-group table join: units (group, run of consecutive reads), count + reserve + write; a hit buffer that was
// too small is sized by what the cursor counted and the kernel runs again.  SEED_WITHOUT_TJOIN: a read has more hits than
// a segment word describes, the call gives the table join up.
static int run_table_join(AlignRun &r, AlignChunk &c, SeedSource &src, SeedRedo *redo)
{
    dh_ctx *ctx = r.ctx;
    const dh_db *B = r.B;
    hipStream_t st = r.st;
    const int32_t cr0 = (int32_t)(c.item0 >> 1), cr1 = (int32_t)((c.item0 + c.ni) >> 1);
    const std::vector<int4> units = tj_units<int4>(B->h_group.data(), cr0, cr1, CONSTS);
    const int64_t cbases = B->h_off[(size_t)cr1] - B->h_off[(size_t)cr0];
    int64_t hcap = tj_first_hitcap(ctx->tj_hit_rate, cbases, r.knobs);
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
    unsigned long long tj_hits = 0;
    for (int attempt = 0;; attempt++) {
        SCR(SLOT_TJ_HITS, tv.hits, (size_t)hcap)
        tv.hits_cap = hcap;
        HIPCHK(hipMemsetAsync(d_tjctr, 0, 4 * sizeof(uint32_t), st));
        dhk_tjoin(st, r.bv, r.iv, r.dopt, tv, ctx->ncu);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&tj_hits, tv.cursor, sizeof(tj_hits), hipMemcpyDeviceToHost, st));
        HIPCHK(hipMemcpyAsync(&tst, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));  // (the upload of units has landed behind this)
        if (!(tst & DH_ST_TJ_HITCAP)) break;
        if (attempt > 0) return fail(DH_EOVERFLOW, "table join: the hit buffer sized by the count pass was too small");
        tst &= ~DH_ST_TJ_HITCAP;
        HIPCHK(hipMemcpyAsync(r.d_status, &tst, sizeof(int32_t), hipMemcpyHostToDevice, st));
        if (getenv("DH_TRACE")) fprintf(stderr, "[tjoin] hit buffer of %lld too small for %llu hits: run again\n", (long long)hcap, tj_hits);
        hcap = (int64_t)tj_hits;
        ctx->tj_reruns++;
    }
    ctx->tj_hit_rate = tj_learned_rate(ctx->tj_hit_rate, tj_hits, cbases, CONSTS);
    if (tst & DH_ST_TJ_OVERFLOW) {
        // (a read with 2^24 hits or more: nothing the segment word can describe) the whole call by the directory
        tst &= ~DH_ST_TJ_OVERFLOW;
        HIPCHK(hipMemcpyAsync(r.d_status, &tst, sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        r.use_tj = false;
        ctx->tj_calls--;
        ctx_count_tj_fallback(ctx);
        *redo = SEED_WITHOUT_TJOIN;
        return DH_OK;
    }
    src.jv.segtab = tv.segtab;
    src.jv.hits = tv.hits;
    src.jv.status = r.d_status;
    src.jv.ns_fixed = 1;
    src.jv.read0 = cr0;
    src.tj_hits = tj_hits;
    return DH_OK;
}

// the hits of the chunk from its source -- the mapping join planned for it, the table join, the call's pile-up join, or
// none yet (the directory is looked up by the seed kernel itself) -- and the mean hits per read
static int obtain_hits(AlignRun &r, AlignChunk &c, SeedSource &src, SeedRedo *redo)
{
    const dh_db *B = r.B;
    if (c.mj_planned && !c.cc.has_n) {
        src.kind = SRC_MAPPING_JOIN;
        if (int rc = run_mapping_join(r, c, src)) return rc;
    } else if (r.use_tj) {
        src.kind = SRC_TABLE_JOIN;
        if (int rc = run_table_join(r, c, src, redo)) return rc;
    } else if (r.use_join) {
        src.kind = SRC_PILEUP_JOIN;
        src.jv = r.jv;
    }
    const int64_t cbases = B->h_off[(size_t)((c.item0 + c.ni) >> 1)] - B->h_off[(size_t)(c.item0 >> 1)];
    src.mean_hits = src.kind == SRC_TABLE_JOIN ? mean_hits_counted(src.tj_hits, c.ni)
                                               : mean_hits_expected(kmers_per_read(cbases, c.ni, r.o.kmer_mod), r.dens);
    return DH_OK;
}

// the first tier over all items of the chunk: the segment-fed back end of a join, or the directory's kernel
static int launch_first_tier(AlignRun &r, AlignChunk &c, const SeedSource &src, const FirstTier &ft)
{
    dh_ctx *ctx = r.ctx;
    uint64_t *d_fscr;
    if (int rc = fscr_scratch(r, ft.fscr_words, &d_fscr)) return rc;
    if (src.kind != SRC_DIRECTORY)
        dhk_seed_join(r.st, ft.capj, r.bv, r.iv, r.dopt, src.jv, (int32_t)c.item0, c.ni, c.candbase, c.ncandbase, c.nhitsbase, r.d_status,
                      r.d_queue + 1, ctx->ncu, d_fscr, nullptr, 0, ft.mid_tier ? 1 : 0);
    else
        dhk_seed(r.st, r.cap, r.bv, r.iv, r.dopt, (int32_t)c.item0, c.ni, c.candbase, c.ncandbase, c.nhitsbase, r.d_status,
                 r.d_queue + 1, ctx->ncu, d_fscr);
    HIPCHK(hipGetLastError());
    return DH_OK;
}

// the status word of the call and the summary of the chunk's items (sm[2]: items that overflowed their LDS buffer)
static int read_first_tier(AlignRun &r, const AlignChunk &c, int32_t *status, unsigned long long (&sm)[4])
{
    dhk_seed_summary(r.st, r.d_ncand, r.d_nhits, c.ni, r.d_summary);
    HIPCHK(hipMemcpyAsync(status, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipMemcpyAsync(sm, r.d_summary, sizeof(sm), hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    return DH_OK;
}

// the overflow states of the mapping join: a hit pool that ran out (SEED_POOL_REGROWN, or past what can be planned for:
// an overflow), a capacity that was exceeded (SEED_BY_DIRECTORY)
static int resolve_mj_overflow(AlignRun &r, const AlignChunk &c, const SeedSource &src, int32_t status, SeedRedo *redo)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = r.st;
    if (src.kind != SRC_MAPPING_JOIN) return DH_OK;
    if ((status & DH_ST_MJ_POOL) && !(status & DH_ST_MJ_OVERFLOW) && !r.knobs.has_mjoin_pages) {
        unsigned long long cnt2[2] = {0, 0};  // hits counted for rhits, survivors that found no page
        HIPCHK(hipMemcpyAsync(cnt2, r.d_mjctr_last + 10, sizeof(cnt2), hipMemcpyDeviceToHost, st));
        status &= ~DH_ST_MJ_POOL;
        HIPCHK(hipMemcpyAsync(r.d_status, &status, sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        const MjRegrow g = mj_pool_regrow(r.mj_npages_last, r.mj_exp_ent_last, cnt2[0], cnt2[1], ctx->mj_hit_frac, CONSTS);
        ctx->mj_hit_frac = g.hit_frac;
        if (getenv("DH_TRACE")) fprintf(stderr, "[mjoin] pool too small (%llu survivors without a page, %llu hits): %.2f per k-mer planned from now on\n", cnt2[1], cnt2[0], ctx->mj_hit_frac);
        if (g.again) {
            *redo = SEED_POOL_REGROWN;
            return DH_OK;
        }
        status |= DH_ST_MJ_OVERFLOW;
    }
    if (status & (DH_ST_MJ_OVERFLOW | DH_ST_MJ_POOL)) {
        // a capacity of the partitioned join was exceeded (repeat-rich reads): this chunk again, by the directory
        if (getenv("DH_TRACE")) fprintf(stderr, "[mjoin] a capacity was exceeded: chunk at item %lld redone by the directory path\n", (long long)c.item0);
        status &= ~(DH_ST_MJ_OVERFLOW | DH_ST_MJ_POOL);
        HIPCHK(hipMemcpyAsync(r.d_status, &status, sizeof(int32_t), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        r.mj_skip_chunk = true;
        ctx->mj_fallbacks++;
        *redo = SEED_BY_DIRECTORY;
    }
    return DH_OK;
}

// items whose hits did not fit the LDS buffer (ncand == -1) are redone: their reads, the largest hit count among them
// (the per-item arrays travel only when some item overflowed its LDS buffer)
static int list_overflowed_reads(AlignRun &r, const AlignChunk &c, bool any, std::vector<int32_t> &big, int32_t *gcap)
{
    *gcap = 0;
    if (!any) return DH_OK;
    HIPCHK(hipMemcpyAsync(r.h_ncand.data(), r.d_ncand, sizeof(int32_t) * (size_t)c.ni, hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipMemcpyAsync(r.h_nhits.data(), r.d_nhits, sizeof(int32_t) * (size_t)c.ni, hipMemcpyDeviceToHost, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    *gcap = list_overflowed(r.h_ncand.data(), r.h_nhits.data(), c.ni, c.item0, big);
    return DH_OK;
}

// what nbig overflowed reads mean for the first tier: a tier the context stops using, the directory path's next cap
// (SEED_CAP_DOUBLED), and -- the chunk stands -- the counters of its path
static void settle_first_tier(AlignRun &r, const AlignChunk &c, const SeedSource &src, const FirstTier &ft, size_t nbig, SeedRedo *redo)
{
    dh_ctx *ctx = r.ctx;
    const int32_t ni = c.ni;
    if (ft.wave_tier && quarter_overflowed(nbig, ni)) {
        ctx->seed_wave_tier = 0;
        if (getenv("DH_TRACE"))
            fprintf(stderr, "[seeds] %zu of %d reads overflow the wavefront-per-read tier: not used by this context any more\n", nbig, ni / 2);
    }
    const size_t redo_all = redo_all_above(ni, r.cap, r.knobs);
    if (getenv("DH_TRACE") && nbig > 0)
        fprintf(stderr, "[seeds] cap %d: %zu of %d reads overflow (whole chunk again above %zu)\n", r.cap, nbig, ni / 2, redo_all);
    if (cap_doubles(src.kind, nbig, redo_all, r.cap)) {
        r.cap *= 2;
        *redo = SEED_CAP_DOUBLED;
        return;
    }
    if (src.kind == SRC_MAPPING_JOIN) ctx->mj_chunks++;
    if (src.kind == SRC_TABLE_JOIN) ctx->tj_last_hits += (int64_t)src.tj_hits;
    r.mj_skip_chunk = false;  // (the next chunk tries the join again)
    if (ft.mid_tier) {
        ctx->seed_mid_chunks++;
        ctx->seed_mid_redone += (int64_t)nbig;
        if (quarter_overflowed(nbig, ni)) ctx->seed_mid_tier = 0;
        if (getenv("DH_TRACE"))
            fprintf(stderr, "[seeds] middle tier (256 threads, 2048 hits, 64 band pairs): %d reads, %zu redone by the 512-thread tiers%s\n",
                    ni / 2, nbig, ctx->seed_mid_tier ? "" : ": not used by this context any more");
    }
}

// the list tiers of a join path above what the first tier held: every rung takes the reads of `big` that fit it; big and
// *gcap become what is left and its largest hit count
static int run_ladder(AlignRun &r, AlignChunk &c, const SeedSource &src, int held, std::vector<int32_t> &big, int32_t *gcap)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = r.st;
    std::vector<int32_t> mid, huge;
    for (int tier : tier_ladder(held, tier_max(r.knobs))) {
        *gcap = split_rung(big, r.h_nhits.data(), c.item0, tier, mid, huge);
        if (!mid.empty()) {
            int32_t *d_mid;
            uint64_t *d_fscr;
            SCR(SLOT_MID_LIST, d_mid, mid.size())
            if (int rc = fscr_scratch(r, tier_fscr_words(tier, CONSTS), &d_fscr)) return rc;
            HIPCHK(hipMemcpyAsync(d_mid, mid.data(), sizeof(int32_t) * mid.size(), hipMemcpyHostToDevice, st));
            HIPCHK(hipMemsetAsync(r.d_queue + 1, 0, sizeof(uint32_t), st));
            dhk_seed_join(st, tier, r.bv, r.iv, r.dopt, src.jv, (int32_t)c.item0, c.ni, c.candbase, c.ncandbase, c.nhitsbase, r.d_status,
                          r.d_queue + 1, ctx->ncu, d_fscr, d_mid, (int32_t)mid.size(), 0);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));  // mid is rewritten by the next rung
        }
        if (getenv("DH_TRACE"))
            fprintf(stderr, "[seeds] join tiers: %zu reads redone with %d entries, %zu left\n", mid.size(), tier, huge.size());
        big.swap(huge);
    }
    return DH_OK;
}

// what is left is redone with its hits staged in HBM: same kernel code, capacity = the largest hit count (gcap), in
// launches of at most 2 GB of slabs
static int run_hbm_pass(AlignRun &r, AlignChunk &c, const SeedSource &src, const std::vector<int32_t> &big, int32_t gcap)
{
    dh_ctx *ctx = r.ctx;
    hipStream_t st = r.st;
    const HbmPass p = hbm_pass(gcap);
    if (p.refused) return fail(DH_EOVERFLOW, "seed filter: more than 4M k-mer hits for one sequence; lower -t");
    int32_t *d_list;
    uint64_t *d_gbuf;
    SCR(SLOT_BIG_LIST, d_list, big.size())
    SCR(SLOT_BIG_HITS, d_gbuf, std::min(p.per_launch, big.size()) * p.slab_words)
    HIPCHK(hipMemcpyAsync(d_list, big.data(), sizeof(int32_t) * big.size(), hipMemcpyHostToDevice, st));
    for (size_t b0 = 0; b0 < big.size(); b0 += p.per_launch) {
        const int32_t cnt = (int32_t)std::min(p.per_launch, big.size() - b0);
        HIPCHK(hipMemsetAsync(r.d_queue + 2, 0, sizeof(uint32_t), st));
        if (src.kind != SRC_DIRECTORY)
            dhk_seed_big_join(st, r.bv, r.iv, r.dopt, src.jv, d_list + b0, cnt, d_gbuf, p.pow2, c.candbase, c.ncandbase,
                              c.nhitsbase, r.d_status, r.d_queue + 2, ctx->ncu);
        else
            dhk_seed_big(st, r.bv, r.iv, r.dopt, d_list + b0, cnt, d_gbuf, p.pow2, c.candbase, c.ncandbase,
                         c.nhitsbase, r.d_status, r.d_queue + 2, ctx->ncu);
        HIPCHK(hipGetLastError());
    }
    int32_t status = 0;
    HIPCHK(hipMemcpyAsync(&status, r.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (status & DH_ST_HIT_OVERFLOW)
        return fail(DH_EOVERFLOW, "seed filter: capacity exceeded in the HBM-staged pass");
    r.stats.big_items += 2 * (int64_t)big.size();
    return DH_OK;
}

// dh_extend_candidates: the chunk's seeds are the caller's rows of its items -- the set-up of seed_chunk, then three copies
int plant_chunk(AlignRun &r, AlignChunk &c, const CandPlant &plant)
{
    if (int rc = shift_bases(r, c)) return rc;
    const size_t at = (size_t)(c.item0 - r.item_first), ni = (size_t)c.ni;
    HIPCHK(hipMemcpyAsync(r.d_cand, plant.cand + at * r.o.max_cand, sizeof(DhCand) * ni * r.o.max_cand, hipMemcpyHostToDevice, r.st));
    HIPCHK(hipMemcpyAsync(r.d_ncand, plant.ncand + at, sizeof(int32_t) * ni, hipMemcpyHostToDevice, r.st));
    HIPCHK(hipMemsetAsync(r.d_nhits, 0, sizeof(int32_t) * ni, r.st));
    HIPCHK(hipStreamSynchronize(r.st));
    return DH_OK;
}

// The seeds of a chunk: the first tier of the seed filter (fed by the mapping join, the pile-up join or the directory),
// then the reads that overflowed it -- further tiers of the join path, the rest staged in HBM.  *redo: the chunk has to
// run again (the join's hit pool ran out, a capacity of the join was exceeded, or the directory path doubled its cap).
int seed_chunk(AlignRun &r, AlignChunk &c, SeedRedo *redo)
{
    *redo = SEED_DONE;
    if (int rc = shift_bases(r, c)) return rc;
    SeedSource src;
    if (int rc = obtain_hits(r, c, src, redo)) return rc;
    if (*redo != SEED_DONE) return DH_OK;
    const FirstTier ft = first_tier(src.kind, r.cap, src.mean_hits, c.mv.nseg, r.ctx->seed_wave_tier != 0, r.ctx->seed_mid_tier != 0,
                                    r.knobs, CONSTS);
    if (int rc = launch_first_tier(r, c, src, ft)) return rc;
    int32_t status = 0;
    unsigned long long sm[4] = {0, 0, 0, 0};
    if (int rc = read_first_tier(r, c, &status, sm)) return rc;
    if (int rc = resolve_mj_overflow(r, c, src, status, redo)) return rc;
    if (*redo != SEED_DONE) return DH_OK;
    std::vector<int32_t> big;
    int32_t gcap = 0;
    if (int rc = list_overflowed_reads(r, c, sm[2] > 0, big, &gcap)) return rc;
    settle_first_tier(r, c, src, ft, big.size(), redo);
    if (*redo != SEED_DONE) return DH_OK;
    // (the middle tier's reads with too many band pairs have at most 2048 hits: the tiers below start at 2048 again)
    const int held = ft.mid_tier ? 0 : ft.capj;
    if (src.kind != SRC_DIRECTORY && !big.empty())
        if (int rc = run_ladder(r, c, src, held, big, &gcap)) return rc;
    if (!big.empty())
        if (int rc = run_hbm_pass(r, c, src, big, gcap)) return rc;
    return DH_OK;
}
