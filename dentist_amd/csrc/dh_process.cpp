// dh_process.cpp -- the process stages of the pile-up consensus path: the call sequence of
// `dentist process` (source/dentist/commands/processPileUps/package.d:283-374) over a BATCH of
// pile-ups, with every tool spawn of the reference replaced by kernels on the context's stream:
//   crop (cropper.d:113-175, 446-550)            -> k_gather_slices
//   daligner pile-up all-vs-all (package.d:478)  -> dh_align_db on the grouped pile-up DB
//   filters (dazzler.d:3879-3899, 4043-4141)     -> host flags (same predicates as the reference)
//   DASqv (dazzler.d:6142-6156)                  -> k_tile_qv
//   reference-read ranking (package.d:518-568)   -> host (the reference's own D logic)
//   daccord (dazzler.d:6185-6231)                -> k_seg_vote + k_emit, `rounds` times
//   daligner -A flanks vs consensus (:655-667)   -> dh_align_db
//   insertion (package.d:699-805, insertions.d:110-146) -> host
// The stages of dh_process_cropped live here; the crop is dh_crop.cpp, the batch drivers dh_batch.cpp, the consensus
// rounds dh_rounds.cpp, the trace-point arithmetic and chain_pair dh_tracepoint.cpp (shared declarations: dh_process.h).
#include <atomic>
#include <cstdlib>
#include <cstring>

#include "dh_process.h"
#include "dh_parallel.h"

using namespace dhp;

extern "C" {
void dhk_gather_ranges16(hipStream_t st, const uint16_t *src, const int64_t *desc, int32_t n, uint16_t *dst);
void dhk_tile_qv(hipStream_t st, const DhLa *las, const uint16_t *trace, const int32_t *la_first,
                 const int64_t *roff, int32_t nreads, int32_t tspace, const int32_t *cov, int32_t maxtiles,
                 uint8_t *qv);
void dhk_pile_funnel(hipStream_t st, DhLa *las, const uint32_t *item_off, int32_t nreads, const int64_t *roff,
                     int32_t max_err_ppm, int32_t tsp, int32_t *la_first, int32_t *live, int32_t *status);
void dhk_gather_read_records(hipStream_t st, const DhLa *las, const int32_t *la_first, const int32_t *sel,
                             const int32_t *dst_off, int32_t nsel, DhLa *out);
}

#define MAXQV 50
#define FLAG_IMPROPER 0x40u /* internal: fails isValidPileUpAlignment, dropped after the tile QVs */

extern "C" void dh_default_process_opts(dh_process_opts *o)
{
    memset(o, 0, sizeof(*o));
    o->tspace_map = 100;
    o->allowance = 100;
    o->min_anchor = 500;
    o->min_reads = 3;
    o->max_reads = 60;
    o->tspace_pile = 126;
    o->rounds = 3;
    o->flank_window = 20000;
    o->max_align_err_ppm = 300000;
    o->max_ins_err_ppm = 100000;
    o->bad_fraction_ppm = 80000;
    o->width = 30;
    o->dust = 1;
    o->min_relative_score_ppm = 1000000;
}

static thread_local ProcStats g_pstats;
ProcStats &dhp::dh_proc_stats() { return g_pstats; }

extern "C" int dh_get_process_work(dh_ctx *ctx, int64_t *work4)
{
    if (!ctx || !work4) return dh_fail(DH_EINVAL, "dh_get_process_work: NULL argument");
    memcpy(work4, g_pstats.work, sizeof(g_pstats.work));
    return DH_OK;
}

extern "C" int dh_get_process_stats(dh_ctx *ctx, float *ms7, int64_t *counters3)
{
    if (!ctx) return dh_fail(DH_EINVAL, "ctx is NULL");
    if (ms7) memcpy(ms7, g_pstats.ms, sizeof(g_pstats.ms));
    if (counters3) memcpy(counters3, g_pstats.counters, sizeof(g_pstats.counters));
    return DH_OK;
}

// ------------------------------------------------------------------------------------ process stages
// dh_process_cropped is the stages below, called in the order they stand in, over these structs.

// what one dh_process_cropped call owns
struct ProcRun {
    dh_ctx *ctx;
    hipStream_t st;
    const dh_process_opts &o;
    dh_db *contigs;
    dh_cropped *crop;
    // trace spacing, width and algorithm of the alignment calls (check_process_opts)
    int32_t tsp, pwidth, palgo;
    dh_insertions *res = nullptr;  // the call's until it is handed over
    ProcStats ps;
    ProcTimer tm;
    DbGuard dbg;
    SetGuard sg;
    ~ProcRun() { delete res; }
    dh_align_opts align_opts(int32_t min_len, int32_t max_la, int32_t max_cand) const
    {
        dh_align_opts ao = pile_align_opts(tsp, min_len, max_la, max_cand);
        ao.width = pwidth;
        ao.algo = palgo;
        return ao;
    }
};

// the pile-up DB (plan_pile_db, build_pile_db): the cropped reads of every pile-up that is large enough, grouped by
// pile-up (group = index among the active pile-ups)
struct PileLayout {
    int32_t na = 0;                       // active pile-ups
    std::vector<int32_t> pile_of_active;  // active index -> pile-up index
    std::vector<int32_t> first_read;      // active index -> first read in pile-up DB
    std::vector<int32_t> read_id;         // pile-up DB read -> read id in `reads`
    std::vector<uint8_t> rkind;           // pile-up DB read -> 0 = it may serve as reference read (alignments on every flank of its pile-up:
                                          // selectAllowedReferenceReadIds, package.d:461-472), else 1 / 2 = on flank 0 / 1 only
    std::vector<uint8_t> rcomp;           // pile-up DB read -> bit f: its alignment on flank f is a complement one
    std::vector<int32_t> sgroup, keep;    // per pile-up DB read: group, index in the crop DB
    dh_db *pile = nullptr;
    // what the stages find out per active pile-up: it is still in the race; its reference read (pile-up DB read, -1: none)
    std::vector<uint8_t> active_ok;
    std::vector<int32_t> ref_of;
};

// what the pile-up alignment, the funnel and the tile QVs hand to the ranking and the consensus rounds
struct FunnelOut {
    dh_la_set *pset = nullptr;
    bool on_dev = false;                       // the records are on the device (pset->d_la) and not in pset->la
    std::vector<int32_t> la_first;             // first record of every pile-up read
    std::vector<int32_t> dev_live;             // device funnel: live records of every pile-up read
    DevBuf<int32_t> d_first_keep;              // ... and la_first on the device: the first consensus round gathers records by it
    std::vector<uint8_t> qv;
    int32_t maxtiles = 1;
    std::vector<int32_t> cov_of;
};

// the flank DB (one slice per flank of an active pile-up, fbase[a] = the first one of a) and its overlaps with the consensus
struct FlankOut {
    std::vector<int32_t> fbeg, flen, fbase;
    dh_la_set *fset = nullptr;
};

static int check_process_opts(dh_ctx *ctx, dh_db *contigs, dh_cropped *crop, const dh_process_opts *opts, dh_insertions **out,
                              int32_t *pwidth_out, int32_t *palgo_out)
{
    if (!ctx || !contigs || !crop || !opts || !out) return dh_fail(DH_EINVAL, "dh_process_cropped: NULL argument");
    const dh_process_opts &o = *opts;
    if (o.max_reads != 0 && (o.max_reads < 3 || o.max_reads > 250))
        return dh_fail(DH_EINVAL, "max_reads must be 0 (no cap) or in [3, 250]");
    if (o.max_partners != 0 && o.max_partners < 4) return dh_fail(DH_EINVAL, "max_partners must be 0 (every pair) or at least 4");
    // (0 is refused: it is what a caller built against the 56-byte struct of ABI 3, or one that zero-fills the struct, would
    // pass without meaning it -- "every chain at or above min_score" is 1)
    if (o.min_relative_score_ppm < 1 || o.min_relative_score_ppm > 1000000)
        return dh_fail(DH_EINVAL, "min_relative_score_ppm must be in [1, 1000000] (1000000 = the default 1.0; fill the struct with dh_default_process_opts)");
    if (o.rounds < 1 || o.rounds > 8) return dh_fail(DH_EINVAL, "rounds must be in [1, 8]");
    if (o.tspace_pile < 16 || o.tspace_pile > SEG_MAX) return dh_fail(DH_EINVAL, "tspace_pile out of range");
    int32_t pwidth = o.width > 0 ? o.width : 30;
    if (const char *e = getenv("DH_PILE_WIDTH")) pwidth = atoi(e);  // development override
    if (pwidth < 1 || pwidth > 62) return dh_fail(DH_EINVAL, "process: width must be in [1, 62]");
    if (o.algo != 0 && o.algo != 1) return dh_fail(DH_EINVAL, "process: algo must be 0 (DH-1) or 1 (DH-2)");
    if (o.algo == 1) pwidth = o.width == 32 ? 32 : 64;  // DH-2: the band (64 rows; dh_process_opts.width = 32 asks for the narrow one)
    *pwidth_out = pwidth;
    *palgo_out = o.algo;
    return DH_OK;
}

// the result with the records of the crop and the read ids of every pile-up
static void init_result(ProcRun &run)
{
    const dh_cropped *crop = run.crop;
    dh_insertions *res = run.res = new dh_insertions();
    const int32_t np = (int32_t)crop->rec.size();
    res->rec = crop->rec;
    res->flank_of.assign((size_t)np, -1);
    res->ids_off.assign((size_t)np + 1, 0);
    for (int32_t p : crop->pile) res->ids_off[(size_t)p + 1]++;
    for (int32_t p = 0; p < np; p++) res->ids_off[(size_t)p + 1] += res->ids_off[(size_t)p];
    res->ids.resize((size_t)res->ids_off.back());
    std::vector<int32_t> at(res->ids_off.begin(), res->ids_off.end() - 1);
    for (size_t i = 0; i < crop->pile.size(); i++) res->ids[(size_t)at[(size_t)crop->pile[i]]++] = crop->read_id[i];
}

// ---- 1. the pile-up DB: which pile-ups are large enough, which cropped reads they bring, the work of the call
static int plan_pile_db(ProcRun &run, PileLayout &lay)
{
    const dh_process_opts &o = run.o;
    const dh_db *contigs = run.contigs;
    const dh_cropped *crop = run.crop;
    dh_insertions *res = run.res;
    ProcStats &ps = run.ps;
    const int32_t np = (int32_t)crop->rec.size(), ncr = (int32_t)crop->pile.size();
    std::vector<int32_t> active_of((size_t)np, -1);
    for (int32_t p = 0; p < np; p++) {
        dh_insertion &r = res->rec[(size_t)p];
        r.nreads = res->ids_off[(size_t)p + 1] - res->ids_off[(size_t)p];
        if (r.status != DH_PILE_OK) continue;
        if (r.join == 0 && r.contig_right == 0 && r.contig_left + 1 < contigs->n) r.contig_right = r.contig_left + 1;  // records made by hand before the field existed
        if (r.contig_left < 0 || r.contig_left >= contigs->n || ((r.join & DH_JOIN_EXTENSION) ? r.contig_right != -1 : (r.contig_right <= r.contig_left || r.contig_right >= contigs->n)))
            return dh_fail(DH_EINVAL, "dh_process_cropped: gap outside the contigs DB");
        if (r.nreads < o.min_reads)
            r.status = DH_PILE_TOO_SMALL;
        else if (o.max_reads > 0 && r.nreads > o.max_reads)
            return dh_fail(DH_EINVAL, "dh_process_cropped: pile-up with more than max_reads reads");
    }
    for (int32_t i = 0; i < ncr; i++) {
        const int32_t p = crop->pile[(size_t)i];
        if (res->rec[(size_t)p].status != DH_PILE_OK) continue;
        if (active_of[(size_t)p] < 0) {
            active_of[(size_t)p] = (int32_t)lay.pile_of_active.size();
            lay.pile_of_active.push_back(p);
            lay.first_read.push_back((int32_t)lay.keep.size());
        }
        lay.sgroup.push_back(active_of[(size_t)p]);
        lay.keep.push_back(i);
        lay.read_id.push_back(crop->read_id[(size_t)i]);
        const uint8_t kd = crop->kind.empty() ? 0 : crop->kind[(size_t)i];
        // (an extension pile-up has one flank: every read of it has its alignment there)
        lay.rkind.push_back((res->rec[(size_t)p].join & DH_JOIN_EXTENSION) ? ((kd & 3) == 1 ? 0 : 2) : (kd & 3));
        lay.rcomp.push_back(kd >> 2);
    }
    const int32_t na = lay.na = (int32_t)lay.pile_of_active.size();
    lay.first_read.push_back((int32_t)lay.keep.size());
    lay.active_ok.assign((size_t)na, 1);
    lay.ref_of.assign((size_t)na, -1);
    const std::vector<int32_t> &first_read = lay.first_read, &keep = lay.keep;
    for (int32_t a = 0; a < na; a++) {
        const int64_t n_ = first_read[(size_t)a + 1] - first_read[(size_t)a];
        int64_t lsum = 0;
        for (int32_t x = first_read[(size_t)a]; x < first_read[(size_t)a + 1]; x++)
            lsum += crop->off[(size_t)keep[(size_t)x] + 1] - crop->off[(size_t)keep[(size_t)x]];
        ps.work[0] += 1;
        ps.work[1] += n_;
        ps.work[2] += lsum;
        ps.work[3] += n_ * lsum + 2 * lsum / std::max<int64_t>(n_, 1);  // (n^2 + 2) L with L = lsum / n
    }
    return DH_OK;
}

// ... and its bases: slices of the cropped reads on the device, DUST
static int build_pile_db(ProcRun &run, PileLayout &lay)
{
    dh_ctx *ctx = run.ctx;
    hipStream_t st = run.st;
    dh_cropped *crop = run.crop;
    const std::vector<int32_t> &keep = lay.keep;
    HIPCHK(run.tm.mark(0));
    if (!crop->dev) {  // cropped reads came over the host (dh_cropped_create): upload them once
        uint8_t *d_alloc = nullptr, *d_bases = nullptr;
        if (int rc = dh_alloc_bases(st, crop->off.back(), &d_alloc, &d_bases)) return rc;
        if (int rc = dh_db_adopt(ctx, d_alloc, d_bases, crop->off, std::vector<int32_t>(), &crop->dev)) {
            dh_dev_free(d_alloc);
            return rc;
        }
        crop->ctx = ctx;
        if (crop->off.back() > 0)
            HIPCHK(hipMemcpyAsync(d_bases, crop->bases.data(), (size_t)crop->off.back(), hipMemcpyHostToDevice, st));
        HIPCHK(hipStreamSynchronize(st));
        run.tm.lap("cropped reads upload");
    }
    std::vector<int32_t> sbeg(keep.size(), 0), slen(keep.size());
    for (size_t x = 0; x < keep.size(); x++)
        slen[x] = (int32_t)(crop->off[(size_t)keep[x] + 1] - crop->off[(size_t)keep[x]]);
    if (int rc = dh_db_from_slices(ctx, crop->dev, keep, sbeg, slen, lay.sgroup, &lay.pile)) return rc;
    run.dbg.dbs.push_back(lay.pile);
    run.tm.lap("pile DB slices");
    if (run.o.dust)  // DBdust pileup.db; daligner ... -mdust (package.d:476-482)
        if (int rc = dh_db_dust_impl(lay.pile)) return rc;
    HIPCHK(run.tm.mark(1));
    if (int rc = run.tm.add_elapsed(0, 1, run.ps.ms[0])) return rc;
    run.tm.lap("pile DB");
    return DH_OK;
}

// The funnel, the tile QVs, the ranking and the first consensus round read the overlaps of the reads that may serve
// as reference read only (selectAllowedReferenceReadIds, package.d:461-472; findReferenceReadCandidates :518-568):
// pairs of two other reads are not aligned, and of a mixed pair only the record of the allowed read is made.  A
// pile-up without any allowed read keeps every pair (it fails later, with the status it always had).
// DH_PILE_ALL_PAIRS=1 aligns everything (what `daligner pile.db pile.db` itself writes; tests compare the two).
// max_partners (dh_process_opts): the B side of the wanted records is bounded as well -- the first max_partners
// reads of the pile-up in the order allowed reads, then the others, each in pile-up order.
// (DH-2 only: with DH-1 every pair is aligned; oracle/process.py and oracle/pile.c set the same flags.)
static int set_pair_flags(ProcRun &run, PileLayout &lay)
{
    if (getenv("DH_PILE_ALL_PAIRS") || run.palgo != 1) return DH_OK;
    const dh_process_opts &o = run.o;
    std::vector<uint8_t> fl((size_t)lay.pile->n, 3);  // bit 0: records with the read as A are wanted, bit 1: it may be their B
    bool any_cut = false;
    for (int32_t a = 0; a < lay.na; a++) {
        const int32_t r0 = lay.first_read[(size_t)a], r1 = lay.first_read[(size_t)a + 1];
        int32_t nallowed = 0;
        for (int32_t r = r0; r < r1; r++) nallowed += lay.rkind[(size_t)r] == 0 ? 1 : 0;
        if (nallowed == 0) continue;
        const bool cut_b = o.max_partners > 0 && r1 - r0 > o.max_partners;
        int32_t seen_allowed = 0, seen_other = 0;
        for (int32_t r = r0; r < r1; r++) {
            const bool al = lay.rkind[(size_t)r] == 0;
            const int32_t rank = al ? seen_allowed++ : nallowed + seen_other++;  // position in (allowed, then others)
            const bool partner = !cut_b || rank < o.max_partners;
            fl[(size_t)r] = (uint8_t)((al ? 1 : 0) | (partner ? 2 : 0));
            any_cut = any_cut || fl[(size_t)r] != 3;
        }
    }
    return dh_db_set_pflags(lay.pile, any_cut ? fl.data() : nullptr);
}

// ---- 2. pile-up all-vs-all: daligner -s126 -l500 -e0.7 (commandline.d:2886-2902)
static int align_pile(ProcRun &run, PileLayout &lay, FunnelOut &fo)
{
    const dh_db *pile = lay.pile;
    const std::vector<int32_t> &first_read = lay.first_read;
    // record slots per (read, strand): a read overlaps at most every other read of its pile-up
    int32_t most = std::min(run.crop->batch_most, 252);
    for (int32_t a = 0; a < lay.na; a++) most = std::max(most, first_read[(size_t)a + 1] - first_read[(size_t)a]);
    if (most > 252) return dh_fail(DH_EOVERFLOW, "process: a pile-up with more than 252 reads (set max_reads)");
    const int32_t max_la = most <= 60 ? 64 : (most <= 124 ? 128 : 256);
    dh_align_opts ao = run.align_opts(500, max_la, std::min(256, 2 * max_la));
    ao.skip_self = 2;  // every unordered pair aligned once, both records emitted (as daligner does)
    if (int rc = set_pair_flags(run, lay)) return rc;
    HIPCHK(run.tm.mark(0));
    // (2: the trace values stay on the device -- the tile QVs read them there, the first consensus round fetches the
    // overlaps of the reference reads only, 1 / n of them)
    // (4: with DH-2 the records stay on the device as well -- the funnel below runs there, only the overlaps of the
    // reference reads travel; DH_HOST_FUNNEL=1 keeps the host path, which is also the fall-back)
    // (below the default --min-relative-score the chains can share LAs, which are then written once per chain: the host
    // funnel inserts them; the kernel reports a pair in which that happens and the batch comes to the host as well)
    const bool want_dev_funnel = run.palgo == 1 && !getenv("DH_HOST_FUNNEL") && run.o.min_relative_score_ppm == 1000000;
    if (int rc = dh_align_db_ex(run.ctx, lay.pile, lay.pile, &ao, 0, want_dev_funnel ? 6 : 2, &fo.pset)) return rc;
    run.sg.sets.push_back(fo.pset);
    run.tm.lap("pile align call");
    fo.on_dev = fo.pset->d_la != nullptr && fo.pset->d_la_n > 0 && fo.pset->d_trace != nullptr;
    fo.maxtiles = std::max(1, (pile->max_len + run.tsp - 1) / run.tsp);
    fo.qv.assign((size_t)pile->n * fo.maxtiles, 255);
    // cov = max(#allowed reference reads, 4 if pile >= 4) == pile size here (package.d:498-503)
    // (allowed reference reads = the reads that span the gap, selectAllowedReferenceReadIds :461-472)
    fo.cov_of.assign((size_t)pile->n, 1);
    for (int32_t a = 0; a < lay.na; a++) {
        const int32_t r0 = first_read[(size_t)a], r1 = first_read[(size_t)a + 1];
        int32_t cov = 0;
        for (int32_t r = r0; r < r1; r++) cov += lay.rkind[(size_t)r] == 0 ? 1 : 0;
        if (cov < 4 && r1 - r0 >= 4) cov = 4;
        for (int32_t r = r0; r < r1; r++) fo.cov_of[(size_t)r] = std::max(cov, 1);
    }
    return DH_OK;
}

// ---- 3' + 4'. the funnel and the tile QVs on the device copy of the records
static int funnel_on_device(ProcRun &run, PileLayout &lay, FunnelOut &fo)
{
    hipStream_t st = run.st;
    const dh_process_opts &o = run.o;
    const dh_db *pile = lay.pile;
    dh_la_set *pset = fo.pset;
    std::vector<uint8_t> &qv = fo.qv;
    const int32_t npr = pile->n, tsp = run.tsp;
    HIPCHK(run.tm.mark(2));
    DevBuf<int32_t> d_live, d_stat, d_cov;
    DevBuf<uint8_t> d_qv;
    HIPCHK(fo.d_first_keep.alloc((size_t)npr + 1));
    HIPCHK(d_live.alloc((size_t)npr));
    HIPCHK(d_stat.alloc(1));
    HIPCHK(d_cov.alloc(fo.cov_of.size()));
    HIPCHK(d_qv.alloc(qv.size()));
    HIPCHK(hipMemsetAsync(d_stat.p, 0, sizeof(int32_t), st));
    HIPCHK(hipMemcpyAsync(d_cov.p, fo.cov_of.data(), sizeof(int32_t) * fo.cov_of.size(), hipMemcpyHostToDevice, st));
    HIPCHK(dhk_memset(st, d_qv.p, 255, qv.size()));
    dhk_pile_funnel(st, pset->d_la, pset->d_item_off, npr, pile->d_off, o.max_align_err_ppm, tsp, fo.d_first_keep.p, d_live.p, d_stat.p);
    dhk_tile_qv(st, pset->d_la, pset->d_trace, fo.d_first_keep.p, pile->d_off, npr, tsp, d_cov.p, fo.maxtiles, d_qv.p);
    HIPCHK(hipGetLastError());
    fo.la_first.resize((size_t)npr + 1);
    fo.dev_live.resize((size_t)npr);
    int32_t fstat = 0;
    HIPCHK(hipMemcpyAsync(qv.data(), d_qv.p, qv.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fo.la_first.data(), fo.d_first_keep.p, sizeof(int32_t) * fo.la_first.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(fo.dev_live.data(), d_live.p, sizeof(int32_t) * fo.dev_live.size(), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&fstat, d_stat.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    HIPCHK(run.tm.mark(3));
    if (int rc = run.tm.add_elapsed(2, 3, run.ps.ms[2])) return rc;
    if (getenv("DH_FUNNEL_FALLBACK")) fstat = 1;  // (tests: the fall-back below must give the same result)
    if (fstat != 0) {
        // a read or a pair beyond the kernel's capacities: the records come to the host after all (the flags the
        // kernel has set are a subset of what the host path sets: it runs on them unchanged)
        fo.on_dev = false;
        pset->la.resize((size_t)pset->d_la_n);
        HIPCHK(hipMemcpy(pset->la.data(), pset->d_la, sizeof(dh_la) * (size_t)pset->d_la_n, hipMemcpyDeviceToHost));
        for (dh_la &la : pset->la) la.flags &= ~FLAG_IMPROPER;
        std::fill(qv.begin(), qv.end(), (uint8_t)255);
    }
    run.tm.lap("funnel + tile qv (device)");
    return DH_OK;
}

// the host records grouped by A read (the symmetric wave kernel already emits them so); traces stay where they are
static void group_by_aread(const PileLayout &lay, FunnelOut &fo)
{
    const dh_db *pile = lay.pile;
    dh_la_set *pset = fo.pset;
    std::atomic<int> out_of_order{0};
    const dh_la *lp = pset->la.data();
    dh_parallel_for((int64_t)pset->la.size(), 1 << 16, [&](int64_t lo, int64_t hi) {
        for (int64_t i = std::max<int64_t>(lo, 1); i < hi; i++)
            if (lp[i - 1].aread > lp[i].aread) {
                out_of_order = 1;
                break;
            }
    });
    if (out_of_order.load() == 0) return;
    // counting sort, stable
    std::vector<int32_t> cnt((size_t)pile->n + 1, 0);
    for (const dh_la &la : pset->la) cnt[(size_t)la.aread + 1]++;
    for (int32_t r = 0; r < pile->n; r++) cnt[(size_t)r + 1] += cnt[(size_t)r];
    LaVec tmp(pset->la.size());
    for (const dh_la &la : pset->la) tmp[(size_t)cnt[(size_t)la.aread]++] = la;
    pset->la.swap(tmp);
}

// reads whose overlaps did not fit the per-read slots: their pile-up is skipped with a status
// (the reference skips a failing pile-up and carries on, package.d:319-363)
static void mark_overflowed(ProcRun &run, PileLayout &lay, FunnelOut &fo)
{
    const dh_db *pile = lay.pile;
    const dh_la_set *pset = fo.pset;
    for (int32_t r : pset->ovf_reads) {
        const int32_t a = pile->h_group[(size_t)r];
        if (lay.active_ok[(size_t)a]) {
            lay.active_ok[(size_t)a] = 0;
            run.res->rec[(size_t)lay.pile_of_active[(size_t)a]].status = DH_PILE_ALIGN_OVERFLOW;
        }
    }
    if (!pset->ovf_reads.empty())
        for (dh_la &la : fo.pset->la)
            if (!lay.active_ok[(size_t)pile->h_group[(size_t)la.aread]]) la.flags |= DH_FLAG_DISABLED;
}

// ---- 3. the alignment funnel of computeQVs (package.d:474-516): averageErrorRate <=
//         maxAlignmentError -> chainLocalAlignments -> isValidPileUpAlignment with
//         allowance = trace spacing (dazzler.d:4066-4141)
static void funnel_on_host(ProcRun &run, const PileLayout &lay, FunnelOut &fo)
{
    const dh_process_opts &o = run.o;
    const dh_db *pile = lay.pile;
    LaVec &pl = fo.pset->la;
    std::vector<int32_t> &la_first = fo.la_first;
    const int32_t tsp = run.tsp;
    // the funnel of one A read is independent of the others: host threads take read groups
    // (LAs are grouped by aread; inside a group order by bread to get (A, B) pairs)
    // la_first[r] = first LA of A read r (the LAs are grouped by aread): boundaries found in parallel
    la_first.assign((size_t)pile->n + 1, 0);
    {
        const int64_t nl = (int64_t)pl.size();
        const dh_la *lp = pl.data();
        int32_t *lf = la_first.data();
        const int32_t npr_ = pile->n;
        dh_parallel_for(nl + 1, 1 << 16, [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++) {
                const int32_t prev = i == 0 ? -1 : lp[i - 1].aread, cur = i == nl ? npr_ : lp[i].aread;
                for (int32_t r = prev + 1; r <= cur; r++) lf[r] = (int32_t)i;
            }
        });
    }
    const double min_rel = (double)o.min_relative_score_ppm / 1e6;
    std::vector<std::vector<ChainDup>> gdups((size_t)pile->n);  // LAs that alternate chains share, per A read
    dh_parallel_for(pile->n, 64, [&](int64_t glo, int64_t ghi) {
        for (int64_t g = glo; g < ghi; g++) {
            const size_t g0 = (size_t)la_first[(size_t)g], g1 = (size_t)la_first[(size_t)g + 1];
            if (g1 <= g0) continue;
            for (size_t i = g0; i < g1; i++) {
                dh_la &la = pl[i];
                if ((int64_t)la.diffs * 1000000 > (int64_t)o.max_align_err_ppm * (la.aepos - la.abpos))
                    la.flags |= DH_FLAG_DISABLED;
            }
            auto by_b = [](const dh_la &x, const dh_la &y) { return x.bread < y.bread; };
            // the device hands over one bread-ordered run per strand: merge them (stable)
            const auto gb = pl.begin() + (long)g0, ge = pl.begin() + (long)g1;
            const auto mid = std::is_sorted_until(gb, ge, by_b);
            if (mid != ge) {
                if (std::is_sorted(mid, ge, by_b))
                    std::inplace_merge(gb, mid, ge, by_b);
                else
                    std::stable_sort(gb, ge, by_b);
            }
            size_t p0 = g0;
            while (p0 < g1) {
                size_t p1 = p0;
                while (p1 < g1 && pl[p1].bread == pl[p0].bread) p1++;
                chain_pair(pl, p0, p1, tsp, min_rel, gdups[(size_t)g]);
                p0 = p1;
            }
            for (size_t i = g0; i < g1; i++) {
                dh_la &la = pl[i];
                if (la.flags & DH_FLAG_DISABLED) continue;
                const int32_t alen = (int32_t)(pile->h_off[(size_t)la.aread + 1] - pile->h_off[(size_t)la.aread]);
                const int32_t blen = (int32_t)(pile->h_off[(size_t)la.bread + 1] - pile->h_off[(size_t)la.bread]);
                // improper overlaps still count for the tile QVs: DASqv runs on the chained
                // file, filterPileUpAlignments comes after it (package.d:492-512)
                if (!valid_pileup_alignment(la, la.aread == la.bread, alen, blen, tsp))
                    la.flags |= FLAG_IMPROPER;
            }
        }
    });
    // the further occurrences of LAs that alternate chains share: behind their first occurrence (same trace).
    // NOTE (record order): the reference writes every accepted chain as ONE contiguous run (composeAlignmentChain
    // per chain, then acceptedChains.sort(): chaining.d:269-312); here a shared LA's copy sits behind its first
    // occurrence and the chain's other members stay where they were, so in record order two chains may interleave
    // (START(a), START(a'), NEXT(b) ...).  Everything downstream of the funnel works per LA (tile QVs, validity,
    // ranking, the first consensus round); code that walks a chain as "START plus the NEXT records behind it"
    // (dh_chain_view, covering_member, intersect_chain) must NOT be pointed at this output.  Only reachable below
    // min_relative_score 1.0 or with equal-score chains sharing a prefix.
    size_t ndup = 0;
    for (const auto &gd : gdups) ndup += gd.size();
    if (!ndup) return;
    LaVec out;
    out.reserve(pl.size() + ndup);
    std::vector<int32_t> nf((size_t)pile->n + 1, 0);
    for (int32_t g = 0; g < pile->n; g++) {
        nf[(size_t)g] = (int32_t)out.size();
        auto &gd = gdups[(size_t)g];
        std::stable_sort(gd.begin(), gd.end(), [](const ChainDup &x, const ChainDup &y) { return x.i < y.i; });
        size_t d = 0;
        for (size_t i = (size_t)la_first[(size_t)g]; i < (size_t)la_first[(size_t)g + 1]; i++) {
            out.push_back(pl[i]);
            for (; d < gd.size() && gd[d].i == i; d++) {
                dh_la c = pl[i];
                c.flags = gd[d].flags | (pl[i].flags & FLAG_IMPROPER);
                out.push_back(c);
            }
        }
    }
    nf[(size_t)pile->n] = (int32_t)out.size();
    pl.swap(out);
    la_first.swap(nf);
}

// ---- 4. tile QVs on the device (LAs are sorted by aread)
static int tile_qv_of_host_records(ProcRun &run, const PileLayout &lay, FunnelOut &fo)
{
    hipStream_t st = run.st;
    const dh_db *pile = lay.pile;
    const dh_la_set *pset = fo.pset;
    LaVec &pl = fo.pset->la;
    std::vector<uint8_t> &qv = fo.qv;
    HIPCHK(run.tm.mark(0));
    {
        DevBuf<DhLa> d_las;
        DevBuf<uint16_t> d_tr;
        DevBuf<int32_t> d_first;
        DevBuf<uint8_t> d_qv;
        HIPCHK(d_las.alloc(pl.size()));
        HIPCHK(d_first.alloc(fo.la_first.size()));
        HIPCHK(d_qv.alloc(qv.size()));
        HIPCHK(hipMemcpyAsync(d_las.p, pl.data(), sizeof(dh_la) * pl.size(), hipMemcpyHostToDevice, st));
        // the traces of the pile-up alignment are still on the device (no alignment call since)
        const uint16_t *d_trp = pset->d_trace;
        if (!d_trp) {
            HIPCHK(d_tr.alloc(pset->trace.size()));
            HIPCHK(hipMemcpyAsync(d_tr.p, pset->trace.data(), sizeof(uint16_t) * pset->trace.size(), hipMemcpyHostToDevice, st));
            d_trp = d_tr.p;
        }
        HIPCHK(hipMemcpyAsync(d_first.p, fo.la_first.data(), sizeof(int32_t) * fo.la_first.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemsetAsync(d_qv.p, 255, qv.size(), st));
        DevBuf<int32_t> d_cov;
        HIPCHK(d_cov.alloc(fo.cov_of.size()));
        HIPCHK(hipMemcpyAsync(d_cov.p, fo.cov_of.data(), sizeof(int32_t) * fo.cov_of.size(), hipMemcpyHostToDevice, st));
        dhk_tile_qv(st, d_las.p, d_trp, d_first.p, pile->d_off, pile->n, run.tsp, d_cov.p, fo.maxtiles, d_qv.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(qv.data(), d_qv.p, qv.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(run.tm.mark(1));
    if (int rc = run.tm.add_elapsed(0, 1, run.ps.ms[2])) return rc;
    // filterPileUpAlignments (properAlignmentAllowance), dazzler.d:4043-4094: after the QVs
    dh_parallel_for((int64_t)pl.size(), 1 << 16, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            dh_la &la = pl[(size_t)i];
            if (la.flags & FLAG_IMPROPER) la.flags = (la.flags & ~FLAG_IMPROPER) | DH_FLAG_DISABLED;
        }
    });
    return DH_OK;
}

// Sections 3 and 4 on the device copy of the records where the alignment left one and the kernel's capacities hold, on
// the host records otherwise.  ps.ms[1], open since align_pile, takes the all-vs-all up to the grouped records.
static int funnel_and_tile_qv(ProcRun &run, PileLayout &lay, FunnelOut &fo)
{
    if (fo.on_dev)
        if (int rc = funnel_on_device(run, lay, fo)) return rc;  // (the fall-back clears fo.on_dev)
    if (!fo.on_dev) group_by_aread(lay, fo);
    HIPCHK(run.tm.mark(1));
    if (int rc = run.tm.add_elapsed(0, 1, run.ps.ms[1])) return rc;
    run.ps.counters[0] = fo.on_dev ? fo.pset->d_la_n : (int64_t)fo.pset->la.size();
    mark_overflowed(run, lay, fo);
    run.tm.lap("group by aread");
    if (!fo.on_dev) funnel_on_host(run, lay, fo);
    run.tm.lap("filter + chain");
    if (!fo.on_dev)
        if (int rc = tile_qv_of_host_records(run, lay, fo)) return rc;
    run.tm.lap("tile qv");
    return DH_OK;
}

// ---- 5. reference read of one pile-up: findReferenceReadCandidates (package.d:518-568)
static void rank_reference_read(ProcRun &run, PileLayout &lay, const FunnelOut &fo, int32_t a)
{
    const dh_db *pile = lay.pile;
    const LaVec &pl = fo.pset->la;
    const std::vector<uint8_t> &rkind = lay.rkind, &qv = fo.qv;
    const int32_t tsp = run.tsp, maxtiles = fo.maxtiles;
    const int32_t r0 = lay.first_read[(size_t)a], r1 = lay.first_read[(size_t)a + 1];
    bool any = false;
    if (fo.on_dev)
        for (int32_t r = r0; r < r1 && !any; r++) any = fo.dev_live[(size_t)r] > 0;
    else
        for (int32_t i = fo.la_first[(size_t)r0]; i < fo.la_first[(size_t)r1]; i++)
            if (!(pl[(size_t)i].flags & DH_FLAG_DISABLED)) any = true;
    dh_insertion &rec = run.res->rec[(size_t)lay.pile_of_active[(size_t)a]];
    if (!any) {
        if (rec.status == DH_PILE_OK) rec.status = DH_PILE_EMPTY_ALIGNMENT;
        lay.active_ok[(size_t)a] = 0;
        return;
    }
    int64_t hist[MAXQV] = {0};
    int64_t total = 0;
    for (int32_t r = r0; r < r1; r++) {
        if (rkind[(size_t)r] != 0) continue;  // only allowed reference reads enter the histogram and the ranking
        const int32_t len = (int32_t)(pile->h_off[(size_t)r + 1] - pile->h_off[(size_t)r]);
        const int32_t nt = (len + tsp - 1) / tsp;
        for (int32_t t = 0; t < nt; t++) {
            const int32_t q = qv[(size_t)r * maxtiles + t];
            if (q < MAXQV) {
                hist[q]++;
                total++;
            }
        }
    }
    const int64_t bad_thres = (int64_t)((double)run.o.bad_fraction_ppm / 1e6 * (double)total);
    int32_t idx = -1;
    int64_t cum = 0;
    for (int32_t x = 0; x < MAXQV; x++) {
        cum += hist[MAXQV - 1 - x];
        if (cum >= bad_thres) {
            idx = x;
            break;
        }
    }
    const int32_t bad_qv = MAXQV - 1 - idx;
    int32_t best = -1;
    int64_t best_nbad = 0;
    double best_mean = 0;
    for (int32_t r = r0; r < r1; r++) {
        if (rkind[(size_t)r] != 0) continue;
        const int32_t len = (int32_t)(pile->h_off[(size_t)r + 1] - pile->h_off[(size_t)r]);
        const int32_t nt = (len + tsp - 1) / tsp;
        int64_t nb = 0, sum = 0;
        for (int32_t t = 0; t < nt; t++) {
            const int32_t q = qv[(size_t)r * maxtiles + t];
            if (q >= bad_qv) nb++;
            sum += q;
        }
        const double mean = nt > 0 ? (double)sum / (double)nt : 0.0;
        if (best < 0 || nb < best_nbad || (nb == best_nbad && mean < best_mean)) {
            best = r;
            best_nbad = nb;
            best_mean = mean;
        }
    }
    if (best < 0) {  // no read spans the gap: "no valid reference read found" (package.d:335-343)
        if (rec.status == DH_PILE_OK) rec.status = DH_PILE_TOO_SMALL;
        lay.active_ok[(size_t)a] = 0;
        return;
    }
    lay.ref_of[(size_t)a] = best;
    rec.ref_read = best - r0;
    rec.ref_read_id = lay.read_id[(size_t)best];
}

// device funnel: the records of the reference reads, fetched now, and their templates
static int fetch_ref_records(ProcRun &run, const PileLayout &lay, const FunnelOut &fo, LaVec &tl, std::vector<int32_t> &ttm)
{
    hipStream_t st = run.st;
    const std::vector<int32_t> &first = fo.la_first;
    std::vector<int32_t> sel, doff{0};
    for (int32_t a = 0; a < lay.na; a++)
        if (lay.active_ok[(size_t)a] && lay.ref_of[(size_t)a] >= 0) {
            const int32_t r = lay.ref_of[(size_t)a];
            sel.push_back(r);
            doff.push_back(doff.back() + (first[(size_t)r + 1] - first[(size_t)r]));
            ttm.insert(ttm.end(), (size_t)(first[(size_t)r + 1] - first[(size_t)r]), a);
        }
    tl.resize((size_t)doff.back());
    if (!sel.empty() && doff.back() > 0) {
        DevBuf<int32_t> d_sel, d_doff;
        DevBuf<DhLa> d_out;
        HIPCHK(d_sel.alloc(sel.size()));
        HIPCHK(d_doff.alloc(doff.size()));
        HIPCHK(d_out.alloc((size_t)doff.back()));
        HIPCHK(hipMemcpyAsync(d_sel.p, sel.data(), sizeof(int32_t) * sel.size(), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_doff.p, doff.data(), sizeof(int32_t) * doff.size(), hipMemcpyHostToDevice, st));
        dhk_gather_read_records(st, fo.pset->d_la, fo.d_first_keep.p, d_sel.p, d_doff.p, (int32_t)sel.size(), d_out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(tl.data(), d_out.p, sizeof(dh_la) * tl.size(), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    return DH_OK;
}

// ---- 6. consensus rounds.  Templates are indexed by active pile-up (group = active idx).  The first round votes with
// the overlaps of the reference reads from the pile-up alignment; *T: the reference reads, then their consensus
static int first_consensus_round(ProcRun &run, const PileLayout &lay, const FunnelOut &fo, dh_db **T)
{
    dh_ctx *ctx = run.ctx;
    hipStream_t st = run.st;
    dh_db *pile = lay.pile;
    const dh_la_set *pset = fo.pset;
    const LaVec &pl = pset->la;
    const bool on_dev = fo.on_dev;
    const int32_t na = lay.na;
    std::vector<int32_t> tidx, tbeg, tlen, tgrp;
    for (int32_t a = 0; a < na; a++) {
        const int32_t r = lay.ref_of[(size_t)a] >= 0 ? lay.ref_of[(size_t)a] : lay.first_read[(size_t)a];
        tidx.push_back(r);
        tbeg.push_back(0);
        tlen.push_back((int32_t)(pile->h_off[(size_t)r + 1] - pile->h_off[(size_t)r]));
        tgrp.push_back(a);
    }
    if (int rc = dh_db_from_slices(ctx, pile, tidx, tbeg, tlen, tgrp, T)) return rc;
    run.dbg.dbs.push_back(*T);
    std::vector<int32_t> tmpl_of(on_dev ? 0 : pl.size());
    if (!on_dev)
        dh_parallel_for((int64_t)pl.size(), 1 << 16, [&](int64_t lo, int64_t hi) {
            for (int64_t i = lo; i < hi; i++) {
                const int32_t a = pile->h_group[(size_t)pl[(size_t)i].aread];
                tmpl_of[(size_t)i] = (lay.active_ok[(size_t)a] && pl[(size_t)i].aread == lay.ref_of[(size_t)a]) ? a : -1;
            }
        });
    HIPCHK(run.tm.mark(0));
    dh_db *nT = nullptr;
    int64_t nseg = 0, ncell = 0;
    if (pset->d_trace_len > 0) {
        // the overlaps of the reference reads and their trace values, gathered on the device
        LaVec tl;
        std::vector<int32_t> ttm;
        if (on_dev) {
            if (int rc = fetch_ref_records(run, lay, fo, tl, ttm)) return rc;
        } else {
            std::vector<size_t> tsel;
            for (size_t i = 0; i < pl.size(); i++)
                if (tmpl_of[i] >= 0) tsel.push_back(i);
            tl.resize(tsel.size());
            ttm.resize(tsel.size());
            for (size_t q = 0; q < tsel.size(); q++) {
                tl[q] = pl[tsel[q]];
                ttm[q] = tmpl_of[tsel[q]];
            }
        }
        std::vector<int64_t, PinnedAlloc<int64_t>> desc(3 * tl.size());
        int64_t tot = 0;
        for (size_t q = 0; q < tl.size(); q++) {
            desc[3 * q] = tl[q].toff;
            desc[3 * q + 1] = tot;
            desc[3 * q + 2] = tl[q].tlen;
            if (tl[q].toff < 0 || tl[q].toff + tl[q].tlen > pset->d_trace_len)
                return dh_fail(DH_EINVAL, "process: trace range outside the pile-up alignment's trace");
            tl[q].toff = tot;
            tot += tl[q].tlen;
        }
        TraceVec ttrace((size_t)tot);
        DevBuf<int64_t> d_desc;
        DevBuf<uint16_t> d_tt;
        HIPCHK(d_desc.alloc(desc.size()));
        HIPCHK(d_tt.alloc((size_t)tot));
        if (!tl.empty()) {
            HIPCHK(hipMemcpyAsync(d_desc.p, desc.data(), sizeof(int64_t) * desc.size(), hipMemcpyHostToDevice, st));
            dhk_gather_ranges16(st, pset->d_trace, d_desc.p, (int32_t)tl.size(), d_tt.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(ttrace.data(), d_tt.p, sizeof(uint16_t) * (size_t)tot, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        if (int rc = consensus_round(ctx, *T, pile, tl, ttrace, ttm, run.tsp, &nT, &nseg, &ncell)) return rc;
    } else if (int rc = consensus_round(ctx, *T, pile, pl, pset->trace, tmpl_of, run.tsp, &nT, &nseg, &ncell))
        return rc;
    run.dbg.dbs.push_back(nT);
    *T = nT;
    run.ps.counters[1] += nseg;
    run.ps.counters[2] += ncell;
    HIPCHK(run.tm.mark(1));
    return run.tm.add_elapsed(0, 1, run.ps.ms[3]);
}

// ---- 7. flank re-alignment: daligner -A -s126 -l126 contigs consensus (commandline.d:2918-2935)
// one slice of the flank DB per flank of a pile-up (package.d:631-667 builds the DB from the croppingPositions'
// contigs): the contig's tail for a back-seeded flank, its head for a front-seeded one
static int align_flanks(ProcRun &run, const PileLayout &lay, dh_db *T, FlankOut &fk)
{
    const dh_process_opts &o = run.o;
    const dh_db *contigs = run.contigs;
    const int32_t na = lay.na, tsp = run.tsp;
    std::vector<int32_t> fidx, fgrp;
    fk.fbase.assign((size_t)na + 1, 0);
    for (int32_t a = 0; a < na; a++) {
        const dh_insertion &rec = run.res->rec[(size_t)lay.pile_of_active[(size_t)a]];
        const int32_t nf = (rec.join & DH_JOIN_EXTENSION) ? 1 : 2;
        // flank_window <= 0: the whole contigs, as the reference hands them to daligner (commandline.d:2918-2935)
        const int32_t fw = o.flank_window > 0 ? o.flank_window : INT32_MAX;
        fk.fbase[(size_t)a] = (int32_t)fidx.size();
        for (int32_t f = 0; f < nf; f++) {
            const int32_t g = f == 0 ? rec.contig_left : rec.contig_right;
            const bool front = f == 0 ? (rec.join & DH_JOIN_FLANK0_FRONT) != 0 : (rec.join & DH_JOIN_FLANK1_BACK) == 0;
            const int32_t cl = (int32_t)(contigs->h_off[(size_t)g + 1] - contigs->h_off[(size_t)g]);
            // (a tail window starts on the trace grid of the contig: tiles, and with them the alignment, are those of the whole contig)
            const int32_t wl = front ? 0 : std::max(0, cl - std::min(cl, fw)) / tsp * tsp;
            fidx.push_back(g);
            fk.fbeg.push_back(wl);
            fk.flen.push_back(front ? std::min(cl, fw) : cl - wl);
            fgrp.push_back(a);
        }
    }
    fk.fbase[(size_t)na] = (int32_t)fidx.size();
    dh_db *F = nullptr;
    if (int rc = dh_db_from_slices(run.ctx, contigs, fidx, fk.fbeg, fk.flen, fgrp, &F, true)) return rc;
    run.dbg.dbs.push_back(F);
    if (o.dust)  // DBdust contigs.dam; daligner -A ... -mdust -mrep (package.d:631-667)
        if (int rc = dh_db_dust_impl(F)) return rc;
    const dh_align_opts fo = run.align_opts(126, 4, 32);
    HIPCHK(run.tm.mark(0));
    if (int rc = dh_align_db_ex(run.ctx, F, T, &fo, 0, 0, &fk.fset)) return rc;
    run.sg.sets.push_back(fk.fset);
    HIPCHK(run.tm.mark(1));
    if (int rc = run.tm.add_elapsed(0, 1, run.ps.ms[5])) return rc;
    run.tm.lap("flank align");
    return DH_OK;
}

// The insertion of active pile-up a from its consensus (cons: the bases of T) and its flank overlaps (fl: their indices
// in fk.fset): the consensus and the splice coordinates go into the record, the status comes back.
static int32_t insertion_of_pile(ProcRun &run, const PileLayout &lay, const FlankOut &fk, const dh_db *T,
                                 const std::vector<uint8_t> &cons, const std::vector<int32_t> &fl, int32_t a)
{
    const dh_process_opts &o = run.o;
    dh_insertions *res = run.res;
    const dh_la_set *fset = fk.fset;
    const std::vector<int32_t> &fbeg = fk.fbeg, &fbase = fk.fbase;
    const int32_t tsp = run.tsp, ref = lay.ref_of[(size_t)a];
    dh_insertion &rec = res->rec[(size_t)lay.pile_of_active[(size_t)a]];
    const int64_t c0 = T->h_off[(size_t)a], c1 = T->h_off[(size_t)a + 1];
    rec.cons_off = (int64_t)res->bases.size();
    rec.cons_len = (int32_t)(c1 - c0);
    res->bases.insert(res->bases.end(), cons.begin() + c0, cons.begin() + c1);
    const int32_t clen = rec.cons_len;
    const int32_t nf = (rec.join & DH_JOIN_EXTENSION) ? 1 : 2;
    const bool front[2] = {(rec.join & DH_JOIN_FLANK0_FRONT) != 0, (rec.join & DH_JOIN_FLANK1_BACK) == 0};
    // the consensus has the orientation of the reference read: an overlap whose complement flag differs from the
    // reference read's alignment on that contig is disabled (package.d:669-690); of the others exactly one per
    // flank must be a proper insertion overlap (:707-745)
    const uint8_t refc = ref >= 0 ? lay.rcomp[(size_t)ref] : 0;
    const bool refc_known = run.crop->comp_known && ref >= 0;
    const dh_la *ov[2] = {nullptr, nullptr};
    int cnt[2] = {0, 0};
    for (int32_t i : fl) {
        const dh_la &la = fset->la[(size_t)i];
        const int32_t f = la.aread - fbase[(size_t)a];
        if (f < 0 || f >= nf) continue;
        if (refc_known && ((la.flags & DH_FLAG_COMP) != 0) != (((refc >> f) & 1) != 0)) continue;
        const int32_t fl_len = fk.flen[(size_t)la.aread];
        const bool proper = front[f] ? (la.abpos <= tsp && la.bepos + tsp >= clen) : (la.aepos + tsp >= fl_len && la.bbpos <= tsp);
        if (proper) {
            ov[f] = &la;
            cnt[f]++;
        }
    }
    if (cnt[0] != 1 || (nf == 2 && cnt[1] != 1)) return DH_PILE_FLANKS_NOT_UNIQUE;
    const dh_la *L = ov[0], *R = ov[1];
    // insertionAlignment.isParallel == referenceRead.isParallel (package.d:757-773): seeds differ <=> complements equal
    if (nf == 2 && ((L->flags & DH_FLAG_COMP) == (R->flags & DH_FLAG_COMP)) != (front[0] != front[1])) return DH_PILE_ORIENTATION;
    rec.left_diffs = L->diffs;
    rec.right_diffs = R ? R->diffs : 0;
    // ensureHighQualityConsensus, output.d:388-410
    for (int32_t f = 0; f < nf; f++)
        if ((int64_t)ov[f]->diffs * 1000000 > (int64_t)o.max_ins_err_ppm * (ov[f]->aepos - ov[f]->abpos))
            return DH_PILE_MAX_INSERTION_ERROR;
    for (int32_t f = 0; f < nf; f++) {  // kept for insertions.db (dh_insertions_write_db)
        dh_la c = *ov[f];
        const int32_t shift = fbeg[(size_t)(fbase[(size_t)a] + f)];
        c.abpos += shift;
        c.aepos += shift;
        c.toff = (int64_t)res->flank_tr.size();
        res->flank_tr.insert(res->flank_tr.end(), fset->trace.begin() + ov[f]->toff, fset->trace.begin() + ov[f]->toff + ov[f]->tlen);
        if (f == 0) res->flank_of[(size_t)lay.pile_of_active[(size_t)a]] = (int32_t)res->flank.size();
        res->flank.push_back(c);
    }
    rec.comp = (L->flags & DH_FLAG_COMP) ? 1 : 0;
    // getCroppingPosition!"contigA" (insertions.d:110-121): front seed = begin of the overlap, back seed = its end
    const int32_t sh0 = fbeg[(size_t)fbase[(size_t)a]];
    rec.left_aepos = sh0 + (front[0] ? L->abpos : L->aepos);
    // getCroppingPosition!"contigB" (:124-146) in the frame of the flank-0 overlap
    const int32_t p0 = front[0] ? L->bbpos : L->bepos;
    if (nf == 2) {
        const int32_t sh1 = fbeg[(size_t)fbase[(size_t)a] + 1];
        rec.right_abpos = sh1 + (front[1] ? R->abpos : R->aepos);
        int32_t p1 = front[1] ? R->bbpos : R->bepos;
        if ((R->flags & DH_FLAG_COMP) != (L->flags & DH_FLAG_COMP)) p1 = clen - p1;
        // walking away from flank 0: past the end of a back-seeded overlap, before the begin of a front-seeded one
        rec.ins_begin = front[0] ? p1 : p0;
        rec.ins_end = front[0] ? p0 : p1;
    } else {
        rec.right_abpos = -1;
        rec.ins_begin = front[0] ? 0 : p0;
        rec.ins_end = front[0] ? p0 : clen;
    }
    return rec.ins_end < rec.ins_begin ? DH_PILE_NEGATIVE_INSERTION : DH_PILE_OK;
}

// ---- 8. consensus bases to the host, insertion per pile-up
static int make_insertions(ProcRun &run, const PileLayout &lay, const FlankOut &fk, const dh_db *T)
{
    const int32_t na = lay.na;
    std::vector<uint8_t> cons((size_t)std::max<int64_t>(T->total, 1));
    if (T->total > 0) HIPCHK(hipMemcpy(cons.data(), T->d_bases, (size_t)T->total, hipMemcpyDeviceToHost));
    // the flank overlaps of a pile-up: B = its consensus; records are grouped by B read or not -- index them once
    const LaVec &fla = fk.fset->la;
    std::vector<std::vector<int32_t>> fl_of((size_t)na);
    for (size_t i = 0; i < fla.size(); i++)
        if (fla[i].bread >= 0 && fla[i].bread < na) fl_of[(size_t)fla[i].bread].push_back((int32_t)i);
    for (int32_t a = 0; a < na; a++)
        if (lay.active_ok[(size_t)a])
            run.res->rec[(size_t)lay.pile_of_active[(size_t)a]].status = insertion_of_pile(run, lay, fk, T, cons, fl_of[(size_t)a], a);
    return DH_OK;
}

// The pile-up stages of `dentist process` after the crop (package.d:283-374): pile-up alignment ->
// filter -> tile QV -> reference read -> consensus -> flank re-alignment -> insertion.
extern "C" int dh_process_cropped(dh_ctx *ctx, dh_db *contigs, dh_cropped *crop, const dh_process_opts *opts,
                                  dh_insertions **out)
{
    int32_t pwidth = 0, palgo = 0;
    if (int rc = check_process_opts(ctx, contigs, crop, opts, out, &pwidth, &palgo)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ProcRun run{ctx, ctx->stream, *opts, contigs, crop, opts->tspace_pile, pwidth, palgo};
    ProcStats &ps = run.ps;
    ps.ms[0] = crop->ms_crop;
    if (int rc = run.tm.init(run.st)) return rc;
    init_result(run);
    PileLayout lay;
    if (int rc = plan_pile_db(run, lay)) return rc;
    if (int rc = build_pile_db(run, lay)) return rc;
    if (lay.na > 0) {
        FunnelOut fo;
        FlankOut fk;
        dh_db *T = nullptr;  // the templates: the reference reads, then the consensus of every round
        if (int rc = align_pile(run, lay, fo)) return rc;
        if (int rc = funnel_and_tile_qv(run, lay, fo)) return rc;
        dh_parallel_for(lay.na, 8, [&](int64_t alo, int64_t ahi) {
            for (int32_t a = (int32_t)alo; a < (int32_t)ahi; a++) rank_reference_read(run, lay, fo, a);  // pile-ups are independent
        });
        run.tm.lap("rank reference reads");
        if (int rc = first_consensus_round(run, lay, fo, &T)) return rc;
        const dh_align_opts ro = run.align_opts(500, 4, 32);
        for (int32_t round = 1; round < run.o.rounds; round++)
            if (int rc = realign_round(ctx, lay.pile, ro, &lay.active_ok, run.dbg, run.sg, &run.tm, &ps, &T)) return rc;
        run.tm.lap("consensus rounds");
        if (int rc = align_flanks(run, lay, T, fk)) return rc;
        if (int rc = make_insertions(run, lay, fk, T)) return rc;
    }
    run.tm.lap("insertions");
    ps.ms[6] = ps.ms[0] + ps.ms[1] + ps.ms[2] + ps.ms[3] + ps.ms[4] + ps.ms[5];
    g_pstats = ps;
    *out = run.res;
    run.res = nullptr;
    return DH_OK;
}
