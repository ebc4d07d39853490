// dh_rounds.cpp -- the consensus rounds of the pile-up path: one vote + emission round over tile descriptors
// (consensus_round: k_seg_vote, k_votes_finish, k_emit), a re-alignment round around it (realign_round), and the two
// stages that are entry points of their own: dh_tile_qv (DAScover + DASqv) and dh_consensus (daccord).
#include <array>
#include <mutex>
#include <numeric>

#include "dh_process.h"
#include "dh_parallel.h"

extern "C" {
void dhk_gather_slices(hipStream_t st, const uint8_t *src, const int64_t *src_off, const int32_t *sidx,
                       const int32_t *sbeg, const int64_t *dst_off, int32_t n, int32_t max_len,
                       uint8_t *dst);
void dhk_tile_qv(hipStream_t st, const DhLa *las, const uint16_t *trace, const int32_t *la_first,
                 const int64_t *roff, int32_t nreads, int32_t tspace, const int32_t *cov, int32_t maxtiles,
                 uint8_t *qv);
void dhk_seg_vote(hipStream_t st, const void *segs, int32_t nseg, DbView T, DbView R,
                  const uint8_t *rrc, const int64_t *voff, uint32_t *dmat, int32_t bandmax, int32_t qmax,
                  int32_t ncolmax, uint8_t *opbuf, uint16_t *nops, uint32_t *votes, uint32_t *cdiff,
                  uint32_t *vother, int32_t *status, int32_t mode);
void dhk_votes_finish(hipStream_t st, DbView T, const int64_t *voff, const int32_t *col_tmpl, int64_t ncols_total,
                      const uint32_t *cexcl, const uint32_t *vother, uint32_t *votes);
void dhk_col_tmpl(hipStream_t st, const int64_t *voff, int32_t ntmpl, int64_t ncols_total, int32_t *col_tmpl);
void dhk_emit(hipStream_t st, DbView T, int32_t ntmpl, const int64_t *voff, const uint32_t *votes,
              const int32_t *col_tmpl, int64_t ncols_total, uint8_t *stage, uint8_t *cnt,
              const int64_t *out_off, uint8_t *out, int32_t *out_len);
}

#define MAXINS 4
#define VSTRIDE (6 + 4 * MAXINS)

namespace {
struct SegDescH {
    int32_t tmpl, a0, a1, bseq, b0, b1, comp, band;
};
}  // namespace

namespace dhp {

// ------------------------------------------------------------------------------------ consensus round

// One voting + emission round.  T: templates (one per active pile-up), R: pile-up reads.
// las: overlaps with A = a template coordinate system; tmpl_of[i] = template of LA i or -1.
int consensus_round(dh_ctx *ctx, dh_db *T, dh_db *R, const LaVec &las,
                           const TraceVec &trace, const std::vector<int32_t> &tmpl_of,
                           int32_t ts, dh_db **newT, int64_t *nseg_out, int64_t *ncell_out)
{
    hipStream_t st = ctx->stream;
    std::vector<SegDescH, PinnedAlloc<SegDescH>> segs;  // page-locked: uploaded every round
    int32_t wmax = 1, bandmax = 1;
    int64_t ncell = 0;
    size_t class_end[3] = {0, 0, 0};  // tiles of the overlaps of each band class end here (classes are contiguous)
    {
        // the selected overlaps and where their tiles go; host threads then fill the tiles
        std::vector<size_t> sel;
        std::vector<size_t> soff(1, 0);
        {
            // selection in input order: host threads scan runs of the LAs, the runs are concatenated
            const int64_t grain = 1 << 16, nch = ((int64_t)las.size() + grain - 1) / grain;
            // overlaps are grouped by the widest band of their tiles (tile diffs + 1): up to 31 / up to 63 cells take
            // the bit-parallel fill with one / two words per matrix row, wider ones the scalar fill (dhk_seg_vote)
            std::vector<std::array<std::vector<size_t>, 3>> part((size_t)std::max<int64_t>(nch, 1));
            dh_parallel_for(nch, 1, [&](int64_t clo, int64_t chi) {
                for (int64_t c = clo; c < chi; c++) {
                    const size_t i1 = std::min(las.size(), (size_t)(c + 1) * (size_t)grain);
                    for (size_t i = (size_t)c * (size_t)grain; i < i1; i++)
                        if (tmpl_of[i] >= 0 && !(las[i].flags & DH_FLAG_DISABLED)) {
                            // an overlap with a tile spanning more than SEG_MAX B bases (a > 100 % local
                            // indel rate) takes no part in the vote
                            const uint16_t *tr = trace.data() + las[i].toff;
                            bool too_long = false;
                            int32_t dmax = 0;
                            for (int32_t e = 0; e < las[i].tlen / 2; e++) {
                                too_long = too_long || tr[2 * e + 1] > SEG_MAX;
                                dmax = std::max<int32_t>(dmax, tr[2 * e]);
                            }
                            if (!too_long) part[(size_t)c][dmax + 1 <= 31 ? 0 : (dmax + 1 <= 63 ? 1 : 2)].push_back(i);
                        }
                }
            });
            for (int cls = 0; cls < 3; cls++) {
                for (const auto &v : part)
                    for (size_t i : v[(size_t)cls]) {
                        sel.push_back(i);
                        soff.push_back(soff.back() + (size_t)(las[i].tlen / 2));
                    }
                class_end[cls] = soff.back();
            }
        }
        segs.resize(soff.back());
        std::mutex red;
        dh_parallel_for((int64_t)sel.size(), 256, [&](int64_t lo_, int64_t hi_) {
            int32_t wm = 1, bm = 1;
            int64_t nc = 0;
            for (int64_t q = lo_; q < hi_; q++) {
                const size_t i = sel[(size_t)q];
                const int32_t t = tmpl_of[i];
                const dh_la &la = las[i];
                const uint16_t *tr = trace.data() + la.toff;
                SegDescH *out = segs.data() + soff[(size_t)q];
                int32_t a0 = la.abpos, b0 = la.bbpos;
                for (int32_t e = 0; e < la.tlen / 2; e++) {
                    int32_t a1 = (a0 / ts + 1) * ts;
                    if (a1 > la.aepos) a1 = la.aepos;
                    const int32_t b1 = b0 + tr[2 * e + 1];
                    // DP band: the trace's own path through the tile bounds the optimum (k_seg_vote)
                    const int32_t band = std::min<int32_t>((int32_t)tr[2 * e], std::max(a1 - a0, b1 - b0)) + 1;
                    out[e] = SegDescH{t, a0, a1, la.bread, b0, b1, (int32_t)(la.flags & DH_FLAG_COMP), band};
                    wm = std::max(wm, b1 - b0);
                    bm = std::max(bm, band);
                    nc += (int64_t)(a1 - a0) * std::min(b1 - b0, 2 * band + 1);
                    a0 = a1;
                    b0 = b1;
                }
            }
            std::lock_guard<std::mutex> lk(red);
            wmax = std::max(wmax, wm);
            bandmax = std::max(bandmax, bm);
            ncell += nc;
        });
    }
    *nseg_out = (int64_t)segs.size();
    *ncell_out = ncell;
    const int32_t nt = T->n;
    std::vector<int64_t> voff((size_t)nt + 1, 0), ooff((size_t)nt + 1, 0);
    for (int32_t t = 0; t < nt; t++) {
        const int64_t len = T->h_off[(size_t)t + 1] - T->h_off[(size_t)t];
        voff[(size_t)t + 1] = voff[(size_t)t] + len + 1;
        ooff[(size_t)t + 1] = ooff[(size_t)t] + len * (1 + 2 * MAXINS) + 8;
    }
    // big per-round buffers come from the context's grow-only scratch arena (the SLOT_PR_* group)
    struct { int64_t *p; } d_voff, d_ooff;
    struct { uint32_t *p; } d_votes;
    struct { uint8_t *p; } d_out, d_stage, d_cnt;
    struct { int32_t *p; } d_status, d_outlen, d_coltmpl;
#define SCRP(id, buf, count)                                                                     \
    if (int rc_ = dh_scratch(ctx, id, sizeof(*buf.p) * std::max<size_t>((size_t)(count), 1), (void **)&buf.p)) return rc_;
    SCRP(SLOT_PR_VOFF, d_voff, voff.size() + ooff.size())
    d_ooff.p = d_voff.p + voff.size();
    SCRP(SLOT_PR_VOTES, d_votes, (size_t)voff.back() * VSTRIDE)
    SCRP(SLOT_PR_OUT, d_out, (size_t)ooff.back())
    SCRP(SLOT_PR_STATUS, d_status, 2 + (size_t)nt + (size_t)voff.back())
    d_outlen.p = d_status.p + 2;
    d_coltmpl.p = d_outlen.p + nt;
    SCRP(SLOT_PR_STAGE, d_stage, (size_t)voff.back() * (2 + 2 * MAXINS))
    d_cnt.p = d_stage.p + (size_t)voff.back() * (1 + 2 * MAXINS);
    HIPCHK(hipMemcpyAsync(d_voff.p, voff.data(), sizeof(int64_t) * voff.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_ooff.p, ooff.data(), sizeof(int64_t) * ooff.size(), hipMemcpyHostToDevice, st));
    HIPCHK(dhk_memset(st, d_votes.p, 0, sizeof(uint32_t) * (size_t)voff.back() * VSTRIDE));
    HIPCHK(hipMemsetAsync(d_status.p, 0, sizeof(int32_t), st));
    // sparse votes: cover difference array and "other code" counts per column, scan partial sums
    const size_t ncolp = (size_t)voff.back() + 2;
    struct { uint32_t *p; } d_cdiff;
    SCRP(SLOT_PR_CDIFF, d_cdiff, 2 * ncolp + ncolp / 2048 + 8)
    uint32_t *d_vother = d_cdiff.p + ncolp, *d_csums = d_vother + ncolp;
    HIPCHK(dhk_memset(st, d_cdiff.p, 0, sizeof(uint32_t) * 2 * ncolp));
    if (int rc = dh_ensure_rc(R)) return rc;
    // the decision matrices of one launch live interleaved in HBM: bound the launch to ~6 GB
    for (int cls = 0; cls < 3; cls++) {
        const size_t c0 = cls ? class_end[cls - 1] : 0, c1 = class_end[cls];
        if (c1 <= c0) continue;
        const int32_t mode = getenv("DH_CONS_SCALAR") ? 0 : (cls == 0 ? 1 : (cls == 1 ? 2 : 0));  // (development: scalar fill for everything)
        // bytes of decisions per matrix row: two bit planes of 64 cells per word, or 2 bits per band cell
        const size_t mrow = mode ? (size_t)16 * (size_t)mode : 4 * (size_t)((2 * bandmax + 16) >> 4);
        const int64_t per_dp = (int64_t)(ts + 1) * (int64_t)mrow + 2 * SEG_MAX;
        const int64_t max_dp = std::max<int64_t>(4096, (6ll << 30) / per_dp);
        for (size_t s0 = c0; s0 < c1; s0 += (size_t)max_dp) {
            const int32_t cnt = (int32_t)std::min<size_t>((size_t)max_dp, c1 - s0);
            struct { SegDescH *p; } ds;
            struct { uint8_t *p; } fm, ob;
            SCRP(SLOT_PR_SEGS, ds, (size_t)cnt)
            SCRP(SLOT_PR_DECISIONS, fm, (size_t)cnt * (size_t)(ts + 1) * mrow + (size_t)cnt * 2 * SEG_MAX + (size_t)cnt * 2 + 32)
            ob.p = fm.p + (((size_t)cnt * (size_t)(ts + 1) * mrow + 7) & ~(size_t)7);  // op words: 8 ops each, 8-byte aligned
            uint16_t *d_nops = (uint16_t *)(ob.p + (((size_t)cnt * 2 * SEG_MAX + 7) & ~(size_t)7));
            HIPCHK(hipMemcpyAsync(ds.p, segs.data() + s0, sizeof(SegDescH) * (size_t)cnt, hipMemcpyHostToDevice, st));
            dhk_seg_vote(st, ds.p, cnt, T->view(), R->view(), R->d_rc, d_voff.p, (uint32_t *)fm.p, bandmax, wmax, ts,
                         ob.p, d_nops, d_votes.p, d_cdiff.p, d_vother, d_status.p, mode);
            HIPCHK(hipGetLastError());
            HIPCHK(hipStreamSynchronize(st));
        }
    }
    {
        // column -> template map of the vote space (-1 for the spare column after each template)
        dhk_col_tmpl(st, d_voff.p, nt, voff.back(), d_coltmpl.p);
        HIPCHK(dhk_memset(st, d_cnt.p, 0, (size_t)voff.back()));
        dhk_scan(st, d_cdiff.p, (int64_t)ncolp, d_csums);  // exclusive: cover of column x = [x + 1]
        dhk_votes_finish(st, T->view(), d_voff.p, d_coltmpl.p, voff.back(), d_cdiff.p, d_vother, d_votes.p);
        dhk_emit(st, T->view(), nt, d_voff.p, d_votes.p, d_coltmpl.p, voff.back(), d_stage.p, d_cnt.p, d_ooff.p,
                 d_out.p, d_outlen.p);
        HIPCHK(hipStreamSynchronize(st));
    }
    HIPCHK(hipGetLastError());
    std::vector<int32_t> outlen((size_t)nt);
    int32_t status = 0;
    HIPCHK(hipMemcpyAsync(outlen.data(), d_outlen.p, sizeof(int32_t) * (size_t)nt, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&status, d_status.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (status) return dh_fail(DH_EOVERFLOW, "consensus: tile exceeds the score-matrix capacity");
    // compact the emitted sequences into the next template DB (device to device)
    std::vector<int64_t> noff((size_t)nt + 1, 0);
    int32_t max_len = 0;
    for (int32_t t = 0; t < nt; t++) {
        noff[(size_t)t + 1] = noff[(size_t)t] + outlen[(size_t)t];
        max_len = std::max(max_len, outlen[(size_t)t]);
    }
    uint8_t *d_alloc = nullptr, *d_bases = nullptr;
    if (int rc = dh_alloc_bases(st, noff.back(), &d_alloc, &d_bases)) return rc;
    if (int rc = dh_db_adopt(ctx, d_alloc, d_bases, noff, T->h_group, newT)) {
        dh_dev_free(d_alloc);
        return rc;
    }
    std::vector<int32_t> ident((size_t)nt), zero((size_t)nt, 0);
    std::iota(ident.begin(), ident.end(), 0);
    DevBuf<int32_t> d_id, d_zero;
    HIPCHK(d_id.alloc((size_t)nt));
    HIPCHK(d_zero.alloc((size_t)nt));
    HIPCHK(hipMemcpyAsync(d_id.p, ident.data(), sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_zero.p, zero.data(), sizeof(int32_t) * (size_t)nt, hipMemcpyHostToDevice, st));
    dhk_gather_slices(st, d_out.p, d_ooff.p, d_id.p, d_zero.p, (*newT)->d_off, nt, max_len, d_bases);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}

// the alignment calls of the pile-up path differ in the shortest overlap and in the record / candidate slots per item
dh_align_opts pile_align_opts(int32_t tspace, int32_t min_len, int32_t max_la, int32_t max_cand)
{
    dh_align_opts ao;
    dh_default_align_opts(&ao);
    ao.tspace = tspace;
    ao.min_len = min_len;
    ao.max_la = max_la;
    ao.max_cand = max_cand;
    return ao;
}

// One re-alignment + vote round: every read of R against the templates *T, the overlaps that fail
// isValidPileUpAlignment dropped, the vote; *T becomes the round's consensus.  active_ok (NULL: all of them): the
// templates that still vote.  tm and ps (both NULL: none kept) take the times and counts of dh_process_cropped.
int realign_round(dh_ctx *ctx, dh_db *R, const dh_align_opts &ro, const std::vector<uint8_t> *active_ok, DbGuard &dbg,
                         SetGuard &sg, ProcTimer *tm, ProcStats *ps, dh_db **T)
{
    const dh_db *T0 = *T;
    dh_la_set *rset = nullptr;
    if (tm) HIPCHK(tm->mark(0));
    if (int rc = dh_align_db_ex(ctx, *T, R, &ro, 0, 0, &rset)) return rc;
    sg.sets.push_back(rset);
    if (tm) {
        HIPCHK(tm->mark(1));
        if (int rc = tm->add_elapsed(0, 1, ps->ms[4])) return rc;
    }
    std::vector<int32_t> tmpl_of(rset->la.size(), -1);
    for (size_t i = 0; i < rset->la.size(); i++) {
        dh_la &la = rset->la[i];
        const int32_t a = la.aread;
        const int32_t alen = (int32_t)(T0->h_off[(size_t)a + 1] - T0->h_off[(size_t)a]);
        const int32_t blen = (int32_t)(R->h_off[(size_t)la.bread + 1] - R->h_off[(size_t)la.bread]);
        if (!valid_pileup_alignment(la, false, alen, blen, ro.tspace)) la.flags |= DH_FLAG_DISABLED;
        if (!active_ok || (*active_ok)[(size_t)a]) tmpl_of[i] = a;
    }
    if (tm) HIPCHK(tm->mark(0));
    dh_db *nT = nullptr;
    int64_t nseg = 0, ncell = 0;
    if (int rc = consensus_round(ctx, *T, R, rset->la, rset->trace, tmpl_of, ro.tspace, &nT, &nseg, &ncell)) return rc;
    dbg.dbs.push_back(nT);
    *T = nT;
    if (tm) {
        ps->counters[1] += nseg;
        ps->counters[2] += ncell;
        HIPCHK(tm->mark(1));
        if (int rc = tm->add_elapsed(0, 1, ps->ms[3])) return rc;
    }
    return DH_OK;
}

}  // namespace dhp

using namespace dhp;

// ------------------------------------------------------------------------------------ stage entry points

static int64_t trace_extent(const dh_la *las, int64_t n)
{
    int64_t m = 0;
    for (int64_t i = 0; i < n; i++) m = std::max<int64_t>(m, las[i].toff + las[i].tlen);
    return m;
}

// DAScover + DASqv for a pile-up DB (dazzler.d:3782-3792, 6142-6156): intrinsic QV of every
// tspace tile of every read from the overlaps of that read (las grouped by aread, ascending).
extern "C" int dh_tile_qv(dh_ctx *ctx, dh_db *db, const dh_la *las, int64_t n, const uint16_t *trace,
                          int32_t tspace, int32_t cov, uint8_t *qv, int32_t maxtiles)
{
    if (!ctx || !db || !qv || (n > 0 && (!las || !trace)) || tspace < 1 || maxtiles < 1 || cov < 1)
        return dh_fail(DH_EINVAL, "dh_tile_qv: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const int32_t npr = db->n;
    std::vector<int32_t> la_first((size_t)npr + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        if (las[i].aread < 0 || las[i].aread >= npr || (i > 0 && las[i].aread < las[i - 1].aread))
            return dh_fail(DH_EINVAL, "dh_tile_qv: overlaps must be grouped by aread (ascending) and inside the DB");
        la_first[(size_t)las[i].aread + 1]++;
    }
    for (int32_t r = 0; r < npr; r++) la_first[(size_t)r + 1] += la_first[(size_t)r];
    const int64_t nt = trace_extent(las, n);
    DevBuf<DhLa> d_las;
    DevBuf<uint16_t> d_tr;
    DevBuf<int32_t> d_first, d_cov;
    DevBuf<uint8_t> d_qv;
    std::vector<int32_t> cov_of((size_t)npr, cov);
    HIPCHK(d_las.alloc((size_t)n));
    HIPCHK(d_tr.alloc((size_t)nt));
    HIPCHK(d_first.alloc(la_first.size()));
    HIPCHK(d_cov.alloc(cov_of.size()));
    HIPCHK(d_qv.alloc((size_t)npr * maxtiles));
    if (n > 0) {
        HIPCHK(hipMemcpyAsync(d_las.p, las, sizeof(dh_la) * (size_t)n, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_tr.p, trace, sizeof(uint16_t) * (size_t)nt, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(d_first.p, la_first.data(), sizeof(int32_t) * la_first.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_cov.p, cov_of.data(), sizeof(int32_t) * cov_of.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_qv.p, 255, (size_t)npr * maxtiles, st));
    dhk_tile_qv(st, d_las.p, d_tr.p, d_first.p, db->d_off, npr, tspace, d_cov.p, maxtiles, d_qv.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(qv, d_qv.p, (size_t)npr * maxtiles, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}

// computeintrinsicqv + daccord -f -I<i>,<i> (dazzler.d:4213-4255, 6172-6231): consensus of read
// ref_read of the DB from its overlaps (the records with aread == ref_read).  rounds > 1 re-aligns
// every read of the DB to the consensus and votes again, as dh_process_pileups does.
extern "C" int dh_consensus(dh_ctx *ctx, dh_db *db, const dh_la *las, int64_t n, const uint16_t *trace,
                            int32_t tspace, int32_t ref_read, int32_t rounds, uint8_t *out, int64_t cap,
                            int64_t *out_len)
{
    if (!ctx || !db || !out || !out_len || (n > 0 && (!las || !trace)) || ref_read < 0 || ref_read >= db->n ||
        rounds < 1 || rounds > 8 || tspace < 16 || tspace > SEG_MAX)
        return dh_fail(DH_EINVAL, "dh_consensus: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DbGuard dbg;
    SetGuard sg;
    LaVec pl(las, las + n);
    const int64_t nt = trace_extent(las, n);
    TraceVec tr(trace, trace + nt);
    dh_db *T = nullptr;
    const int32_t rlen = (int32_t)(db->h_off[(size_t)ref_read + 1] - db->h_off[(size_t)ref_read]);
    const int32_t grp = db->h_group.empty() ? 0 : db->h_group[(size_t)ref_read];
    if (int rc = dh_db_from_slices(ctx, db, {ref_read}, {0}, {rlen}, {grp}, &T)) return rc;
    dbg.dbs.push_back(T);
    {
        std::vector<int32_t> tmpl_of(pl.size(), -1);
        for (size_t i = 0; i < pl.size(); i++)
            if (pl[i].aread == ref_read) tmpl_of[i] = 0;
        dh_db *nT = nullptr;
        int64_t nseg = 0, ncell = 0;
        if (int rc = consensus_round(ctx, T, db, pl, tr, tmpl_of, tspace, &nT, &nseg, &ncell)) return rc;
        dbg.dbs.push_back(nT);
        T = nT;
    }
    const dh_align_opts ro = pile_align_opts(tspace, 500, 4, 32);
    for (int32_t round = 1; round < rounds; round++)
        if (int rc = realign_round(ctx, db, ro, nullptr, dbg, sg, nullptr, nullptr, &T)) return rc;
    *out_len = T->total;
    if (T->total > cap) return dh_fail(DH_EOVERFLOW, "dh_consensus: output buffer too small");
    if (T->total > 0) HIPCHK(hipMemcpyAsync(out, T->d_bases, (size_t)T->total, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}
