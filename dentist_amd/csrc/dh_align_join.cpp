// dh_align_join.cpp -- the pile-up join of an alignment call (a grouped DB against itself): its plan on the host
// (plan_join: whether the call takes it, JoinPlan), the capacity of its hit buffer, and its build on the device (build_join).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dh_align.h"

#define fail dh_fail

void plan_join(AlignRun &r, JoinPlan &jp)
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
int build_join(AlignRun &r, const JoinPlan &jp)
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
