// dh_crop.cpp -- the crop stage of `dentist process` (cropPileUp, cropper.d:113-175, 446-550): the accessors and creators
// of a dh_cropped, and dh_crop_pileups* -- common trace points and read slices per pile-up on the host threads, the parts
// of every cropped read laid out serially, their bases gathered on the device (k_gather_parts).
#include <array>
#include <atomic>
#include <cstring>

#include "dh_process.h"
#include "dh_parallel.h"

using namespace dhp;

extern "C" {
void dhk_gather_parts(hipStream_t st, const uint8_t *src0, const int64_t *off0, const uint8_t *src1,
                      const int64_t *off1, const void *parts, int32_t n, int32_t max_len, uint8_t *dst);
}

// ------------------------------------------------------------------------------------ crop stage
// (struct dh_cropped: dh_process.h)

extern "C" void dh_cropped_destroy(dh_cropped *c)
{
    if (!c) return;
    if (c->dev) dh_db_destroy(c->dev);
    delete c;
}
extern "C" int32_t dh_cropped_npiles(const dh_cropped *c) { return c ? (int32_t)c->rec.size() : 0; }
extern "C" const dh_insertion *dh_cropped_records(const dh_cropped *c) { return c ? c->rec.data() : nullptr; }
extern "C" int32_t dh_cropped_nreads(const dh_cropped *c) { return c ? (int32_t)c->pile.size() : 0; }
extern "C" const int32_t *dh_cropped_pile(const dh_cropped *c) { return c ? c->pile.data() : nullptr; }
extern "C" const int32_t *dh_cropped_entry(const dh_cropped *c) { return c ? c->entry.data() : nullptr; }
extern "C" const int32_t *dh_cropped_read_id(const dh_cropped *c) { return c ? c->read_id.data() : nullptr; }
extern "C" const uint8_t *dh_cropped_kind(const dh_cropped *c) { return c ? c->kind.data() : nullptr; }
extern "C" const int64_t *dh_cropped_offsets(const dh_cropped *c) { return c ? c->off.data() : nullptr; }
extern "C" const uint8_t *dh_cropped_bases(dh_cropped *c)
{
    if (!c) return nullptr;
    if (!c->host_valid) {
        c->bases.resize((size_t)std::max<int64_t>(c->off.back(), 1));
        if (c->dev && c->off.back() > 0) {
            if (hipSetDevice(c->ctx->device) != hipSuccess ||
                hipMemcpyAsync(c->bases.data(), c->dev->d_bases, (size_t)c->off.back(), hipMemcpyDeviceToHost,
                               c->ctx->stream) != hipSuccess ||
                hipStreamSynchronize(c->ctx->stream) != hipSuccess) {
                dh_fail(DH_EHIP, "dh_cropped_bases: device to host copy failed");
                return nullptr;
            }
        }
        c->host_valid = true;
    }
    return c->bases.data();
}

extern "C" int dh_cropped_create(const dh_insertion *rec, int32_t npiles, int32_t nreads, const int32_t *pile,
                                 const int32_t *entry, const int32_t *read_id, const int64_t *off,
                                 const uint8_t *bases, dh_cropped **out)
{
    return dh_cropped_create2(rec, npiles, nreads, pile, entry, read_id, nullptr, off, bases, out);
}

// kind: per read 0 / 1 / 2 (see dh_cropped_kind), NULL = every read spans its gap
extern "C" int dh_cropped_create2(const dh_insertion *rec, int32_t npiles, int32_t nreads, const int32_t *pile,
                                  const int32_t *entry, const int32_t *read_id, const uint8_t *kind, const int64_t *off,
                                  const uint8_t *bases, dh_cropped **out)
{
    if (npiles < 0 || nreads < 0 || !out || (npiles > 0 && !rec) ||
        (nreads > 0 && (!pile || !entry || !read_id || !off || !bases)))
        return dh_fail(DH_EINVAL, "dh_cropped_create: bad argument");
    dh_cropped *c = new dh_cropped();
    c->rec.assign(rec, rec + npiles);
    if (nreads > 0) {
        if (off[0] != 0) {
            delete c;
            return dh_fail(DH_EINVAL, "dh_cropped_create: off[0] must be 0");
        }
        for (int32_t i = 0; i < nreads; i++)
            if (pile[i] < 0 || pile[i] >= npiles || off[i + 1] < off[i] ||
                (i > 0 && (pile[i] < pile[i - 1] || (pile[i] == pile[i - 1] && entry[i] <= entry[i - 1])))) {
                delete c;
                return dh_fail(DH_EINVAL, "dh_cropped_create: reads must be ordered by (pile, entry)");
            }
        c->pile.assign(pile, pile + nreads);
        c->entry.assign(entry, entry + nreads);
        c->read_id.assign(read_id, read_id + nreads);
        if (kind)
            c->kind.assign(kind, kind + nreads);
        else {
            c->kind.assign((size_t)nreads, 0);
            c->comp_known = false;
        }
        for (uint8_t k : c->kind)
            if ((k & 3) > 2 || k > 15) {
                delete c;
                return dh_fail(DH_EINVAL, "dh_cropped_create: kind must be 0, 1 or 2 (| 4, 8: complement alignment on flank 0, 1)");
            }
        c->off.assign(off, off + nreads + 1);
        c->bases.assign(bases, bases + off[nreads]);
    }
    c->host_valid = true;
    *out = c;
    return DH_OK;
}

// ------------------------------------------------------------------------------------ crop stages
// dh_crop_pileups_masked is the stages below, called in the order they stand in, over these structs.
namespace {

// what one dh_crop_pileups call works on
struct CropRun {
    dh_ctx *ctx;
    hipStream_t st;
    const dh_process_opts &o;
    dh_db *contigs, *reads;
    int32_t read_first;
    const dh_la *las;
    int64_t n;
    const uint16_t *trace;
    const dh_pileups *piles;
    const int64_t *rep_ptr;  // the repeat mask (NULL: none)
    const int32_t *rep_iv;
    dh_cropped *c;  // under construction: the entry point's until it is handed over
};

// every pile-up read = [support patch] + read slice + [support patch]; parts are gathered on
// the device from the reads DB (src 0) and the contigs DB (src 1)
struct Slice {
    int32_t e, rd, lrd, b0, b1, kind;  // kind: 0 / 1 / 2 | complement of the alignment on flank 0 << 2 | on flank 1 << 3
};
struct PileCrop {
    int32_t pc[2] = {-1, -1}, p0[2] = {0, 0}, p1[2] = {0, 0};  // support patch of flank f: contig pc[f], [p0, p1)
    std::vector<Slice> sl;
};

// ---- 1. one pile-up: its flanks and join bits, the common trace point of every flank, the support patches and the slice
// of every read held here.  Pile-ups are independent: host threads take them (the trace walks are cache misses into the
// mapping's trace array).  Returns 0, or what the call fails with: 1 gap outside, 2 LA index, 3 trace NULL, 4 trace does not fit
int crop_one_pile(const CropRun &run, int64_t p, PileCrop &q)
{
    const dh_process_opts &o = run.o;
    const dh_db *contigs = run.contigs, *reads = run.reads;
    const dh_la *las = run.las;
    const int64_t n = run.n;
    const uint16_t *trace = run.trace;
    const dh_pileups *piles = run.piles;
    const int64_t *rep_ptr = run.rep_ptr;
    const int32_t *rep_iv = run.rep_iv;
    const int32_t read_first = run.read_first, tsm = o.tspace_map;
    dh_insertion &r = run.c->rec[(size_t)p];
    memset(&r, 0, sizeof(r));
    // the two flanks (cropper.d:113-175 treats every pile-up alike: one common trace point per involved
    // contig, taken from the alignments seeded there)
    const std::array<int32_t, 4> jn = piles->join_of((size_t)p);
    const int32_t nf = jn[2] < 0 ? 1 : 2;
    const int32_t fc[2] = {jn[0], jn[2]};
    const bool front[2] = {jn[1] == DH_SEED_FRONT, jn[3] == DH_SEED_FRONT};
    if (fc[0] < 0 || fc[0] >= contigs->n || (nf == 2 && fc[1] >= contigs->n)) return 1;
    r.contig_left = fc[0];
    r.contig_right = nf == 2 ? fc[1] : -1;
    r.join = (front[0] ? DH_JOIN_FLANK0_FRONT : 0) | (nf == 2 && !front[1] ? DH_JOIN_FLANK1_BACK : 0) | (nf == 1 ? DH_JOIN_EXTENSION : 0);
    r.ref_read = r.ref_read_id = -1;
    r.crop_left = r.crop_right = -1;
    if (nf == 2 && fc[0] == fc[1]) {
        r.status = DH_PILE_UNSUPPORTED_JOIN;
        return 0;
    }
    const std::vector<int32_t> &tr3 = piles->triples[(size_t)p];
    const int32_t ne = (int32_t)tr3.size() / 3;
    Region reg[2] = {Region{{0, INT32_MAX}}, Region{{0, INT32_MAX}}};
    bool bad = false;
    for (int32_t e = 0; e < ne && !bad; e++) {
        // an entry is a read spanning the gap (two alignments) or an extension over one contig end
        // merged into the gap's pile-up (one alignment, the other index is -1: scaffold.d:789-816)
        const int32_t ix[2] = {tr3[(size_t)e * 3 + 1], tr3[(size_t)e * 3 + 2]};
        if (ix[0] < -1 || ix[0] >= n || ix[1] < -1 || ix[1] >= n || (ix[0] < 0 && ix[1] < 0) || (nf == 1 && ix[1] >= 0)) {
            bad = true;
            break;
        }
        for (int f = 0; f < nf; f++)
            if (ix[f] >= 0) {
                if (las[ix[f]].aread != fc[f])
                    bad = true;
                else
                    intersect_chain(reg[f], las, n, ix[f]);
            }
    }
    if (bad) return 2;
    int32_t clen[2] = {0, 0}, crop[2] = {-1, -1};
    for (int f = 0; f < nf; f++) {
        clen[f] = (int32_t)(contigs->h_off[(size_t)fc[f] + 1] - contigs->h_off[(size_t)fc[f]]);
        const int64_t m0 = rep_ptr ? rep_ptr[fc[f]] : 0, m1 = rep_ptr ? rep_ptr[fc[f] + 1] : 0;
        crop[f] = common_trace_point(reg[f], clen[f], tsm, front[f], rep_iv ? rep_iv + 2 * m0 : nullptr, m1 - m0);
    }
    r.crop_left = crop[0];
    r.crop_right = crop[1];
    if (crop[0] < 0 || (nf == 2 && crop[1] < 0)) {
        r.status = DH_PILE_NO_COMMON_TRACE_POINT;
        return 0;
    }
    // fetchSupportPatches, cropper.d:224-262
    for (int f = 0; f < nf; f++) {
        q.pc[f] = fc[f];
        if (front[f]) {
            if (crop[f] < o.min_anchor) {
                q.p0[f] = crop[f];
                q.p1[f] = std::min(clen[f], o.min_anchor);
            }
        } else if (clen[f] - crop[f] < o.min_anchor) {
            q.p0[f] = std::max(0, clen[f] - o.min_anchor);
            q.p1[f] = crop[f];
        }
    }
    for (int32_t e = 0; e < ne; e++) {
        const int32_t rd = tr3[(size_t)e * 3];
        const int64_t lrd = (int64_t)rd - read_first;
        if (lrd < 0 || lrd >= reads->n) continue;  // held by another rank
        if (!trace) return 3;
        const int32_t ix[2] = {tr3[(size_t)e * 3 + 1], tr3[(size_t)e * 3 + 2]};
        const int32_t rl = (int32_t)(reads->h_off[(size_t)lrd + 1] - reads->h_off[(size_t)lrd]);
        // getCroppingSlice per alignment, intersected (cropper.d:339-348, 503-550): a back-seeded alignment
        // keeps [crop point, read end), a front-seeded one [0, crop point) of the read as the alignment sees it
        // -- mirrored for a complement alignment (:533-538)
        // (a chain translates through the first of its members that covers the crop point)
        int32_t b0 = 0, b1 = rl, kind = ix[1] < 0 ? 1 : (ix[0] < 0 ? 2 : 0);
        bool fail = false;
        for (int f = 0; f < nf && !fail; f++) {
            if (ix[f] < 0) continue;
            const int64_t m = covering_member(las, n, ix[f], crop[f]);
            if (m < 0) {
                fail = true;
                break;
            }
            const int32_t b = translate_floor_b(las[m], trace + las[m].toff, tsm, crop[f]);
            int32_t lo = front[f] ? 0 : b, hi = front[f] ? b : rl;
            if (las[ix[f]].flags & DH_FLAG_COMP) {
                const int32_t t = lo;
                lo = rl - hi;
                hi = rl - t;
                kind |= 4 << f;
            }
            b0 = std::max(b0, lo);
            b1 = std::min(b1, hi);
        }
        if (fail) return 4;
        if (b1 - b0 < 14) continue;  // records shorter than 14 bp are dropped (dazzler.d:150)
        if (b0 < 0 || b1 > rl) return 4;
        q.sl.push_back(Slice{e, rd, (int32_t)lrd, b0, b1, kind});
    }
    return 0;
}

// ---- 2. the parts of every cropped read, laid out serially in (pile, entry) order: pre-patch, read slice, post-patch
void lay_out_parts(CropRun &run, const std::vector<PileCrop> &pc, std::vector<PartDescH> &parts, int32_t &pile_max_len)
{
    const dh_pileups *piles = run.piles;
    dh_cropped *c = run.c;
    const int32_t np = (int32_t)pc.size();
    for (int32_t p = 0; p < np; p++) {
        const PileCrop &q = pc[(size_t)p];
        const std::array<int32_t, 4> jn = piles->join_of((size_t)p);
        const bool front[2] = {jn[1] == DH_SEED_FRONT, jn[3] == DH_SEED_FRONT};
        dh_insertion &r = c->rec[(size_t)p];
        for (const Slice &x : q.sl) {
            int64_t dst = c->off.back();
            // getSingleReadPatch / getReadPatches, cropper.d:351-378: the patch of an alignment goes to the read's front
            // when (contig seed == front) == complement, else to its back, reverse-complemented for a complement
            // alignment; an extension entry gets the patch of its own contig only
            int pre = -1, post = -1;
            for (int f = 0; f < 2; f++) {
                const bool has = f == 0 ? (x.kind & 3) != 2 : ((x.kind & 3) != 1 && q.pc[1] >= 0);
                if (!has || q.p1[f] <= q.p0[f]) continue;
                const bool comp = (x.kind & (4 << f)) != 0;
                if (front[f] == comp)
                    pre = f;
                else
                    post = f;
            }
            if (pre >= 0) {
                parts.push_back(PartDescH{1, q.pc[pre], q.p0[pre], q.p1[pre] - q.p0[pre], (x.kind & (4 << pre)) ? 1 : 0, 0, dst});
                dst += q.p1[pre] - q.p0[pre];
            }
            parts.push_back(PartDescH{0, x.lrd, x.b0, x.b1 - x.b0, 0, 0, dst});
            dst += x.b1 - x.b0;
            if (post >= 0) {
                parts.push_back(PartDescH{1, q.pc[post], q.p0[post], q.p1[post] - q.p0[post], (x.kind & (4 << post)) ? 1 : 0, 0, dst});
                dst += q.p1[post] - q.p0[post];
            }
            pile_max_len = std::max<int32_t>(pile_max_len, (int32_t)(dst - c->off.back()));
            c->off.push_back(dst);
            c->pile.push_back(p);
            c->entry.push_back(x.e);
            c->read_id.push_back(x.rd);
            c->kind.push_back((uint8_t)x.kind);
            r.nreads++;
        }
    }
}

// ---- 3. the bases of the cropped reads, gathered on the device into the crop's own DB
int gather_cropped_bases(CropRun &run, const std::vector<PartDescH> &parts, int32_t pile_max_len)
{
    dh_ctx *ctx = run.ctx;
    hipStream_t st = run.st;
    const dh_db *contigs = run.contigs, *reads = run.reads;
    dh_cropped *c = run.c;
    uint8_t *d_alloc = nullptr, *d_bases = nullptr;
    if (int rc = dh_alloc_bases(st, c->off.back(), &d_alloc, &d_bases)) return rc;
    if (int rc = dh_db_adopt(ctx, d_alloc, d_bases, c->off, std::vector<int32_t>(), &c->dev)) {
        dh_dev_free(d_alloc);
        return rc;
    }
    if (!parts.empty()) {
        DevBuf<PartDescH> d_parts;
        HIPCHK(d_parts.alloc(parts.size()));
        HIPCHK(hipMemcpyAsync(d_parts.p, parts.data(), sizeof(PartDescH) * parts.size(), hipMemcpyHostToDevice, st));
        dhk_gather_parts(st, reads->d_bases, reads->d_off, contigs->d_bases, contigs->d_off, d_parts.p,
                         (int32_t)parts.size(), pile_max_len, d_bases);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(st));
    }
    return DH_OK;
}

}  // namespace

// cropPileUp for a batch (cropper.d:113-175, 446-550): common trace point per flank from ALL entries
// of a pile-up; bases are cut for the entries whose read is in `reads` -- read ids in the triples
// are ids of the whole reads DB, `reads` holds [read_first, read_first + reads->n) of it (one rank's
// share when the mapping is sharded; read_first = 0 and the whole DB otherwise).  LAs of reads that
// are not held here only need their A intervals (no trace).
extern "C" int dh_crop_pileups(dh_ctx *ctx, dh_db *contigs, dh_db *reads, int32_t read_first, const dh_la *las,
                               int64_t n, const uint16_t *trace, const dh_pileups *piles,
                               const dh_process_opts *opts, dh_cropped **out)
{
    return dh_crop_pileups_masked(ctx, contigs, reads, read_first, las, n, trace, piles, nullptr, nullptr, opts, out);
}

// rep_ptr[ncontigs + 1] / rep_iv: the repeat mask (sorted disjoint (begin, end) pairs per contig) the common trace points
// keep out of when they can (cropper.d:446-500); NULL = no mask
extern "C" int dh_crop_pileups_masked(dh_ctx *ctx, dh_db *contigs, dh_db *reads, int32_t read_first, const dh_la *las,
                                      int64_t n, const uint16_t *trace, const dh_pileups *piles, const int64_t *rep_ptr,
                                      const int32_t *rep_iv, const dh_process_opts *opts, dh_cropped **out)
{
    if (!ctx || !contigs || !reads || !piles || !opts || !out || (n > 0 && !las) || (rep_ptr && !rep_iv && rep_ptr[contigs->n] > 0))
        return dh_fail(DH_EINVAL, "dh_crop_pileups: NULL argument");
    const dh_process_opts &o = *opts;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    hipEvent_t ev[2];
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    struct EvGuard {
        hipEvent_t *e;
        ~EvGuard()
        {
            for (int i = 0; i < 2; i++) (void)hipEventDestroy(e[i]);
        }
    } evg{ev};
    HIPCHK(hipEventRecord(ev[0], st));
    dh_cropped *c = new dh_cropped();
    c->ctx = ctx;
    struct CGuard {
        dh_cropped *&c;
        bool ok = false;
        ~CGuard()
        {
            if (!ok) dh_cropped_destroy(c);
        }
    } cg{c};
    const int32_t np = (int32_t)piles->contig_left.size();
    c->rec.resize((size_t)np);
    CropRun run{ctx, st, o, contigs, reads, read_first, las, n, trace, piles, rep_ptr, rep_iv, c};
    std::vector<PileCrop> pc((size_t)np);
    std::atomic<int> err{0};
    dh_parallel_for(np, 4, [&](int64_t plo, int64_t phi) {
        for (int64_t p = plo; p < phi; p++)
            if (int e = crop_one_pile(run, p, pc[(size_t)p])) err = e;
    });
    switch (err.load()) {
        case 1: return dh_fail(DH_EINVAL, "dh_crop_pileups: gap outside the contigs DB");
        case 2: return dh_fail(DH_EINVAL, "dh_crop_pileups: LA index out of range, or an alignment that is not on its flank's contig");
        case 3: return dh_fail(DH_EINVAL, "dh_crop_pileups: trace is NULL");
        case 4: return dh_fail(DH_EINVAL, "dh_crop_pileups: trace does not fit its read");
        default: break;
    }
    std::vector<PartDescH> parts;
    int32_t pile_max_len = 0;
    lay_out_parts(run, pc, parts, pile_max_len);
    if (int rc = gather_cropped_bases(run, parts, pile_max_len)) return rc;
    HIPCHK(hipEventRecord(ev[1], st));
    HIPCHK(hipEventSynchronize(ev[1]));
    HIPCHK(hipEventElapsedTime(&c->ms_crop, ev[0], ev[1]));
    cg.ok = true;
    *out = c;
    return DH_OK;
}
