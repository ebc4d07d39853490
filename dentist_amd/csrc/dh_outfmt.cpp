// dh_outfmt.cpp -- dh_output_db: `dentist output` (source/dentist/commands/output.d) with the FASTA text formatted on the
// device.  The walk of dh_output.cpp hands its pieces to a sink that records a plan (dh_outfmt.h); the plan's bytes are then
// produced chunk by chunk by k_outfmt (dh_outfmt.hip) and written while the next chunk is formatted.  AGP and BED are written
// by the walk on the host, as for dh_output_assembly.  Replaces the per-base fputc loop of the host writer (LineWriter,
// dh_output.cpp) for callers that have the contigs on the device.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dh_internal.h"
#include "dh_outfmt.h"

extern "C" void dhk_outfmt(hipStream_t st, const of::Plan *p, int64_t q0, int64_t q1, void *out);

namespace {
// DH_OUT_CHUNK_MB: bytes of a chunk of the file (a decimal number of MiB, default 256), a multiple of 16, at least 64.  Two
// device buffers and two page-locked host buffers of this size are in use at a time.
int64_t chunk_bytes()
{
    double mb = 256.0;
    if (const char *e = getenv("DH_OUT_CHUNK_MB")) {
        char *end = nullptr;
        const double v = strtod(e, &end);
        if (end != e && std::isfinite(v) && v > 0) mb = v;
    }
    const double bytes = std::min(std::ceil(mb * 1048576.0), 1e15);
    return std::max<int64_t>(64, ((int64_t)bytes + 15) / 16 * 16);
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct PlanSink : DhOutSink {
    dh_ctx *ctx;            // NULL: the plan alone (dh_output_plan)
    const dh_db *contigs;   // ... and then NULL as well
    const int64_t *contig_off;
    int64_t contig_total;
    const uint8_t *cons;
    int64_t cons_len;
    const char *path;  // NULL: stdout
    int32_t width;
    FILE *f = nullptr;
    std::vector<uint8_t> hdr;
    std::vector<int64_t> hdr_off{0}, seg_first, seg_base{0}, seg_src;
    std::vector<uint32_t> seg_flags;
    bool bad = false;  // a segment outside its buffer

    std::vector<int64_t> rec_off;
    PlanSink(dh_ctx *c, const dh_db *db, const int64_t *off, int32_t ncontigs, const uint8_t *cons_, int64_t cons_len_, const char *path_,
             int32_t width_)
        : ctx(c), contigs(db), contig_off(off), contig_total(off[ncontigs]), cons(cons_), cons_len(cons_len_), path(path_), width(width_)
    {
    }
    int begin() override
    {
        if (!ctx) return DH_OK;
        f = path ? fopen(path, "w") : stdout;
        return f ? DH_OK : dh_fail(DH_EIO, std::string("cannot open ") + path);
    }
    void header(const std::string &line) override
    {
        hdr.insert(hdr.end(), line.begin(), line.end());
        hdr_off.push_back((int64_t)hdr.size());
        seg_first.push_back((int64_t)seg_src.size());
    }
    // n bases whose first output base is src[at]; the others follow upwards, or downwards with OF_REV
    void segment(uint32_t flags, int64_t at, int64_t n, int64_t buf_len)
    {
        if (n <= 0) return;
        if ((flags & of::OF_KIND) != of::OF_NRUN) {
            const int64_t lo = (flags & of::OF_REV) ? at - (n - 1) : at, hi = (flags & of::OF_REV) ? at : at + (n - 1);
            if (lo < 0 || hi >= buf_len) bad = true;
        }
        seg_src.push_back(at);
        seg_flags.push_back(flags);
        seg_base.push_back(seg_base.back() + n);
    }
    void contig(int32_t c, int64_t from, int64_t upto, bool comp) override
    {
        const int64_t o = contig_off[c];
        if (from < 0 || o + upto > contig_off[c + 1]) bad = true;
        segment(of::OF_CONTIG | (comp ? of::OF_REV : 0u), o + (comp ? upto - 1 : from), upto - from, contig_total);
    }
    void nrun(int64_t len) override { segment(of::OF_NRUN, 0, len, 0); }
    void insertion(int64_t cons_off, int64_t sb, int64_t se, bool comp, bool upper) override
    {
        segment(of::OF_CONS | (comp ? of::OF_REV : 0u) | (upper ? of::OF_UPPER : 0u), cons_off + (comp ? se - 1 : sb), se - sb, cons_len);
    }
    void end_record() override {}
    void abandon() override
    {
        if (f && f != stdout) fclose(f);
        f = nullptr;
    }
    int finish() override
    {
        int rc = bad ? dh_fail(DH_EINVAL, "dh_output_db: a piece of the assembly lies outside its sequence") : DH_OK;
        if (rc == DH_OK) {
            layout();
            if (ctx) rc = format();
        }
        bool closed = true;
        if (f == stdout)
            closed = fflush(f) == 0;
        else if (f)
            closed = fclose(f) == 0;
        f = nullptr;
        if (rc != DH_OK) return rc;
        return closed ? DH_OK : dh_fail(DH_EIO, std::string("short write to ") + (path ? path : "stdout"));
    }
    void layout();
    int format();
};

// what a call holds on the device and in page-locked memory; released on every way out
struct Buffers {
    dh_ctx *ctx;
    int64_t chunk = 0;
    void *pin[2] = {nullptr, nullptr};
    DevBuf<uint8_t> plan, cons, out[2];
    hipEvent_t ks[2] = {}, ke[2] = {}, ce[2] = {};
    explicit Buffers(dh_ctx *c) : ctx(c) {}
    ~Buffers()
    {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipStreamSynchronize(ctx->cstream);
        for (int b = 0; b < 2; b++) {
            if (pin[b]) dh_pinned_free(pin[b], (size_t)chunk);
            if (ks[b]) (void)hipEventDestroy(ks[b]);
            if (ke[b]) (void)hipEventDestroy(ke[b]);
            if (ce[b]) (void)hipEventDestroy(ce[b]);
        }
    }
};

// the byte offsets of the records
void PlanSink::layout()
{
    const int64_t nrec = (int64_t)seg_first.size(), nseg = (int64_t)seg_src.size();
    seg_first.push_back(nseg);
    rec_off.assign((size_t)nrec + 1, 0);
    for (int64_t r = 0; r < nrec; r++) {
        const int64_t nb = seg_base[(size_t)seg_first[(size_t)r + 1]] - seg_base[(size_t)seg_first[(size_t)r]];
        rec_off[(size_t)r + 1] = rec_off[(size_t)r] + (hdr_off[(size_t)r + 1] - hdr_off[(size_t)r]) + of::body_bytes(nb, width);
    }
}

int PlanSink::format()
{
    const double t_begin = now_ms();
    const int64_t nrec = (int64_t)seg_first.size() - 1, nseg = (int64_t)seg_src.size();
    const int64_t total = rec_off[(size_t)nrec];
    double ms_kernel = 0, ms_copy = 0, ms_write = 0;
    if (total > 0) {
        HIPCHK(hipSetDevice(ctx->device));
        Buffers B(ctx);
        B.chunk = std::min(chunk_bytes(), (total + 15) / 16 * 16);
        // the plan in one upload: the 64-bit arrays, the flags, the header bytes
        const size_t n64 = 3 * ((size_t)nrec + 1) + ((size_t)nseg + 1) + (size_t)nseg;
        const size_t flags_at = n64 * 8, hdr_at = flags_at + ((size_t)nseg * 4 + 7) / 8 * 8;
        std::vector<uint8_t> blob(hdr_at + hdr.size() + 8, 0);
        int64_t *w = (int64_t *)blob.data();
        of::Plan p;
        memset(&p, 0, sizeof(p));
        HIPCHK(B.plan.alloc(blob.size()));
        auto put = [&](const std::vector<int64_t> &v, size_t n, const int64_t *&dev) {
            if (n) memcpy(w, v.data(), n * 8);
            dev = (const int64_t *)(B.plan.p + ((uint8_t *)w - blob.data()));
            w += n;
        };
        put(rec_off, (size_t)nrec + 1, p.rec_off);
        put(hdr_off, (size_t)nrec + 1, p.hdr_off);
        put(seg_first, (size_t)nrec + 1, p.seg_first);
        put(seg_base, (size_t)nseg + 1, p.seg_base);
        put(seg_src, (size_t)nseg, p.seg_src);
        if (nseg) memcpy(blob.data() + flags_at, seg_flags.data(), (size_t)nseg * 4);
        memcpy(blob.data() + hdr_at, hdr.data(), hdr.size());
        p.seg_flags = (const uint32_t *)(B.plan.p + flags_at);
        p.hdr = B.plan.p + hdr_at;
        p.contig = contigs->d_bases;
        p.nrec = nrec;
        p.nseg = nseg;
        p.width = width;
        HIPCHK(B.cons.alloc((size_t)cons_len));
        p.cons = B.cons.p;
        HIPCHK(hipMemcpyAsync(B.plan.p, blob.data(), blob.size(), hipMemcpyHostToDevice, ctx->stream));
        if (cons_len > 0) HIPCHK(hipMemcpyAsync(B.cons.p, cons, (size_t)cons_len, hipMemcpyHostToDevice, ctx->stream));
        for (int b = 0; b < 2; b++) {
            HIPCHK(B.out[b].alloc((size_t)B.chunk));
            if (!(B.pin[b] = dh_pinned_alloc((size_t)B.chunk))) return dh_fail(DH_ENOMEM, "dh_output_db: no page-locked memory for a chunk (DH_OUT_CHUNK_MB)");
            HIPCHK(hipEventCreate(&B.ks[b]));
            HIPCHK(hipEventCreate(&B.ke[b]));
            HIPCHK(hipEventCreate(&B.ce[b]));
        }
        // the contigs were uploaded on their own context's stream; the plan's host copy goes away with this scope
        if (contigs->ctx && contigs->ctx->stream != ctx->stream) HIPCHK(hipStreamSynchronize(contigs->ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        const int64_t nchunks = (total + B.chunk - 1) / B.chunk;
        bool wrote = true;
        // chunk j is in pin[j & 1] once its copy has ended: write it (while chunk j + 1 is formatted and copied)
        auto drain = [&](int64_t j) -> int {
            const int b = (int)(j & 1);
            const int64_t q0 = j * B.chunk, n = std::min(total, q0 + B.chunk) - q0;
            HIPCHK(hipEventSynchronize(B.ce[b]));
            float k = 0, c = 0;
            HIPCHK(hipEventElapsedTime(&k, B.ks[b], B.ke[b]));
            HIPCHK(hipEventElapsedTime(&c, B.ke[b], B.ce[b]));
            ms_kernel += k;
            ms_copy += c;
            const double t0 = now_ms();
            if (fwrite(B.pin[b], 1, (size_t)n, f) != (size_t)n) wrote = false;
            ms_write += now_ms() - t0;
            return DH_OK;
        };
        for (int64_t i = 0; i < nchunks; i++) {
            const int b = (int)(i & 1);
            const int64_t q0 = i * B.chunk, q1 = std::min(total, q0 + B.chunk);
            if (i >= 2) HIPCHK(hipStreamWaitEvent(ctx->stream, B.ce[b], 0));  // the copy of chunk i - 2 has left out[b]
            HIPCHK(hipEventRecord(B.ks[b], ctx->stream));
            dhk_outfmt(ctx->stream, &p, q0, q1, B.out[b].p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(B.ke[b], ctx->stream));
            HIPCHK(hipStreamWaitEvent(ctx->cstream, B.ke[b], 0));
            HIPCHK(hipMemcpyAsync(B.pin[b], B.out[b].p, (size_t)(q1 - q0), hipMemcpyDeviceToHost, ctx->cstream));
            HIPCHK(hipEventRecord(B.ce[b], ctx->cstream));
            if (i >= 1)
                if (int rc = drain(i - 1)) return rc;
        }
        if (int rc = drain(nchunks - 1)) return rc;
        if (!wrote) return dh_fail(DH_EIO, std::string("short write to ") + (path ? path : "stdout"));
    }
    ctx->out_ms[0] = ms_kernel;
    ctx->out_ms[1] = ms_copy;
    ctx->out_ms[2] = ms_write;
    ctx->out_ms[3] = now_ms() - t_begin;
    return DH_OK;
}
}  // namespace

extern "C" int dh_output_db(dh_ctx *ctx, dh_db *contigs, const char *fasta_path, const char *bed_path, const char *agp_path,
                            const int32_t *scaffold_of, const char *const *headers, const int32_t *gap_len,
                            const dh_insertions *ins, int32_t nreads, const char *const *read_names,
                            const dh_output_opts *opts, const dh_output_filter *filter, int32_t *dropped)
{
    if (!ctx || !ctx->stream || !ctx->cstream) return dh_fail(DH_EINVAL, "dh_output_db: needs a context with a device (there is no CPU route)");
    if (!contigs || !scaffold_of || !headers || !opts || !ins) return dh_fail(DH_EINVAL, "dh_output_db: NULL argument");
    if (filter && (filter->nskip < 0 || (filter->nskip > 0 && !filter->skip_gaps2))) return dh_fail(DH_EINVAL, "dh_output_db: bad filter");
    const int32_t nall = (int32_t)ins->rec.size();
    const bool has_ids = ins->ids_off.size() == ins->rec.size() + 1;
    for (int32_t i = 0; i < nall; i++) {
        const dh_insertion &r = ins->rec[(size_t)i];
        if (r.status == DH_PILE_OK && (r.cons_off < 0 || r.cons_len < 0 || r.cons_off + r.cons_len > (int64_t)ins->bases.size()))
            return dh_fail(DH_EINVAL, "dh_output_db: insertion " + std::to_string(i) + ": consensus outside the sequence buffer");
    }
    // The filter acts on the list of insertions, before the graph exists.  The reference filters by quality while it fills
    // the graph (ensureHighQualityConsensus, output.d:318, 388-410) and removes the blacklisted joins from the graph before
    // enforceJoinPolicy (removeBlacklisted, output.d:331, scaffold.d:735-768).  That is the same thing: a gap join enters the
    // graph only through an insertion, removeBlacklisted touches gap joins only (join.isGap), and nothing between the two
    // steps (appendUnkownJoins) looks at gap joins.  Filtered insertions are not counted in *dropped, which counts the join
    // policy's as before.
    std::vector<dh_insertion> kept;
    std::vector<int32_t> ids, ids_off;
    const dh_insertion *rec = ins->rec.data();
    int32_t nins = nall;
    const int32_t *rid = has_ids ? ins->ids.data() : nullptr, *rid_off = has_ids ? ins->ids_off.data() : nullptr;
    if (filter && (filter->max_insertion_error_ppm > 0 || filter->nskip > 0)) {
        std::vector<std::pair<int32_t, int32_t>> skip;
        for (int32_t k = 0; k < filter->nskip; k++) {
            const int32_t a = filter->skip_gaps2[2 * k], b = filter->skip_gaps2[2 * k + 1];
            if (a < 0 || a >= b || b >= contigs->n) return dh_fail(DH_EINVAL, "dh_output_db: skip_gaps2 needs 0 <= first < second < contigs");
            skip.emplace_back(a, b);
        }
        std::sort(skip.begin(), skip.end());
        ids_off.push_back(0);
        for (int32_t i = 0; i < nall; i++) {
            const dh_insertion &r = ins->rec[(size_t)i];
            bool keep = true;
            if (r.status == DH_PILE_OK) {
                const bool ext = (r.join & DH_JOIN_EXTENSION) != 0;
                const int32_t fo = i < (int32_t)ins->flank_of.size() ? ins->flank_of[(size_t)i] : -1;
                if (filter->max_insertion_error_ppm > 0 && fo >= 0)
                    for (int32_t s = 0; s < (ext ? 1 : 2) && keep; s++) {  // averageErrorRate > maxInsertionError, base.d:695-698
                        const dh_la &l = ins->flank[(size_t)fo + (size_t)s];
                        const int64_t cov = ins->flank_cov.empty() ? (int64_t)l.aepos - l.abpos : ins->flank_cov[(size_t)fo + (size_t)s];
                        if ((int64_t)l.diffs * 1000000 > (int64_t)filter->max_insertion_error_ppm * cov) keep = false;
                    }
                if (keep && !ext) {
                    const int32_t c1 = r.join == 0 && r.contig_right == 0 ? r.contig_left + 1 : r.contig_right;
                    if (std::binary_search(skip.begin(), skip.end(), std::make_pair(r.contig_left, c1))) keep = false;
                }
            }
            if (!keep) continue;
            kept.push_back(r);
            if (has_ids) {
                ids.insert(ids.end(), ins->ids.begin() + ins->ids_off[(size_t)i], ins->ids.begin() + ins->ids_off[(size_t)i + 1]);
                ids_off.push_back((int32_t)ids.size());
            }
        }
        rec = kept.data();
        nins = (int32_t)kept.size();
        if (has_ids) {
            rid = ids.data();
            rid_off = ids_off.data();
        }
    }
    PlanSink sink(ctx, contigs, contigs->h_off.data(), contigs->n, ins->bases.data(), (int64_t)ins->bases.size(), fasta_path, opts->line_width);
    return dh_output_walk("dh_output_db", sink, fasta_path ? fasta_path : "stdout", bed_path, agp_path, contigs->h_off.data(), contigs->n,
                          scaffold_of, headers, gap_len, rec, nins, rid, rid_off, nreads, read_names, opts, dropped);
}

// the last dh_output_db of the context in ms: kernels, copies back (each from the end of its kernel), fwrite, the whole
// formatting (plan upload to last write)
extern "C" int dh_get_output_stats(dh_ctx *ctx, double *ms4)
{
    if (!ctx || !ms4) return dh_fail(DH_EINVAL, "dh_get_output_stats: NULL");
    for (int i = 0; i < 4; i++) ms4[i] = ctx->out_ms[i];
    return DH_OK;
}

// Test surface of the plan (tests/outfmt_ref.py restates plan -> bytes; tests/native/outfmt_host.cpp plays the lane code on it):
// the walk of dh_output_assembly on host arrays, no file written and no device used.  ins_bases_len bounds the consensus slices.
struct dh_out_plan {
    std::vector<int64_t> rec_off, hdr_off, seg_first, seg_base, seg_src;
    std::vector<uint32_t> seg_flags;
    std::vector<uint8_t> hdr;
    int32_t dropped = 0;
};
extern "C" int dh_output_plan(const int64_t *contig_off, int32_t ncontigs, const int32_t *scaffold_of, const char *const *headers,
                              const int32_t *gap_len, const dh_insertion *ins, int32_t nins, int64_t ins_bases_len,
                              const dh_output_opts *opts, dh_out_plan **out)
{
    if (!contig_off || ncontigs < 0 || !scaffold_of || !headers || !opts || !out || (nins > 0 && !ins))
        return dh_fail(DH_EINVAL, "dh_output_plan: NULL argument");
    for (int32_t i = 0; i < nins; i++)
        if (ins[i].status == DH_PILE_OK && (ins[i].cons_off < 0 || ins[i].cons_len < 0 || ins[i].cons_off + ins[i].cons_len > ins_bases_len))
            return dh_fail(DH_EINVAL, "dh_output_plan: insertion " + std::to_string(i) + ": consensus outside the sequence buffer");
    PlanSink sink(nullptr, nullptr, contig_off, ncontigs, nullptr, ins_bases_len, nullptr, opts->line_width);
    int32_t dropped = 0;
    if (int rc = dh_output_walk("dh_output_plan", sink, "", nullptr, nullptr, contig_off, ncontigs, scaffold_of, headers, gap_len, ins, nins,
                                nullptr, nullptr, -1, nullptr, opts, &dropped))
        return rc;
    dh_out_plan *p = new dh_out_plan();
    p->rec_off.swap(sink.rec_off);
    p->hdr_off.swap(sink.hdr_off);
    p->seg_first.swap(sink.seg_first);
    p->seg_base.swap(sink.seg_base);
    p->seg_src.swap(sink.seg_src);
    p->seg_flags.swap(sink.seg_flags);
    p->hdr.swap(sink.hdr);
    p->dropped = dropped;
    *out = p;
    return DH_OK;
}
extern "C" void dh_out_plan_destroy(dh_out_plan *p) { delete p; }
// which: 0 rec_off, 1 hdr_off, 2 seg_first, 3 seg_base, 4 seg_src (int64), 5 seg_flags (uint32), 6 hdr (bytes); *n = entries
extern "C" const void *dh_out_plan_array(const dh_out_plan *p, int32_t which, int64_t *n)
{
    if (!p || !n) return nullptr;
    const std::vector<int64_t> *v[5] = {&p->rec_off, &p->hdr_off, &p->seg_first, &p->seg_base, &p->seg_src};
    if (which >= 0 && which < 5) {
        *n = (int64_t)v[which]->size();
        return v[which]->data();
    }
    if (which == 5) {
        *n = (int64_t)p->seg_flags.size();
        return p->seg_flags.data();
    }
    if (which == 6) {
        *n = (int64_t)p->hdr.size();
        return p->hdr.data();
    }
    *n = 0;
    return nullptr;
}
