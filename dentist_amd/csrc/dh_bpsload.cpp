// dh_bpsload.cpp -- dh_dazz_load_reads: selected reads of a DAZZ_DB from disk to a device DB without the host unpack of
// dh_dazz_open.  The stub and the .idx give every read's place in the .bps (dh_dazzfmt.h: the view and its trim rule are
// dh_dazz_open's); the selected reads' packed byte ranges are merged into runs where they touch in the file, read chunk by
// chunk into one of two page-locked buffers, and uploaded and unpacked by k_bps_unpack (dh_bpsload.hip) on the context's
// stream while the next chunk is read.  Not a byte of the .bps outside the runs is read, and the packed copies and the
// index of the new DB stay as lazy as for any other DB.  Also dh_db_get_bases, the way back to the host.
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "dh_internal.h"
#include "dh_bpsload.h"
#include "dh_dazzfmt.h"

extern "C" void dhk_bps_unpack(hipStream_t st, const bl::Chunk *c, int64_t d0, int64_t d1, uint8_t *out);

namespace {
// DH_LOAD_CHUNK_MB: packed bytes of a chunk (a decimal number of MiB, default 64); a chunk always holds at least one read.
// Two device buffers and two page-locked host buffers of this size are in use at a time.
int64_t chunk_bytes()
{
    double mb = 64.0;
    if (const char *e = getenv("DH_LOAD_CHUNK_MB")) {
        char *end = nullptr;
        const double v = strtod(e, &end);
        if (end != e && std::isfinite(v) && v > 0) mb = v;
    }
    return std::max<int64_t>(1, (int64_t)std::min(std::ceil(mb * 1048576.0), 1e15));
}

double now_ms()
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

struct Run {
    int64_t file_off, len;
};
struct ChunkPlan {
    int32_t r0, r1;     // reads of the selection
    size_t run0, run1;  // their runs
    int64_t bytes;
};

// what a call holds on the device and in page-locked memory; released on every way out
struct Buffers {
    dh_ctx *ctx;
    int fd = -1;
    int64_t cap = 0;
    void *pin[2] = {nullptr, nullptr};
    DevBuf<uint8_t> pk[2];
    DevBuf<int64_t> pk_off;
    hipEvent_t cs[2] = {}, ks[2] = {}, ke[2] = {};
    explicit Buffers(dh_ctx *c) : ctx(c) {}
    ~Buffers()
    {
        (void)hipStreamSynchronize(ctx->stream);
        if (fd >= 0) close(fd);
        for (int b = 0; b < 2; b++) {
            if (pin[b]) dh_pinned_free(pin[b], (size_t)cap);
            if (cs[b]) (void)hipEventDestroy(cs[b]);
            if (ks[b]) (void)hipEventDestroy(ks[b]);
            if (ke[b]) (void)hipEventDestroy(ke[b]);
        }
    }
};
}  // namespace

extern "C" int dh_dazz_load_reads(dh_ctx *ctx, const char *db_path, const int32_t *ids, int32_t n, dh_db **out)
{
    if (!ctx || !ctx->stream) return dh_fail(DH_EINVAL, "dh_dazz_load_reads: needs a context with a device (there is no CPU route)");
    if (!db_path || !out) return dh_fail(DH_EINVAL, "dh_dazz_load_reads: NULL argument");
    if (n < 1 || !ids) return dh_fail(DH_EINVAL, "dh_dazz_load_reads: needs at least one read id");
    const double t_begin = now_ms();
    DazzView v;
    if (int rc = dh_dazz_view_open(db_path, v)) return rc;
    std::vector<int32_t> kept;  // view id -> untrimmed id
    for (int i = v.ulo; i < v.uhi; i++)
        if (v.keep(v.reads[(size_t)i])) kept.push_back(i);
    const int32_t nview = (int32_t)kept.size();
    for (int32_t k = 0; k < n; k++) {
        if (ids[k] < 0 || ids[k] >= nview)
            return dh_fail(DH_EINVAL, "dh_dazz_load_reads: read id " + std::to_string(ids[k]) + " outside the view's " + std::to_string(nview) + " reads");
        if (k > 0 && ids[k] <= ids[k - 1])
            return dh_fail(DH_EINVAL, std::string("dh_dazz_load_reads: read ids must be ascending and distinct (") +
                                          (ids[k] == ids[k - 1] ? "duplicate" : "unsorted") + " id " + std::to_string(ids[k]) + ")");
    }
    // the plan: offsets of the output, the packed offset of every read inside its chunk, the runs, the chunks (a chunk is
    // empty only when it is the only one and no selected read has a base)
    std::vector<int64_t> off((size_t)n + 1, 0), pk_off((size_t)n, 0);
    std::vector<Run> runs;
    std::vector<ChunkPlan> chunks;
    struct stat sb;
    Buffers B(ctx);
    B.fd = open(v.bps_path.c_str(), O_RDONLY);
    if (B.fd < 0 || fstat(B.fd, &sb) != 0) return dh_fail(DH_EIO, "cannot open hidden files of " + v.stub);

    const int64_t limit = chunk_bytes();
    int64_t max_chunk = 0, packed_total = 0;
    for (int32_t k = 0; k < n; k++) {
        const DazzRead &r = v.reads[(size_t)kept[(size_t)ids[k]]];
        if (r.rlen < 0 || r.rlen >= (1 << 24)) return dh_fail(DH_EINVAL, "dh_dazz_load_reads: sequence length must be in [0, 2^24)");
        const int64_t nb = ((int64_t)r.rlen + 3) / 4;
        if (r.boff < 0 || r.boff + nb > (int64_t)sb.st_size) return dh_fail(DH_EIO, "short .bps");
        off[(size_t)k + 1] = off[(size_t)k] + r.rlen;
        if (chunks.empty() || (chunks.back().bytes > 0 && chunks.back().bytes + nb > limit))
            chunks.push_back(ChunkPlan{k, k, runs.size(), runs.size(), 0});
        ChunkPlan &c = chunks.back();
        pk_off[(size_t)k] = c.bytes;
        if (nb > 0) {
            if (c.run1 > c.run0 && runs.back().file_off + runs.back().len == r.boff)
                runs.back().len += nb;
            else {
                runs.push_back(Run{r.boff, nb});
                c.run1 = runs.size();
            }
        }
        c.bytes += nb;
        c.r1 = k + 1;
        max_chunk = std::max(max_chunk, c.bytes);
        packed_total += nb;
    }

    HIPCHK(hipSetDevice(ctx->device));
    uint8_t *d_alloc = nullptr, *d_bases = nullptr;
    if (int rc = dh_alloc_bases(ctx->stream, off.back(), &d_alloc, &d_bases, true)) return rc;
    dh_db *db = nullptr;
    if (int rc = dh_db_adopt(ctx, d_alloc, d_bases, off, std::vector<int32_t>(), &db)) {
        dh_dev_free(d_alloc);
        return rc;
    }
    struct DbGuard {  // the half-filled DB on any early return
        dh_db *d;
        ~DbGuard()
        {
            if (d) dh_db_destroy(d);
        }
    } guard{db};
    double ms_file = 0, ms_copy = 0, ms_kernel = 0;
    if (max_chunk > 0) {
        B.cap = max_chunk;
        HIPCHK(B.pk_off.alloc((size_t)n));
        HIPCHK(hipMemcpyAsync(B.pk_off.p, pk_off.data(), sizeof(int64_t) * (size_t)n, hipMemcpyHostToDevice, ctx->stream));
        const int nbuf = chunks.size() > 1 ? 2 : 1;
        for (int b = 0; b < nbuf; b++) {
            HIPCHK(B.pk[b].alloc((size_t)B.cap));
            if (!(B.pin[b] = dh_pinned_alloc((size_t)B.cap)))
                return dh_fail(DH_ENOMEM, "dh_dazz_load_reads: no page-locked memory for a chunk (DH_LOAD_CHUNK_MB)");
            HIPCHK(hipEventCreate(&B.cs[b]));
            HIPCHK(hipEventCreate(&B.ks[b]));
            HIPCHK(hipEventCreate(&B.ke[b]));
        }
        // chunk j's kernel has ended: its buffers are free again and its times are known
        auto retire = [&](size_t j) -> int {
            const int b = (int)(j & 1);
            HIPCHK(hipEventSynchronize(B.ke[b]));
            float c = 0, k = 0;
            HIPCHK(hipEventElapsedTime(&c, B.cs[b], B.ks[b]));
            HIPCHK(hipEventElapsedTime(&k, B.ks[b], B.ke[b]));
            ms_copy += c;
            ms_kernel += k;
            return DH_OK;
        };
        for (size_t i = 0; i < chunks.size(); i++) {
            const ChunkPlan &c = chunks[i];
            const int b = (int)(i & 1);
            if (i >= 2)
                if (int rc = retire(i - 2)) return rc;
            const double t0 = now_ms();
            uint8_t *dst = (uint8_t *)B.pin[b];
            for (size_t q = c.run0; q < c.run1; q++) {
                int64_t done = 0;
                while (done < runs[q].len) {
                    const ssize_t got = pread(B.fd, dst + done, (size_t)(runs[q].len - done), (off_t)(runs[q].file_off + done));
                    if (got <= 0) return dh_fail(DH_EIO, "short .bps");
                    done += got;
                }
                dst += runs[q].len;
            }
            ms_file += now_ms() - t0;
            HIPCHK(hipEventRecord(B.cs[b], ctx->stream));
            HIPCHK(hipMemcpyAsync(B.pk[b].p, B.pin[b], (size_t)c.bytes, hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipEventRecord(B.ks[b], ctx->stream));
            bl::Chunk ck{B.pk[b].p, B.pk_off.p + c.r0, db->d_off + c.r0, (int64_t)(c.r1 - c.r0)};
            dhk_bps_unpack(ctx->stream, &ck, off[(size_t)c.r0], off[(size_t)c.r1], db->d_bases);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(B.ke[b], ctx->stream));
        }
        for (size_t j = chunks.size() >= 2 ? chunks.size() - 2 : 0; j < chunks.size(); j++)
            if (int rc = retire(j)) return rc;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->load_ms[0] = ms_file;
    ctx->load_ms[1] = ms_copy;
    ctx->load_ms[2] = ms_kernel;
    ctx->load_ms[3] = now_ms() - t_begin;
    ctx->load_bytes[0] = packed_total;
    ctx->load_bytes[1] = off.back();
    ctx->load_bytes[2] = (int64_t)runs.size();
    ctx->load_bytes[3] = (int64_t)chunks.size();
    guard.d = nullptr;
    *out = db;
    return DH_OK;
}

// the last dh_dazz_load_reads of the context: ms4 = file reads, uploads, kernels, the whole call; counts4 = packed bytes
// read from the .bps, bases written, runs, chunks
extern "C" int dh_get_load_stats(dh_ctx *ctx, double *ms4, int64_t *counts4)
{
    if (!ctx || !ms4 || !counts4) return dh_fail(DH_EINVAL, "dh_get_load_stats: NULL");
    for (int i = 0; i < 4; i++) {
        ms4[i] = ctx->load_ms[i];
        counts4[i] = ctx->load_bytes[i];
    }
    return DH_OK;
}

extern "C" int dh_db_get_bases(dh_db *db, int32_t first, int32_t count, uint8_t *out, int64_t cap)
{
    if (!db || first < 0 || count < 0 || (int64_t)first + count > db->n) return dh_fail(DH_EINVAL, "dh_db_get_bases: sequences outside the DB");
    const int64_t a = db->h_off[(size_t)first], nb = db->h_off[(size_t)first + (size_t)count] - a;
    if (nb > cap || (nb > 0 && !out)) return dh_fail(DH_EINVAL, "dh_db_get_bases: the buffer holds " + std::to_string(cap) + " of " + std::to_string(nb) + " bases");
    if (nb == 0) return DH_OK;
    HIPCHK(hipSetDevice(db->ctx->device));
    HIPCHK(hipMemcpyAsync(out, db->d_bases + a, (size_t)nb, hipMemcpyDeviceToHost, db->ctx->stream));
    HIPCHK(hipStreamSynchronize(db->ctx->stream));
    return DH_OK;
}

// off[n + 1] of any DB (the host copy every DB keeps)
extern "C" int dh_db_get_offsets(const dh_db *db, int64_t *off)
{
    if (!db || !off) return dh_fail(DH_EINVAL, "dh_db_get_offsets: NULL");
    memcpy(off, db->h_off.data(), sizeof(int64_t) * db->h_off.size());
    return DH_OK;
}
