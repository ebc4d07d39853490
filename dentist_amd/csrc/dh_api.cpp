// dh_api.cpp -- the context of libdentist_hip.so: error reporting (dh_fail / dh_last_error), the ABI version, the life
// cycle of a dh_ctx with its scratch arena (dh_scratch; the slots are DhSlot in dh_internal.h), the statistics getters
// and the default alignment options.  No CPU fallback: every compute entry point needs a working HIP device.
#include <cstring>

#include "dh_internal.h"

static_assert(sizeof(dh_align_opts) == sizeof(DhOpts), "opts layout");
static_assert(sizeof(dh_la) == sizeof(DhLa), "la layout");
static_assert(sizeof(dh_la) == 48, "la size");

static thread_local std::string g_err;

int dh_fail(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
#define fail dh_fail

extern "C" const char *dh_last_error(void) { return g_err.c_str(); }
extern "C" int32_t dh_abi_version(void) { return 5; }  // 5: dh_extend_candidates (no struct changed); 4: dh_process_opts.max_partners, .min_relative_score_ppm (64 bytes); 3: dh_align_opts.algo

// ------------------------------------------------------------------------------------ context


extern "C" int dh_ctx_create(int32_t device, void *stream, dh_ctx **out)
{
    if (!out) return fail(DH_EINVAL, "dh_ctx_create: out is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail(DH_ENODEV, "no HIP device available (libdentist_hip has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(DH_EINVAL, "dh_ctx_create: bad device index");
    HIPCHK(hipSetDevice(device));
    dh_ctx *c = new dh_ctx();
    struct CtxCreateGuard {
        dh_ctx *&c;
        bool ok = false;
        ~CtxCreateGuard()
        {
            if (!ok && c) {
                for (auto &e : c->ev)
                    if (e) (void)hipEventDestroy(e);
                for (auto &e : c->cev)
                    if (e) (void)hipEventDestroy(e);
                if (c->cstream) (void)hipStreamDestroy(c->cstream);
                if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
                delete c;
            }
        }
    } cguard{c};
    c->device = device;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    c->ncu = prop.multiProcessorCount;
    if (stream) {
        c->stream = (hipStream_t)stream;
    } else {
        HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
        c->own_stream = true;
    }
    for (auto &e : c->ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    for (auto &e : c->cev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    cguard.ok = true;
    *out = c;
    return DH_OK;
}

extern "C" void dh_ctx_destroy(dh_ctx *c)
{
    if (!c) return;
    for (dh_ctx *s : c->sub)
        if (s) dh_ctx_destroy(s);
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    if (c->cstream) (void)hipStreamSynchronize(c->cstream);
    for (auto &e : c->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &e : c->cev)
        if (e) (void)hipEventDestroy(e);
    if (c->cstream) (void)hipStreamDestroy(c->cstream);
    for (auto &a : c->arena)
        if (a.p) dh_dev_free(a.p);
    dh_dev_trim();
    dh_pinned_trim();
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int dh_scratch(dh_ctx *ctx, DhSlot id, size_t bytes, void **out)
{
    dh_ctx::Arena &a = ctx->arena[id];
    if (bytes > a.cap) {
        if (a.p) {
            HIPCHK(hipStreamSynchronize(ctx->stream));
            dh_dev_free(a.p);
            a.p = nullptr;
            a.cap = 0;
        }
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = dh_dev_alloc(&a.p, want);
        if (e != hipSuccess) {
            // (the other slots cannot be released from here: the caller holds pointers into the ones it asked for earlier
            // in the same call.  Between calls the host can: dh_ctx_release_scratch)
            a.p = nullptr;
            a.cap = 0;
            return fail(DH_EHIP, std::string("device scratch of ") + std::to_string(want >> 20) + " MB: " +
                                     hipGetErrorString(e) + " (dh_ctx_release_scratch frees what earlier calls keep)");
        }
        a.cap = want;
    }
    *out = a.p;
    return DH_OK;
}

extern "C" int dh_ctx_release_scratch(dh_ctx *c)
{
    if (!c) return fail(DH_EINVAL, "ctx is NULL");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (c->cstream) HIPCHK(hipStreamSynchronize(c->cstream));
    for (dh_ctx *s2 : c->sub)
        if (s2) (void)dh_ctx_release_scratch(s2);
    for (auto &a : c->arena)
        if (a.p) {
            dh_dev_free(a.p);
            a.p = nullptr;
            a.cap = 0;
        }
    dh_dev_trim();
    return DH_OK;
}

extern "C" int dh_ctx_sync(dh_ctx *c)
{
    if (!c) return fail(DH_EINVAL, "ctx is NULL");
    HIPCHK(hipStreamSynchronize(c->stream));
    return DH_OK;
}

extern "C" int dh_get_mjoin_counts(dh_ctx *c, int64_t *out2, int32_t reset)
{
    if (!c || !out2) return fail(DH_EINVAL, "dh_get_mjoin_counts: NULL");
    out2[0] = c->mj_chunks;
    out2[1] = c->mj_fallbacks;
    if (reset) c->mj_chunks = c->mj_fallbacks = 0;
    return DH_OK;
}

extern "C" int dh_get_tjoin_counts(dh_ctx *c, int64_t *out4, int32_t reset)
{
    if (!c || !out4) return fail(DH_EINVAL, "dh_get_tjoin_counts: NULL");
    out4[0] = c->tj_calls;
    out4[1] = c->tj_fallbacks;
    out4[2] = c->tj_last_hits;
    out4[3] = c->tj_reruns;
    if (reset) c->tj_calls = c->tj_fallbacks = c->tj_last_hits = c->tj_reruns = 0;
    return DH_OK;
}

extern "C" int dh_get_seed_tier_counts(dh_ctx *c, int64_t *out2, int32_t reset)
{
    if (!c || !out2) return fail(DH_EINVAL, "dh_get_seed_tier_counts: NULL");
    out2[0] = c->seed_mid_chunks;
    out2[1] = c->seed_mid_redone;
    if (reset) c->seed_mid_chunks = c->seed_mid_redone = 0;
    return DH_OK;
}

extern "C" int dhk_seed_band_counts(unsigned long long *out, int reset);

// (the kernels count on the device: the figures are those of the context's device, whichever context launched)
extern "C" int dh_get_seed_band_counts(dh_ctx *c, int64_t *out2, int32_t reset)
{
    if (!c || !out2) return fail(DH_EINVAL, "dh_get_seed_band_counts: NULL");
    HIPCHK(hipSetDevice(c->device));
    unsigned long long v[2] = {0, 0};
    if (dhk_seed_band_counts(v, reset)) return fail(DH_EHIP, "dh_get_seed_band_counts: the counters could not be read");
    out2[0] = (int64_t)v[0];
    out2[1] = (int64_t)v[1];
    return DH_OK;
}

extern "C" int dh_get_join_counts(dh_ctx *c, int64_t *out4, int32_t reset)
{
    if (!c || !out4) return fail(DH_EINVAL, "dh_get_join_counts: NULL");
    out4[0] = c->join_launches;
    out4[1] = c->join_reruns;
    out4[2] = c->join_last_hits;
    out4[3] = c->join_first_cap;
    if (reset) c->join_launches = c->join_reruns = c->join_last_hits = c->join_first_cap = 0;
    return DH_OK;
}

extern "C" int dh_get_align_stats(dh_ctx *c, dh_align_stats *out)
{
    if (!c || !out) return fail(DH_EINVAL, "dh_get_align_stats: NULL");
    *out = c->stats;
    return DH_OK;
}

extern "C" int dh_get_cum_stats(dh_ctx *c, dh_cum_stats *out, int32_t reset)
{
    if (!c || !out) return fail(DH_EINVAL, "dh_get_cum_stats: NULL");
    *out = c->cum;
    if (reset) c->cum = dh_cum_stats();
    return DH_OK;
}

extern "C" void dh_default_align_opts(dh_align_opts *o)
{
    memset(o, 0, sizeof(*o));
    o->k = 14;
    o->hmin = 35;
    o->band_shift = 6;
    o->tspace = 100;
    o->min_len = 500;
    o->pen = 6;
    o->xdrop = 120;
    o->max_err_ppm = 300000;
    o->max_cand = 32;
    o->max_la = 4;
    o->tcap = 64;
    o->strands = 3;
    o->skip_self = 0;
    o->dmax = 60000;
    o->width = 30;  /* two alignments per wavefront (k_wave2); up to 62 selects one per wavefront */
    o->kmer_mod = 1;
}
