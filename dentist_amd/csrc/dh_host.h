// dh_host.h -- what the host drivers of the batched commands share (dh_editpath.cpp, dh_nw.cpp, dh_nwa.cpp, dh_locate.cpp,
// dh_chain.cpp, dh_pmask.cpp, dh_vreg.cpp, dh_cfilt.cpp): typed scratch slots, uploads on the context's stream, environment
// knobs, the clock of the DH_TRACE lines, the front of the set forms and the runner of the host plans.
#ifndef DH_HOST_H
#define DH_HOST_H

#include "dh_internal.h"

#include <stdlib.h>

#include <chrono>
#include <functional>

#include "dh_parallel.h"

// slot `id` of the context's scratch arena as `count` elements of T (an empty request still gets a buffer)
template <typename T>
int dh_scr(dh_ctx *ctx, DhSlot id, size_t count, T **out)
{
    return dh_scratch(ctx, id, sizeof(T) * std::max<size_t>(count, 1), (void **)out);
}

// a host array into its slot: an asynchronous copy on the context's stream, so `v` stays untouched until the stream has passed it
template <typename T>
int dh_upload(dh_ctx *ctx, DhSlot id, const T *v, size_t count, T **out)
{
    if (int rc = dh_scr(ctx, id, count, out)) return rc;
    if (count) HIPCHK(hipMemcpyAsync(*out, v, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
    return DH_OK;
}
template <typename T>
int dh_upload(dh_ctx *ctx, DhSlot id, const std::vector<T> &v, T **out)
{
    return dh_upload(ctx, id, v.data(), v.size(), out);
}

// an integer of the environment clamped to [lo, hi], `dflt` when it is not set (development knobs; no upper bound: pass the
// type's maximum)
inline int64_t dh_env_knob(const char *name, int64_t dflt, int64_t lo, int64_t hi)
{
    if (const char *e = getenv(name)) return std::min<int64_t>(std::max<int64_t>(lo, atoll(e)), hi);
    return dflt;
}

inline double dh_ms_since(std::chrono::steady_clock::time_point t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// The front of a *_set_* entry point `fn`: refuses a missing argument (args_ok: the entry point's other pointers) and a set
// whose records were left on the device, else hands back the set's host records.  Set / La: const or not, as the entry point has them.
template <class Set, class La>
int dh_set_host_records(const char *fn, bool args_ok, Set *set, La **las, int64_t *n)
{
    if (!args_ok || !set) return dh_fail(DH_EINVAL, std::string(fn) + ": bad argument");
    if (set->la.empty() && set->d_la_n > 0) return dh_fail(DH_EINVAL, std::string(fn) + ": the set's records are on the device only");
    *las = set->la.data();
    *n = (int64_t)set->la.size();
    return DH_OK;
}

// what the build_plan functions take to run their loops on the host threads, in chunks of GRAIN indices
template <int64_t GRAIN>
void dh_plan_runner(int64_t m, const std::function<void(int64_t, int64_t)> &body)
{
    dh_parallel_for(m, GRAIN, body);
}
const int64_t DH_PLAN_GRAIN = 1 << 14;  // the per-record loops of a plan

#endif
