// dh_laset.cpp -- a dh_la_set on the host: its accessors, LAsort order (dh_la_less, dh_lasort), damapper's chain flags
// (dh_select_best_range, the near-best settings, dh_finish_transposed_set), the .las codec and the merges.  Owns
// g_near_best_ppm.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "dh_internal.h"
#include "dh_parallel.h"

#define fail dh_fail

// ------------------------------------------------------------------------------------ LA sets


extern "C" void dh_la_set_destroy(dh_la_set *s) { delete s; }
extern "C" int64_t dh_la_set_count(const dh_la_set *s) { return s ? (int64_t)s->la.size() : 0; }
dh_la_set::~dh_la_set()
{
    if (d_trace_own) {
        (void)hipSetDevice(device);
        dh_dev_free(d_trace_own);
    }
}
int dh_la_set_ensure_host_trace(dh_la_set *s)
{
    if (!s || !s->trace.empty() || s->d_trace_own_len <= 0) return DH_OK;
    HIPCHK(hipSetDevice(s->device));
    s->trace.resize((size_t)s->d_trace_own_len);
    HIPCHK(hipMemcpy(s->trace.data(), s->d_trace_own, sizeof(uint16_t) * (size_t)s->d_trace_own_len, hipMemcpyDeviceToHost));
    return DH_OK;
}
extern "C" int32_t dh_la_set_trace_on_device(const dh_la_set *s) { return s && s->d_trace_own_len > 0 && s->trace.empty() ? 1 : 0; }
extern "C" int64_t dh_la_set_trace_len(const dh_la_set *s)
{
    return s ? (s->trace.empty() && s->d_trace_own_len > 0 ? s->d_trace_own_len : (int64_t)s->trace.size()) : 0;
}
extern "C" const dh_la *dh_la_set_records(const dh_la_set *s) { return s ? s->la.data() : nullptr; }
extern "C" const uint16_t *dh_la_set_trace(const dh_la_set *s)
{
    if (!s) return nullptr;
    if (dh_la_set_ensure_host_trace(const_cast<dh_la_set *>(s)) != DH_OK) return nullptr;  // (left on the device: fetched now)
    return s->trace.data();
}
extern "C" int32_t dh_la_set_tspace(const dh_la_set *s) { return s ? s->tspace : 0; }

// LAsort order (a, b, comp, abpos, aepos, bbpos, bepos, diffs): base.d:1787-1809
static bool la_less(const dh_la &p, const dh_la &q)
{
    if (p.aread != q.aread) return p.aread < q.aread;
    if (p.bread != q.bread) return p.bread < q.bread;
    const uint32_t pc = p.flags & DH_FLAG_COMP, qc = q.flags & DH_FLAG_COMP;
    if (pc != qc) return pc < qc;
    if (p.abpos != q.abpos) return p.abpos < q.abpos;
    if (p.aepos != q.aepos) return p.aepos < q.aepos;
    if (p.bbpos != q.bbpos) return p.bbpos < q.bbpos;
    if (p.bepos != q.bepos) return p.bepos < q.bepos;
    return p.diffs < q.diffs;
}

// damapper-style chain flags per B read: every LA is a chain of its own (START); it is BEST
// unless a higher-scoring LA of the same read and orientation covers more than half of it on B
// (consumer: dazzler.d:1728-1758 reads START without BEST as alternateChain).
// `la` must be grouped by bread (the kernels emit it that way).
// damapper's chain flags (consumer: source/dentist/dazzler.d:1728-1758, 1991-1998).  Per read:
//   1. the local alignments on one contig and strand, ordered by their A interval, are linked into chains: an LA
//      continues the chain of its predecessor when it lies after it on both sequences (up to CHAIN_OVERLAP bases of
//      overlap), the gaps are at most CHAIN_GAP on either sequence and differ by at most CHAIN_INDEL (a read that
//      carries a long indel maps as two collinear LAs -- SURVEY section 7, K6);
//   2. score of a chain = sum of (A length - 2 * diffs) of its LAs;
//   3. a chain is the BEST one of its stretch of the read unless a higher-scoring chain of the same strand (ties:
//      the one whose first LA sorts later in LAsort order) covers more than half of its B span;
//   4. flags: START on the first LA of a chain, NEXT on the others, BEST on every LA of a best chain; START without
//      BEST reads as `alternateChain`.  near_best_ppm > 0 (damapper -n): an alternate chain scoring less than that
//      fraction of the chain that beats it is DISABLED (damapper does not report it).
#define CHAIN_GAP 10000
#define CHAIN_INDEL 6000
#define CHAIN_OVERLAP 100
// process-wide default (dh_set_near_best) and the per-context override (dh_ctx_set_near_best, -1 = use the default):
// a library user who never asked for -n is not affected by another context's setting
static std::atomic<int32_t> g_near_best_ppm{0};
extern "C" void dh_set_near_best(int32_t ppm) { g_near_best_ppm.store(ppm < 0 ? 0 : ppm); }
extern "C" int dh_ctx_set_near_best(dh_ctx *ctx, int32_t ppm)
{
    if (!ctx) return fail(DH_EINVAL, "dh_ctx_set_near_best: NULL context");
    ctx->near_best_ppm = ppm < 0 ? -1 : ppm;
    return DH_OK;
}

void dh_select_best_range(dh_la *la, size_t nla, int32_t near_ppm)
{
    // groups of equal bread are independent: host threads take runs of groups
    const std::vector<int64_t> gstart = dh_run_starts((int64_t)nla, [la](int64_t i) { return la[i].bread; });
    dh_parallel_for((int64_t)gstart.size() - 1, 2048, [&](int64_t glo, int64_t ghi) {
        struct Chain {  // members = ord[k0 .. k1): a chain only ever continues the chain before it (no vector per chain:
            int64_t score;  // half a million small allocations per chunk from 256 threads were most of the hook's 2.5 ms)
            int32_t bb, be, comp;
            size_t first;
            size_t k0, k1;
        };
        std::vector<size_t> ord;
        std::vector<Chain> chains;
        for (int64_t g = glo; g < ghi; g++) {
            const size_t g0 = (size_t)gstart[(size_t)g], g1 = (size_t)gstart[(size_t)g + 1];
            ord.clear();
            for (size_t x = g0; x < g1; x++) ord.push_back(x);
            std::sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return la_less(la[x], la[y]); });  // (a, b, comp, abpos, ...)
            chains.clear();
            for (size_t k = 0; k < ord.size(); k++) {
                const dh_la &q = la[ord[k]];
                bool linked = false;
                if (!chains.empty()) {
                    Chain &c = chains.back();
                    const dh_la &p = la[ord[c.k1 - 1]];
                    const int64_t ga = (int64_t)q.abpos - p.aepos, gb = (int64_t)q.bbpos - p.bepos;
                    linked = p.aread == q.aread && (p.flags & DH_FLAG_COMP) == (q.flags & DH_FLAG_COMP) && ga >= -CHAIN_OVERLAP &&
                             gb >= -CHAIN_OVERLAP && ga <= CHAIN_GAP && gb <= CHAIN_GAP && std::llabs(ga - gb) <= CHAIN_INDEL &&
                             q.aepos > p.aepos && q.bepos > p.bepos;
                    if (linked) {
                        c.k1 = k + 1;
                        c.score += (int64_t)(q.aepos - q.abpos) - 2 * (int64_t)q.diffs;
                        c.be = q.bepos;
                    }
                }
                if (!linked)
                    chains.push_back(Chain{(int64_t)(q.aepos - q.abpos) - 2 * (int64_t)q.diffs, q.bbpos, q.bepos,
                                           (int32_t)(q.flags & DH_FLAG_COMP), ord[k], k, k + 1});
            }
            for (size_t x = 0; x < chains.size(); x++) {
                const Chain &p = chains[x];
                bool best = true, drop = false;
                for (size_t y = 0; y < chains.size(); y++) {
                    if (x == y) continue;
                    const Chain &q = chains[y];
                    // ties: the chain whose first LA sorts later (LAsort order) wins
                    if (q.score < p.score || (q.score == p.score && la_less(la[q.first], la[p.first]))) continue;
                    if (q.comp != p.comp) continue;
                    const int32_t lo = std::max(p.bb, q.bb), hi = std::min(p.be, q.be);
                    if (hi - lo > (p.be - p.bb) / 2) {
                        best = false;
                        if (near_ppm > 0 && p.score * 1000000ll < (int64_t)near_ppm * q.score) drop = true;
                    }
                }
                for (size_t m = 0; m < p.k1 - p.k0; m++) {
                    dh_la &l = la[ord[p.k0 + m]];
                    l.flags &= ~(DH_FLAG_START | DH_FLAG_NEXT | DH_FLAG_BEST);
                    l.flags |= (m == 0 ? DH_FLAG_START : DH_FLAG_NEXT) | (best ? DH_FLAG_BEST : 0u) | (drop ? DH_FLAG_DISABLED : 0u);
                }
            }
            // the records of the read in LAsort order: a chain's members are then neighbours (a chain only ever continues the
            // chain before it), START followed by its NEXT records -- how damapper writes them and how every consumer
            // rebuilds the chains (dazzler.d:1728-1758); the trace values stay where they are (toff)
            if (!std::is_sorted(ord.begin(), ord.end())) {
                std::vector<dh_la> tmp(ord.size());
                for (size_t k = 0; k < ord.size(); k++) tmp[k] = la[ord[k]];
                for (size_t k = 0; k < ord.size(); k++) la[g0 + k] = tmp[k];
            }
        }
    });
}

int32_t dh_ctx_near_best_ppm(const dh_ctx *ctx) { return ctx->near_best_ppm >= 0 ? ctx->near_best_ppm : g_near_best_ppm.load(); }

// chain flags of a set of transposed records (aread = read, bread = contig), grouped by aread: the same rule with the
// roles of the sequences exchanged (chains of a read on one contig, ordered along the read); then LAsort order
void dh_finish_transposed_set(dh_la_set *set, bool want_best, int32_t near_ppm)
{
    auto swap_roles = [&]() {
        for (dh_la &l : set->la) {
            std::swap(l.aread, l.bread);
            std::swap(l.abpos, l.bbpos);
            std::swap(l.aepos, l.bepos);
        }
    };
    if (want_best) {
        swap_roles();
        dh_select_best_range(set->la.data(), set->la.size(), near_ppm);
        swap_roles();
    }
    std::sort(set->la.begin(), set->la.end(), la_less);
}
bool dh_la_less(const dh_la &p, const dh_la &q) { return la_less(p, q); }

// LAsort order of a B-major (bread, strand, ...) list in O(n): stable counting sort by aread
// keeps (bread, comp) ascending inside every aread; the rare runs with equal (aread, bread, comp)
// are finished with an insertion sort.
void dh_lasort(dh_la_set *res, int32_t na)
{
    const size_t n = res->la.size();
    LaVec out(n);
    const int64_t chunk = 8192, nchunks = ((int64_t)n + chunk - 1) / chunk;
    if (na <= 4096 && nchunks > 1) {
        // stable counting sort by aread with one histogram per input chunk (threads scatter)
        std::vector<int64_t> hist((size_t)nchunks * ((size_t)na + 1), 0);
        dh_parallel_for(nchunks, 1, [&](int64_t clo, int64_t chi) {
            for (int64_t c = clo; c < chi; c++) {
                int64_t *h = hist.data() + (size_t)c * ((size_t)na + 1);
                const size_t e = std::min(n, (size_t)(c + 1) * (size_t)chunk);
                for (size_t i = (size_t)c * (size_t)chunk; i < e; i++) h[(size_t)res->la[i].aread]++;
            }
        });
        int64_t run = 0;
        for (int32_t a = 0; a <= na; a++)
            for (int64_t c = 0; c < nchunks; c++) {
                int64_t &h = hist[(size_t)c * ((size_t)na + 1) + (size_t)a];
                const int64_t cnt = h;
                h = run;
                run += cnt;
            }
        dh_parallel_for(nchunks, 1, [&](int64_t clo, int64_t chi) {
            for (int64_t c = clo; c < chi; c++) {
                int64_t *h = hist.data() + (size_t)c * ((size_t)na + 1);
                const size_t e = std::min(n, (size_t)(c + 1) * (size_t)chunk);
                for (size_t i = (size_t)c * (size_t)chunk; i < e; i++) {
                    const dh_la &l = res->la[i];
                    out[(size_t)h[(size_t)l.aread]++] = l;
                }
            }
        });
    } else {
        std::vector<int64_t> first((size_t)na + 2, 0);
        for (const dh_la &l : res->la) first[(size_t)l.aread + 1]++;
        for (int32_t a = 0; a <= na; a++) first[(size_t)a + 1] += first[(size_t)a];
        for (const dh_la &l : res->la) out[(size_t)first[(size_t)l.aread]++] = l;
    }
    for (size_t i = 1; i < n; i++) {
        if (!la_less(out[i], out[i - 1])) continue;
        dh_la x = out[i];
        size_t j = i;
        while (j > 0 && la_less(x, out[j - 1])) {
            out[j] = out[j - 1];
            j--;
        }
        out[j] = x;
    }
    // the traces stay where the device compaction put them: every record's toff still points at
    // its (diffs, bbases) pairs, only the records are permuted (saves re-laying out tens of MB)
    res->la.swap(out);
}

// ------------------------------------------------------------------------------------ .las

// header int64 novl + int32 tspace; record = 40 bytes (9 x int32 + pad); trace values are u8 when
// tspace <= 125 (TRACE_XOVR) else u16 -- dazzler.d:1665-1834, 1988-2032, 2130-2170.
extern "C" int dh_las_write(const char *path, const dh_la *las, int64_t n, const uint16_t *trace,
                            int32_t tspace)
{
    if (!path || (n > 0 && (!las || !trace))) return fail(DH_EINVAL, "dh_las_write: NULL argument");
    FILE *f = fopen(path, "wb");
    if (!f) return fail(DH_EIO, std::string("cannot open ") + path);
    bool ok = fwrite(&n, 8, 1, f) == 1 && fwrite(&tspace, 4, 1, f) == 1;
    const bool small = tspace <= 125;
    std::vector<uint8_t> tmp;
    for (int64_t i = 0; ok && i < n; i++) {
        const dh_la &l = las[i];
        const int32_t rec[10] = {l.tlen, l.diffs, l.abpos, l.bbpos, l.aepos,
                                 l.bepos, (int32_t)l.flags, l.aread, l.bread, 0};
        ok = fwrite(rec, 4, 10, f) == 10;
        const uint16_t *t = trace + l.toff;
        if (small) {
            tmp.resize((size_t)l.tlen);
            for (int32_t j = 0; j < l.tlen; j++) {
                if (t[j] > 255) {
                    fclose(f);
                    return fail(DH_EINVAL, "dh_las_write: trace value exceeds 8 bits at tspace <= 125");
                }
                tmp[(size_t)j] = (uint8_t)t[j];
            }
            ok = ok && (l.tlen == 0 || fwrite(tmp.data(), 1, (size_t)l.tlen, f) == (size_t)l.tlen);
        } else
            ok = ok && (l.tlen == 0 || fwrite(t, 2, (size_t)l.tlen, f) == (size_t)l.tlen);
    }
    if (fclose(f) != 0) ok = false;
    return ok ? DH_OK : fail(DH_EIO, std::string("short write to ") + path);
}

extern "C" int dh_las_read(const char *path, dh_la_set **out)
{
    if (!path || !out) return fail(DH_EINVAL, "dh_las_read: NULL argument");
    FILE *f = fopen(path, "rb");
    if (!f) return fail(DH_EIO, std::string("cannot open ") + path);
    int64_t novl = 0;
    int32_t ts = 0;
    if (fread(&novl, 8, 1, f) != 1 || fread(&ts, 4, 1, f) != 1) {
        fclose(f);
        return fail(DH_EIO, std::string("error reading LAS file `") + path + "`: unexpected end of file");
    }
    dh_la_set *s = new dh_la_set();
    s->tspace = ts;
    const bool small = ts <= 125;
    std::vector<uint8_t> tmp;
    for (int64_t i = 0; i < novl; i++) {
        int32_t rec[10];
        if (fread(rec, 4, 10, f) != 10) {
            fclose(f);
            delete s;
            return fail(DH_EIO, std::string("error reading LAS file `") + path +
                                    "`: unexpected end of file; expected overlapHead");
        }
        dh_la l = {};
        l.tlen = rec[0];
        l.diffs = rec[1];
        l.abpos = rec[2];
        l.bbpos = rec[3];
        l.aepos = rec[4];
        l.bepos = rec[5];
        l.flags = (uint32_t)rec[6];
        l.aread = rec[7];
        l.bread = rec[8];
        l.toff = (int64_t)s->trace.size();
        if (l.tlen < 0 || l.tlen % 2) {
            fclose(f);
            delete s;
            return fail(DH_EIO, "illegal value for tlen: must be multiple of 2");
        }
        s->trace.resize(s->trace.size() + (size_t)l.tlen);
        uint16_t *t = s->trace.data() + l.toff;
        bool ok;
        if (small) {
            tmp.resize((size_t)l.tlen);
            ok = l.tlen == 0 || fread(tmp.data(), 1, (size_t)l.tlen, f) == (size_t)l.tlen;
            for (int32_t j = 0; ok && j < l.tlen; j++) t[j] = tmp[(size_t)j];
        } else
            ok = l.tlen == 0 || fread(t, 2, (size_t)l.tlen, f) == (size_t)l.tlen;
        if (!ok) {
            fclose(f);
            delete s;
            return fail(DH_EIO, std::string("error reading LAS file `") + path +
                                    "`: unexpected end of file; expected tracePoints");
        }
        s->la.push_back(l);
    }
    fclose(f);
    *out = s;
    return DH_OK;
}

// LAmerge in memory: the result sets of the read blocks (dh_align_db_block) merged into one set in
// LAsort order; traces are concatenated in set order and every record's toff is rebased.
extern "C" int dh_la_set_merge(const dh_la_set *const *sets, int32_t nsets, dh_la_set **out)
{
    if (!sets || nsets < 1 || !out) return fail(DH_EINVAL, "dh_la_set_merge: bad argument");
    int32_t tspace = -1;
    size_t nla = 0, ntr = 0;
    for (int32_t i = 0; i < nsets; i++) {
        if (!sets[i]) return fail(DH_EINVAL, "dh_la_set_merge: NULL set");
        if (int rc = dh_la_set_ensure_host_trace(const_cast<dh_la_set *>(sets[i]))) return rc;
        if (!sets[i]->la.empty()) {
            if (tspace >= 0 && sets[i]->tspace != tspace)
                return fail(DH_EINVAL, "dh_la_set_merge: sets with different trace spacing");
            tspace = sets[i]->tspace;
        }
        nla += sets[i]->la.size();
        ntr += sets[i]->trace.size();
    }
    dh_la_set *res = new dh_la_set();
    res->tspace = tspace >= 0 ? tspace : sets[0]->tspace;
    res->la.resize(nla);
    res->trace.resize(ntr);
    size_t l0 = 0, t0 = 0;
    int32_t na = 0;
    for (int32_t i = 0; i < nsets; i++) {
        const dh_la_set *x = sets[i];
        if (!x->trace.empty()) memcpy(res->trace.data() + t0, x->trace.data(), sizeof(uint16_t) * x->trace.size());
        for (size_t j = 0; j < x->la.size(); j++) {
            dh_la l = x->la[j];
            l.toff += (int64_t)t0;
            na = std::max(na, l.aread + 1);
            res->la[l0 + j] = l;
        }
        l0 += x->la.size();
        t0 += x->trace.size();
    }
    // every input is in LAsort order: a stable sort of the concatenation is the merge
    std::stable_sort(res->la.begin(), res->la.end(), la_less);
    *out = res;
    return DH_OK;
}

// LAmerge (workflow rule snakemake/Snakefile:1173-1185): the alignment files of the read blocks
// (one per GPU / per block) merged into one file in LAsort order.  Host only.
extern "C" int dh_las_merge(const char *const *paths, int32_t npaths, const char *out_path)
{
    if (!paths || npaths < 1 || !out_path) return fail(DH_EINVAL, "dh_las_merge: bad argument");
    std::vector<dh_la_set *> sets((size_t)npaths, nullptr);
    struct Guard {
        std::vector<dh_la_set *> &s;
        ~Guard()
        {
            for (dh_la_set *x : s) dh_la_set_destroy(x);
        }
    } guard{sets};
    int32_t tspace = -1;
    size_t total = 0;
    for (int32_t i = 0; i < npaths; i++) {
        if (int rc = dh_las_read(paths[i], &sets[(size_t)i])) return rc;
        if (tspace >= 0 && sets[(size_t)i]->tspace != tspace && !sets[(size_t)i]->la.empty())
            return fail(DH_EINVAL, "dh_las_merge: files with different trace spacing");
        if (!sets[(size_t)i]->la.empty() || tspace < 0) tspace = sets[(size_t)i]->tspace;
        total += sets[(size_t)i]->la.size();
    }
    // records of all files with the index of their file; traces stay in their sets
    std::vector<std::pair<dh_la, int32_t>> all;
    all.reserve(total);
    for (int32_t i = 0; i < npaths; i++)
        for (const dh_la &l : sets[(size_t)i]->la) all.emplace_back(l, i);
    std::stable_sort(all.begin(), all.end(),
                     [](const std::pair<dh_la, int32_t> &x, const std::pair<dh_la, int32_t> &y) { return la_less(x.first, y.first); });
    std::vector<dh_la> las(all.size());
    std::vector<uint16_t> trace;
    for (size_t i = 0; i < all.size(); i++) {
        dh_la l = all[i].first;
        const uint16_t *t = sets[(size_t)all[i].second]->trace.data() + l.toff;
        l.toff = (int64_t)trace.size();
        trace.insert(trace.end(), t, t + l.tlen);
        las[i] = l;
    }
    static const uint16_t none = 0;
    return dh_las_write(out_path, las.data(), (int64_t)las.size(), trace.empty() ? &none : trace.data(), tspace);
}
