// dh_db.cpp -- everything a dh_db owns on the device: its bases, the two layers of the soft mask and their
// recomposition (dh_db_set_mask, DBdust, coverage masks), the derived copies (reverse complement, 2-bit packed) and the
// k-mer index (dh_build_index).
#include <cmath>
#include <cstdlib>

#include "dh_internal.h"
#include "dh_tjoin.h"

#define fail dh_fail

// ------------------------------------------------------------------------------------ DB

// pads_only: the caller writes every base itself (dh_db_create: one copy of the whole array) -- only the DB_PAD bytes
// on both sides get the code 4.  Filling all of a reads DB first wrote 15.7 GB for configs[2] that the copy then overwrote.
int dh_alloc_bases(hipStream_t st, int64_t total, uint8_t **alloc, uint8_t **base, bool pads_only)
{
    const size_t nb = (size_t)std::max<int64_t>(total, 0) + 2 * DB_PAD;
    HIPCHK(dh_dev_alloc(alloc, nb));
    if (pads_only) {
        HIPCHK(hipMemsetAsync(*alloc, 4, DB_PAD, st));
        HIPCHK(hipMemsetAsync(*alloc + nb - DB_PAD, 4, DB_PAD, st));
    } else
        HIPCHK(dhk_memset(st, *alloc, 4, nb));
    *base = *alloc + DB_PAD;
    return DH_OK;
}



extern "C" int dh_db_create(dh_ctx *ctx, const uint8_t *bases, const int64_t *off, int32_t n,
                            const int32_t *group, dh_db **out)
{
    if (!ctx || !off || !out || n < 0) return fail(DH_EINVAL, "dh_db_create: bad argument");
    if (n > 0 && !bases) return fail(DH_EINVAL, "dh_db_create: bases is NULL");
    HIPCHK(hipSetDevice(ctx->device));
    dh_db *db = new dh_db();
    struct DbCreateGuard {  // releases the half-built DB on any early return
        dh_db *&d;
        bool ok = false;
        ~DbCreateGuard()
        {
            if (!ok && d) {
                dh_dev_free(d->d_bases_alloc);
                dh_dev_free(d->d_off);
                dh_dev_free(d->d_group);
                delete d;
            }
        }
    } guard{db};
    db->ctx = ctx;
    db->n = n;
    db->h_off.assign(off, off + n + 1);
    db->total = off[n] - off[0];
    if (off[0] != 0) return fail(DH_EINVAL, "dh_db_create: off[0] must be 0");
    for (int32_t i = 0; i < n; i++) {
        const int64_t l = off[i + 1] - off[i];
        if (l < 0 || l >= (1 << 24)) return fail(DH_EINVAL, "dh_db_create: sequence length must be in [0, 2^24)");
        db->max_len = std::max<int32_t>(db->max_len, (int32_t)l);
    }
    if (group) {
        db->h_group.assign(group, group + n);
        for (int32_t g : db->h_group) {
            if (g < 0) return fail(DH_EINVAL, "dh_db_create: negative group id");
            db->ngroups = std::max(db->ngroups, g + 1);
        }
    }
    if (int rc = dh_alloc_bases(ctx->stream, db->total, &db->d_bases_alloc, &db->d_bases, true)) return rc;
    HIPCHK(dh_dev_alloc(&db->d_off, sizeof(int64_t) * (size_t)(n + 1)));
    if (db->total > 0)
        HIPCHK(hipMemcpyAsync(db->d_bases, bases, (size_t)db->total, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(db->d_off, off, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice,
                          ctx->stream));
    if (group && n > 0) {
        HIPCHK(dh_dev_alloc(&db->d_group, sizeof(int32_t) * (size_t)n));
        HIPCHK(hipMemcpyAsync(db->d_group, group, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice,
                              ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    guard.ok = true;
    *out = db;
    return DH_OK;
}

extern "C" void dh_db_destroy(dh_db *db)
{
    if (!db) return;
    (void)hipSetDevice(db->ctx->device);
    (void)hipStreamSynchronize(db->ctx->stream);
    dh_dev_free(db->d_bases_alloc);
    dh_dev_free(db->d_rc_alloc);
    dh_dev_free(db->d_pk_alloc);
    dh_dev_free(db->d_rcpk_alloc);
    dh_dev_free(db->d_off);
    dh_dev_free(db->d_group);
    dh_mask_free(db);
    dh_dev_free(db->d_pflags);
    if (db->has_ix) db->ix.release();
    delete db;
}

int dh_db_set_pflags(dh_db *db, const uint8_t *flags)
{
    if (!db) return fail(DH_EINVAL, "dh_db_set_pflags: NULL");
    if (!flags) {
        dh_dev_free(db->d_pflags);
        db->d_pflags = nullptr;
        return DH_OK;
    }
    if (!db->d_pflags) HIPCHK(dh_dev_alloc(&db->d_pflags, (size_t)std::max(db->n, 1)));
    HIPCHK(hipMemcpyAsync(db->d_pflags, flags, (size_t)db->n, hipMemcpyHostToDevice, db->ctx->stream));
    HIPCHK(hipStreamSynchronize(db->ctx->stream));
    return DH_OK;
}

static size_t mask_bytes(const dh_db *db) { return (size_t)((db->total + 31) / 32) * 4 + 16; }

void dh_mask_free(dh_db *db)
{
    if (db->d_mask_bits != db->d_mask_user && db->d_mask_bits != db->d_mask_derived) dh_dev_free(db->d_mask_bits);
    dh_dev_free(db->d_mask_user);
    dh_dev_free(db->d_mask_derived);
    db->d_mask_bits = db->d_mask_user = db->d_mask_derived = nullptr;
}

int dh_ensure_mask_layer(dh_db *db, int derived, uint8_t **out)
{
    uint8_t *&layer = derived ? db->d_mask_derived : db->d_mask_user;
    if (!layer) {
        HIPCHK(dh_dev_alloc(&layer, mask_bytes(db)));
        HIPCHK(dhk_memset(db->ctx->stream, layer, 0, mask_bytes(db)));
    }
    *out = layer;
    return DH_OK;
}

// d_mask_bits = the only layer there is, or the OR of the two in a buffer of its own
int dh_mask_recompose(dh_db *db)
{
    uint8_t *u = db->d_mask_user, *d = db->d_mask_derived;
    const bool own = db->d_mask_bits && db->d_mask_bits != u && db->d_mask_bits != d;
    if (u && d) {
        if (!own) {
            db->d_mask_bits = nullptr;
            HIPCHK(dh_dev_alloc(&db->d_mask_bits, mask_bytes(db)));
        }
        dhk_or_words(db->ctx->stream, (uint32_t *)db->d_mask_bits, (const uint32_t *)u, (const uint32_t *)d,
                     (int64_t)(mask_bytes(db) / 4));
        HIPCHK(hipGetLastError());
        return DH_OK;
    }
    if (own) {
        HIPCHK(hipStreamSynchronize(db->ctx->stream));
        dh_dev_free(db->d_mask_bits);
    }
    db->d_mask_bits = u ? u : d;
    return DH_OK;
}

// soft mask of the DB (union of the daligner -m tracks): per sequence sorted, disjoint intervals.
// SET semantics: the call replaces the tracks of an earlier call; what the library derived itself
// (dh_db_dust, dh_db_mask_coverage) is a layer of its own and stays -- the effective mask is the OR
// of the two.  Passing ptr == NULL clears the whole mask, both layers.  The cached k-mer index is dropped.
extern "C" int dh_db_set_mask(dh_db *db, const int64_t *ptr, const int32_t *iv)
{
    if (!db) return fail(DH_EINVAL, "db is NULL");
    HIPCHK(hipSetDevice(db->ctx->device));
    HIPCHK(hipStreamSynchronize(db->ctx->stream));
    if (db->has_ix) db->ix.release();
    db->has_ix = false;
    if (!ptr) {
        dh_mask_free(db);
        return DH_OK;
    }
    for (int32_t s = 0; s < db->n; s++) {
        if (ptr[s] > ptr[s + 1]) return fail(DH_EINVAL, "dh_db_set_mask: pointers must be non-decreasing");
        const int64_t len = db->h_off[(size_t)s + 1] - db->h_off[(size_t)s];
        for (int64_t j = ptr[s]; j < ptr[s + 1]; j++)
            if (iv[2 * j] < 0 || iv[2 * j] > iv[2 * j + 1] || iv[2 * j + 1] > len ||
                (j > ptr[s] && iv[2 * j] < iv[2 * j - 1]))
                return fail(DH_EINVAL, "dh_db_set_mask: intervals must be sorted, disjoint and inside the sequence");
    }
    std::vector<uint8_t> bits(mask_bytes(db), 0);
    for (int32_t s = 0; s < db->n; s++)
        for (int64_t j = ptr[s]; j < ptr[s + 1]; j++)
            for (int64_t g = db->h_off[(size_t)s] + iv[2 * j]; g < db->h_off[(size_t)s] + iv[2 * j + 1]; g++)
                bits[(size_t)(g >> 3)] |= (uint8_t)(1u << (g & 7));
    uint8_t *layer;
    if (int rc = dh_ensure_mask_layer(db, 0, &layer)) return rc;
    HIPCHK(hipMemcpyAsync(layer, bits.data(), bits.size(), hipMemcpyHostToDevice, db->ctx->stream));
    if (int rc = dh_mask_recompose(db)) return rc;
    HIPCHK(hipStreamSynchronize(db->ctx->stream));
    return DH_OK;
}

int dh_db_dust_impl(dh_db *db)
{
    dh_ctx *ctx = db->ctx;
    if (db->has_ix) db->ix.release();
    db->has_ix = false;
    uint8_t *layer;
    if (int rc = dh_ensure_mask_layer(db, 1, &layer)) return rc;
    const int32_t chunk = db->max_len < 16384 ? 64 : 512;
    const int64_t tile = 256ll * chunk;
    std::vector<int2> tiles;
    for (int32_t s = 0; s < db->n; s++) {
        const int64_t len = db->h_off[(size_t)s + 1] - db->h_off[(size_t)s];
        for (int64_t a = 0; a < len - 15; a += tile) tiles.push_back(int2{s, (int32_t)a});
    }
    if (tiles.empty()) return dh_mask_recompose(db);
    DevBuf<int2> d_tiles;
    HIPCHK(d_tiles.alloc(tiles.size()));
    HIPCHK(hipMemcpyAsync(d_tiles.p, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice, ctx->stream));
    dhk_dust(ctx->stream, db->d_bases, db->d_off, d_tiles.p, (int32_t)tiles.size(), chunk, (uint32_t *)layer);
    HIPCHK(hipGetLastError());
    if (int rc = dh_mask_recompose(db)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return DH_OK;
}

// DBdust (symmetric DUST, -w64 -t2.0 -m10; the reference runs it on every DB it aligns with -mdust,
// processPileUps/package.d:476, 655): the low-complexity mask is computed on the device and ORed
// into the DB's soft mask
extern "C" int dh_db_dust(dh_db *db)
{
    if (!db) return fail(DH_EINVAL, "db is NULL");
    HIPCHK(hipSetDevice(db->ctx->device));
    return dh_db_dust_impl(db);
}

// maskRepetitiveRegions (commands/maskRepetitiveRegions.d:129-176, 238-430): sequence regions whose
// alignment coverage lies outside [lower, upper] are ORed into the DB's soft mask; improper_only
// restricts the coverage to alignments that are not proper within `allowance` (the second assessor of
// the reads case, :157-176).  No alignments, no mask (:347-348).  The coverage is computed on the device:
// +1 / -1 events, one scan, one classification pass.
extern "C" int dh_db_mask_coverage(dh_db *db, const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads,
                                   int32_t lower, int32_t upper, int32_t improper_only, int32_t allowance)
{
    if (!db || (n > 0 && !las) || n < 0 || (improper_only && !read_off))
        return fail(DH_EINVAL, "dh_db_mask_coverage: bad argument");
    for (int64_t i = 0; i < n; i++) {
        const dh_la &l = las[i];
        if (l.aread < 0 || l.aread >= db->n || (improper_only && (l.bread < 0 || l.bread >= nreads)))
            return fail(DH_EINVAL, "dh_db_mask_coverage: id out of range");
        const int64_t alen = db->h_off[(size_t)l.aread + 1] - db->h_off[(size_t)l.aread];
        if (l.abpos < 0 || l.aepos > alen || l.abpos > l.aepos)
            return fail(DH_EINVAL, "dh_db_mask_coverage: alignment outside its contig");
    }
    if (n == 0) return DH_OK;
    dh_ctx *ctx = db->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (db->has_ix) db->ix.release();
    db->has_ix = false;
    uint8_t *layer;
    if (int rc = dh_ensure_mask_layer(db, 1, &layer)) return rc;
    const int64_t nslots = db->total + db->n + 2;
    DevBuf<uint32_t> d_cov, d_sums;
    DevBuf<dh_la> d_las;
    DevBuf<int64_t> d_roff;
    HIPCHK(d_cov.alloc((size_t)nslots));
    HIPCHK(d_sums.alloc((size_t)nslots / 2048 + 4));
    HIPCHK(d_las.alloc((size_t)n));
    HIPCHK(dhk_memset(st, d_cov.p, 0, sizeof(uint32_t) * (size_t)nslots));
    HIPCHK(hipMemcpyAsync(d_las.p, las, sizeof(dh_la) * (size_t)n, hipMemcpyHostToDevice, st));
    if (improper_only) {
        HIPCHK(d_roff.alloc((size_t)nreads + 1));
        HIPCHK(hipMemcpyAsync(d_roff.p, read_off, sizeof(int64_t) * ((size_t)nreads + 1), hipMemcpyHostToDevice, st));
    }
    dhk_cov_events(st, (const DhLa *)d_las.p, n, db->d_off, d_roff.p, improper_only ? 1 : 0, allowance, d_cov.p);
    HIPCHK(hipGetLastError());
    dhk_scan(st, d_cov.p, nslots, d_sums.p);
    HIPCHK(hipGetLastError());
    dhk_cov_mask(st, d_cov.p, db->d_off, db->n, db->max_len, lower, upper, (uint32_t *)layer);
    HIPCHK(hipGetLastError());
    if (int rc = dh_mask_recompose(db)) return rc;
    HIPCHK(hipStreamSynchronize(st));
    return DH_OK;
}

// --max-coverage-reads / --max-improper-coverage-reads from --read-coverage (commandline.d:1876-1889,
// 1957-1970)
extern "C" int32_t dh_max_coverage_reads(double x)
{
    return (int32_t)(x / std::log(std::log(std::log(0.1650612 * x + 5.9354533) / std::log(1.65))));
}
extern "C" int32_t dh_max_improper_coverage_reads(double x) { return (int32_t)(0.5 * x + std::exp(0.1875 * (8.0 - x))); }

// the mask as intervals (what `DBdust` writes into the `dust` track, dazzler.d:4943-5170): ptr gets
// n + 1 entries; iv may be NULL to size; returns the number of intervals or a negative error
extern "C" int64_t dh_db_get_mask(dh_db *db, int64_t *ptr, int32_t *iv, int64_t iv_cap)
{
    if (!db || !ptr) return fail(DH_EINVAL, "dh_db_get_mask: NULL argument");
    std::vector<uint8_t> bits(mask_bytes(db), 0);
    if (db->d_mask_bits) {
        if (hipSetDevice(db->ctx->device) != hipSuccess || hipStreamSynchronize(db->ctx->stream) != hipSuccess ||
            hipMemcpy(bits.data(), db->d_mask_bits, bits.size(), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(DH_EHIP, "dh_db_get_mask: device to host copy failed");
    }
    int64_t m = 0;
    for (int32_t s = 0; s < db->n; s++) {
        ptr[s] = m;
        const int64_t o = db->h_off[(size_t)s], e = db->h_off[(size_t)s + 1];
        int64_t g = o;
        while (g < e) {
            if (!(bits[(size_t)(g >> 3)] >> (g & 7) & 1)) {
                g++;
                continue;
            }
            int64_t h = g;
            while (h < e && (bits[(size_t)(h >> 3)] >> (h & 7) & 1)) h++;
            if (iv && m < iv_cap) {
                iv[2 * m] = (int32_t)(g - o);
                iv[2 * m + 1] = (int32_t)(h - o);
            }
            m++;
            g = h;
        }
    }
    ptr[db->n] = m;
    return m;
}

extern "C" int32_t dh_db_nreads(const dh_db *db) { return db ? db->n : 0; }
extern "C" int64_t dh_db_total_bases(const dh_db *db) { return db ? db->total : 0; }

// drop cached derived data (k-mer index, reverse complement) so the next call rebuilds it
extern "C" int dh_db_drop_cache(dh_db *db)
{
    if (!db) return fail(DH_EINVAL, "db is NULL");
    (void)hipSetDevice(db->ctx->device);
    (void)hipStreamSynchronize(db->ctx->stream);
    if (db->has_ix) db->ix.release();
    db->has_ix = false;
    dh_dev_free(db->d_rc_alloc);
    db->d_rc = db->d_rc_alloc = nullptr;
    dh_dev_free(db->d_pk_alloc);
    dh_dev_free(db->d_rcpk_alloc);
    db->d_pk = db->d_pk_alloc = db->d_rcpk = db->d_rcpk_alloc = nullptr;
    db->has_n = -1;
    return DH_OK;
}

int dh_ensure_rc(dh_db *db)
{
    if (db->d_rc) return DH_OK;
    if (int rc = dh_alloc_bases(db->ctx->stream, db->total, &db->d_rc_alloc, &db->d_rc)) return rc;
    dhk_revcomp(db->ctx->stream, db->d_bases, db->d_rc, db->d_off, db->n, db->max_len);
    HIPCHK(hipGetLastError());
    return DH_OK;
}

// 2-bit packed copies for the wave kernel; leaves has_n = 1 (and no packed copy) when the DB
// holds codes outside 0..3
int dh_ensure_packed(dh_db *db, bool with_rc)
{
    if (db->has_n == 1) return DH_OK;
    hipStream_t st = db->ctx->stream;
    const size_t bytes = (size_t)((db->total + 31) / 32) * 8 + 2 * PK_PAD;
    if (!db->d_pk) {
        int32_t *d_flag;
        if (int rc = dh_scratch(db->ctx, SLOT_STATUS, DH_STW_COUNT * sizeof(int32_t), (void **)&d_flag)) return rc;
        HIPCHK(dh_dev_alloc((void **)&db->d_pk_alloc, bytes));
        db->d_pk = db->d_pk_alloc + PK_PAD;
        HIPCHK(hipMemsetAsync(d_flag + DH_STW_PACK, 0, sizeof(int32_t), st));
        dhk_pack2(st, db->d_bases, db->total, db->d_pk, d_flag + DH_STW_PACK);
        HIPCHK(hipGetLastError());
        int32_t flag = 0;
        HIPCHK(hipMemcpyAsync(&flag, d_flag + DH_STW_PACK, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        db->has_n = flag ? 1 : 0;
        if (flag) {
            dh_dev_free(db->d_pk_alloc);
            db->d_pk = db->d_pk_alloc = nullptr;
            return DH_OK;
        }
    }
    if (with_rc && !db->d_rcpk) {
        if (int rc = dh_ensure_rc(db)) return rc;
        int32_t *d_flag;
        if (int rc = dh_scratch(db->ctx, SLOT_STATUS, DH_STW_COUNT * sizeof(int32_t), (void **)&d_flag)) return rc;
        HIPCHK(dh_dev_alloc((void **)&db->d_rcpk_alloc, bytes));
        db->d_rcpk = db->d_rcpk_alloc + PK_PAD;
        dhk_pack2(st, db->d_rc, db->total, db->d_rcpk, d_flag + DH_STW_PACK_RC);
        HIPCHK(hipGetLastError());
    }
    return DH_OK;
}

int32_t dh_ceil_log2(uint64_t x)
{
    int32_t b = 0;
    while ((1ull << b) < x) b++;
    return b;
}

// light: only the virtual axis (goff, page table) -- what the seed filter's back end needs when the hits come from the
// per-pile-up k-mer join (dh_join.hip) instead of directory lookups
int dh_build_index(dh_db *A, int32_t k, int32_t sepv, int32_t kmer_mod, bool light)
{
    dh_ctx *ctx = A->ctx;
    if (A->has_ix && A->ix.k == k && A->ix.sepv == sepv && A->ix.kmer_mod == kmer_mod && (light || !A->ix.light)) return DH_OK;
    if (A->has_ix) A->ix.release();
    A->has_ix = false;
    dh_index &ix = A->ix;
    ix = dh_index();
    ix.k = k;
    ix.sepv = sepv;
    ix.kmer_mod = kmer_mod;
    ix.na = A->n;
    ix.light = light;
    // virtual offsets and tile table
    std::vector<int64_t> goff((size_t)A->n + 1);
    std::vector<int2> tiles;
    int64_t g = 0, nk = 0;
    for (int32_t s = 0; s < A->n; s++) {
        goff[(size_t)s] = g;
        const int64_t len = A->h_off[(size_t)s + 1] - A->h_off[(size_t)s];
        g += (len + sepv + 4095) & ~4095ll;  // 4096-aligned starts: see sepv in align_range
        if (len >= k && !light) {
            nk += len - k + 1;
            for (int64_t st = 0; st < len - k + 1; st += KM_TILE) tiles.push_back(int2{s, (int32_t)st});
        }
    }
    goff[(size_t)A->n] = g;
    if (g >= (1ll << 39))
        return fail(DH_EINVAL, "index: virtual coordinate space exceeds 2^39 (every sequence takes its length + the longest "
                               "B read + 64, rounded up to 4096)");
    if (A->n >= (1 << 24)) return fail(DH_EINVAL, "index: more than 2^24 sequences");
    if (light) {
        HIPCHK(dh_dev_alloc(&ix.d_goff, sizeof(int64_t) * (size_t)(A->n + 1)));
        HIPCHK(hipMemcpyAsync(ix.d_goff, goff.data(), sizeof(int64_t) * goff.size(), hipMemcpyHostToDevice, ctx->stream));
        std::vector<int32_t> page_seq((size_t)(g >> 12) + 1, A->n > 0 ? A->n - 1 : 0);
        for (int32_t s2 = 0; s2 < A->n; s2++)
            for (int64_t pg = goff[(size_t)s2] >> 12; pg < (goff[(size_t)s2 + 1] >> 12); pg++) page_seq[(size_t)pg] = s2;
        HIPCHK(dh_dev_alloc(&ix.d_page_seq, sizeof(int32_t) * page_seq.size()));
        HIPCHK(hipMemcpyAsync(ix.d_page_seq, page_seq.data(), sizeof(int32_t) * page_seq.size(), hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));  // the vectors go out of scope
        A->has_ix = true;
        return DH_OK;
    }
    const int32_t keybits = 2 * k + dh_ceil_log2((uint64_t)A->ngroups);
    if (keybits > 62) return fail(DH_EINVAL, "index: k-mer key does not fit 62 bits");
    int32_t pbits = dh_ceil_log2((uint64_t)std::max<int64_t>(nk, 1));
    int32_t pmax = 27;
    // more indexed k-mers than 2^27 buckets can keep apart (a 3 Gb assembly at kmer_mod 4: 750 M): about one bucket per
    // entry, up to 2^30 -- at 5.6 entries per bucket every lookup walked a chain of dependent loads (configs[4]: seeds
    // 631 -> 223 ms per 25 Gbp of reads, index build 81 -> 128 ms; 17 GB of directory, the part has 288)
    const int64_t expect = nk / std::max(1, kmer_mod);
    if (expect > (1ll << 27)) pmax = std::min(30, dh_ceil_log2((uint64_t)expect) + 1);
    if (const char *e = getenv("DH_INDEX_PBITS")) pmax = std::max(10, std::min(30, atoi(e)));  // development
    pbits = std::max(10, std::min(pbits, std::min(keybits, pmax)));
    ix.pbits = pbits;
    ix.shift = keybits - pbits;
    // the largest key is ngroups * 4^k - 1, so buckets up to (that >> shift) are addressable
    const int64_t nb = (int64_t)((((uint64_t)A->ngroups << (2 * k)) - 1) >> ix.shift) + 1;
    // bucket offsets are 32 bits wide: the k-mers actually indexed (about nk / kmer_mod of the positions: the
    // modimer hash samples evenly) have to stay below 2^32, with 1/16 of headroom for the sampling's spread
    if (nk / std::max(1, kmer_mod) >= (1ll << 32) - (1ll << 28))
        return fail(DH_EINVAL, "index: more than 2^32 indexed k-mers (32-bit bucket offsets); raise kmer_mod");
    HIPCHK(dh_dev_alloc(&ix.d_dir_alloc, sizeof(uint32_t) * (size_t)(nb + 2)));
    ix.d_dir = ix.d_dir_alloc + 1;
    HIPCHK(dh_dev_alloc(&ix.d_goff, sizeof(int64_t) * (size_t)(A->n + 1)));
    int2 *d_tiles = nullptr;
    uint32_t *d_sums = nullptr;
    const int64_t nsum = (nb + 1 + 2047) / 2048 + 1;
    HIPCHK(dh_dev_alloc(&d_tiles, sizeof(int2) * std::max<size_t>(tiles.size(), 1)));
    HIPCHK(dh_dev_alloc(&d_sums, sizeof(uint32_t) * (size_t)nsum));
    HIPCHK(hipMemcpyAsync(ix.d_goff, goff.data(), sizeof(int64_t) * goff.size(), hipMemcpyHostToDevice,
                          ctx->stream));
    // sequence of every page of the virtual axis: one load instead of a binary search over goff per candidate
    std::vector<int32_t> page_seq((size_t)(g >> 12) + 1, A->n > 0 ? A->n - 1 : 0);
    for (int32_t s2 = 0; s2 < A->n; s2++)
        for (int64_t pg = goff[(size_t)s2] >> 12; pg < (goff[(size_t)s2 + 1] >> 12); pg++) page_seq[(size_t)pg] = s2;
    HIPCHK(dh_dev_alloc(&ix.d_page_seq, sizeof(int32_t) * page_seq.size()));
    HIPCHK(hipMemcpyAsync(ix.d_page_seq, page_seq.data(), sizeof(int32_t) * page_seq.size(), hipMemcpyHostToDevice, ctx->stream));
    if (!tiles.empty())
        HIPCHK(hipMemcpyAsync(d_tiles, tiles.data(), sizeof(int2) * tiles.size(), hipMemcpyHostToDevice,
                              ctx->stream));
    HIPCHK(dhk_memset(ctx->stream, ix.d_dir_alloc, 0, sizeof(uint32_t) * (size_t)(nb + 2)));
    const DbView av = A->view();
    // grouped DB (pile-ups): a group's keys share their top bits, i.e. its buckets are one contiguous range; when the
    // sequences come group by group and a group is cut into few slices, the passes count in LDS (k_group_index)
    // instead of 2 x nk device-scope atomics on random counters (configs[2]: see LABNOTES 8)
    int32_t *d_gtile = nullptr;
    int32_t gi_slices = 0, gi_slice = 0;
    struct GtGuard {
        int32_t *&p;
        ~GtGuard() { dh_dev_free(p); }
    } gtg{d_gtile};
    // (a small grouped DB -- the templates of a consensus round: 500 sequences -- takes the generic passes: a block per
    // group and slice that zeroes and writes back 128 KB of LDS counters cost 8.6 ms per step at configs[2] for 1.3 M
    // k-mers; DH_INDEX_LDS_MIN overrides the threshold, tests run both paths)
    int64_t gi_min = 1 << 24;
    if (const char *e = getenv("DH_INDEX_LDS_MIN")) gi_min = atoll(e);
    if (A->d_group && A->ngroups > 1 && ix.shift <= 2 * k && nk >= gi_min && !getenv("DH_INDEX_ATOMICS")) {
        const int64_t nbg = 1ll << (2 * k - ix.shift);
        gi_slice = (int32_t)std::min<int64_t>(nbg, DH_GI_SLICE);
        gi_slices = (int32_t)(nbg / gi_slice);
        bool ordered = true;
        for (int32_t s2 = 1; s2 < A->n && ordered; s2++) ordered = A->h_group[(size_t)s2] >= A->h_group[(size_t)s2 - 1];
        if (!ordered || gi_slices > 16 || (int64_t)A->ngroups * gi_slices > (1ll << 30)) gi_slices = 0;
    }
    std::vector<int32_t> gtile;  // tiles of group g: [gtile[g], gtile[g + 1]); alive until the stream is synchronised below
    if (gi_slices > 0) {
        gtile.assign((size_t)A->ngroups + 1, 0);
        for (const int2 &t : tiles) gtile[(size_t)A->h_group[(size_t)t.x] + 1]++;
        for (int32_t g2 = 0; g2 < A->ngroups; g2++) gtile[(size_t)g2 + 1] += gtile[(size_t)g2];
        HIPCHK(dh_dev_alloc(&d_gtile, sizeof(int32_t) * gtile.size()));
        HIPCHK(hipMemcpyAsync(d_gtile, gtile.data(), sizeof(int32_t) * gtile.size(), hipMemcpyHostToDevice, ctx->stream));
        dhk_group_index(ctx->stream, 0, av, d_tiles, d_gtile, A->ngroups, gi_slices, gi_slice, k, kmer_mod, ix.shift,
                        ix.d_dir, ix.d_ent, ix.d_goff);
    } else
        dhk_kmer_pass(ctx->stream, 0, av, d_tiles, (int32_t)tiles.size(), k, kmer_mod, ix.shift, ix.d_dir, ix.d_ent,
                      ix.d_goff);
    // (the k-mers actually indexed are known only now -- modimer sampling is not even on repetitive sequence --: the scan
    // also sums them in 64 bits, a total that does not fit the 32-bit bucket offsets is an error, never a wrapped directory)
    unsigned long long *d_total = nullptr;
    struct TotGuard {
        unsigned long long *&p;
        ~TotGuard() { dh_dev_free(p); }
    } totg{d_total};
    HIPCHK(dh_dev_alloc(&d_total, sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(d_total, 0, sizeof(unsigned long long), ctx->stream));
    dhk_scan_total(ctx->stream, ix.d_dir, nb + 1, d_sums, d_total);
    // the entry array is sized by the k-mers that were actually indexed (sampled, unmasked): the
    // exclusive scan leaves their number in dir[nb]
    uint32_t nent = 0;
    unsigned long long total = 0;
    HIPCHK(hipMemcpyAsync(&nent, ix.d_dir + nb, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&total, d_total, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (total != (unsigned long long)nent || total >= (1ull << 32) - 16)
        return fail(DH_EOVERFLOW, "index: more than 2^32 indexed k-mers (32-bit bucket offsets); raise kmer_mod");
    ix.n = (int64_t)nent;
    HIPCHK(dh_dev_alloc(&ix.d_ent, sizeof(ulonglong2) * (size_t)std::max<int64_t>(ix.n, 1)));
    if (gi_slices > 0)
        dhk_group_index(ctx->stream, 1, av, d_tiles, d_gtile, A->ngroups, gi_slices, gi_slice, k, kmer_mod, ix.shift,
                        ix.d_dir, ix.d_ent, ix.d_goff);
    else
        dhk_kmer_pass(ctx->stream, 1, av, d_tiles, (int32_t)tiles.size(), k, kmer_mod, ix.shift, ix.d_dir, ix.d_ent,
                      ix.d_goff);
    HIPCHK(hipGetLastError());
    // the directory the seed kernel reads: 16 bytes per bucket that hold the bucket's only entry itself, so that a
    // looked-up k-mer costs one random line unless its bucket holds several entries
    HIPCHK(dh_dev_alloc(&ix.d_fat, sizeof(ulonglong2) * (size_t)nb));
    dhk_fat_dir(ctx->stream, ix.d_dir, ix.d_ent, nb, ix.d_fat);
    HIPCHK(hipGetLastError());
    // the per-group table join reads a group's entries as one range of the entry array: the group is the top key bits
    // and the index lies in bucket order, so the range ends where the group's last bucket does (groups own whole buckets
    // when the bucket shift leaves the group bits alone)
    std::vector<uint32_t> gent;
    if (A->d_group && ix.shift <= 2 * k) {
        gent.resize((size_t)A->ngroups + 1);
        HIPCHK(dh_dev_alloc(&ix.d_gent, sizeof(uint32_t) * gent.size()));
        dhk_tj_group_offsets(ctx->stream, ix.d_dir, A->ngroups, k, ix.shift, nb, ix.d_gent);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(gent.data(), ix.d_gent, sizeof(uint32_t) * gent.size(), hipMemcpyDeviceToHost, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));  // tiles vector goes out of scope
    for (size_t g2 = 0; g2 + 1 < gent.size(); g2++) ix.max_gent = std::max<int64_t>(ix.max_gent, (int64_t)gent[g2 + 1] - (int64_t)gent[g2]);
    dh_dev_free(d_tiles);
    dh_dev_free(d_sums);
    dh_dev_free(ix.d_dir_alloc);
    ix.d_dir_alloc = ix.d_dir = nullptr;
    A->has_ix = true;
    return DH_OK;
}

// ------------------------------------------------------------------------------------ DBs the library makes for itself

extern "C" void dhk_gather_slices(hipStream_t st, const uint8_t *src, const int64_t *src_off, const int32_t *sidx,
                                  const int32_t *sbeg, const int64_t *dst_off, int32_t n, int32_t max_len,
                                  uint8_t *dst);

int dh_db_adopt(dh_ctx *ctx, uint8_t *d_alloc, uint8_t *d_bases, const std::vector<int64_t> &off,
                const std::vector<int32_t> &group, dh_db **out)
{
    dh_db *db = new dh_db();
    db->ctx = ctx;
    db->n = (int32_t)off.size() - 1;
    db->h_off = off;
    db->total = off.back();
    db->d_bases = d_bases;
    db->d_bases_alloc = d_alloc;
    for (int32_t i = 0; i < db->n; i++)
        db->max_len = std::max<int32_t>(db->max_len, (int32_t)(off[(size_t)i + 1] - off[(size_t)i]));
    HIPCHK(dh_dev_alloc(&db->d_off, sizeof(int64_t) * off.size()));
    HIPCHK(hipMemcpyAsync(db->d_off, off.data(), sizeof(int64_t) * off.size(), hipMemcpyHostToDevice,
                          ctx->stream));
    if (!group.empty()) {
        db->h_group = group;
        for (int32_t g : group) db->ngroups = std::max(db->ngroups, g + 1);
        HIPCHK(dh_dev_alloc(&db->d_group, sizeof(int32_t) * group.size()));
        HIPCHK(hipMemcpyAsync(db->d_group, group.data(), sizeof(int32_t) * group.size(),
                              hipMemcpyHostToDevice, ctx->stream));
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *out = db;
    return DH_OK;
}

int dh_db_from_slices(dh_ctx *ctx, const dh_db *src, const std::vector<int32_t> &sidx,
                      const std::vector<int32_t> &sbeg, const std::vector<int32_t> &slen,
                      const std::vector<int32_t> &group, dh_db **out, bool inherit_mask)
{
    const int32_t n = (int32_t)sidx.size();
    std::vector<int64_t> off((size_t)n + 1, 0);
    int32_t max_len = 0;
    for (int32_t i = 0; i < n; i++) {
        off[(size_t)i + 1] = off[(size_t)i] + slen[(size_t)i];
        max_len = std::max(max_len, slen[(size_t)i]);
    }
    uint8_t *d_alloc = nullptr, *d_bases = nullptr;
    if (int rc = dh_alloc_bases(ctx->stream, off.back(), &d_alloc, &d_bases)) return rc;
    if (int rc = dh_db_adopt(ctx, d_alloc, d_bases, off, group, out)) {
        dh_dev_free(d_alloc);
        return rc;
    }
    if (n > 0) {
        DevBuf<int32_t> d_sidx, d_sbeg;
        HIPCHK(d_sidx.alloc((size_t)n));
        HIPCHK(d_sbeg.alloc((size_t)n));
        HIPCHK(hipMemcpyAsync(d_sidx.p, sidx.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(d_sbeg.p, sbeg.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice,
                              ctx->stream));
        dhk_gather_slices(ctx->stream, src->d_bases, src->d_off, d_sidx.p, d_sbeg.p, (*out)->d_off, n,
                          max_len, d_bases);
        if (inherit_mask && src->d_mask_bits) {  // slices keep the soft mask of their source (the flank DB's -mrep)
            uint8_t *layer;
            if (int rc = dh_ensure_mask_layer(*out, 0, &layer)) return rc;
            dhk_mask_slices(ctx->stream, (const uint32_t *)src->d_mask_bits, src->d_off, d_sidx.p, d_sbeg.p, (*out)->d_off, n,
                            max_len, (uint32_t *)layer);
            if (int rc = dh_mask_recompose(*out)) return rc;
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return DH_OK;
}
