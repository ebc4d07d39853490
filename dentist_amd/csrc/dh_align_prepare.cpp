// dh_align_prepare.cpp -- what an alignment call sets up before its seeds: the chunk size and the copies that live with the
// DBs (prepare_dbs), the scratch of the call (alloc_scratch), and per chunk the derived copies of B (copy_chunk).
#include <cstdio>
#include <cstdlib>

#include "dh_align.h"

#define fail dh_fail

// planes: plane-packed copies for k_tile instead of the 2-bit packed ones (a DH-2 mapping that does not keep the packed
// words for the transposed pairs): the conversion passes over both copies -- 8 of the 24 GB a chunk of configs[2] moves
// for its copies -- fall away
static int chunk_copies(dh_ctx *ctx, dh_db *B, int32_t r0, int32_t r1, bool want_packed, bool need_bytes,
                        ChunkCopies *out, bool planes = false)
{
    hipStream_t st = ctx->stream;
    const int64_t o0 = B->h_off[(size_t)r0], o1 = B->h_off[(size_t)r1];
    const int64_t a0 = o0 & ~31ll;  // packed words hold 32 bases: start the chunk on a word boundary
    uint8_t *d_rc, *d_pk, *d_rcpk;
    int32_t *d_flag;
    out->has_n = false;
    auto rc_bytes = [&]() -> int {
        // reverse complement as bytes (only the wave kernels' byte path reads it): every read mirrored
        // inside its own [off, off + len) range
        if (int rc = dh_scratch(ctx, SLOT_CHUNK_RC, (size_t)(o1 - a0) + 2 * DB_PAD, (void **)&d_rc)) return rc;
        HIPCHK(dhk_memset(st, d_rc, 4, (size_t)(o1 - a0) + 2 * DB_PAD));
        uint8_t *rc_shift = d_rc + DB_PAD - a0;
        dhk_revcomp(st, B->d_bases, rc_shift, B->d_off + r0, r1 - r0, B->max_len);
        HIPCHK(hipGetLastError());
        out->rc = rc_shift;
        return DH_OK;
    };
    if (!want_packed) return rc_bytes();
    // 2-bit packed forward copy and, straight from the forward bytes, the packed reverse complements
    const size_t pbytes = (size_t)((o1 - a0 + 31) / 32) * 8 + 2 * PK_PAD;
    if (int rc = dh_scratch(ctx, SLOT_CHUNK_PK, pbytes, (void **)&d_pk)) return rc;
    if (int rc = dh_scratch(ctx, SLOT_CHUNK_RCPK, pbytes, (void **)&d_rcpk)) return rc;
    if (int rc = dh_scratch(ctx, SLOT_STATUS, DH_STW_COUNT * sizeof(int32_t), (void **)&d_flag)) return rc;
    HIPCHK(hipMemsetAsync(d_flag + DH_STW_PACK, 0, 2 * sizeof(int32_t), st));  // DH_STW_PACK and DH_STW_PACK_RC
    // k_pack2_rc stores the words inside a read whole and ORs into the words reads share: only those (and the padding on
    // both sides) are zeroed -- the memset of the whole buffer was 2 GB per chunk of the mapping
    HIPCHK(hipMemsetAsync(d_rcpk, 0, PK_PAD + 8, st));
    HIPCHK(hipMemsetAsync(d_rcpk + pbytes - PK_PAD - 8, 0, PK_PAD + 8, st));
    if (planes) {
        dhk_pack2_planes(st, B->d_bases + a0, o1 - a0, d_pk + PK_PAD, d_flag + DH_STW_PACK);
        // (the reverse-complement planes from the forward planes: the chunk's bytes are read once, not twice)
        dhk_planes_rc(st, d_pk + PK_PAD, B->d_off + r0, r1 - r0, B->max_len, a0, d_rcpk + PK_PAD);
    } else {
        dhk_pack2_rc_bounds(st, B->d_off + r0, r1 - r0, a0, d_rcpk + PK_PAD);
        dhk_pack2(st, B->d_bases + a0, o1 - a0, d_pk + PK_PAD, d_flag + DH_STW_PACK);
        dhk_pack2_rc(st, B->d_bases, B->d_off + r0, r1 - r0, B->max_len, a0, d_rcpk + PK_PAD);
    }
    out->planes = planes;
    HIPCHK(hipGetLastError());
    int32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, d_flag + DH_STW_PACK, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    out->has_n = flag != 0;
    out->pk = d_pk + PK_PAD - (a0 >> 2);
    out->rcpk = d_rcpk + PK_PAD - (a0 >> 2);
    out->pk_words = (o1 - a0 + 31) / 32;
    out->pk_w0 = d_pk + PK_PAD;
    out->rcpk_w0 = d_rcpk + PK_PAD;
    // codes outside 0..3 (here or in A): the wave kernels slide over the byte arrays
    if (out->has_n || need_bytes) return rc_bytes();
    return DH_OK;
}

IndexView index_view(const dh_db *A)
{
    return IndexView{A->ix.d_fat, A->ix.d_ent, A->ix.d_goff, A->ix.d_page_seq, A->ix.n,
                     A->ix.na,    A->ix.sepv,   A->ix.shift,  A->ix.pbits};
}

// the chunk size and the copies of A and B that live with the DBs
int prepare_dbs(AlignRun &r)
{
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    // B's derived copies (reverse complement, 2-bit packed) live with the DB when the whole DB is
    // one chunk of this call (pile-up and template DBs are re-aligned several times); a block of a
    // larger DB gets them chunk by chunk in the scratch arena, so the resident footprint of a reads
    // DB stays at one byte per base however large it is
    // items per launch.  k_tile runs one alignment per lane: a launch needs several alignments per
    // resident lane (262 144 of them) to keep the wavefronts full until the queue drains -- measured on
    // configs[2]: 2^18 items per launch 70 ms of k_tile per step, 2^20 37 ms (the host filters of a chunk
    // still overlap the next chunk's kernels)
    int32_t chunk = o.algo == 1 ? 1 << 20 : 1 << 18;
    if (const char *e = getenv("DH_ALIGN_CHUNK")) chunk = std::max(2, atoi(e)) & ~1;
    // symmetric mode writes records into the slots of other items: everything is one chunk
    if (o.skip_self == 2) {
        if (r.first != 0 || r.count != B->n) return fail(DH_EINVAL, "symmetric mode needs the whole DB");
        chunk = (int32_t)std::min<int64_t>(std::max<int64_t>(r.nitems_total, 2), INT32_MAX - 1);
    }
    r.chunk = chunk;
    // (DH-2 reads B from plane-packed copies made chunk by chunk in the scratch arena)
    r.db_copies = !r.tiled && (A == B || (r.first == 0 && r.count == B->n && r.nitems_total <= chunk));
    r.want_packed = !getenv("DH_WAVE_BYTES");
    // the wave kernel slides over 2-bit packed copies unless a DB holds codes outside 0..3
    if (int rc = dh_ensure_packed(A, false)) return rc;
    if (r.db_copies) {
        if (int rc = dh_ensure_rc(B)) return rc;
        if (int rc = dh_ensure_packed(B, true)) return rc;
    }
    // up to 30 live diagonals fit a 32-lane half: two alignments per wavefront (k_wave2); its
    // reverse extensions run forward over the reverse complements, so A needs one as well
    r.dual = r.tiled || (o.width <= 30 && !getenv("DH_WAVE_SINGLE"));
    if (r.dual) {
        if (int rc = dh_ensure_rc(A)) return rc;
        if (A->has_n == 0)
            if (int rc = dh_ensure_packed(A, true)) return rc;
    }
    if (r.tiled && (A->has_n != 0 || !A->d_pk || !A->d_rcpk))
        return fail(DH_EINVAL, "algo 1 (DH-2) needs sequences of a, c, g, t only (2-bit copies), A holds other codes");
    return DH_OK;
}

// capacity planning and the scratch buffers of the call
int alloc_scratch(AlignRun &r)
{
    dh_ctx *ctx = r.ctx;
    dh_db *A = r.A, *B = r.B;
    const dh_align_opts &o = r.o;
    hipStream_t st = r.st;
    const int64_t nitems_total = r.nitems_total;
    const int64_t maxext =
        std::min<int64_t>(A->max_len, (int64_t)B->max_len + (2ll * B->max_len + o.xdrop) / (o.pen - 1) + 1);
    r.nbmax = (int32_t)(maxext / o.tspace + 3);
    r.trmax = 2 * (2 * r.nbmax + 2);
    const int32_t nbmax = r.nbmax, trmax = r.trmax;
    // resident alignment slots: one per wavefront of k_wave (<= 64 VGPRs -> 8 waves/SIMD), one per
    // 32-lane half of k_wave2 (two per wavefront, 6 waves/SIMD)
    // alignments per wavefront of k_wave2: 2 (32 lanes each, width <= 30) or 4 (16 lanes, width <= 14)
    r.per_wave = (o.width <= 14 && !getenv("DH_WAVE_G32")) ? 4 : 2;
    int32_t slots_per_cu = 32;
    // k_wave2: 80 VGPRs -> 6 waves/SIMD = 24 wavefronts per CU (two per wavefront); 96 VGPRs -> 5 waves/SIMD = 20 (four)
    if (o.width <= 30) slots_per_cu = r.per_wave == 4 ? 20 * 4 : 24 * 2;
    if (const char *e = getenv("DH_WAVE_SLOTS_PER_CU")) slots_per_cu = std::max(4, atoi(e)) & ~3;
    // trace-node pool of one alignment slot.  k_wave2: every lane of the group owns a stretch (a lane
    // crosses each boundary of either grid at most once per diagonal it serves; twice that is the
    // capacity, an overflow is reported); k_wave: one shared pool.  At the END of a sequence that is a boundary itself (the
    // start of A' always is one for the reverse extension) a diagonal that cannot advance gets a new cell from its lower
    // neighbour on every level and crosses that boundary again: one more node per level, grid and extension for as long as
    // the wave outlives its best point -- about (xdrop + 64) / pen + 2 levels, never more than dmax.  Sequences of a few tile
    // lengths (nbmax 3 or 4) overflowed 4 nbmax + 8 that way, symmetric calls first (two grids).  Like 4 nbmax + 8 this is an
    // EMPIRICAL allowance, sized on node counts of constructed cases (LABNOTES 32: at most a third of it was used), not a
    // proven bound: the best point can still move while a diagonal sits at the end.  A lane that runs out writes nothing
    // past its stretch and the call reports DH_EOVERFLOW.  (64-bit: xdrop and dmax are the caller's; the stretch of a lane
    // is capped at 2^20 nodes.)
    const int64_t end_levels = std::min<int64_t>((std::max<int64_t>(o.xdrop, 0) + 64) / o.pen + 2, std::max<int64_t>(o.dmax, 0));
    const int64_t end_nodes = 2 * (o.skip_self == 2 ? 2 : 1) * end_levels;
    const int64_t lane_nodes = std::min<int64_t>(4ll * nbmax + 8 + end_nodes, 1ll << 20);
    r.poolcap = r.dual ? (int32_t)((64 / r.per_wave) * lane_nodes) : 96 * nbmax;
    r.nslots = r.tiled ? 4 : (int32_t)std::min<int64_t>((int64_t)ctx->ncu * slots_per_cu,
                                                        (std::max<int64_t>(nitems_total, 4) + 3) & ~3ll);
    // DH-2: one alignment per lane; wavefronts resident = CUs x waves per CU, no more than the items need
    if (r.tiled) {
        // symmetric launches spend most of a wavefront's time waiting on the records and scratch of short alignments:
        // all 16 wavefronts the registers allow (configs[2]: pile-up launch -2.5 ms against 12; mapping +1 ms with 16)
        int32_t per_cu = o.skip_self == 2 ? 16 : dhk_tile_waves_per_cu();
        if (const char *e = getenv("DH_TILE_WAVES_PER_CU")) per_cu = std::max(1, atoi(e));
        if (o.skip_self == 2)
            if (const char *e = getenv("DH_TILE_SYM_WAVES_PER_CU")) per_cu = std::max(1, atoi(e));  // development
        // (symmetric mode: the work units are groups of candidates, many per item -- a pile-up read meets every other
        // read of its pile-up -- so the items do not bound the lanes that find work)
        const int64_t lanes_wanted = o.skip_self == 2 ? nitems_total * (int64_t)o.max_cand : nitems_total;
        r.tile_waves = (int32_t)std::min<int64_t>((int64_t)ctx->ncu * per_cu, (std::max<int64_t>(lanes_wanted, 1) + 63) / 64);
    }
    r.cn = (int32_t)std::min<int64_t>(r.chunk, std::max<int64_t>(nitems_total, 2));
    const int32_t cn = r.cn;
    SCR(SLOT_CAND, r.d_cand, (size_t)cn * o.max_cand)
    SCR(SLOT_NCAND, r.d_ncand, cn)
    SCR(SLOT_NHITS, r.d_nhits, cn)
    SCR(SLOT_STATUS, r.d_status, DH_STW_COUNT)
    r.d_status += DH_STW_STATUS;  // the call's own word of the slot; the packers use the others
    SCR(SLOT_NLA, r.d_nla, cn + 1)
    SCR(SLOT_NTR, r.d_ntr, cn + 1)
    SCR(SLOT_POOL, r.d_pool, (size_t)r.nslots * r.poolcap)
    SCR(SLOT_CDJ, r.d_cdj, (size_t)r.nslots * 8 * nbmax)
    SCR(SLOT_QUEUE, r.d_queue, 4)
    // (symmetric DH-2 launches keep their records in candidate-indexed slots, sized once the candidates are counted)
    r.sym_tiled = r.tiled && o.skip_self == 2;
    // want_sorted & 8 (dh_map_reads): the trace values of every chunk stay on the device in a buffer the result owns
    r.keep_dev = (r.want_sorted & 8) && r.hook && r.tiled && !r.res2 && !r.sym_tiled;
    if (!r.sym_tiled) {
        SCR(SLOT_LA, r.d_la, (size_t)cn * o.max_la)
        SCR(SLOT_TRSLOTS, r.d_trslots, (size_t)cn * o.max_la * trmax)
    }
    SCR(SLOT_COUNTERS, r.d_counters, 2)
    SCR(SLOT_SUMS, r.d_sums, (size_t)cn / 2048 + 4)
    SCR(SLOT_SUMMARY, r.d_summary, 4)
    SCR(SLOT_OVF, r.d_ovf, cn)
    if (r.tiled) SCR(SLOT_REGS, r.d_regs, (size_t)r.tile_waves * 64 * dhtile::MAXREG * dhtile::REGF)
    if (r.tiled) SCR(SLOT_COLD, r.d_cold, (size_t)r.tile_waves * 64)
    if (r.res2) {
        SCR(SLOT_LA2, r.d_la2, (size_t)cn * o.max_la)
        SCR(SLOT_TRSLOTS2, r.d_trslots2, (size_t)cn * o.max_la * trmax)
        SCR(SLOT_NLA2, r.d_nla2, cn + 1)
        SCR(SLOT_NTR2, r.d_ntr2, cn + 1)
        const size_t awords = (size_t)((A->total + 31) / 32), abytes = awords * 8 + 2 * PK_PAD;
        SCR(SLOT_A_PLANES, r.d_app, abytes)
        SCR(SLOT_A_RC_PLANES, r.d_arcpp, abytes)
        HIPCHK(hipMemcpyAsync(r.d_app, A->d_pk_alloc, abytes, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(r.d_arcpp, A->d_rcpk_alloc, abytes, hipMemcpyDeviceToDevice, st));
        dhk_pk2planes(st, r.d_app + PK_PAD, (int64_t)awords);
        dhk_pk2planes(st, r.d_arcpp + PK_PAD, (int64_t)awords);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemsetAsync(r.d_status, 0, sizeof(int32_t), st));
    HIPCHK(hipMemsetAsync(r.d_counters, 0, 2 * sizeof(unsigned long long), st));
    return DH_OK;
}

// the chunk's derived copies of B (plane-packed for DH-2), then the previous chunk's deferred copy and hook
int copy_chunk(AlignRun &r, AlignChunk &c)
{
    dh_ctx *ctx = r.ctx;
    dh_db *A = r.A, *B = r.B;
    hipStream_t st = r.st;
    ChunkCopies &cc = c.cc;
    if (r.db_copies) {
        cc.rc = B->d_rc;
        cc.pk = B->d_pk;
        cc.rcpk = B->d_rcpk;
        cc.has_n = B->has_n != 0;
    } else if (int rc = chunk_copies(ctx, B, (int32_t)(c.item0 >> 1), (int32_t)((c.item0 + c.ni) >> 1), r.want_packed, A->has_n != 0,
                                     &cc, r.tiled && r.want_packed && !r.res2 && !getenv("DH_PLANES_BY_PASS")))
        return rc;
    c.packed = r.want_packed && A->has_n == 0 && !cc.has_n && cc.pk && cc.rcpk;
    if (r.tiled) {
        if (!c.packed) return fail(DH_EINVAL, "algo 1 (DH-2) needs sequences of a, c, g, t only (2-bit copies), B holds other codes");
        if (r.res2) {
            // the transposed pairs read this chunk of B as their A'': keep its 2-bit copies
            const size_t pbytes = (size_t)cc.pk_words * 8 + 2 * PK_PAD;
            SCR(SLOT_B_PK2, c.d_bpk2, pbytes)
            SCR(SLOT_B_RC_PK2, c.d_brcpk2, pbytes)
            HIPCHK(hipMemcpyAsync(c.d_bpk2, cc.pk_w0 - PK_PAD, pbytes, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipMemcpyAsync(c.d_brcpk2, cc.rcpk_w0 - PK_PAD, pbytes, hipMemcpyDeviceToDevice, st));
        }
        if (!cc.planes) {
            dhk_pk2planes(st, cc.pk_w0, cc.pk_words);
            dhk_pk2planes(st, cc.rcpk_w0, cc.pk_words);
        }
        HIPCHK(hipGetLastError());
    }
    if (r.deferred) {
        HIPCHK(hipEventRecord(ctx->ev[6], st));
        HIPCHK(hipStreamWaitEvent(ctx->cstream, ctx->ev[6], 0));
        const int rc = r.deferred();
        r.deferred = nullptr;
        if (rc) return rc;
    }
    return DH_OK;
}
