// dh_internal.h -- declarations shared by the host translation units of libdentist_hip.so.
#ifndef DH_INTERNAL_H
#define DH_INTERNAL_H

#include "../../include/dentist_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <new>
#include <utility>
#include <vector>

#include "dh_device.h"

#define DB_PAD 64
#define PK_PAD 128 /* bytes of padding on both sides of a packed copy (k_tile reads 64 bytes past a window origin) */

// Caching device allocator: hipMalloc / hipFree synchronise the device and cost 0.1-1 ms each;
// the same buffer sizes recur on every call, so freed blocks are kept in size-class free lists and
// handed out again (all work runs on one stream, so stream order protects reuse).  The cache is
// released when the last context is destroyed.
hipError_t dh_dev_alloc(void **p, size_t bytes);
void dh_dev_free(void *p);
void dh_dev_trim();
template <typename T>
inline hipError_t dh_dev_alloc(T **p, size_t bytes)
{
    return dh_dev_alloc((void **)p, bytes);
}

// memset that fills the chip for large buffers (dh_kernels.hip: k_fill16); small ones go to the runtime
extern "C" hipError_t dhk_memset(hipStream_t st, void *ptr, int value, size_t nbytes);

int dh_fail(int code, const std::string &msg);
#include <memory>
#include <utility>
#include <vector>
// a vector whose resize() leaves trivially constructible elements unwritten: the gathered records of a plan are written
// once by the host threads (a value-initialising resize was 2.2 of the plan's 6.3 ms: 14 MB of first-touch page faults on
// one thread)
template <class T>
struct dh_noinit_alloc : std::allocator<T> {
    template <class U>
    struct rebind {
        using other = dh_noinit_alloc<U>;
    };
    template <class U, class... A>
    void construct(U *p, A &&...a)
    {
        if constexpr (sizeof...(A) == 0)
            ::new ((void *)p) U;
        else
            ::new ((void *)p) U(std::forward<A>(a)...);
    }
};
typedef std::vector<dh_la, dh_noinit_alloc<dh_la>> dh_la_vec;  // (the plan of the sharded collector: dh_shard.cpp, dh_scaffold.h)
// allocate total + 2 * DB_PAD bytes filled with code 4; *base = alloc + DB_PAD
int dh_alloc_bases(hipStream_t st, int64_t total, uint8_t **alloc, uint8_t **base, bool pads_only = false);

#define HIPCHK(expr)                                                                             \
    do {                                                                                         \
        hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess)                                                                    \
            return dh_fail(DH_EHIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

// The slots of a context's scratch arena (dh_ctx::arena, dh_scratch): one enumerator per device buffer, named after what
// it holds, grouped by the entry point that owns it.  A slot is one grow-only buffer.  A few slots are requested at
// several sites by design (marked "several requests" below): every request is the same buffer and the largest request
// wins -- a request that grows the buffer synchronises the stream and drops what it held, so such sites never need each
// other's contents.  Groups do not share buffers, so an entry point never overwrites what another one left on the context.
enum DhSlot : int {
    // words shared by an alignment call and the 2-bit packers (several requests, all of DH_STW_COUNT words): DH_STW_* below
    SLOT_STATUS,
    // dh_align_db* / dh_map_reads (alloc_scratch, dh_align_prepare.cpp, and the chunk stages): live for one call, rewritten by
    // every chunk; the compacted records and trace values of the last chunk stay valid until the next alignment call
    // (dh_la_set.d_trace / d_la / d_item_off point into SLOT_TROUT, SLOT_LAOUT, SLOT_NLA).  Several requests: SLOT_LA and
    // SLOT_TRSLOTS (alloc_scratch, or extend_chunk once a symmetric launch has counted its candidates), SLOT_FSCR (one per
    // seed tier, sized by the tier: fscr_scratch, dh_align_seed.cpp), SLOT_UNITS (one per kind of unit)
    SLOT_CAND, SLOT_NCAND, SLOT_NHITS, SLOT_NLA, SLOT_NTR, SLOT_POOL, SLOT_CDJ, SLOT_QUEUE, SLOT_LA, SLOT_TRSLOTS,
    SLOT_COUNTERS, SLOT_SUMS, SLOT_SUMMARY, SLOT_OVF, SLOT_REGS, SLOT_COLD, SLOT_LAOUT, SLOT_TROUT,
    SLOT_FSCR, SLOT_MID_LIST, SLOT_BIG_LIST, SLOT_BIG_HITS,            // seed tiers: slab scratch, the reads of a tier, HBM-staged hits
    SLOT_UNITS, SLOT_CANDOFF, SLOT_RECLIST, SLOT_RECCUR,               // symmetric launches (skip_self 2)
    // the transposed file of dh_align_db_transposed: same life as the group above
    SLOT_LA2, SLOT_TRSLOTS2, SLOT_NLA2, SLOT_NTR2, SLOT_A_PLANES, SLOT_A_RC_PLANES, SLOT_B_PK2, SLOT_B_RC_PK2, SLOT_LAOUT2,
    SLOT_TROUT2,
    // the per-chunk copies of B (chunk_copies, dh_align_prepare.cpp): made at the start of a chunk, read by its extension
    SLOT_CHUNK_RC, SLOT_CHUNK_PK, SLOT_CHUNK_RCPK,
    // the pile-up join (build_join, dh_align_join.cpp): built once per call, read by the seeds of every chunk
    SLOT_JOIN_BLOB, SLOT_JOIN_PSUB, SLOT_JOIN_ENTRIES, SLOT_JOIN_SEGTAB, SLOT_JOIN_CURSOR, SLOT_JOIN_HITS,
    // the mapping join (plan_mj_chunk, dh_align_seed.cpp): planned per chunk, read by that chunk's seeds
    SLOT_MJ_ENT, SLOT_MJ_SEGOFF, SLOT_MJ_TILE_N, SLOT_MJ_TILE_R, SLOT_MJ_SEG, SLOT_MJ_HSEG, SLOT_MJ_HITS, SLOT_MJ_RHITS,
    SLOT_MJ_SEGTAB, SLOT_MJ_CTR,
    // the per-group table join (run_table_join, dh_align_seed.cpp): the units, hit segments and hits of one chunk, read by its seeds
    SLOT_TJ_UNITS, SLOT_TJ_SEGTAB, SLOT_TJ_HITS, SLOT_TJ_CTR,
    // the process rounds (the vote and emit pass of a consensus round, dh_rounds.cpp): live for one round
    SLOT_PR_VOFF, SLOT_PR_VOTES, SLOT_PR_OUT, SLOT_PR_STATUS, SLOT_PR_STAGE, SLOT_PR_SEGS, SLOT_PR_DECISIONS, SLOT_PR_CDIFF,
    // comm (dh_comm.cpp: the staging buffers of a collective): live for one collective; several requests (one per kind)
    SLOT_COMM_SEND, SLOT_COMM_RECV,
    // edit paths (run_chunk, dh_editpath.cpp): live for one chunk of tiles; SLOT_EP_OPS is read by the transposition
    SLOT_EP_TILES, SLOT_EP_DM, SLOT_EP_OW, SLOT_EP_RES, SLOT_EP_GEN_TILES, SLOT_EP_GEN_DM, SLOT_EP_GEN_OW, SLOT_EP_GEN_OFF,
    SLOT_EP_GEN_RES, SLOT_EP_COPY, SLOT_EP_OPS,
    // transpose (transpose_chunk, dh_editpath.cpp): live for one chunk of records, behind the edit paths of that chunk
    SLOT_TR_RECS, SLOT_TR_BOUND, SLOT_TR_PAIRS, SLOT_TR_STATUS,
    // global alignment (run_launch, dh_nw.cpp): live for one launch group of pairs; SLOT_NW_REF / SLOT_NW_QRY hold the
    // sequences of a chunk for all its launches
    SLOT_NW_REF, SLOT_NW_QRY, SLOT_NW_PAIRS, SLOT_NW_DM, SLOT_NW_OW, SLOT_NW_RES, SLOT_NW_COPY, SLOT_NW_OPS,
    // affine-gap global alignment (run_launch, dh_nwa.cpp): the same lifetimes
    SLOT_NWA_REF, SLOT_NWA_QRY, SLOT_NWA_PAIRS, SLOT_NWA_DM, SLOT_NWA_OW, SLOT_NWA_RES, SLOT_NWA_COPY, SLOT_NWA_OPS,
    // exact-match locator (dh_exact_locate, dh_locate.cpp): the packed text, the record starts and the plan of the queries
    // live for one call; SLOT_LOC_CANDS / SLOT_LOC_COUNTER are rewritten by every scanned range, SLOT_LOC_UNITS by every
    // batch of verify units
    SLOT_LOC_TEXT, SLOT_LOC_STARTS, SLOT_LOC_PW, SLOT_LOC_PATS, SLOT_LOC_MEMB, SLOT_LOC_TABLE, SLOT_LOC_BITMAP, SLOT_LOC_SHORTS,
    SLOT_LOC_CANDS, SLOT_LOC_COUNTER, SLOT_LOC_UNITS,
    // chaining (dh_la_chain, dh_chain.cpp): all live for one call.  The nodes, pair offsets and tier lists are the plan;
    // SLOT_CH_WOFF / SLOT_CH_SLAB are the global tier's array offsets and its slab (rewritten by every launch group);
    // SLOT_CH_STATE / SLOT_CH_KEY are per node, SLOT_CH_CNT_* per pair (counts, then their exclusive scans), SLOT_CH_SUMS /
    // SLOT_CH_TOTAL the scans' block sums and 64-bit totals, SLOT_CH_OUT_* the result arrays before they are copied back
    SLOT_CH_NODES, SLOT_CH_PAIR_OFF, SLOT_CH_LIST, SLOT_CH_WOFF, SLOT_CH_SLAB, SLOT_CH_STATE, SLOT_CH_KEY, SLOT_CH_CNT_REC,
    SLOT_CH_CNT_CH, SLOT_CH_SUMS, SLOT_CH_TOTAL, SLOT_CH_OUT_OFF, SLOT_CH_OUT_SCORE, SLOT_CH_OUT_SRC, SLOT_CH_OUT_FLAGS,
    // mask propagation (dh_la_propagate_mask, dh_pmask.cpp): all live for one call.  The compact records, the mask, the bit
    // offsets of the destination sequences and (unless the set holds them on the device) the trace values are the input;
    // SLOT_PM_LO / CNT / OFF / HAS are per record (first interval, count, and the scans that place the raw intervals and
    // compact the records), SLOT_PM_LIST the records with any, SLOT_PM_RAW the raw list, written once; SLOT_PM_BITMAP,
    // SLOT_PM_CS / CE (run starts and ends per group of words, then their scans) and SLOT_PM_IV are rewritten by every
    // destination range; SLOT_PM_PTR collects ptr, SLOT_PM_SUMS / SLOT_PM_TOTAL are the scans' block sums and the counters
    SLOT_PM_RECS, SLOT_PM_MASK_PTR, SLOT_PM_MASK_IV, SLOT_PM_BOFF, SLOT_PM_TRACE, SLOT_PM_LO, SLOT_PM_CNT, SLOT_PM_OFF, SLOT_PM_HAS,
    SLOT_PM_LIST, SLOT_PM_RAW, SLOT_PM_BITMAP, SLOT_PM_CS, SLOT_PM_CE, SLOT_PM_IV, SLOT_PM_PTR, SLOT_PM_SUMS, SLOT_PM_TOTAL,
    // region validation (dh_la_validate_regions, dh_vreg.cpp): all live for one call.  The compact records, the regions in plan
    // order and their per-contig offsets are the input, SLOT_VR_CNT the three counters per region; the others are rewritten by
    // every launch group: the segment starts and claimed slots of its regions (AT, CUR), its jobs, pair list, spanning records
    // (indices, then bread in order), slab, interval counts and intervals
    SLOT_VR_RECS, SLOT_VR_REGS, SLOT_VR_RPTR, SLOT_VR_CNT, SLOT_VR_AT, SLOT_VR_CUR, SLOT_VR_JOBS, SLOT_VR_PAIRS, SLOT_VR_SPAN_IDX,
    SLOT_VR_SPAN_OUT, SLOT_VR_SLAB, SLOT_VR_RCNT, SLOT_VR_IV,
    // collect filters (dh_la_collect_filter, dh_cfilt.cpp): all live for one call.  The compact records, the contig and read lengths
    // and the mask with its prefix sums are the input; SLOT_CF_FLAG / UID / FIRST are per record (starts a chain, its unit, a unit's
    // first record), SLOT_CF_SUMS the block sums of both scans (dhk_scan: one per 2048 values), SLOT_CF_UNITS / WHY per chain; SLOT_CF_CNT (counts, then their scan),
    // SLOT_CF_CUR and SLOT_CF_USED are per read, SLOT_CF_GIDX the units grouped by read; the tier lists, the slab offsets of the
    // global tier and its slab; SLOT_CF_CTR the counters of the call, SLOT_CF_OUT a byte per record, SLOT_CF_CNT6 the six counts and, as a seventh 64-bit word, the
    // number of chains (the total of the flag scan)
    SLOT_CF_RECS, SLOT_CF_ALEN, SLOT_CF_BLEN, SLOT_CF_MASK_PTR, SLOT_CF_MASK_IV, SLOT_CF_MASK_PRE, SLOT_CF_FLAG, SLOT_CF_UID, SLOT_CF_SUMS,
    SLOT_CF_FIRST, SLOT_CF_UNITS, SLOT_CF_WHY, SLOT_CF_CNT, SLOT_CF_CUR, SLOT_CF_GIDX, SLOT_CF_USED, SLOT_CF_OUT, SLOT_CF_CTR, SLOT_CF_CNT6,
    SLOT_CF_LWAVE, SLOT_CF_LLDS, SLOT_CF_LGLOB, SLOT_CF_SLAB_AT, SLOT_CF_SLAB,
    // chain padder (dh_la_chain_paths, dh_chainpad.cpp): all live for one launch group of chains.  The compact records, their trace
    // values and the chains' record ranges are the input; SLOT_CP_NSEG / NTILE / NFILL are per chain (counts, then their scans),
    // SLOT_CP_STATUS per chain, SLOT_CP_SEGS / TILES / FILLS what the plan writes; SLOT_CP_TILE_OP the first op of every tile in
    // SLOT_EP_OPS, SLOT_CP_FILL_SRC / FILL_NOPS / FILL_OPS the fillers' ops; SLOT_CP_LEN per chain (length, then its scan),
    // SLOT_CP_OUT / SCORE the stitched ops and scores, SLOT_CP_SUMS / TOTAL the scans' block sums and totals
    SLOT_CP_RECS, SLOT_CP_TRACE, SLOT_CP_CHAIN_OFF, SLOT_CP_NSEG, SLOT_CP_NTILE, SLOT_CP_NFILL, SLOT_CP_STATUS, SLOT_CP_SEGS,
    SLOT_CP_TILES, SLOT_CP_FILLS, SLOT_CP_TILE_OP, SLOT_CP_FILL_SRC, SLOT_CP_FILL_NOPS, SLOT_CP_FILL_OPS, SLOT_CP_LEN, SLOT_CP_OUT,
    SLOT_CP_SCORE, SLOT_CP_SUMS, SLOT_CP_TOTAL,
    // repeat mask (dh_la_repeat_mask, dh_rmask.cpp).  SLOT_RM_ALEN / BLEN live for one call; the others are rewritten by every
    // launch group: its compact records and the first record of each of its contigs (ROFF); SLOT_RM_FLAG / UID per record
    // (starts a chain, the scanned flags with the number of units behind the last), SLOT_RM_SUMS the block sums of the scans;
    // SLOT_RM_EV two keys per unit, SLOT_RM_SEG the key segment of every contig; SLOT_RM_CTR the counters and the number of
    // units; the tier lists, the slab offsets of the global tier and its slab; per mask the run counts (then their scan) and
    // the intervals
    SLOT_RM_RECS, SLOT_RM_ALEN, SLOT_RM_BLEN, SLOT_RM_ROFF, SLOT_RM_FLAG, SLOT_RM_UID, SLOT_RM_SUMS, SLOT_RM_EV, SLOT_RM_SEG, SLOT_RM_CTR,
    SLOT_RM_LWAVE, SLOT_RM_LLDS, SLOT_RM_LGLOB, SLOT_RM_SLAB_AT, SLOT_RM_SLAB, SLOT_RM_CNT_ALL, SLOT_RM_CNT_IMP, SLOT_RM_CNT_MASK,
    SLOT_RM_IV_ALL, SLOT_RM_IV_IMP, SLOT_RM_IV_MASK,
    // mask algebra (dh_mask_combine, dh_la_tandem_mask, dh_maskops.cpp): every buffer of a launch group, carved from one request
    // (the input, the keys twice, the scanned words, the boundaries, the runs in two stages, the output)
    SLOT_MO_WORK,
    // gap analysis (dh_check_gaps, dh_checkgaps.cpp): all live for one call.  SLOT_CG_IN is the uploaded input (mapped triples, the
    // mappings sorted by input contig, the N-runs, the dust mask), SLOT_CG_SUM the summaries, SLOT_CG_ROFF / QOFF the pair lengths and
    // then their scans, SLOT_CG_SUMS the scans' block sums, SLOT_CG_REF / QRY the gathered sequences in the aligner's padded layout,
    // SLOT_CG_OPS the ops of the aligned pairs with their offsets in front
    SLOT_CG_IN, SLOT_CG_SUM, SLOT_CG_ROFF, SLOT_CG_QOFF, SLOT_CG_SUMS, SLOT_CG_REF, SLOT_CG_QRY, SLOT_CG_OPS,
    DH_SLOT_COUNT
};
// The words of SLOT_STATUS (DH_STW_COUNT x int32), one buffer with three users.  All of them run on the context's stream:
//   DH_STW_STATUS   the DH_ST_* bits of an alignment call.  Written: cleared by alloc_scratch and by build_join (hit buffer
//                   retry, fall-back to the directory), rewritten from the host by seed_chunk (a chunk that runs again),
//                   ORed into by the join, mapping-join, seed, wave and tile kernels.  Read: build_join, seed_chunk,
//                   gather_chunk.
//   DH_STW_PACK     "a code outside 0..3 was met" of a forward packing.  Cleared, written (k_pack2, k_pack2_planes) and read
//                   back by dh_ensure_packed (a DB's own copy) and by chunk_copies (a chunk's copy); both synchronise the
//                   stream before they return, and neither runs while the other does.
//   DH_STW_PACK_RC  the same flag of dh_ensure_packed's packing of the reverse complement: written by k_pack2, read by
//                   nobody (the forward pass has decided); chunk_copies clears it along with DH_STW_PACK.
// The fourth word is unused.  No word has two writers in flight at once: the packers run before alloc_scratch or between
// two chunks' kernels of the same stream, and they never touch DH_STW_STATUS.
enum { DH_STW_STATUS = 0, DH_STW_PACK = 1, DH_STW_PACK_RC = 2, DH_STW_COUNT = 4 };
static_assert(DH_STW_PACK_RC == DH_STW_PACK + 1, "chunk_copies clears the two flag words with one memset");

// The hit buffer of the pile-up join (build_join, dh_align_join.cpp) is sized by pile-up depth.  Every template position has
// about n p intact copies among the n reads of a pile-up (p: a k-mer survives the errors), every unordered pair of copies
// is one hit, a group has n L bases: n p^2 / 2 hits per base, i.e. a constant per base PER READ OF DEPTH.  Measured at 13 %
// error, k = 14: 0.77 hits per base at 60 reads (0.0128 per read of depth), 1.94 at 166 (0.0117) -- the larger one starts a
// context.  The margin covers depth and cropped length varying between the pile-ups of one call.
#define DH_JOIN_HIT_RATE0 0.0128
#define DH_JOIN_HIT_MARGIN 1.5
// ... and the buffer never takes more than this fraction of the device memory free at that moment (three concurrent parts
// of the process stage size theirs side by side); above it the rerun with the exact size stays the way out
#define DH_JOIN_HIT_MEM_FRACTION 0.25

#define DH_TJ_HIT_RATE0 0.14

struct dh_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    int ncu = 0;
    hipEvent_t ev[8] = {};
    // second stream for the device-to-host copies of a chunk's records (they overlap the next chunk's
    // kernels); cev[0..1]: compaction done (main stream), cev[2..3]: copy done (copy stream), by chunk parity
    hipStream_t cstream = nullptr;
    hipEvent_t cev[4] = {};
    dh_align_stats stats = {};
    dh_cum_stats cum = {};
    double mj_hit_frac = 0.2;  // hits per sampled k-mer the hit pool of the partitioned join is sized for (raised when a pool overflowed)
    int seed_wave_tier = 1;  // the wavefront-per-read first tier of the segment-fed seed back end (0: most reads overflowed it)
    // the middle tier of that back end (256 threads, 2048 hits, 64 band pairs per read; 0: a quarter of a chunk's reads
    // overflowed it) and dh_get_seed_tier_counts' two counters: chunks whose first tier it was, reads redone behind it
    int seed_mid_tier = 1;
    int64_t seed_mid_chunks = 0, seed_mid_redone = 0;
    int64_t mj_chunks = 0, mj_fallbacks = 0;  // chunks seeded by the partitioned join / redone by the directory (dh_get_mjoin_counts)
    // the per-group table join (dh_tjoin.h; dh_get_tjoin_counts): calls seeded by it, grouped calls A != B that kept the
    // directory because a limit was not met, hits of the last call, reruns of the hit buffer -- and the hits per base of B
    // the buffer is sized for: 0.87^14 = 0.14 true seeds per base at k = 14 to start with, then what the last call produced
    int64_t tj_calls = 0, tj_fallbacks = 0, tj_last_hits = 0, tj_reruns = 0;
    double tj_hit_rate = DH_TJ_HIT_RATE0;
    // the pile-up join's hit buffer (build_join): hits per base per read of depth it is sized for -- raised to what a join
    // produced, never lowered (a capacity hint: results do not depend on it) -- and dh_get_join_counts' four counters
    double join_hit_rate = DH_JOIN_HIT_RATE0;
    int64_t join_launches = 0, join_reruns = 0, join_last_hits = 0, join_first_cap = 0;
    double out_ms[4] = {0, 0, 0, 0};  // dh_output_db's last call: kernels, copies back, fwrite, the whole call (dh_get_output_stats)
    // dh_dazz_load_reads' last call (dh_get_load_stats): ms of file reads, uploads, kernels, the whole call; packed bytes read,
    // bases written, runs, chunks
    double load_ms[4] = {0, 0, 0, 0};
    int64_t load_bytes[4] = {0, 0, 0, 0};
    int32_t near_best_ppm = -1;  // damapper -n of this context (dh_ctx_set_near_best); -1 = the process default
    // second context of the same device (own streams and scratch), created on first use: the process stage runs the
    // two halves of a batch of pile-ups concurrently, one on each (dh_process_pileups)
    dh_ctx *sub[3] = {nullptr, nullptr, nullptr};  // contexts of the concurrent parts of dh_process_pileups
    // grow-only device scratch buffers reused across calls (hipMalloc/hipFree of GB-sized
    // buffers per call costs milliseconds and synchronises the device)
    struct Arena {
        void *p = nullptr;
        size_t cap = 0;
    } arena[DH_SLOT_COUNT];
};
// slot `id` of the context's scratch arena, at least `bytes` large
int dh_scratch(dh_ctx *ctx, DhSlot id, size_t bytes, void **out);
// per-sequence flags of a symmetric all-vs-all (DbView::pflags); NULL clears them
int dh_db_set_pflags(struct dh_db *db, const uint8_t *flags);

struct dh_index {
    // d_dir (build only, released afterwards) points one word into its allocation: d_dir[-1] == 0, so that
    // bucket b is [d_dir[b - 1], d_dir[b]) for every b; the seed kernel reads d_fat (dh_device.h)
    uint32_t *d_dir = nullptr, *d_dir_alloc = nullptr;
    ulonglong2 *d_fat = nullptr;
    ulonglong2 *d_ent = nullptr;
    int64_t *d_goff = nullptr;
    int32_t *d_page_seq = nullptr;  // virtual page (4096 bases) -> sequence
    int64_t n = 0;
    int32_t k = 0, sepv = 0, shift = 0, pbits = 0, na = 0, kmer_mod = 1;
    // presence bitmap of the entries' keys for the partitioned join of a mapping pass (dh_mjoin.h): bit key >> (2k - nbbits),
    // built on first use
    uint32_t *d_bitmap = nullptr;
    int32_t nbbits = 0;
    bool light = false;  // virtual axis only (no directory): the hits come from the k-mer join (dh_join.hip)
    // grouped A whose groups own whole buckets: first entry of every group (ngroups + 1 values, taken from the directory
    // before it is released) for the per-group table join (dh_tjoin.h); max_gent: entries of the largest group
    uint32_t *d_gent = nullptr;
    int64_t max_gent = 0;
    void release()
    {
        dh_dev_free(d_gent);
        d_gent = nullptr;
        max_gent = 0;
        dh_dev_free(d_dir_alloc);
        d_dir_alloc = nullptr;
        dh_dev_free(d_ent);
        dh_dev_free(d_goff);
        dh_dev_free(d_fat);
        d_fat = nullptr;
        dh_dev_free(d_page_seq);
        d_page_seq = nullptr;
        dh_dev_free(d_bitmap);
        d_bitmap = nullptr;
        nbbits = 0;
        d_dir = nullptr;
        d_ent = nullptr;
        d_goff = nullptr;
    }
};

struct dh_db {
    dh_ctx *ctx = nullptr;
    int32_t n = 0, max_len = 0, ngroups = 1;
    int64_t total = 0;
    // bases/rc point DB_PAD bytes into their allocations: kernels read 8 bases at a time on both
    // sides of a position, the padding (code 4) keeps those loads inside the buffer
    uint8_t *d_bases = nullptr, *d_rc = nullptr, *d_bases_alloc = nullptr, *d_rc_alloc = nullptr;
    // 2-bit packed copies for the wave kernel (built on demand; 16 bytes of padding on both sides);
    // has_n: -1 unknown, 0 only codes 0..3 (packed path usable), 1 other codes present
    uint8_t *d_pk = nullptr, *d_rcpk = nullptr, *d_pk_alloc = nullptr, *d_rcpk_alloc = nullptr;
    int32_t has_n = -1;
    int64_t *d_off = nullptr;
    int32_t *d_group = nullptr;
    std::vector<int64_t> h_off;
    std::vector<int32_t> h_group;
    dh_index ix;
    bool has_ix = false;
    // soft mask: one bit per base of d_bases (bit g of the buffer = base g), 16 bytes of slack at the
    // end for the kernels' unaligned 8-byte reads; nullptr = nothing masked
    uint8_t *d_mask_bits = nullptr;
    // the two layers behind it: the caller's tracks (dh_db_set_mask replaces this layer only; slices
    // inherit into it) and what the library derived (DBdust, alignment coverage).  d_mask_bits is the
    // layer itself while only one exists, their OR in a buffer of its own when both do.
    uint8_t *d_mask_user = nullptr, *d_mask_derived = nullptr;
    uint8_t *d_pflags = nullptr;  // see DbView::pflags (dh_db_set_pflags)
    DbView view() const { return DbView{d_bases, d_off, d_group, n, d_mask_bits, d_pflags}; }
};

// Result buffers live in pooled page-locked host memory: device-to-host copies into them run at
// PCIe speed without the runtime's staging pass, and resize() does not zero-fill.  Without a
// device (CPU-only use of the .las codec) the pool falls back to malloc.
void *dh_pinned_alloc(size_t bytes);
void dh_pinned_free(void *p, size_t bytes);
void dh_pinned_trim();
template <typename T>
struct PinnedAlloc {
    using value_type = T;
    PinnedAlloc() = default;
    template <class U>
    PinnedAlloc(const PinnedAlloc<U> &) {}
    T *allocate(size_t n)
    {
        void *p = dh_pinned_alloc(n * sizeof(T));
        if (!p) throw std::bad_alloc();
        return (T *)p;
    }
    void deallocate(T *p, size_t n) { dh_pinned_free(p, n * sizeof(T)); }
    template <class U>
    void construct(U *p) { ::new ((void *)p) U; }  // default-init: no zero fill on resize()
    template <class U, class... Args>
    void construct(U *p, Args &&...a) { ::new ((void *)p) U(std::forward<Args>(a)...); }
    bool operator==(const PinnedAlloc &) const { return true; }
    bool operator!=(const PinnedAlloc &) const { return false; }
};
using LaVec = std::vector<dh_la, PinnedAlloc<dh_la>>;
using TraceVec = std::vector<uint16_t, PinnedAlloc<uint16_t>>;

struct dh_la_set {
    LaVec la;
    TraceVec trace;
    int32_t tspace = 0;
    // device copy of `trace` left behind by dh_align_db_ex (scratch arena): valid until the next
    // alignment call on the same context, nullptr when the result came in several chunks
    const uint16_t *d_trace = nullptr;
    int64_t d_trace_len = 0;  // > 0: `trace` was left on the device on request (dh_align_db_ex want_sorted & 2), the host vector is empty
    // want_sorted & 4 (with & 2, symmetric DH-2 call in one chunk): the RECORDS stay on the device as well -- d_la_n of them,
    // grouped by A-read item, d_item_off[item] = first record of item (read * 2 + strand), nitems + 1 entries; `la` is empty.
    // Valid until the next alignment call on the context.
    DhLa *d_la = nullptr;
    int64_t d_la_n = 0;
    const uint32_t *d_item_off = nullptr;
    // B reads whose items overflowed a per-item capacity (dropped records / no candidates), see
    // dh_align_stats.overflow_items; the pile-up path skips the pile-ups of such reads
    std::vector<int32_t> ovf_reads;
    // dh_map_reads(want_sorted & 8): the trace values of ALL chunks stay on the device in a buffer this set owns (toff
    // indexes it); `trace` is empty until somebody asks for it (dh_la_set_trace downloads it then).  The cropper of the
    // process stage reads the trace of one record in ten: dh_process_pileups_set gathers those on the device.
    uint16_t *d_trace_own = nullptr;
    int64_t d_trace_own_len = 0, d_trace_own_cap = 0;
    int device = 0;
    ~dh_la_set();
};
// the host copy of a set's trace values, downloaded on first use when they were left on the device
int dh_la_set_ensure_host_trace(dh_la_set *s);
// damapper -n of a context: its own value or the process default
int32_t dh_ctx_near_best_ppm(const dh_ctx *ctx);
// what dh_align_db_transposed and dh_la_transpose do last with their transposed records (aread = read, bread = contig;
// grouped by aread): chain flags by dh_select_best_range with the roles of the sequences exchanged, then LAsort order
void dh_finish_transposed_set(dh_la_set *set, bool want_best, int32_t near_ppm);
bool dh_la_less(const dh_la &p, const dh_la &q);  // LAsort order (base.d:1787-1809)
// damapper's chain flags (START / NEXT / BEST, DISABLED below near_ppm) of records grouped by bread (dh_laset.cpp)
void dh_select_best_range(dh_la *la, size_t nla, int32_t near_ppm);
// LAsort order of a B-major list of records over `na` A reads, in O(n)
void dh_lasort(dh_la_set *res, int32_t na);

// result of the process stage (made by dh_process.cpp, spliced by dh_batch.cpp, read by dh_insertions.cpp; dh_comm.cpp assembles the gathered result of all ranks)
struct dh_insertions {
    std::vector<dh_insertion> rec;
    std::vector<uint8_t> bases;
    // what insertions.db stores besides the sequence (insertiondb.d:987-1031): the two flank overlaps
    // of every closed gap with their trace points (A coordinates on the whole contig) and the read
    // ids of the pile-up
    std::vector<dh_la> flank;        // 2 per closed gap: left, right; toff into flank_tr
    std::vector<uint16_t> flank_tr;
    std::vector<int32_t> flank_of;   // per record: index of its left overlap in `flank`, -1 if none
    std::vector<int32_t> ids_off, ids;  // per record [ids_off[i], ids_off[i+1]): read ids of the pile-up
    // dh_insertions_from_db only: per entry of `flank` the A bases its local alignments cover (coveredBases!"contigA",
    // base.d:640-659) -- `flank` then holds one pseudo record per overlap (first A begin, last A end, diffs summed); empty:
    // every overlap is one local alignment and covers aepos - abpos
    std::vector<int64_t> flank_cov;
};

// dh_output.cpp: the walk of `dentist output` (graph, fixCropping, scaffold starts, linear walks; AGP and BED written on the
// way) hands the FASTA to a sink, piece by piece in file order.  dh_output_assembly's sink writes through LineWriter; the sink
// of dh_output_db (dh_outfmt.cpp) records a plan and formats it on the device.
struct DhOutSink {
    virtual ~DhOutSink() {}
    virtual int begin() = 0;                              // open the FASTA: DH_OK, or a failure reported through dh_fail
    virtual void header(const std::string &line) = 0;     // a record starts: its header line with '>' and '\n'
    virtual void contig(int32_t c, int64_t from, int64_t upto, bool comp) = 0;  // bases [from, upto) of contig c; comp: reverse-complemented
    virtual void nrun(int64_t len) = 0;
    virtual void insertion(int64_t cons_off, int64_t sb, int64_t se, bool comp, bool upper) = 0;  // consensus bases [sb, se) behind cons_off
    virtual void end_record() = 0;
    virtual void abandon() = 0;                           // the walk failed: close what begin() opened
    virtual int finish() = 0;                             // write what is left and close: DH_OK, or a failure reported through dh_fail
};
int dh_output_walk(const char *who, DhOutSink &sink, const char *fasta_name, const char *bed_path, const char *agp_path,
                   const int64_t *contig_off, int32_t ncontigs, const int32_t *scaffold_of, const char *const *headers,
                   const int32_t *gap_len, const dh_insertion *ins, int32_t nins, const int32_t *read_ids,
                   const int32_t *read_ids_off, int32_t nreads, const char *const *read_names, const dh_output_opts *opts,
                   int32_t *dropped);

// Alignment chains as units (base.d:306-421; chain flags dazzler.d:1728-1758, 1991-1998): a record with NEXT (and not
// START) continues the chain of the record before it (same contig, read and strand).  The view holds one pseudo record
// per chain -- the first member's fields with aepos / bepos of the last member and diffs summed, i.e. what
// first.contigX.begin / last.contigX.end / totalDiffs read -- plus the A bases its members cover (coveredBases!"contigA")
// and where the chain's members are.  `trivial`: every chain is one record (the view is not filled).
struct dh_chain_view {
    bool trivial = true;
    std::vector<dh_la> unit;       // one per chain
    std::vector<int64_t> first;    // chain -> index of its first record; first[nchains] = n
    std::vector<int64_t> covered;  // chain -> sum of (aepos - abpos) over its members
};
void dh_chain_view_build(const dh_la *las, int64_t n, dh_chain_view &v);
inline bool dh_continues_chain(const dh_la &prev, const dh_la &cur)
{
    return (cur.flags & DH_FLAG_NEXT) && !(cur.flags & DH_FLAG_START) && cur.aread == prev.aread && cur.bread == prev.bread &&
           (cur.flags & DH_FLAG_COMP) == (prev.flags & DH_FLAG_COMP);
}

// result of dh_la_edit_paths / dh_la_set_edit_paths (dh_editpath.cpp) and of dh_nw_batch (dh_nw.cpp)
struct dh_edit_paths {
    std::vector<int64_t> op_off{0}, tile_off{0};
    std::vector<uint8_t> ops;
    std::vector<int32_t> score;
    std::vector<uint16_t> tile_score;
    int64_t general_tiles = 0;
    int64_t fillers = 0;                 // dh_la_chain_paths: fillers the global-alignment kernel aligned ...
    std::vector<int32_t> entry_fillers;  // ... and how many of them every chain has (empty for the other calls)
};

// dh_nw.cpp: the widening protocol of the global alignment on pairs whose sequences are on the device (dh_nw_batch's chunks, the
// chain padder's fillers)
struct DhNwSeq {
    int64_t roff, qoff;  // first base in the device reference / query bytes
    int32_t rl, ql;
};
struct DhNwPairOut {
    int64_t at = 0;  // first op in the staging vector
    int32_t nops = 0, score = 0, status = 0;  // status: DH_NW_OK / DH_NW_BAND_EXCEEDED
};
int dh_nw_run_pairs(dh_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_qry, const DhNwSeq *seq, const std::vector<int64_t> &todo,
                    int32_t fs, std::vector<DhNwPairOut> &out, std::vector<uint8_t> &stage);
// dh_nwa.cpp: the same for the affine-gap alignment (dh_nw_affine_batch's chunks, dh_check_gaps' gathered pairs); sc NULL: the
// default; *groups (or NULL) counts the launch groups
int dh_nwa_run_pairs(dh_ctx *ctx, const uint8_t *d_ref, const uint8_t *d_qry, const DhNwSeq *seq, const std::vector<int64_t> &todo,
                     const dh_nw_scoring *sc, std::vector<DhNwPairOut> &out, std::vector<uint8_t> &stage, int64_t *groups);
// dh_editpath.cpp: validation of one record as dh_la_edit_paths validates it (its tiles are appended to `tiles`), and the tiles [t0, t1) of `tiles` through the edit-path kernels with their
// ops left on the device, tile after tile (*d_ops; NULL when there is none): res[t] = nops / score per tile
struct EpTile;
struct EpResult;
int dh_ep_check_record(const dh_db *A, const dh_db *B, const dh_la &la, int64_t idx, const uint16_t *trace, int64_t trace_len,
                       int32_t ts, std::vector<EpTile> &tiles);
size_t dh_ep_chunk_tiles();  // DH_EDIT_CHUNK
int dh_ep_run_tiles(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t ts, const std::vector<EpTile> &tiles, size_t t0, size_t t1,
                    std::vector<EpResult> &res, dh_edit_paths *out, const uint8_t **d_ops);

// dh_pileups.cpp: LA indices shifted by a constant; pile-ups of several parts concatenated gap by gap
void dh_pileups_shift(dh_pileups *p, int32_t by);
int dh_pileups_concat(dh_pileups *const *parts, int32_t nparts, dh_pileups **out);

template <typename T>
struct DevBuf {
    T *p = nullptr;
    ~DevBuf() { dh_dev_free(p); }
    hipError_t alloc(size_t n) { return dh_dev_alloc(&p, sizeof(T) * std::max<size_t>(n, 1)); }
};

// dh_db.cpp: build a DB whose bases are slices [beg, beg+len) of sequences of `src` (device-to-device)
int dh_db_from_slices(dh_ctx *ctx, const dh_db *src, const std::vector<int32_t> &sidx,
                      const std::vector<int32_t> &sbeg, const std::vector<int32_t> &slen,
                      const std::vector<int32_t> &group, dh_db **out, bool inherit_mask = false);
// adopt device bases allocated with dh_alloc_bases (ownership moves to the DB)
int dh_db_adopt(dh_ctx *ctx, uint8_t *d_alloc, uint8_t *d_bases, const std::vector<int64_t> &off,
                const std::vector<int32_t> &group, dh_db **out);
int dh_ensure_rc(dh_db *db);
// a layer of the DB's mask bitmap (derived != 0: the library's own bits, else the caller's / inherited
// tracks), allocated and zeroed on first use; write into it, then call dh_mask_recompose
int dh_ensure_mask_layer(dh_db *db, int derived, uint8_t **out);
int dh_mask_recompose(dh_db *db);
void dh_mask_free(dh_db *db);
// DBdust: ORs the low-complexity mask (k_dust) into the DB's mask bitmap; drops the cached index
int dh_db_dust_impl(dh_db *db);
int dh_ensure_packed(dh_db *db, bool with_rc);
// the k-mer index of A (cached with the DB); light: the virtual axis only, for the calls whose hits come from the pile-up join
int dh_build_index(dh_db *A, int32_t k, int32_t sepv, int32_t kmer_mod, bool light = false);
int32_t dh_ceil_log2(uint64_t x);
// dh_align_db with the final LAsort made optional (internal callers regroup on their own): want_sorted bit 0 = LAsort,
// bit 1 = leave the trace values on the device (dh_la_set.d_trace / d_trace_len) when the call is one chunk
int dh_align_db_ex(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, int32_t want_best,
                   int32_t want_sorted, dh_la_set **out);

#endif
