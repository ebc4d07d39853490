/*
 * dentist_hip.h -- C ABI of libdentist_hip.so, the MI355X (gfx950) implementation of DENTIST's
 * alignment + consensus hot path.
 *
 * The reference reaches this path through process spawns, not FFI (source/dentist/dazzler.d:
 * 6121-6231 wrappers, 6519-6594 executeCommand).  Each entry point below states the reference
 * interface it replaces; INTEGRATION.md shows the D `extern(C)` module a maintainer would add.
 * Conventions: plain pointers and sizes, POD structs, no exceptions across the boundary, every
 * function returns 0 on success or a negative DH_E* code (message via dh_last_error()).
 * Sequences are base codes a,c,g,t = 0..3 (DAZZ_DB order), anything else = 4.
 * The library never falls back to the CPU: without a usable HIP device every compute entry
 * point fails with DH_ENODEV.
 */
#ifndef DENTIST_HIP_H
#define DENTIST_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DH_OK 0
#define DH_EINVAL (-1)
#define DH_ENODEV (-2)
#define DH_EHIP (-3)
#define DH_EOVERFLOW (-4) /* a device-side capacity planned from the input (trace pool, hit slab) was exceeded */
#define DH_EIO (-5)
#define DH_ENOMEM (-6)

const char *dh_last_error(void);
/* library / ABI version, bumped on any struct change (4: dh_process_opts is 64 bytes -- max_partners,
 * min_relative_score_ppm; 5: dh_extend_candidates, no struct changed; callers check it before passing structs) */
int32_t dh_abi_version(void);

/* ---- context: one per process == one per GPU (torch.distributed launches one rank per GPU) */
typedef struct dh_ctx dh_ctx;
/* stream: a hipStream_t created by the caller (e.g. torch's current stream) or NULL for the
 * library's own stream. */
int dh_ctx_create(int32_t device, void *stream, dh_ctx **out);
void dh_ctx_destroy(dh_ctx *ctx);
int dh_ctx_sync(dh_ctx *ctx);

/* ---- alignment options: the flag subset DENTIST derives for daligner/damapper
 *      (source/dentist/commandline.d:2886-2902, 2918-2935, 2943-2955; enums dazzler.d:5745-6019) */
typedef struct {
    int32_t k;           /* -k  k-mer length, default 14                                     */
    int32_t hmin;        /* -h  covered bases in a band pair needed to trigger, default 35   */
    int32_t band_shift;  /* -w  log2 band width, default 6                                   */
    int32_t tspace;      /* -s  trace spacing: 100 (damapper), 126 (pile-up daligner)        */
    int32_t min_len;     /* -l  minimum A-length of a reported local alignment               */
    int32_t pen;         /* derived from -e: floor(2 / (1 - e)); e = 0.7 -> 6                */
    int32_t xdrop;       /* wave trimmed to points within xdrop of the best score            */
    int32_t max_err_ppm; /* (1 - e) * 1e6: 2*diffs*1e6 <= max_err_ppm * (alen + blen)        */
    int32_t max_cand;    /* seed candidates kept per (B read, strand)                        */
    int32_t max_la;      /* local alignments reported per (B read, strand)                   */
    int32_t tcap;        /* -t  k-mers occurring more often in A are ignored                 */
    int32_t strands;     /* bit0 forward B, bit1 reverse-complement B                        */
    int32_t skip_self;   /* A is B: 1 = skip aread == bread (absence of -I); 2 = symmetric: every
                          * unordered pair is aligned once and both records are emitted;
                          * 3 = tandem (`datander`, DAMASKER; DENTIST's call commandline.d:2866-2876): every read is
                          *     aligned with ITSELF only, below the main diagonal -- seeds with A position > B position,
                          *     cells in which B's base does not come before A's never match; records have aread ==
                          *     bread and abpos > bbpos.  DH-2 (algo 1), strands = 1 */
    int32_t dmax;        /* cap on differences per extension                                 */
    int32_t width;       /* live diagonals of the wave, <= 62 (one 64-lane wavefront)        */
    int32_t kmer_mod;    /* -%  modimer sampling: only k-mers with hash % kmer_mod == 0; 1 = all     */
    int32_t algo;        /* extension algorithm: 0 = DH-1, the O(ND) furthest-reaching wave (k_wave2);
                          * 1 = DH-2, tile-by-tile banded bit-parallel DP, one alignment per lane (k_tile);
                          *     band = width, which must be 64; with skip_self = 2 the second record of a pair is the
                          *     tiled alignment of the transposed pair through the same seed */
} dh_align_opts;
void dh_default_align_opts(dh_align_opts *o);

/* ---- device-resident sequence DB: replaces the DAZZ_DB .db/.dam the tools open
 *      (DB stub + .idx/.bps; created by dazzler.d:6233-6330 fasta2DB/DAM). */
typedef struct dh_db dh_db;
/* bases: concatenated codes, off[n+1] offsets, group: optional per-sequence group id (pile-up
 * index when many pile-ups are batched in one DB; alignments never cross groups) or NULL.     */
int dh_db_create(dh_ctx *ctx, const uint8_t *bases, const int64_t *off, int32_t n,
                 const int32_t *group, dh_db **out);
void dh_db_destroy(dh_db *db);
/* soft mask = union of the daligner/damapper -m tracks (commandline.d:2886-2955 passes -mdust,
 * -mdentist-self, -mtan, -mrep): per sequence sorted disjoint intervals iv[2j], iv[2j+1] for j in
 * [ptr[s], ptr[s+1]).  k-mers touching a masked interval are neither indexed (A side) nor looked
 * up (B side); alignments still extend through masked sequence.  The call REPLACES the tracks of an
 * earlier dh_db_set_mask; the bits the library derived itself (dh_db_dust, dh_db_mask_coverage) are a
 * layer of their own and stay -- the effective mask is the OR of the two layers.  ptr == NULL clears
 * the whole mask, both layers. */
int dh_db_set_mask(dh_db *db, const int64_t *ptr, const int32_t *iv);
/* DBdust (symmetric DUST, -w64 -t2.0 -m10; DENTIST runs it on every DB it aligns with -mdust,
 * processPileUps/package.d:476-482, 655-667): low-complexity windows are found on the device and
 * ORed into the DB's soft mask.  A window of L = 16, 32 or 64 bases is masked when its triplets
 * repeat with a DUST score above 2.0: sum_t c_t (c_t - 1) / 2 > 2 (L - 3).
 * dh_db_get_mask returns the current soft mask as intervals (what DBdust writes into the `dust`
 * track): ptr gets n + 1 entries, iv may be NULL to size; returns the interval count or < 0. */
int dh_db_dust(dh_db *db);
int64_t dh_db_get_mask(dh_db *db, int64_t *ptr, int32_t *iv, int64_t iv_cap);
/* drop cached derived data (k-mer index, reverse complement): the next dh_align_db rebuilds it */
int dh_db_drop_cache(dh_db *db);
int32_t dh_db_nreads(const dh_db *db);
int64_t dh_db_total_bases(const dh_db *db);

/* ---- local alignments: the .las record (struct Overlap/Path of dalign.h as mirrored at
 *      source/dentist/dazzler.d:1988-2032; bytes [8,48) of it are what goes to disk)          */
#define DH_FLAG_COMP 0x1u
#define DH_FLAG_START 0x4u
#define DH_FLAG_NEXT 0x8u
#define DH_FLAG_BEST 0x10u
#define DH_FLAG_DISABLED 0x20u
typedef struct {
    int32_t tlen, diffs, abpos, bbpos, aepos, bepos;
    uint32_t flags;
    int32_t aread, bread; /* 0-based as on disk; DENTIST adds 1 in memory (dazzler.d:1731-1734) */
    int32_t pad;
    int64_t toff; /* offset of this LA's (diffs, bbases) pairs in the u16 trace array */
} dh_la;

typedef struct dh_la_set dh_la_set; /* host-side result set owned by the library */
void dh_la_set_destroy(dh_la_set *s);
int64_t dh_la_set_count(const dh_la_set *s);
int64_t dh_la_set_trace_len(const dh_la_set *s);
const dh_la *dh_la_set_records(const dh_la_set *s);
const uint16_t *dh_la_set_trace(const dh_la_set *s);
int32_t dh_la_set_tspace(const dh_la_set *s);

/* statistics of the last dh_align_db call on this context */
typedef struct {
    int64_t hits, cands, alignments, wave_cells, las;
    int64_t b_bases;       /* bases of B processed (both strands counted once)               */
    float ms_index, ms_seed, ms_wave, ms_gather, ms_total; /* HIP-event times on ctx stream   */
    int32_t wave_launches;
    int32_t overflow_items; /* (read, strand) items that exceeded a per-item capacity: more than 256
                             * candidate band pairs (the item yields no alignments) or, in symmetric
                             * mode, more than max_la overlaps (the excess records are dropped).  The
                             * call still succeeds; dh_process_pileups skips the pile-ups concerned
                             * with DH_PILE_ALIGN_OVERFLOW, as the reference skips a failing pile-up
                             * (processPileUps/package.d:319-363) */
    int64_t big_items;     /* (read, strand) items whose hits were staged in HBM instead of LDS  */
} dh_align_stats;
int dh_get_align_stats(dh_ctx *ctx, dh_align_stats *out);

/* cumulative over every dh_align_db executed on the context since the last reset (the pile-up
 * path calls it several times per batch): HIP-event kernel times and work counters */
typedef struct {
    double ms_index, ms_seed, ms_wave, ms_gather;
    int64_t wave_launches, wave_cells, alignments, las, aligned_bp, trace_values, hits, b_bases;
} dh_cum_stats;
int dh_get_cum_stats(dh_ctx *ctx, dh_cum_stats *out, int32_t reset);
/* Releases the context's device scratch (grow-only buffers kept between calls so that no call pays for GB-sized
 * allocations: the wave / tile slots, the derived copies of a read chunk, the partitioned join's entry and hit pools --
 * about 100 GB after an unsampled mapping of configs[2]).  For a long-lived host that moves on to another workload; the
 * next call allocates what it needs again.  (The reference's tools are processes: their memory goes with them,
 * dazzler.d:6519-6594.) */
int dh_ctx_release_scratch(dh_ctx *ctx);
/* Chunks of reads of the mapping calls on this context whose seeds came from the radix-partitioned k-mer join
 * (csrc/dh_mjoin.h: the damapper role, dazzler.d:6158-6170, without a random directory line per k-mer) -- out2[0] --
 * and chunks that exceeded one of its capacities and were redone by the directory lookups -- out2[1].  Both paths give
 * the same alignments; the counts say which one ran (tests, traces). */
int dh_get_mjoin_counts(dh_ctx *ctx, int64_t *out2, int32_t reset);
/* The pile-up join (csrc/dh_join.h) of the grouped all-vs-all calls on this context: out4[0] k_join launches, out4[1] those
 * of them that were reruns (the hit buffer of the launch before was too small), out4[2] the hits of the last join, out4[3]
 * the capacity (hits) its first attempt ran with.  After dh_process_pileups the counters of its concurrent parts are added
 * to the context's: out4[2] and out4[3] are then sums over the parts of that call.  reset clears all four. */
int dh_get_join_counts(dh_ctx *ctx, int64_t *out4, int32_t reset);
/* The per-group table join (csrc/dh_tjoin.h) of the calls of a grouped A against a grouped B on this context (the
 * consensus re-alignment: templates against the reads of their pile-ups): out4[0] calls whose seeds came from the group's
 * k-mer table on chip, out4[1] such calls that kept the directory lookups because a limit was not met (a group with more
 * index entries than the table is planned for, k > 16, B not grouped), out4[2] the hits of the last call, out4[3] reruns of
 * the hit buffer.  After dh_process_pileups the counters of its concurrent parts are added to the context's.  Both paths
 * give the same alignments.  reset clears all four. */
int dh_get_tjoin_counts(dh_ctx *ctx, int64_t *out4, int32_t reset);
/* The middle tier of the segment-fed seed back end (256 threads, 2048 hits and 64 candidate band pairs per read: the first
 * tier of a chunk of the mapping join or the table join whose reads have 342 to 1365 hits on average): out2[0] chunks whose
 * first tier it was, out2[1] reads it could not hold (more hits or more band pairs), redone by the 512-thread tiers.  After
 * dh_process_pileups the counters of its concurrent parts are added to the context's.  Every tier gives the same
 * candidates.  reset clears both. */
int dh_get_seed_tier_counts(dh_ctx *ctx, int64_t *out2, int32_t reset);
/* The band phase of the segment-fed 8192- and 16384-entry seed tiers (the pile-up all-vs-all's): out2[0] reads whose band
 * heads went to a table in the unused tail of their LDS hit buffer, out2[1] reads whose table did not fit and which kept the
 * per-hit arrays in global scratch (all of them under DH_SEED_SLAB_BANDS=1).  Counted on the context's device since the
 * last reset, over every context of the process; the call waits for the device.  Both ways give the same candidates.
 * reset clears both. */
int dh_get_seed_band_counts(dh_ctx *ctx, int64_t *out2, int32_t reset);
/* The capacity (hits) that join's first attempt asks for -- host arithmetic only, no device needed.  bases[g] / reads[g]:
 * bases and reads of group g; rate: hits per base per read of depth (<= 0: the initial figure of a fresh context);
 * free_bytes: device memory free at that moment (< 0: not known, no clamp).  See dh_join_hit_capacity in csrc/dh_join.h. */
int64_t dh_join_hit_capacity(const int64_t *bases, const int32_t *reads, int32_t ngroups, int32_t skip_self, double rate,
                             int64_t free_bytes);

/*
 * dh_align_db -- every sequence of B against all of A: k-mer seeds, diagonal band filter, wave
 * local alignment with trace points.  Replaces the spawns
 *   `damapper -C -T<t> -e0.7 ... <ref> <reads>`   dazzler.d:6158-6170 (getDamapping :3855-3866,
 *                                                 workflow call snakemake/Snakefile:1143-1170)
 *   `daligner -T<a> -B -s126 -l500 -e0.7 db db`   dazzler.d:6121-6140 (getDalignment :3829-3844)
 *   `daligner -A ... contigs consensus`           processPileUps/package.d:655-667
 * Output: LAs in LAsort order (base.d:1787-1809); each record's toff locates its trace pairs in
 * the trace array (the trace array itself is not reordered).  select_best != 0 additionally sets the
 * chain flags damapper emits (START/BEST, consumer dazzler.d:1728-1758).
 */
int dh_align_db(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, int32_t select_best,
                dh_la_set **out);
typedef struct { int32_t score, aseq, apos, bpos; } dh_seed_cand;   /* == DhCand */
/* The seed stage of dh_align_db alone: for every item (2 * read + strand) of B the candidates as the extension would
 * receive them, in stored order. cand: 2 * n(B) * opts->max_cand entries, row i = item i; ncand, nhits: 2 * n(B).
 * Items of a strand that opts->strands leaves out: 0 / 0.  ncand -2: the seed filter gave up on the item (more than 256
 * candidate band pairs; dh_align_db reports such reads as overflow).  The index, the joins, the tier selection, what the
 * context learns and the counters (dh_get_seed_tier_counts, dh_get_mjoin_counts, dh_get_join_counts,
 * dh_get_tjoin_counts) are those of the dh_align_db call with the same arguments; no alignment is computed.
 * dh_get_align_stats then gives hits, cands, overflow_items, big_items and b_bases of the seed stage, the rest 0; the
 * cumulative statistics do not count the call.  (Tests: which tier or join disagrees on which item.) */
int dh_seed_candidates(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts,
                       dh_seed_cand *cand, int32_t *ncand, int32_t *nhits);
/* The extension stage of dh_align_db alone, the mirror of dh_seed_candidates: the call runs as dh_align_db does, but every
 * item (2 * read + strand of B) extends the caller's candidates -- cand[item * opts->max_cand + c], c < ncand[item], taken
 * as they stand -- where the seed stage would have produced them (symmetric mode, skip_self 2: the candidates of an item
 * grouped by aseq, every unordered pair in one item only, as the seed stage leaves them).  No k-mer is looked up; the
 * result does not depend on what A and B share.  want_sorted 0: records in item and slot order (symmetric mode: slots are
 * claimed in arrival order); 1: LAsort order.  out_transposed may be NULL; it is accepted under the conditions of
 * dh_align_db_transposed.  Checked on the host before anything is launched, DH_EINVAL otherwise: 0 <= ncand <= max_cand,
 * 0 <= aseq < n(A), 0 <= apos <= alen, 0 <= bpos <= blen; ncand = 0 for the items of a strand that opts->strands leaves out;
 * skip_self 1 and 2: aseq != read; skip_self 3: aseq == read and apos > bpos.  dh_get_align_stats then gives alignments, wave_cells, las, overflow_items and wave_launches of the call
 * (hits 0, cands the sum of ncand).  (Tests: which kernel disagrees on which candidate.) */
int dh_extend_candidates(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, const dh_seed_cand *cand,
                         const int32_t *ncand, int32_t want_sorted, dh_la_set **out, dh_la_set **out_transposed);
/* select_best: damapper's chains.  The LAs of a read on one contig and strand that follow each other (gaps <= 10 kb,
 * gap difference <= 6 kb: a long indel splits a mapping into collinear LAs) form a chain: START (0x4) on its first
 * LA, NEXT (0x8) on the others, BEST (0x10) on the LAs of the chain that no higher-scoring chain of the strand covers
 * by more than half (consumer: dazzler.d:1728-1758).  dh_set_near_best(ppm) is damapper's -n: alternate chains scoring
 * less than that fraction of the chain that beats them are DISABLED; 0 (default) keeps every chain.  dh_set_near_best sets
 * the process-wide default, dh_ctx_set_near_best the value of one context (-1: back to the process default) -- a library
 * user who never asked for -n is not affected by what another context set.  (damapper's own default is -n1.00,
 * commandline.d:2943-2955 always passes -n.7.) */
void dh_set_near_best(int32_t ppm);
int dh_ctx_set_near_best(dh_ctx *ctx, int32_t ppm);

/* One read block against the whole reference, the unit the workflow shards the mapping by
 * (`damapper <ref> <reads>.<block>`, snakemake/Snakefile:1143-1170; blocks = DBsplit ranges of one
 * DB): reads [first, first + count) of B; bread in the records are ids of the whole DB.  The k-mer
 * index of A is built once and stays with A between calls.  dh_la_set_merge is LAmerge
 * (Snakefile:1173-1185) on the in-memory results: one set in LAsort order. */
int dh_align_db_block(dh_ctx *ctx, dh_db *A, dh_db *B, int32_t first, int32_t count,
                      const dh_align_opts *opts, int32_t select_best, dh_la_set **out);
/* `damapper -C`: the mapping of B onto A and, in one pass, the set of its transposed records (aread = B read, bread = A
 * sequence; source/dentist/dazzler.d:6158-6170 writes them as <B>.<A>.las, getLasFile :4339-4354).  DH-2 only
 * (opts->algo = 1, A != B): for every accepted local alignment the transposed pair -- A'' = the read on its forward
 * strand, B'' = the contig, complemented for a reverse-strand mapping -- is aligned through the same seed and accepted
 * on its own (min_len, max_err_ppm); its trace lies on the read's grid.  want_best: chain flags on both sets (the
 * transposed set with the roles of the sequences exchanged).  Both sets in LAsort order. */
int dh_align_db_transposed(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_align_opts *opts, int32_t want_best,
                           dh_la_set **out, dh_la_set **out_transposed);
int dh_la_set_merge(const dh_la_set *const *sets, int32_t nsets, dh_la_set **out);

/* ---- .las files: replaces the reader/writer pair of source/dentist/dazzler.d:1665-1834
 *      (LocalAlignmentReader) and :1913-1960, 2130-2170 (writeAlignments/writeDazzlerOverlap). */
int dh_las_write(const char *path, const dh_la *las, int64_t n, const uint16_t *trace,
                 int32_t tspace);
int dh_las_read(const char *path, dh_la_set **out);
/* LAmerge (snakemake/Snakefile:1173-1185): the .las files of read blocks (one per GPU) merged into one
 * file in LAsort order; all inputs must share the trace spacing.  Host only. */
int dh_las_merge(const char *const *paths, int32_t npaths, const char *out_path);


/* ---- trace-point arithmetic of the alignment model (Trace.translateTracePoint!"contigA",
 *      source/dentist/common/alignments/base.d:185-244; the cropper is built on it, cropper.d:503-550):
 *      apos is assigned to a trace point of the LA (mode 0 = RoundingMode.floor, 1 = ceil); out_a /
 *      out_b = that trace point on A and on B.  trace = the u16 array the record's toff indexes.
 *      DH_EINVAL when apos lies outside [abpos, aepos] (the reference asserts). Host only. */
int dh_translate_trace_point(const dh_la *la, const uint16_t *trace, int32_t tspace, int32_t apos,
                             int32_t mode, int32_t *out_a, int32_t *out_b);

/* getCommonTracePoint (commands/processPileUps/cropper.d:446-500) of one flank of a pile-up as an entry of its own:
 * first[count] names the first record of every alignment chain of the flank (same contig, same seed; chain members
 * follow their first record, dazzler.d:1728-1758); the common region is the intersection of the chains' A regions
 * (union of the members' A intervals, common/package.d:228-241).  Candidates are the trace points of the region plus
 * the contig end, taken from the inner side for seed_front != 0; the region minus the repeat mask (mask_iv = nmask
 * sorted disjoint (begin, end) pairs of this contig) is tried first, then the region itself.  *out = -1: none. Host only. */
int dh_common_trace_point(const dh_la *las, int64_t n, const int32_t *first, int32_t count, int32_t contig_len,
                          int32_t tspace, int32_t seed_front, const int32_t *mask_iv, int64_t nmask, int32_t *out);

/* ---- pile-ups: which reads span which gap.  Host-side stand-in for the part of `dentist collect`
 *      the consensus path needs (spanning reads only; the scaffold-graph builder of
 *      source/dentist/commands/collectPileUps/pileups.d is outside this library). */
typedef struct {
    int32_t tspace_map;        /* trace spacing of the read->contig LAs (100)                       */
    int32_t allowance;         /* proper-alignment-allowance of the mapping LAs (= tspace_map)      */
    int32_t min_anchor;        /* --min-anchor-length, commandline.d:2036 (500)                     */
    int32_t min_reads;         /* --min-reads-per-pile-up, commandline.d:2125-2187 (3)              */
    int32_t max_reads;         /* reads kept per pile-up (default 60); 0 = every read, as the reference
                                * (commandline.d:2125-2187 knows minimum counts only)                */
    int32_t tspace_pile;       /* -s126 of the pile-up daligner call, commandline.d:2886-2902       */
    int32_t rounds;            /* consensus rounds (1 = reference read + its overlaps only)         */
    int32_t flank_window;      /* bases of each flanking contig given to the flank re-alignment (default 20 000);
                                * 0 = the whole contigs, as the reference does (commandline.d:2918-2935) */
    int32_t max_align_err_ppm; /* --max-alignment-error 0.30, commandline.d:1808                    */
    int32_t max_ins_err_ppm;   /* --max-insertion-error 0.10, commandline.d:1997                    */
    int32_t bad_fraction_ppm;  /* --bad-fraction 0.08, commandline.d:1101                           */
    int32_t width;             /* live diagonals of the wave in the pile-up stages (dh_align_opts.width), 0 = 30 */
    int32_t dust;              /* 1: DBdust + -mdust on the pile-up DB and the flank DB (package.d:476-482,
                                * 655-667); the flank DB also inherits the contigs' soft mask (-mrep)       */
    int32_t algo;              /* alignments of the process stages (pile-up all-vs-all, re-alignment to the template,
                                * flanks): 0 = DH-1 (wave, `width` live diagonals), 1 = DH-2 (tiled band of 64, k_tile) */
    int32_t max_partners;      /* 0 (default) = the pile-up all-vs-all aligns every read with every other, as
                                * `daligner pile.db pile.db` does (package.d:474-485).  n > 0 (DH-2 only): a pile-up of more
                                * than n reads takes n PARTNER reads -- the first n in the order: reads that may serve as
                                * reference read (:461-472), then the others, each in pile-up order -- and aligns a read with
                                * the partners only: the tile QVs that rank the reference-read candidates (:498-568) and the
                                * first consensus round see n overlaps per read instead of all, the later consensus rounds
                                * still re-align EVERY read of the pile-up to the template.  The n^2 stage becomes n x
                                * max_partners; every read keeps its vote.  oracle/process.py, oracle/pile.c: same rule. */
    int32_t min_relative_score_ppm; /* --min-relative-score of the pile-up chaining (commandline.d:2141-2153; 1 000 000 =
                                * the default 1.0: only chains with the pair's best score; valid range [1, 1 000 000], 0 is
                                * refused as the mark of a zero-filled or too short struct).  Below it the chains of a pair
                                * within that fraction of its best chain are kept, per connected component of the
                                * chainability relation, ALTERNATE chains (sharing a prefix with a better chain) included:
                                * the LAs they share then count once per chain, as in the reference's chained .las
                                * (chaining.d:166-312, dazzler.d:2050-2085).  The funnel then runs on the host. */
} dh_process_opts;
void dh_default_process_opts(dh_process_opts *o);

typedef struct dh_pileups dh_pileups;
/* las/trace: read->contig LAs (A = contig, B = read) as returned by dh_align_db.  A read spans
 * the gap between contig c and c+1 when it has an LA reaching the end of c and an LA starting at
 * the begin of c+1, same orientation, in read order, both anchors >= min_anchor.  Every read
 * enters a pile-up once (its pair of LAs with the longest anchors); pile-ups with fewer than
 * min_reads reads are dropped (commandline.d:2125-2187); of more than max_reads the max_reads
 * reads whose anchoring LAs have the lowest error rate are kept (ties: lower read id).
 *   dh_collect_spanning   = dh_collect_candidates + dh_pileups_select
 *   dh_collect_candidates   every spanning read of every gap, no cut (the multi-GPU path exchanges
 *                           candidates between ranks first)
 *   dh_pileups_create       pile-ups from explicit arrays: npiles gaps ordered by contig_left,
 *                           count[i] (read, left LA index, right LA index) triples each
 *   dh_pileups_select       the min_reads / max_reads cut on a candidate set */
int dh_collect_spanning(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                        const dh_process_opts *opts, dh_pileups **out);
int dh_collect_candidates(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                          const dh_process_opts *opts, dh_pileups **out);
int dh_pileups_create(const int32_t *contig_left, const int32_t *count, int32_t npiles,
                      const int32_t *triples, dh_pileups **out);
int dh_pileups_select(const dh_pileups *cands, const dh_la *las, int64_t n, const dh_process_opts *opts,
                      dh_pileups **out);
void dh_pileups_destroy(dh_pileups *p);
int32_t dh_pileups_count(const dh_pileups *p);
/* pile-up i: left contig id (gap lies between it and the next contig), number of reads, and the
 * (read, left LA index, right LA index) triples */
int32_t dh_pileups_get(const dh_pileups *p, int32_t i, int32_t *contig_left, const int32_t **triples);
/* Pile-ups of ANY join of the scaffold graph (ReadAlignment types of common/alignments/base.d:2160-2330; PileUp types
 * :2725-2805; cropper.d:113-175 crops them all the same way): nodes4[4 * i ..] = (contig0, seed0, contig1, seed1) of
 * pile-up i -- flank 0 = contig0 cropped at its seed0 side (DH_SEED_FRONT: the reads hang over the contig's begin,
 * DH_SEED_BACK: over its end), flank 1 likewise; contig1 = -1: an extension pile-up (one flank).  The gap between
 * contig c and c + 1 of dh_pileups_create is (c, DH_SEED_BACK, c + 1, DH_SEED_FRONT); (c, BACK, d, BACK) and
 * (c, FRONT, d, FRONT) are anti-parallel joins, d > c + 1 skips contigs.  contig0 < contig1 (a contig joined with
 * itself is refused), pile-ups ordered by their nodes, triples = (read, LA on flank 0 or -1, LA on flank 1 or -1).
 * dh_pileups_get_join returns the four values of pile-up i (also for pile-ups made by the other creators). */
#define DH_SEED_FRONT 0
#define DH_SEED_BACK 1
int dh_pileups_create_joins(const int32_t *nodes4, const int32_t *count, int32_t npiles, const int32_t *triples,
                            dh_pileups **out);
int dh_pileups_get_join(const dh_pileups *p, int32_t i, int32_t *nodes4);

/* maskRepetitiveRegions (commands/maskRepetitiveRegions.d:129-176 assessRepeatStructure, :238-430
 * BadAlignmentCoverageAssessor): ORs into the soft mask of `db` every region whose coverage by the
 * alignment intervals [abpos, aepos) of `las` is < lower or > upper; improper_only != 0 counts only
 * alignments that are not proper within `allowance` (base.d:537-557; needs read_off).  The command's mask
 * is the union of one call over all alignments with --max-coverage-reads and one improper-only call with
 * --max-improper-coverage-reads; read the result with dh_db_get_mask, write it with dh_dazz_write_mask.
 * n == 0 masks nothing (:347-348). */
int dh_db_mask_coverage(dh_db *db, const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads,
                        int32_t lower, int32_t upper, int32_t improper_only, int32_t allowance);
/* the bounds DENTIST derives from --read-coverage (commandline.d:1876-1889, 1957-1970) */
int32_t dh_max_coverage_reads(double read_coverage);
int32_t dh_max_improper_coverage_reads(double read_coverage);

/* `dentist propagate-mask` (commands/propagateMask.d:136-305): the contig mask (mask_ptr[ncontigs + 1],
 * mask_iv = sorted disjoint (begin, end) pairs) carried over to the reads through the trace points of the
 * read->contig LAs -- begin rounded down, end rounded up, mirrored for complement alignments -- and merged
 * per read.  out_ptr gets nreads + 1 entries, out_iv (begin, end) pairs on the forward read; out_iv may be
 * NULL to size (cap = pairs it can hold); returns the number of intervals or a negative error.  Host only. */
int64_t dh_propagate_mask(const dh_la *las, int64_t n, const uint16_t *trace, int32_t tspace, const int64_t *mask_ptr,
                          const int32_t *mask_iv, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                          int64_t *out_ptr, int32_t *out_iv, int64_t cap);

/* `dentist validate-regions` (commands/validateRegions.d:141-203 region context, :325-512 RegionValidator):
 * every region (closed gap on the gap-closed assembly) extended by region_context (default 1000,
 * commandline.d:2411) is valid iff every window of weak_coverage_window bases (default 500, :2497) inside
 * it is spanned by >= min_coverage_reads alignments (from --read-coverage: 0.5 * x / ploidy, :2080-2085)
 * and >= min_spanning_reads alignments span the whole extended region.  las: reads aligned to that
 * assembly, grouped by aread.  reports[nregions]; weak_iv (may be NULL, cap triples) = weakly covered
 * (contig, begin, end) per region in region order (--weak-coverage-mask); returns their number.  Host only. */
typedef struct dh_region { int32_t contig, begin, end; } dh_region;
typedef struct dh_region_report { int32_t num_spanning_reads, weak_bp, is_valid, ctx_begin, ctx_end; } dh_region_report;
int64_t dh_validate_regions(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                            const dh_region *regions, int32_t nregions, int32_t region_context,
                            int32_t weak_coverage_window, int32_t min_coverage_reads, int32_t min_spanning_reads,
                            dh_region_report *reports, int32_t *weak_iv, int64_t cap);

/* The mapping pass with the six filters of `dentist collect` applied on the way: `damapper` per read block
 * (snakemake/Snakefile:1143-1170) + collectPileUps/filter.d:122-356.  Every filter decides per read, so
 * the records of a finished chunk of reads get their chain flags and are filtered on a host thread while
 * the device maps the next chunk.  want_sorted != 0: result = dh_align_db_block(want_best = 1) followed by
 * dh_collect_filter (same records, flags and dropped6 counts, LAsort order).  want_sorted == 0: the same
 * records in mapping order (by read, strand); then `cands` (may be NULL) receives the spanning-read
 * candidates of dh_collect_candidates, collected chunk by chunk as well (indices into the result).
 * want_sorted is a bit set: 1 = LAsort order; 8 = the trace values stay on the device in a buffer the result owns
 * (dh_la_set_trace downloads them when asked; dh_process_pileups_set gathers what the cropper needs there). */
int dh_map_reads(dh_ctx *ctx, dh_db *contigs, dh_db *reads, int32_t first, int32_t count, const dh_align_opts *opts,
                 const dh_process_opts *popts, const int64_t *rep_ptr, const int32_t *rep_iv, int32_t want_sorted,
                 int64_t *dropped6, dh_la_set **out, dh_pileups **cands);

/* ---- the scaffold-graph pile-up builder of `dentist collect` (collectPileUps/pileups.d:173-208 build;
 * collectPileUps/package.d:174-184 is the call site).  Nodes are (contig, part) with part 0 = pre,
 * 1 = begin, 2 = end, 3 = post (scaffold.d:75-90); a read alignment is one seeded LA (an extension over
 * a contig end) or two (a read spanning a gap), seed 0 = front, 1 = back (base.d:1938-1944).  Steps:
 * collectReadAlignments per read (pileups.d:821-888), joins merged per edge (pileups.d:626-636), forks
 * resolved by read support with a bonus for joins of the input assembly (pileups.d:1592-1657,
 * 1754-1804), min_spanning_reads (pileups.d:1807-1838), extensions merged into their gap
 * (scaffold.d:789-816), pile-ups in edge order (pileups.d:435-444).  resolveBubbles (pileups.d:1124-1590): see
 * dh_scaffold_pileups_resolved below.  DISABLED LAs are ignored.  input_gaps: ngaps pairs (begin contig, end contig) of the
 * input assembly's scaffolding (pileups.d:796-811).  Host only. */
typedef struct dh_scaffold_opts {
    int32_t min_spanning_reads;  /* --min-spanning-reads, default 3 */
    int32_t merge_extensions;    /* 0 = --no-merge-extension */
    double best_pile_up_margin;  /* --best-pile-up-margin, default 3.0 */
    double existing_gap_bonus;   /* --existing-gap-bonus, default 6.0 */
    int32_t only_joins;          /* the SHARDED plan only (dh_shard_graph_plan_create, dh_shard_run): 0 (default) = the gap
                                  * pile-ups between neighbouring contigs with the extension entries merged into them
                                  * (dh_scaffold_gap_pileups; --only spanning --join-policy scaffoldGaps); otherwise every
                                  * pile-up of the scaffold `dentist process` is handed, as dh_scaffold_all_pileups(only):
                                  * & 1 the gap joins of any two contig ends (anti-parallel, contig-skipping), & 2 the
                                  * extension joins -- what `process --batch` jobs take (snakemake/Snakefile:1315-1334,
                                  * processPileUps/package.d:146-159).  Ignored by dh_scaffold_pileups*. */
    int32_t pad_;
} dh_scaffold_opts;
void dh_default_scaffold_opts(dh_scaffold_opts *o);
typedef struct dh_join {        /* one pile-up = the payload of one edge of the scaffold graph */
    int32_t contig0, part0, contig1, part1; /* (contig0, part0) <= (contig1, part1) */
    int32_t type;                /* ReadAlignmentType (base.d:2052-2070): 0 front extension, 1 gap, 2 back extension */
    int32_t count;               /* read alignments of the pile-up: entries[first .. first + count) */
    int64_t first;
} dh_join;
typedef struct dh_read_alignment {
    int32_t read, la0, la1;      /* LA indices into the input; la1 = -1 for an extension */
    uint8_t seed0, seed1, n, pad; /* n = 1 | 2 seeded alignments */
} dh_read_alignment;
typedef struct dh_scaffold dh_scaffold;
int dh_scaffold_pileups(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                        const int64_t *read_off, int32_t nreads, const int32_t *input_gaps, int32_t ngaps,
                        const dh_scaffold_opts *opts, dh_scaffold **out);
/* The same builder WITH resolveBubbles (pileups.d:1100-1315, 1387-1590; position in build(): pileups.d:186): cycles of
 * at most max_bubble_size nodes (0 = the reference's 8, commandline.d:1826-1833) with exactly two nodes of degree >= 3
 * joined by an edge that carries a pile-up -- its reads skip the contigs on the other side of the cycle, whose
 * alignments a mask or a filter removed -- are linearised: the skipping reads are mapped onto the intermediate contigs
 * again without any mask (getReadAlignmentsOnContigs :1316-1385), their read alignments are collected from old and new
 * alignments together, kept iff they walk the skipped path in order (collectFixedSimpleBubbles :1414-1491), and replace
 * the skipping pile-up; at most max_iterations sweeps (0 = 4, :1835-1837).  The alignments added on the way come back in
 * *extra: LA index n + i in the result's read alignments = record i of *extra.  *resolved (optional) = bubbles handled.
 *   dh_scaffold_pileups_resolved  the device maps (dh_remap_skipping_reads with map_opts; chains must cover their contig
 *                                 within `allowance`); contig / read offsets are those of the DBs; *extra carries the traces
 *   dh_scaffold_pileups_cb        host only: `remap` supplies the alignments (las_out malloc'd by the callback, freed here;
 *                                 ids of the full DBs, DISABLED unless the chain covers its contig) */
typedef int (*dh_remap_fn)(void *user, const int32_t *contig_ids, int32_t ncontig_ids, const int32_t *read_ids, int32_t nread_ids,
                           dh_la **las_out, int64_t *n_out);
int dh_scaffold_pileups_cb(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                           int32_t nreads, const int32_t *input_gaps, int32_t ngaps, const dh_scaffold_opts *opts,
                           int32_t max_bubble_size, int32_t max_iterations, dh_remap_fn remap, void *user, dh_scaffold **out,
                           dh_la_set **extra, int32_t *resolved);
int dh_scaffold_pileups_resolved(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const dh_la *las, int64_t n, const int32_t *input_gaps,
                                 int32_t ngaps, const dh_scaffold_opts *opts, const dh_align_opts *map_opts, int32_t allowance,
                                 int32_t max_bubble_size, int32_t max_iterations, dh_scaffold **out, dh_la_set **extra,
                                 int32_t *resolved);
int32_t dh_scaffold_npiles(const dh_scaffold *s);
int64_t dh_scaffold_nentries(const dh_scaffold *s);
const dh_join *dh_scaffold_joins(const dh_scaffold *s);
const dh_read_alignment *dh_scaffold_entries(const dh_scaffold *s);
void dh_scaffold_destroy(dh_scaffold *s);
/* the pile-ups dh_process_pileups handles -- gap joins (c, end)--(c + 1, begin) -- with their spanning
 * read alignments as (read, left LA, right LA) triples; *skipped = pile-ups of any other kind */
/* The re-mapping call of `resolveBubbles` (getReadAlignmentsOnContigs, collectPileUps/pileups.d:1316-1385): the reads
 * read_ids[] (those of a pile-up whose join skips contigs) are mapped, without any mask, onto the intermediate contigs
 * contig_ids[] alone -- the reference builds two DB subsets and spawns damapper on them (:1337-1366); here the subsets
 * are gathered on the device.  Chains that do not cover their contig completely within `allowance`
 * (completelyCovers!"contigA", common/alignments/base.d:562-566) come back DISABLED; ids are those of the full DBs
 * (:1373-1380).  Ids 0-based, ascending, distinct.  The graph surgery of BubbleResolver stays with the caller. */
int dh_remap_skipping_reads(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const int32_t *contig_ids, int32_t ncontig_ids,
                            const int32_t *read_ids, int32_t nread_ids, const dh_align_opts *opts, int32_t allowance,
                            dh_la_set **out);
int dh_scaffold_spanning(const dh_scaffold *s, const dh_la *las, int64_t n, dh_pileups **out, int32_t *skipped);
/* the same pile-ups with EVERY read alignment the builder put into them, as `dentist process` gets them
 * (pile-ups.db): besides the spanning reads the extension-type read alignments that mergeExtensionsWithGaps
 * (scaffold.d:789-816) moved into the gap -- (read, LA, -1): back extension of the left contig, (read, -1, LA):
 * front extension of the right one.  The cropper cuts them from their crop point to the read's end
 * (cropper.d:339-361, 503-550); they are members of the pile-up but never its reference read
 * (processPileUps/package.d:461-472). */
int dh_scaffold_gap_pileups(const dh_scaffold *s, const dh_la *las, int64_t n, dh_pileups **out, int32_t *skipped);
/* Every pile-up of the scaffold `dentist process` is handed (collectPileUps/package.d:88-96 writes them all; which
 * insertions are used is `dentist output`'s --only, commandline.d:2230-2250): only & 1 = the gap joins of any two
 * contig ends (same orientation, anti-parallel, contig-skipping), only & 2 = the extension joins.  The pile-ups carry
 * their nodes (dh_pileups_create_joins / dh_pileups_get_join); entries as in dh_scaffold_gap_pileups with flank 0 / 1
 * in place of left / right.  *skipped = joins without entries. */
int dh_scaffold_all_pileups(const dh_scaffold *s, const dh_la *las, int64_t n, int32_t only, dh_pileups **out,
                            int32_t *skipped);

/* the six alignment filters of `dentist collect` (collectPileUps/filter.d:122-356, order of
 * collectPileUps/package.d:130-141) on the read->contig LAs: LQ (averageErrorRate > max_align_err),
 * Improper (allowance), WeaklyAnchored (<= min_anchor bases outside the repeat mask rep_ptr / rep_iv of
 * the contigs, may be NULL), Contained, Ambiguous (reads with alignments overlapping on the read),
 * Redundant (reads that fit inside one contig).  Dropped LAs get DH_FLAG_DISABLED in place;
 * dropped6[stage] = LAs dropped per stage, read_used[r] = 0 for reads discarded by 5 / 6 (either may be
 * NULL).  Host only. */
int dh_collect_filter(dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                      int32_t nreads, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                      int64_t *dropped6, uint8_t *read_used);

/* all pile-ups at once: contig_left[npiles], count[npiles], triples[3 * total] (any may be NULL);
 * returns the total number of triples */
int64_t dh_pileups_flat(const dh_pileups *p, int32_t *contig_left, int32_t *count, int32_t *triples);

/* ---- `dentist process` for a batch of pile-ups: crop -> pile-up alignment -> filter -> tile QV
 *      -> reference read -> consensus -> flank re-alignment -> insertion
 *      (source/dentist/commands/processPileUps/package.d:283-374; cropper.d:446-550;
 *      common/insertions.d:110-146).  Replaces the ~15 tool spawns per pile-up of
 *      package.d:474-697 (daligner, DAScover/DASqv, computeintrinsicqv, daccord, daligner -A). */
#define DH_PILE_OK 0
#define DH_PILE_NO_COMMON_TRACE_POINT 1
#define DH_PILE_TOO_SMALL 2
#define DH_PILE_EMPTY_ALIGNMENT 3
#define DH_PILE_FLANKS_NOT_UNIQUE 4
#define DH_PILE_ORIENTATION 5
#define DH_PILE_MAX_INSERTION_ERROR 6
#define DH_PILE_NEGATIVE_INSERTION 7
#define DH_PILE_ALIGN_OVERFLOW 8 /* a read of the pile-up exceeded a per-read capacity of the aligner */
#define DH_PILE_UNSUPPORTED_JOIN 9 /* a contig joined with itself */
/* dh_insertion.join: 0 = the gap between contig_left and contig_left + 1 in the same orientation
 * ((contig_left, end) -> (contig_right, begin)); otherwise bits */
#define DH_JOIN_FLANK0_FRONT 1 /* flank 0 is the BEGIN of contig_left (seed front) instead of its end     */
#define DH_JOIN_FLANK1_BACK 2  /* flank 1 is the END of contig_right (seed back) instead of its begin     */
#define DH_JOIN_EXTENSION 4    /* no flank 1: the consensus extends contig_left over the flank-0 side     */
typedef struct {
    int32_t contig_left;   /* flank 0 (the `left` fields below); the contig with the smaller id                */
    int32_t status;        /* DH_PILE_*                                                             */
    int32_t nreads;        /* reads in the cropped pile-up                                          */
    int32_t ref_read;      /* index of the reference read inside the pile-up, -1 if none            */
    int32_t ref_read_id;   /* its read id in the reads DB                                           */
    int32_t crop_left;     /* common trace point on the flank-0 contig                              */
    int32_t crop_right;    /* common trace point on the flank-1 contig (-1 for an extension)        */
    int32_t left_aepos;    /* getCroppingPosition!"contigA" of the flank-0 overlap (insertions.d:110-121): the
                            * contig is kept up to here for seed back, from here for seed front       */
    int32_t right_abpos;   /* the same for flank 1                                                  */
    int32_t ins_begin;     /* insertion = oriented consensus [ins_begin, ins_end) (the slice of        */
    int32_t ins_end;       /* getInfoForNewSequenceInsertion, insertions.d:230-284, in the frame of `comp`) */
    int32_t comp;          /* 1: the flank-0 overlap is a complement one -- walking from flank 0 to flank 1 (a
                            * front-seeded flank 0: from flank 1 to flank 0) the consensus is reverse-complemented */
    int32_t cons_len;
    int32_t left_diffs, right_diffs; /* of the two flank overlaps                                   */
    int32_t join;          /* DH_JOIN_* bits, 0 for the plain gap                                   */
    int64_t cons_off;      /* consensus bases (read orientation) in the result's sequence buffer    */
    int32_t contig_right;  /* flank 1: its contig (contig_left + 1 for the plain gap, -1 for an extension) */
    int32_t pad;
} dh_insertion;

typedef struct dh_insertions dh_insertions;
int dh_process_pileups(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const dh_la *las, int64_t n,
                       const uint16_t *trace, const dh_pileups *piles, const dh_process_opts *opts,
                       dh_insertions **out);
void dh_insertions_destroy(dh_insertions *r);
int32_t dh_insertions_count(const dh_insertions *r);
const dh_insertion *dh_insertions_records(const dh_insertions *r);
const uint8_t *dh_insertions_bases(const dh_insertions *r);
int64_t dh_insertions_bases_len(const dh_insertions *r);
/* read ids (0-based) of every record's pile-up, the Insertion.readIds of makeInsertion (processPileUps/
 * package.d:789-798): ids[off[i] .. off[i + 1]), off has count + 1 entries; NULL when the result carries none */
const int32_t *dh_insertions_read_ids(const dh_insertions *r);
const int32_t *dh_insertions_read_ids_off(const dh_insertions *r);
/* The two halves of dh_process_pileups as entry points of their own (dh_process_pileups runs them
 * back to back with the cropped reads staying on the device):
 *   dh_crop_pileups     cropPileUp (cropper.d:113-175, 446-550) for a batch: the common trace point of
 *                       each flank from ALL entries of a pile-up, then [support patch] + read slice +
 *                       [support patch] for the entries whose read is in `reads`.  Read ids in the
 *                       triples are ids of the whole reads DB; `reads` holds [read_first, read_first +
 *                       nreads(reads)) of it -- one rank's share when the mapping is sharded (SURVEY
 *                       8(e)); LAs of reads held elsewhere only need their A intervals.
 *   dh_cropped_create   cropped pile-ups assembled from parts received from other ranks: rec = the
 *                       per-pile-up records of dh_crop_pileups (crop points, status), reads ordered by
 *                       (pile, entry)
 *   dh_process_cropped  pile-up alignment -> filter -> tile QV -> reference read -> consensus -> flank
 *                       re-alignment -> insertion on cropped pile-ups (package.d:283-374 after crop()) */
typedef struct dh_cropped dh_cropped;
int dh_crop_pileups(dh_ctx *ctx, dh_db *contigs, dh_db *reads, int32_t read_first, const dh_la *las, int64_t n,
                    const uint16_t *trace, const dh_pileups *piles, const dh_process_opts *opts,
                    dh_cropped **out);
/* the same with the repeat mask of the contigs (`dentist process --mask`): rep_ptr[ncontigs + 1] / rep_iv = sorted
 * disjoint (begin, end) pairs per contig, as dh_map_reads takes them; the common trace point of a flank is taken
 * outside the mask when one exists there (cropper.d:446-500).  NULL = no mask. */
int dh_crop_pileups_masked(dh_ctx *ctx, dh_db *contigs, dh_db *reads, int32_t read_first, const dh_la *las, int64_t n,
                           const uint16_t *trace, const dh_pileups *piles, const int64_t *rep_ptr, const int32_t *rep_iv,
                           const dh_process_opts *opts, dh_cropped **out);
int dh_process_pileups_masked(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const dh_la *las, int64_t n,
                              const uint16_t *trace, const dh_pileups *piles, const int64_t *rep_ptr, const int32_t *rep_iv,
                              const dh_process_opts *opts, dh_insertions **out);
/* dh_process_pileups_masked on the result set of a mapping itself.  For a set whose trace values stayed on the device
 * (dh_map_reads with want_sorted & 8) only the trace of the pile-up reads' records is brought to the host -- the cropper
 * (cropper.d:446-550) reads nothing else; otherwise the same as passing dh_la_set_records / dh_la_set_trace. */
int dh_process_pileups_set(dh_ctx *ctx, dh_db *contigs, dh_db *reads, dh_la_set *set, const dh_pileups *piles,
                           const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts, dh_insertions **out);
/* 1: the set's trace values are on the device only (dh_la_set_trace would fetch them now) */
int32_t dh_la_set_trace_on_device(const dh_la_set *s);
int dh_cropped_create(const dh_insertion *rec, int32_t npiles, int32_t nreads, const int32_t *pile,
                      const int32_t *entry, const int32_t *read_id, const int64_t *off, const uint8_t *bases,
                      dh_cropped **out);
/* the same with the kind of every read (dh_cropped_kind); kind == NULL: every read spans its gap */
int dh_cropped_create2(const dh_insertion *rec, int32_t npiles, int32_t nreads, const int32_t *pile,
                       const int32_t *entry, const int32_t *read_id, const uint8_t *kind, const int64_t *off,
                       const uint8_t *bases, dh_cropped **out);
void dh_cropped_destroy(dh_cropped *c);
int32_t dh_cropped_npiles(const dh_cropped *c);
/* per cropped read, bits 0-1: 0 = it has alignments on both flanks (spans the gap), 1 = on flank 0 only (plain gap: back
 * extension of the left contig), 2 = on flank 1 only (front extension of the right contig) -- entries with one
 * alignment, see dh_scaffold_gap_pileups; bit 2 / 3: its alignment on flank 0 / 1 is a complement one (the flank
 * overlaps of the consensus are checked against the reference read's, package.d:669-690) */
const uint8_t *dh_cropped_kind(const dh_cropped *c);

/* ---- the host work of one rank between the collectives of the sharded path (one process per GPU): what LAmerge +
 *      `dentist collect` + `process --batch` do through the file system in the reference (snakemake/Snakefile:
 *      1173-1185, 1315-1334).  Blobs are what the caller hands to the collective as they are:
 *        candidates  records of 104 bytes {int32 gap, int32 read, dh_la left, dh_la right} in (gap, read) order
 *        cropped     int64 k, k x {int32 pile, entry, read, len}, then the k reads' bases back to back
 *      dh_shard_pack_candidates  this rank's candidates (dh_collect_candidates / dh_map_reads) -> blob
 *      dh_shard_plan_create      all ranks' blobs (rank order) -> the same pile-ups on every rank (entries of a gap by
 *                                read id, min / max reads cut) and their owners (greedy bin-packing of n^2 L)
 *      dh_shard_read_joins       (scaffold-graph collector) the raw joins of this rank's reads -- collectReadAlignments,
 *                                pileups.d:821-888, a per-read computation -- as a blob of 120-byte records {4 x int32
 *                                edge (contig, part) x 2, int32 read, u8 seed0, seed1, n, pad, dh_la, dh_la}; las[].bread
 *                                are global read ids, read_off the offsets of the rank's reads [read_first, +nreads)
 *      dh_shard_graph_plan_create  all ranks' join blobs (rank order) -> the scaffold every rank derives (forks, min
 *                                spanning reads, extensions merged into gaps), its gap pile-ups incl. extension entries,
 *                                the min / max reads cut, owners -- the pile-ups are those of dh_scaffold_pileups +
 *                                dh_scaffold_gap_pileups + dh_pileups_select on the merged alignments
 *      dh_shard_pack_cropped     the reads this rank cropped -> one blob per owner (one malloc, free blobs[0])
 *      dh_shard_unpack_cropped   the blobs an owner received -> its cropped pile-ups for dh_process_cropped */
typedef struct dh_shard_plan dh_shard_plan;
void dh_shard_free(void *p);
int dh_shard_pack_candidates(const dh_pileups *cands, const dh_la *las, int64_t n, int32_t read_shift, uint8_t **out,
                             int64_t *nbytes);
int dh_shard_plan_create(const uint8_t *const *blobs, const int64_t *sizes, int32_t world, const dh_process_opts *opts,
                         dh_shard_plan **out);
int dh_shard_read_joins(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                        int32_t read_first, int32_t nreads, uint8_t **blob, int64_t *nbytes);
int dh_shard_graph_plan_create(const uint8_t *const *blobs, const int64_t *sizes, int32_t world, int32_t ncontigs,
                               const int32_t *input_gaps, int32_t ngaps, const dh_scaffold_opts *sopts,
                               const dh_process_opts *opts, dh_shard_plan **out);
void dh_shard_plan_destroy(dh_shard_plan *p);
const dh_la *dh_shard_plan_las(const dh_shard_plan *p);
int64_t dh_shard_plan_nlas(const dh_shard_plan *p);
const dh_pileups *dh_shard_plan_pileups(const dh_shard_plan *p);   /* owned by the plan */
const int32_t *dh_shard_plan_owner(const dh_shard_plan *p);         /* one per pile-up of dh_shard_plan_pileups */
int dh_shard_pack_cropped(dh_cropped *crop, const int32_t *owner, int32_t world, uint8_t **blobs, int64_t *sizes);
int dh_shard_unpack_cropped(const uint8_t *const *blobs, const int64_t *sizes, int32_t world, const dh_insertion *rec,
                            int32_t npiles, const int32_t *owner, int32_t rank, dh_cropped **out);
const dh_insertion *dh_cropped_records(const dh_cropped *c);
/* ---- the multi-GPU entry (dh_comm.cpp): one process per GPU, the exchanges over RCCL / xGMI.  Replaces the file system
 *      between the workflow's jobs: LAmerge of the per-block mappings (snakemake/Snakefile:1173-1185), the
 *      `dentist process --batch` jobs (:1315-1358) and `dentist merge-insertions` (commands/mergeInsertions.d:60-164).
 *      Rank 0 calls dh_comm_unique_id and hands the 128 bytes to the other processes (file, socket, MPI ...); every
 *      process calls dh_comm_create(id, rank, world, its context) once and dh_shard_run per batch.  RCCL is loaded on
 *      first use (dlopen); without it these calls fail with DH_ENODEV, everything else works.
 *      dh_comm_create_local: `world` communicators inside ONE process that exchange through memory -- one per host
 *      thread and context (tests, the N-rank emulation on one GPU); same calls, same dh_shard_run.
 *      dh_comm_all_gather / dh_comm_all_to_all: the two collectives on host blobs (staged through page-locked memory and
 *      the context's device scratch); *out = one malloc'd block with the blobs in rank order, release with dh_shard_free.
 *      dh_shard_run: `collect` + `process` of this rank's share of the reads (reads = the reads [read_first, read_first +
 *      nreads(reads)) of the whole DB; las / trace its mapping, bread = ids of the whole DB).  cands != NULL: the
 *      spanning-read collector on the candidates dh_map_reads listed; cands == NULL: the scaffold-graph collector of
 *      `dentist collect` (read_off = offsets of this rank's reads, input_gaps / ngaps / sopts as dh_scaffold_pileups; sopts
 *      NULL = defaults with min_spanning_reads = opts->min_reads).  *out = the closed-gap records of ALL ranks ordered by
 *      gap, identical on every rank and bit-identical to the single-GPU result; info4 (optional) = pile-ups, pile-ups
 *      owned by this rank, entries, bytes of cropped reads sent. */
typedef struct dh_comm dh_comm;
int dh_comm_unique_id(uint8_t *id128);
int dh_comm_create(const uint8_t *id128, int32_t rank, int32_t world, dh_ctx *ctx, dh_comm **out);
int dh_comm_create_local(int32_t world, dh_ctx *const *ctxs, dh_comm **out);
void dh_comm_destroy(dh_comm *c);
int32_t dh_comm_rank(const dh_comm *c);
int32_t dh_comm_world(const dh_comm *c);
int dh_comm_all_gather(dh_comm *c, const uint8_t *payload, int64_t nbytes, uint8_t **out, int64_t *sizes);
int dh_comm_all_to_all(dh_comm *c, const uint8_t *const *per_dest, const int64_t *send_sizes, uint8_t **out,
                       int64_t *recv_sizes);
int dh_shard_run(dh_comm *c, dh_db *contigs, dh_db *reads, int32_t read_first, const int64_t *contig_off, int32_t ncontigs,
                 const dh_la *las, int64_t n, const uint16_t *trace, const dh_process_opts *opts, const dh_pileups *cands,
                 const int64_t *read_off, const int32_t *input_gaps, int32_t ngaps, const struct dh_scaffold_opts *sopts,
                 dh_insertions **out, int64_t *info4);

int32_t dh_cropped_nreads(const dh_cropped *c);
const int32_t *dh_cropped_pile(const dh_cropped *c);     /* pile-up of every cropped read               */
const int32_t *dh_cropped_entry(const dh_cropped *c);    /* its position in the pile-up's read list      */
const int32_t *dh_cropped_read_id(const dh_cropped *c);
const int64_t *dh_cropped_offsets(const dh_cropped *c);  /* nreads + 1                                   */
const uint8_t *dh_cropped_bases(dh_cropped *c);          /* copies device -> host on first use           */
int dh_process_cropped(dh_ctx *ctx, dh_db *contigs, dh_cropped *crop, const dh_process_opts *opts,
                       dh_insertions **out);
/* per-stage HIP-event times (ms) of the last dh_process_pileups call on this context:
 * [0] crop+gather [1] pile-up alignment [2] tile QV [3] consensus vote+emit (all rounds)
 * [4] read->consensus re-alignment (rounds > 1) [5] flank re-alignment [6] total;
 * counters: [0] pile LAs [1] tiles aligned (NW) [2] NW cells */
int dh_get_process_stats(dh_ctx *ctx, float *ms7, int64_t *counters3);
/* the work of the same call: [0] pile-ups processed [1] their entries (cropped reads) [2] cropped bases [3] algorithmic
 * bytes, sum over pile-ups of (n^2 + 2) L for n entries of mean cropped length L (the process stage's roofline figure:
 * every read streamed once per partner, once for the consensus, the flanks and the output) */
int dh_get_process_work(dh_ctx *ctx, int64_t *work4);


/* ---- stage-level entry points (the fused dh_process_pileups runs the same code):
 *  dh_tile_qv    DAScover + DASqv -c<cov> (dazzler.d:3782-3792, 6142-6156): qv[r * maxtiles + t] in
 *                [0, 50] for tile t of read r of the pile-up DB, 255 behind the last tile; las must be
 *                grouped by aread (ascending), traces at tspace.
 *  dh_consensus  computeintrinsicqv + daccord -f -I<i>,<i> (dazzler.d:4213-4255, 6172-6231): consensus
 *                of read ref_read from the overlaps with aread == ref_read; rounds > 1 re-aligns the
 *                reads of the DB to the consensus and votes again.  out: caller's buffer of cap bases. */
int dh_tile_qv(dh_ctx *ctx, dh_db *db, const dh_la *las, int64_t n, const uint16_t *trace, int32_t tspace,
               int32_t cov, uint8_t *qv, int32_t maxtiles);
int dh_consensus(dh_ctx *ctx, dh_db *db, const dh_la *las, int64_t n, const uint16_t *trace, int32_t tspace,
                 int32_t ref_read, int32_t rounds, uint8_t *out, int64_t cap, int64_t *out_len);

/* ---- base-level alignments from trace points: getExactAlignment's per-trace-point part (dazzler.d:2405-2426) for the
 *      records [first, first + count) of las.  Every trace tile of a record (A from abpos to the next multiple of
 *      tspace, then in steps of tspace, ending at aepos; B the running sum of the trace's B bases; COMP records in the
 *      reverse-complement frame of the B read) is aligned by findAlignment(a, b, indelPenalty = 1, No.freeShift) with
 *      its traceback rule (util/string.d:478-520, 775-831), the tile results are concatenated.  One byte per op:
 *      0 match, 1 deletion (A base without B base), 2 insertion (B base without A base), 3 mismatch.
 *        op_off[i] .. op_off[i + 1]      ops of record first + i, in alignment order
 *        score[i]                        sum of its tiles' scores = its number of non-zero ops
 *        tile_off[i] .. tile_off[i + 1]  its tiles in tile_score (the exact edit distance of each tile)
 *        general_tiles                   tiles the banded kernel could not prove exact from the trace's diffs (band =
 *                                        diffs + 1 at most 63) and the full-matrix kernel aligned instead
 *      Limits: tspace <= 250, a tile's B side <= 4 x tspace.  A malformed record (odd tlen, a tile count that disagrees
 *      with abpos / aepos, B bases that do not sum to bepos - bbpos, coordinates outside the sequences, a tile over
 *      the limits) is DH_EINVAL, found on the host before anything is launched; dh_last_error names the record.
 *      dh_format_cigar / dh_format_alignment are host only and need no device: runs of =, X, I, D (extended != 0) or
 *      M, I, D; SequenceAlignment.toString(width)'s three lines per block ('|' match, '*' mismatch, ' ' and '-' for
 *      gaps; a / b: base codes 0..4 print as acgtn, other bytes as they are).  Both return the length of the text
 *      (without the terminating 0) and write it only when out is not NULL and cap is larger than that; a negative
 *      value is an error code. */
typedef struct dh_edit_paths dh_edit_paths;
int dh_la_edit_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace,
                     int32_t tspace, int64_t first, int64_t count, dh_edit_paths **out);
int dh_la_set_edit_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la_set *set, int64_t first, int64_t count,
                         dh_edit_paths **out);
void dh_edit_paths_destroy(dh_edit_paths *p);
int64_t dh_edit_paths_count(const dh_edit_paths *p);
const int64_t *dh_edit_paths_op_off(const dh_edit_paths *p);    /* count + 1 */
const uint8_t *dh_edit_paths_ops(const dh_edit_paths *p);
const int32_t *dh_edit_paths_score(const dh_edit_paths *p);     /* per LA: sum of its tiles' NW scores */
const int64_t *dh_edit_paths_tile_off(const dh_edit_paths *p);  /* count + 1 */
const uint16_t *dh_edit_paths_tile_score(const dh_edit_paths *p);
int64_t dh_edit_paths_general_tiles(const dh_edit_paths *p);
int64_t dh_format_cigar(const uint8_t *ops, int64_t nops, int32_t extended, char *out, int64_t cap);
int64_t dh_format_alignment(const uint8_t *a, const uint8_t *b, const uint8_t *ops, int64_t nops, int32_t width,
                            char *out, int64_t cap);

/* ---- base-level alignment of whole chains: AlignmentPadder (dazzler.d:2249-2607) over every chain from the start of its
 *      first record to the end of its last.  A chain is the records [chain_off[i], chain_off[i + 1]) (what dh_la_chains_off
 *      and dh_la_chains_to_set produce), or, with chain_off == NULL (nchains is ignored then), read from the flags: a record
 *      without DH_FLAG_NEXT starts a chain and every following DH_FLAG_NEXT record continues it.  The records of a chain
 *      share aread, bread and DH_FLAG_COMP and do not decrease in abpos; DH_FLAG_DISABLED is ignored.
 *      Per chain one op string in dh_la_edit_paths' codes (COMP chains in the reverse-complement frame of B) that consumes
 *      exactly A [abpos of the first record, aepos of the last) and B [bbpos of the first, bepos of the last).  It is the
 *      concatenation of tile runs (a contiguous range of a record's trace tiles, their ops exactly dh_la_edit_paths') and of
 *      fillers between a record p and the next record q: dh_nw_batch's free-shift alignment of an A range against a B range.
 *      Trace points: a record's begin, its tile ends and its end; floor = the last one at or before a position, ceil = the
 *      first one at or behind it, on A or on the trace's running B sum.
 *        gap (p.aepos <= q.abpos and p.bepos <= q.bbpos): p keeps its remaining tiles, the filler is A [p.aepos, q.abpos) x
 *          B [p.bepos, q.bbpos), q starts at its first tile; a filler without bases is no segment.
 *        overlap (getNonOverlappingCoordinates, :2512-2560): on every sequence X that overlaps, begin = p's floor point of
 *          q.Xbpos and end = q's ceil point of p.Xepos; of two the begin with the smaller A and the end with the larger A.  p's
 *          tile run ends at begin, q's starts at end, the filler is A [begin.A, end.A) x B [begin.B, end.B).
 *      status (one entry per chain -- n entries always suffice -- or NULL); the call succeeds in every case:
 *        DH_CP_OK
 *        DH_CP_FAKED   a filler came back DH_NW_BAND_EXCEEDED or exceeds DH_NW_MAX_LEN and was written as the reference's
 *                      "faking too long alignment gap" (:2450-2474): |la - lb| indels (insertions if A is the shorter side),
 *                      then min(la, lb) columns, each 0 or 3 by comparing the bases
 *        DH_CP_NESTED  a junction whose begin lies before the point where p's own tile run starts, or whose end lies before
 *                      its begin on A or on B.  The chain has no ops and score -1.
 *      Deviation: cleanUpLocalAlignments (findTilings, :2354-2394) is not restated -- dh_la_chain's max_relative_overlap
 *      keeps nested records out of its chains, and what still arrives is reported as DH_CP_NESTED, not guessed.
 *      out: a dh_edit_paths of one entry per chain (dh_edit_paths_count; every accessor and both formatters apply): op_off /
 *      ops, score[i] = its number of non-zero ops, tile_off all zero, general_tiles as for dh_la_edit_paths;
 *      dh_edit_paths_fillers = the fillers the global-alignment kernel aligned (0 for results of the other calls),
 *      dh_edit_paths_entry_fillers = how many of them every chain has (one value per chain; NULL for the other calls).
 *      DH_EINVAL, found on the host before anything is launched: whatever dh_la_edit_paths refuses; chain_off not starting
 *      at 0, decreasing or ending past n; an empty chain; a chain whose records differ in aread / bread / COMP or decrease in
 *      abpos (dh_last_error names the record).  No chains is no error and launches nothing. */
#define DH_CP_OK 0
#define DH_CP_FAKED 1
#define DH_CP_NESTED 2
int dh_la_chain_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace,
                      int32_t tspace, const int64_t *chain_off /* nchains + 1, or NULL: by flags */, int64_t nchains,
                      dh_edit_paths **out, int32_t *status /* per chain, or NULL */);
int dh_la_set_chain_paths(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la_set *set, dh_edit_paths **out,
                          int32_t *status); /* by flags */
int64_t dh_edit_paths_fillers(const dh_edit_paths *p);
const int32_t *dh_edit_paths_entry_fillers(const dh_edit_paths *p);

/* ---- exact transposition of local alignments: the records `damapper -C` writes as <B>.<A>.las (dazzler.d:6158-6170,
 *      getLasFile :4339-4354) for alignments that already exist -- the SAME alignments with the roles of the sequences
 *      exchanged, not a second alignment of the transposed pair (dh_align_db_transposed).  Per record, from the ops of
 *      dh_la_edit_paths:
 *        aread', bread'     bread, aread
 *        abpos', aepos'     bbpos, bepos           (COMP: blen - bepos, blen - bbpos)
 *        bbpos', bepos'     abpos, aepos           (COMP: alen - aepos, alen - abpos)
 *        path               the ops with codes 1 and 2 exchanged (COMP: in reverse order as well)
 *        flags              COMP kept; START, NEXT, BEST and DISABLED cleared
 *      The trace lies on the grid of A' (the B read on its forward strand): a tile ends right after the op that brings the
 *      A' position to the next multiple of tspace strictly inside (abpos', aepos'), ops that follow it without advancing
 *      A' belong to the next tile, the last tile takes the rest; a tile is (its non-zero ops, its ops that advance B').
 *      tlen' = 2 x tiles; diffs' = the non-zero ops of the path = dh_edit_paths_score of the source record (it may be
 *      smaller than the source's diffs).
 *      out: a host-resident set of the same tspace with exactly n records in LAsort order (records equal in every key
 *      keep the order of their sources); src_index[i] (n entries, or NULL) = index in las of the source of record i.
 *      want_best != 0: chain flags as on the second set of dh_align_db_transposed (roles exchanged, the context's -n).
 *      A and B may be the same DB.  DH_EINVAL, found on the host before anything is launched: whatever dh_la_edit_paths
 *      refuses, and a record with bepos == bbpos (no A' interval).  DH_EOVERFLOW: a transposed tile whose diffs or bases
 *      do not fit 16 bits (found on the device; dh_last_error names the record). */
int dh_la_transpose(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la *las, int64_t n, const uint16_t *trace,
                    int32_t tspace, int32_t want_best, dh_la_set **out, int64_t *src_index /* n entries or NULL */);
int dh_la_set_transpose(dh_ctx *ctx, dh_db *A, dh_db *B, const dh_la_set *set, int32_t want_best,
                        dh_la_set **out, int64_t *src_index);

/* ---- global alignment of arbitrary sequence pairs: findAlignment(reference, query, indelPenalty = 1, freeShift)
 *      with its traceback (util/string.d:478-520, 775-831) for n pairs of host sequences.  Pair i is
 *      ref[ref_off[i] .. ref_off[i + 1]) against qry[qry_off[i] .. qry_off[i + 1]); two bases match when their bytes are
 *      equal.  free_shift != 0: F[i][0] = F[0][j] = 0; the score is still F[rl][ql] and the traceback still starts at
 *      that corner and pads with deletions, then insertions, at a border.  Ties: diagonal, then insertion, then deletion.
 *      out: a dh_edit_paths of n entries (every accessor and both formatters apply): op_off / ops as for records,
 *      score[i] = F[rl][ql], tile_off all zero, no tile scores, general_tiles = 0.
 *      status (n entries or NULL): DH_NW_OK, or DH_NW_BAND_EXCEEDED for a pair whose alignment cannot be proven exact
 *      inside the widest band the kernel serves (DH_NW_MAX_BAND diagonals; a pair with rl + ql < DH_NW_MAX_BAND always
 *      fits).  Such a pair has score -1 and no ops, the call still succeeds (the reference's AlignmentException, which a
 *      caller catches per alignment).
 *      DH_EINVAL, found on the host before anything is launched: offsets that do not start at >= 0 or decrease, a sequence
 *      longer than DH_NW_MAX_LEN (which bounds the decision scratch of one pair at the widest band to 64 MiB).
 *      A pair with an empty sequence is answered on the host. */
#define DH_NW_OK 0
#define DH_NW_BAND_EXCEEDED 1
#define DH_NW_MAX_LEN 65536
#define DH_NW_MAX_BAND 4096
int dh_nw_batch(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off /* n + 1 */, const uint8_t *qry,
                const int64_t *qry_off /* n + 1 */, int64_t n, int32_t free_shift, dh_edit_paths **out,
                int32_t *status /* n entries or NULL */);

/* ---- global alignment with affine gap costs (Gotoh): what EMBOSS `stretcher` computes for `dentist check-results`
 *      (commands/checkResults.d:1270-1291, 2059-2162), for n pairs of host sequences laid out as for dh_nw_batch.
 *      Scoring: two equal bytes score match, any other pair mismatch; a gap of k bases scores -(gap_open + k gap_extend),
 *      end gaps included.  sc == NULL: {5, -4, 16, 4}, the values EMBOSS documents for nucleotide stretcher (EDNAFULL,
 *      gapopen 16, gapextend 4).  UNPINNED: whether EMBOSS charges open + k ext or open + (k - 1) ext for a gap, and which
 *      of several optimal alignments it reports, could not be checked against its source; the other convention is
 *      {match, mismatch, gap_open - gap_extend, gap_extend}.
 *      Ties: among the sources that attain a cell's value the diagonal, then the insertion, then the deletion, except
 *      that the diagonal yields a tie to a gap state unless its step costs at least a gap base (an equal pair always
 *      yields; an unequal one keeps the tie only if 2 (match - mismatch) >= 2 gap_extend + match, as 18 >= 13 under the
 *      default scoring); inside a gap, closing it wins over extending it.  This is findAlignment's
 *      walk, which moves to the neighbour of the smallest score: with {0, -1, 0, 1} ops and -score are dh_nw_batch's
 *      (free_shift = 0).
 *      out: a dh_edit_paths as dh_nw_batch returns it, score[i] = the alignment score (maximised, signed).
 *      status: DH_NW_OK, or DH_NW_BAND_EXCEEDED (score -1, no ops, the call still succeeds) for a pair whose alignment cannot
 *      be proven exact inside DH_NWA_MAX_BAND diagonals.
 *      DH_EINVAL, found on the host before anything is launched: what dh_nw_batch refuses (with DH_NWA_MAX_LEN), match <
 *      mismatch, 2 gap_extend + match <= 0, gap_open < 0, and values so large that the cost of two sequences of
 *      DH_NWA_MAX_LEN could overflow.  A pair with an empty sequence is answered on the host: one gap.
 *      dh_format_pair (host only) writes the alignment as EMBOSS `pair` text: comment lines (among them "# Identity:
 *      n/m (p%)"), then per block of `width` columns (0: one block) "%-13.13s %6d <bases> %6d" for a, 21 blanks and the
 *      markup ('|' equal, '.' unequal, ' ' gap, as long as the block), the same for b.  Bases print as ACGTN (codes 0..4 or
 *      letters; anything else N), gaps as '-'.  The sizing convention is dh_format_alignment's. */
typedef struct {
    int32_t match, mismatch, gap_open, gap_extend;
} dh_nw_scoring;
#define DH_NWA_MAX_LEN 65536
#define DH_NWA_MAX_BAND 2048
int dh_nw_affine_batch(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off /* n + 1 */, const uint8_t *qry,
                       const int64_t *qry_off /* n + 1 */, int64_t n, const dh_nw_scoring *sc /* NULL: 5,-4,16,4 */,
                       dh_edit_paths **out, int32_t *status /* n entries or NULL */);
int64_t dh_format_pair(const char *name_a, const uint8_t *a, int64_t la, const char *name_b, const uint8_t *b, int64_t lb,
                       const uint8_t *ops, int64_t nops, int32_t score, const dh_nw_scoring *sc /* NULL: the default */,
                       int64_t width, char *out, int64_t cap);

/* ---- exact-match locator: every exact occurrence of every query, and of its reverse complement, in a reference of nref
 *      records -- what the reference's own external/fm-index.cpp answers when `dentist check-results` places the cropped
 *      contigs of the true assembly in the result (commands/checkResults.d:511-565); tools/fm-index is the drop-in.  No
 *      index is built: the reference is packed 2 bits per base, streamed once against a hash table of the queries' first
 *      32 bases, and the candidates are compared word by word.
 *      ref / qry: codes 0..3 (a, c, g, t), one per byte; record i is ref[ref_off[i], ref_off[i + 1]), query j likewise.
 *      The reverse complement of a query is its codes reversed, each replaced by 3 - code.
 *      A hit never spans two records.  Overlapping occurrences are all reported.  An empty query has no hits.
 *      Order of the hits: by query; within a query the forward occurrences (complement 0) first, then, if both_strands,
 *      those of the reverse complement (complement 1) -- a query equal to its own reverse complement is reported twice --
 *      each ascending by (record, begin).  The result is the same from run to run.
 *      begin / end: 0-based, right-open, relative to the record; for complement 1 they are where the reverse complement
 *      lies on the forward reference.
 *      Answered on the host without a launch: nref == 0, nqry == 0, queries longer than the longest record.
 *      DH_EINVAL, found on the host before anything is launched: offsets that start below 0 or decrease, a code above 3,
 *      more than 2^31 - 1 records or queries.  A reference that does not fit the device is an error, never a fallback.
 *      Queries of 1..31 bases cost (reference bases x short queries) compares; contigs are never that short.
 *      Development knobs (tests): DH_LOCATE_SEG (bases per verify unit, default 1 Mi), DH_LOCATE_CAND_CAP (entries of the
 *      candidate buffer, default 1 Mi; an overflowing range is scanned again in halves, nothing is dropped). */
typedef struct { int32_t query, ref; int64_t begin, end; int32_t complement, pad_; } dh_exact_hit;  /* 32 bytes */
typedef struct dh_exact_hits dh_exact_hits;
int dh_exact_locate(dh_ctx *ctx, const uint8_t *ref, const int64_t *ref_off /* nref + 1 */, int64_t nref,
                    const uint8_t *qry, const int64_t *qry_off /* nqry + 1 */, int64_t nqry,
                    int32_t both_strands, dh_exact_hits **out);
void dh_exact_hits_destroy(dh_exact_hits *h);
int64_t dh_exact_hits_count(const dh_exact_hits *h);
const dh_exact_hit *dh_exact_hits_records(const dh_exact_hits *h);

/* ---- chaining of local alignments: chainLocalAlignments / buildAlignmentChains (common/alignments/chaining.d:122-334) with
 *      its ChainingOptions (:78-118) as a call of its own -- what `dentist chain-local-alignments` writes and what
 *      `dentist check-results` runs on the alignments of the result against the true contigs (commands/checkResults.d:
 *      617-624); tools/chain-local-alignments is the drop-in.  Kernels: csrc/dh_chain.hip (one wavefront per pair).
 *   Input.  Records with DISABLED are dropped (chaining.d:130).  The enabled records must be non-decreasing in (aread,
 *      bread) (:132-141); otherwise the call returns DH_EINVAL naming the first offending record, found before any launch.
 *      Both strands of a pair form one group.  START, NEXT and BEST on the input are ignored and cleared: the call is for
 *      unchained input.  Re-chaining a chained file (the reference carries an alternate flag over) is outside the contract.
 *   Per pair.  The nodes are ordered by (abpos, bbpos, input index): a topological order of areChainable (:434-451).  Node
 *      weight is -alignmentScore (:455-461), edge weight is chainScore (:467-475), both in int32 arithmetic.  Relaxation runs
 *      with u ascending and a strict > decides: a later predecessor of equal distance does not replace an earlier one.  The
 *      two overlap tests and both thresholds use double, as the reference does: overlap <= max_relative_overlap * minLength
 *      and (int32_t) max((double) min_score, min_relative_score * best).
 *   Components and selection.  Components are those of the undirected relation (:182).  Per component the end nodes within
 *      that component's threshold are taken best first; ties go to the lower position in the node order; a node already on a
 *      taken chain is no end node.  A chain whose path runs into taken nodes is an alternate chain and consists of its whole
 *      path (:254-287).  The chains scoring at least the pair's threshold are accepted (:307-318).
 *   Output.  Each accepted chain is one contiguous run.  Its first record carries COMP | START, plus BEST unless the chain is
 *      alternate; the other records carry COMP | NEXT (dazzler.d:2046-2082) -- COMP as on the input record, like every flag
 *      bit that is no chain flag.  Pairs come in input order.  Inside a pair chains ascend by (first.abpos, first.bbpos,
 *      last.aepos, last.bepos) (base.d:766-777); remaining ties go to the position of the end node in the node order.  The
 *      reference uses an unstable sort at :241 and :320 and a depth-first topological order; those tie rules are not
 *      properties of the data, ours are the ones oracle/process.py:chain_pile_las documents.
 *   Edge cases.  A pair with no accepted chain emits nothing (the reference would index an empty array there, :308-309; that
 *      cannot happen with min_score = trace spacing and daligner -l500).  n == 0, or everything disabled, returns an empty
 *      result without a launch.  More than 2^31 - 1 output records (or enabled input records) is DH_EOVERFLOW.
 *   Argument checks.  max_relative_overlap outside (0, 1), min_relative_score outside [0, 1], min_score <= 0, or a negative
 *      max_indel / max_chain_gap is DH_EINVAL.
 *   Tiers by enabled records per pair: 1 (a flat kernel, one lane per pair), 2..64 (registers), 65..1536 (LDS), more (a slab
 *      of global memory; never the host).  Development knobs (tests): DH_CHAIN_LDS_NODES lowers the LDS tier's limit,
 *      DH_CHAIN_CHUNK_KB bounds the slab of one launch of the global tier (default 1 GiB; one pair always fits). */
typedef struct dh_chain_opts {          /* ChainingOptions, chaining.d:78-118; 32 bytes */
    int32_t max_indel;                  /* --max-indel, 1000  (commandline.d:1982) */
    int32_t max_chain_gap;              /* --max-chain-gap, 10000 (:1819) */
    int32_t min_score;                  /* --min-score; default = trace spacing (:2165-2173) */
    int32_t pad_;
    double  max_relative_overlap;       /* (0, 1), 0.3 (:2014) */
    double  min_relative_score;         /* [0, 1], 1.0 (:2153) */
} dh_chain_opts;
void dh_default_chain_opts(dh_chain_opts *o, int32_t tspace);

typedef struct dh_la_chains dh_la_chains;
int dh_la_chain(dh_ctx *ctx, const dh_la *las, int64_t n, const dh_chain_opts *o, dh_la_chains **out);
int dh_la_set_chain(dh_ctx *ctx, const dh_la_set *set, const dh_chain_opts *o, dh_la_chains **out);
void dh_la_chains_destroy(dh_la_chains *c);
int64_t dh_la_chains_count(const dh_la_chains *c);              /* chains */
int64_t dh_la_chains_records(const dh_la_chains *c);            /* output records, >= chains */
const int64_t  *dh_la_chains_off(const dh_la_chains *c);        /* count + 1: chain i = output records [off[i], off[i+1]) */
const int32_t  *dh_la_chains_score(const dh_la_chains *c);      /* per chain: -distance of its end node */
const int64_t  *dh_la_chains_src_index(const dh_la_chains *c);  /* per output record: index in las */
const uint32_t *dh_la_chains_flags(const dh_la_chains *c);      /* per output record: the flags it is written with */
int64_t dh_la_chains_big_pairs(const dh_la_chains *c);          /* pairs that took the global-memory tier (tests) */
/* host only: the chained set, records and traces gathered in output order (a shared record's trace is copied per occurrence).
 * trace == NULL: records only (tlen kept, toff 0, no trace values: such a set is not for dh_las_write) */
int dh_la_chains_to_set(const dh_la_chains *c, const dh_la *las, int64_t n, const uint16_t *trace /* or NULL */,
                        int32_t tspace, dh_la_set **out);

/* ---- mask propagation on the device: `dentist propagate-mask` (commands/propagateMask.d:136-305), which the workflow runs
 *      twice per mask and read block over the full mapping (snakemake/Snakefile:1218-1255); tools/propagate-mask is the
 *      drop-in.  Kernels: csrc/dh_pmask.hip.  The result is that of dh_propagate_mask above.
 *   Contract.  For every record and every mask interval of its A sequence that intersects [abpos, aepos): the interval is cut
 *      to [abpos, aepos) (:214-262); its begin is translated with translateTracePoint(floor), its end with (ceil) (:264-293,
 *      base.d:185-203); records with DH_FLAG_COMP mirror it to [blen - e, blen - b) (:295-300); empty results are dropped.
 *      Per destination sequence the result is the union of what is left: sorted, intersecting or touching intervals merged
 *      (:307-313, util/region.d:776-816).  No flag other than COMP matters; the records may come in any order.
 *   Input.  trace_len = entries of `trace`.  mask_ptr[ncontigs + 1] / mask_iv as for dh_propagate_mask; read_off[nreads + 1]
 *      gives the lengths of the destination sequences.  The set form takes records, trace values and tspace from the set; trace
 *      values that dh_map_reads left on the device (want_sorted & 8) are used where they are and are still there afterwards.
 *   Refusals, all DH_EINVAL, never a fault; dh_last_error names the lowest offending record index (the contig for the mask).
 *      Found on the host before anything is launched: aread or bread out of range; abpos < 0 or abpos > aepos; tlen negative,
 *      odd or not 2 * ((aepos + tspace - 1) / tspace - abpos / tspace); toff + tlen behind trace_len; a mask that is not, per
 *      contig, sorted with 0 <= begin < end and begin >= the end before it (touching is allowed, an empty interval is not: the
 *      reference's Region never holds one).  Found by the kernel before anything is painted: a translated position outside
 *      [0, blen], i.e. a trace whose b-bases run past the read.
 *   How.  One bit per destination base; sequence r starts at a bit offset that is a multiple of 32 and is followed by at
 *      least one bit that is never set.  The destination is handled in consecutive ranges of sequences whose bitmap fits
 *      DH_PMASK_BITMAP_MB (default 4096; one sequence always fits); the raw intervals are computed once.  The result does not
 *      depend on the knob, and is the same from run to run.  n == 0, an empty mask and nreads == 0 give an all-zero ptr
 *      without a launch.  Development knob (tests): DH_PMASK_GROUP_RAW bounds the raw intervals of one launch group of
 *      records (default and most 2^31, so that the 32-bit scans of a group cannot wrap; one record always fits). */
typedef struct dh_mask_result dh_mask_result;
int dh_la_propagate_mask(dh_ctx *ctx, const dh_la *las, int64_t n, const uint16_t *trace, int64_t trace_len,
                         int32_t tspace, const int64_t *mask_ptr, const int32_t *mask_iv, int32_t ncontigs,
                         const int64_t *read_off, int32_t nreads, dh_mask_result **out);
int dh_la_set_propagate_mask(dh_ctx *ctx, const dh_la_set *set, const int64_t *mask_ptr, const int32_t *mask_iv,
                             int32_t ncontigs, const int64_t *read_off, int32_t nreads, dh_mask_result **out);
void dh_mask_result_destroy(dh_mask_result *m);
int64_t dh_mask_result_count(const dh_mask_result *m);        /* intervals */
const int64_t *dh_mask_result_ptr(const dh_mask_result *m);   /* nreads + 1 */
const int32_t *dh_mask_result_iv(const dh_mask_result *m);    /* (begin, end) pairs on the forward read */
int64_t dh_mask_result_raw(const dh_mask_result *m);          /* non-empty intervals before the union (tests) */
int64_t dh_mask_result_hit(const dh_mask_result *m);          /* records with an intersecting mask interval */
int32_t dh_mask_result_passes(const dh_mask_result *m);       /* destination ranges (tests) */

/* ---- region validation on the device: `dentist validate-regions` (commands/validateRegions.d:141-512), which the workflow
 *      runs per validation block over the mapping of all reads onto the gap-closed assembly (snakemake/Snakefile:1425-1466);
 *      tools/validate-regions is the drop-in.  Kernels: csrc/dh_vreg.hip.  Reports and weak triples are those of
 *      dh_validate_regions above.
 *   Contract.  For region r = (contig, begin, end): cb = begin > region_context ? begin - region_context : 0 and
 *      ce = min(end + region_context, contig length) (:178-190).  A record of the contig spans the region iff abpos < cb and
 *      ce < aepos (:409-420); num_spanning_reads is their number and their bread values are the region's spanning ids, in
 *      ascending record index.  wlen = min(weak_coverage_window, ce - cb); the windows [w, w + wlen), w = cb .. ce - wlen, are
 *      considered iff wlen > 0 and a record of the contig has abpos < ce && cb < aepos (:458); a record spans a window iff
 *      abpos <= w && w + wlen <= aepos; a window spanned by fewer than min_coverage_reads records is weak.  Weak windows are
 *      intervals, one fused with the one before it when its begin is <= that one's end (:485-498); weak_bp = the sum of the
 *      interval lengths; is_valid = num_spanning_reads >= min_spanning_reads && weak_bp == 0.  The mask is, per contig, the union
 *      of the weak intervals of all regions: sorted, intersecting or touching intervals merged (util/region.d:776-816).
 *      Regions may come in any order, overlap, nest and repeat.
 *   Input.  las: sorted at least by aread; contig_off[ncontigs + 1] gives the contig lengths.  The set form takes the records
 *      of the set.
 *   Refusals, all DH_EINVAL, found on the host before anything is launched, never a fault; dh_last_error names the lowest
 *      offending index: the bad arguments of dh_validate_regions; a contig longer than 2^31 - 1; a record with aread outside
 *      [0, ncontigs), with aread below that of the record before it ("reads-alignment must be sorted at least by a-read ID"),
 *      with abpos < 0, abpos > aepos or aepos behind the end of its contig; a region with contig outside [0, ncontigs),
 *      begin < 0 or end < begin.
 *   How.  One lane per record finds the regions of its contig that it touches (the regions sorted by cb, two binary searches)
 *      and counts; the regions are then handled in launch groups whose pair lists, spanning lists and slab parts fit
 *      DH_VREG_SLAB_MB (default 1024; one region always fits), one workgroup per region.  The result does not depend on the
 *      knob and is the same from run to run.  n == 0 or nregions == 0 give the answer of dh_validate_regions without a launch.
 *      Development knob (tests): DH_VREG_LDS_WINDOWS, the most entries (window starts + 1) of a region whose difference array
 *      stays in LDS (default 8192, at most 16000). */
typedef struct dh_region_result dh_region_result;
int dh_la_validate_regions(dh_ctx *ctx, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                           const dh_region *regions, int32_t nregions, int32_t region_context,
                           int32_t weak_coverage_window, int32_t min_coverage_reads, int32_t min_spanning_reads,
                           dh_region_result **out);
int dh_la_set_validate_regions(dh_ctx *ctx, const dh_la_set *set, const int64_t *contig_off, int32_t ncontigs,
                               const dh_region *regions, int32_t nregions, int32_t region_context,
                               int32_t weak_coverage_window, int32_t min_coverage_reads, int32_t min_spanning_reads,
                               dh_region_result **out);
void dh_region_result_destroy(dh_region_result *r);
int32_t dh_region_result_count(const dh_region_result *r);                    /* regions */
const dh_region_report *dh_region_result_reports(const dh_region_result *r);  /* in input order */
int64_t dh_region_result_weak_count(const dh_region_result *r);               /* weak intervals of all regions */
const int32_t *dh_region_result_weak(const dh_region_result *r);              /* (contig, begin, end) triples in region order */
const int64_t *dh_region_result_span_off(const dh_region_result *r);          /* nregions + 1 */
const int32_t *dh_region_result_span_ids(const dh_region_result *r);          /* bread of the spanning records */
const int64_t *dh_region_result_mask_ptr(const dh_region_result *r);          /* ncontigs + 1 */
const int32_t *dh_region_result_mask_iv(const dh_region_result *r);           /* (begin, end) pairs of the merged mask */
int64_t dh_region_result_mask_count(const dh_region_result *r);               /* intervals of the merged mask */
int64_t dh_region_result_pairs(const dh_region_result *r);        /* (record, region) pairs with abpos < ce && cb < aepos (tests) */
int64_t dh_region_result_big_regions(const dh_region_result *r);  /* regions whose difference array took the slab (tests) */
int64_t dh_region_result_groups(const dh_region_result *r);       /* launch groups (tests) */

/* ---- the alignment filters of `dentist collect` on the device (collectPileUps/filter.d:122-356 in the order of
 *      collectPileUps/package.d:130-141); tools/collect is the drop-in of the command.  Kernels: csrc/dh_cfilt.hip.
 *   Contract.  The result is that of dh_collect_filter above on the same input: DH_FLAG_DISABLED of every record, dropped6 (chains
 *      per stage, not records), read_used[nreads].  A unit is an alignment chain: a record continues the chain of the record
 *      before it iff it has NEXT without START and the same aread, bread and strand.  The unit has the first member's fields,
 *      aepos / bepos of the last, diffs summed, covered = the sum of aepos - abpos over the members, and is disabled on entry iff
 *      a member is; such a unit is skipped by every stage, never counted, and never makes a read ambiguous or redundant.
 *      Per unit, judged by the first stage it fails: LQ iff (int64)diffs * 10^6 > (int64)max_align_err_ppm * covered; Improper
 *      unless (abpos <= allowance || bbpos <= allowance) && (aepos + allowance >= alen || bepos + allowance >= blen);
 *      WeaklyAnchored iff unmasked <= min_anchor, unmasked = the union of the members' A intervals minus the contig's mask (the
 *      members in record order with the host's running `done` position).  Per read, over all units of one bread: Contained -- the
 *      units sorted by (aread, abpos, bbpos, aepos, bepos, place in the input); for every enabled x the units y behind it are
 *      scanned while y has x's aread and x.abpos <= y.abpos && y.aepos <= x.aepos (the first y that does not ends the scan), and
 *      an enabled y of x's strand whose forward read interval lies inside x's is dropped; Ambiguous -- two enabled units whose
 *      forward read intervals intersect drop every unit of the read (counted: those still enabled) and clear read_used;
 *      Redundant -- an enabled unit with bbpos <= abpos && aepos + blen - bepos < alen does the same.  read_used is 1 for every
 *      other read.
 *   Input.  Records in any order in which the members of a chain are consecutive (grouped by read, or LAsort order by contig).
 *      rep_ptr[ncontigs + 1] / rep_iv: the repeat mask (rep_ptr may be NULL: no mask); unlike the host function this one needs
 *      the intervals of a contig sorted and disjoint (touching is allowed), the layout documented for every mask here.
 *      dropped6 and read_used may be NULL.  The first form is in place; the second writes the flags into the set's records
 *      (which must be on the host).
 *   Refusals, made on the host before anything is launched or written (las is untouched): DH_EINVAL "bad argument" for a NULL
 *      pointer, a negative count or opts missing; DH_EINVAL naming the lowest record with aread or bread out of range; DH_EINVAL
 *      naming the lowest contig whose mask is not sorted and disjoint or leaves the contig; DH_EOVERFLOW for 2^30 records or
 *      more.  n == 0 is no error: zeros, read_used all 1, no launch.
 *   How.  One lane per record finds the chain starts, a scan numbers the chains; one lane per chain walks its members (two
 *      binary searches per member into the prefix sums of the mask's interval lengths) and judges stages 1-3; the chains are
 *      grouped by read (histogram, scan, scatter -- for either input order); a read of one unit is one lane's, of 2..64 one
 *      wavefront's (in registers), of up to DH_CFILT_LDS_UNITS one workgroup's with the order of its units in LDS, of more the
 *      same code on a slab of global memory.  No read falls back to the host.  32 bytes per record go up, one byte per record,
 *      one per read and six counts come back.  The result does not depend on the knob and is the same from run to run.
 *      Development knob (tests): DH_CFILT_LDS_UNITS, 64 .. 8192 (default 8192).
 *   Unpinned.  Nothing: every record, count and read_used byte is pinned to dh_collect_filter (tests/test_parity_cfilter_gpu.py),
 *      which tests/test_collect_filters.py pins to the oracle. */
int dh_la_collect_filter(dh_ctx *ctx, dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                         int32_t nreads, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                         int64_t *dropped6, uint8_t *read_used);
int dh_la_set_collect_filter(dh_ctx *ctx, dh_la_set *set, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                             int32_t nreads, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                             int64_t *dropped6, uint8_t *read_used);

/* ---- `dentist mask-repetitive-regions` on the device (commands/maskRepetitiveRegions.d:129-430), from records and lengths to
 *      intervals, without a dh_db; tools/mask-repetitive-regions is the drop-in of the command.  Kernels: csrc/dh_rmask.hip.
 *   Units.  A unit is an alignment chain, as dh_la_collect_filter defines it: a record continues the chain of the record before
 *      it iff it has NEXT without START and the same aread, bread and strand.  Its interval on contig aread is [abpos of its
 *      first record, aepos of its last record): the gaps between the members are covered.  It is proper within `allowance` iff
 *      (abpos <= allowance || bbpos <= allowance) && (aepos + allowance >= alen || bepos + allowance >= blen) with the first
 *      record's begins and the last record's ends (base.d:537-557; the Improper rule of the collect filters).  DH_FLAG_DISABLED
 *      is not looked at.
 *   One assessor (BadAlignmentCoverageAssessor.opCall :344-391) with bounds (lower, upper): cov(c, p) = the counted units of
 *      contig c whose interval contains base p; base p of [0, len(c)) is bad iff cov < lower || cov > upper; the result is the
 *      maximal runs of bad bases per contig -- ascending, disjoint, never touching.  A contig without counted units is one run
 *      [0, len) iff 0 < lower.  An assessor that counts no unit at all gives nothing (:350-351).
 *   The call.  all = the assessor over every unit with (lower, upper); improper = the assessor over the units that are not
 *      proper with (improper_lower, improper_upper), only if with_improper (the reads case :160-180); mask = all | improper, the
 *      ReferenceRegion union: intersecting or touching intervals are merged (util/region.d:776-816).  Without with_improper,
 *      improper is empty and mask = all.
 *   Input.  Records sorted at least by aread with the members of a chain consecutive (LAsort order).  contig_off[ncontigs + 1]
 *      and read_off[nreads + 1] give the lengths; read_off may be NULL iff with_improper == 0.
 *   Refusals, all made on the host before anything is launched, naming the lowest offending index: DH_EINVAL "bad argument" for
 *      a NULL pointer, a negative count or opts missing; DH_EINVAL for lower > upper, improper_lower > improper_upper, a negative
 *      bound or allowance; DH_EINVAL naming the lowest contig longer than 2^31 - 1; DH_EINVAL naming the lowest record with
 *      aread (with_improper: or bread) out of range, aread below the record before it, abpos < 0, abpos > aepos, aepos behind
 *      the contig's end, or that starts a chain whose last aepos lies before its first abpos; DH_EINVAL naming the lowest
 *      contig with more than 2^29 records; DH_EOVERFLOW for 2^30 records or more.  n == 0 is no error: three empty masks, no launch.
 *   How.  Per launch group (whole contigs, as many as DH_RMASK_CHUNK_MB hold; one contig always fits): one lane per record finds
 *      the chain starts, a scan numbers the chains; the lane of a chain start writes two keys position << 2 | is_end << 1 |
 *      improper -- records are grouped by aread, so a contig's keys are consecutive without a partition pass; a contig of up to
 *      64 events is sorted by one wavefront in registers, of up to DH_RMASK_LDS_EVENTS by one workgroup in LDS, of more by the
 *      same network on a slab of global memory, one launch per step over all workgroups; one wavefront per contig walks the sorted keys with two running sums and counts,
 *      then (after a scan) places the runs without atomics; one lane per contig merges the two lists.  No contig falls back to
 *      the host, nothing is sized by bases.  The result does not depend on the knobs and is the same from run to run.
 *      Development knobs (tests): DH_RMASK_LDS_EVENTS, 1024 .. 8192 (default 8192); DH_RMASK_CHUNK_MB, a decimal number of MiB
 *      (default 1024).
 *   Result.  Per mask (mask, all, improper): ptr[ncontigs + 1], (begin, end) pairs, their number.  Counters (tests): units,
 *      improper units (0 without with_improper), contigs per tier (0 no event, 1 wavefront, 2 LDS, 3 global), launch groups.
 *   Unpinned.  Nothing: every interval is pinned to the restatement tests/repeat_ref.py over oracle/maskcov.py
 *      (tests/test_parity_repeat_gpu.py). */
typedef struct dh_repeat_opts {
    int32_t lower, upper, improper_lower, improper_upper, allowance, with_improper;
} dh_repeat_opts;
typedef struct dh_repeat_result dh_repeat_result;
int dh_la_repeat_mask(dh_ctx *ctx, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                      int32_t nreads, const dh_repeat_opts *opts, dh_repeat_result **out);
int dh_la_set_repeat_mask(dh_ctx *ctx, const dh_la_set *set, const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off,
                          int32_t nreads, const dh_repeat_opts *opts, dh_repeat_result **out);
void dh_repeat_result_destroy(dh_repeat_result *r);
const int64_t *dh_repeat_result_mask_ptr(const dh_repeat_result *r);      /* ncontigs + 1 */
const int32_t *dh_repeat_result_mask_iv(const dh_repeat_result *r);       /* (begin, end) pairs */
int64_t dh_repeat_result_mask_count(const dh_repeat_result *r);
const int64_t *dh_repeat_result_all_ptr(const dh_repeat_result *r);
const int32_t *dh_repeat_result_all_iv(const dh_repeat_result *r);
int64_t dh_repeat_result_all_count(const dh_repeat_result *r);
const int64_t *dh_repeat_result_improper_ptr(const dh_repeat_result *r);
const int32_t *dh_repeat_result_improper_iv(const dh_repeat_result *r);
int64_t dh_repeat_result_improper_count(const dh_repeat_result *r);
int64_t dh_repeat_result_units(const dh_repeat_result *r);                /* chains (tests) */
int64_t dh_repeat_result_improper_units(const dh_repeat_result *r);       /* chains that are not proper (tests) */
int64_t dh_repeat_result_tier_contigs(const dh_repeat_result *r, int32_t tier); /* contigs of tier 0..3 (tests) */
int64_t dh_repeat_result_groups(const dh_repeat_result *r);               /* launch groups (tests) */

/* ---- mask algebra on the device: `dentist merge-masks` (commands/mergeMasks.d:47-53), `dentist filter-mask`
 *      (commands/filterMask.d:124-159) and the ReferenceRegion operators | & - (util/region.d:776-1149) as one call;
 *      tools/merge-masks and tools/filter-mask are the drop-ins of the commands.  Kernels: csrc/dh_maskops.hip.
 *   Input.  nmasks >= 1 masks, each as ptr[ncontigs + 1] plus (begin, end) pairs: the layout of dh_dazz_read_mask and of every
 *      mask result of the library.  Within a contig the intervals come in any order and may overlap, nest, touch, repeat or be
 *      empty (begin == end), as the ReferenceRegion constructor takes them.  sub_ptr / sub_iv: the mask to subtract, both NULL
 *      for none.  contig_off[ncontigs + 1] gives the lengths.
 *   Semantics, per contig c and base p of [0, len(c)).  cov(p) = the number of input masks with at least one interval that
 *      contains p: a mask counts once, however many of its intervals have p.  sub(p) = an interval of the subtract mask
 *      contains p.  p is kept iff cov(p) >= min_count && !sub(p).  min_count 1 is |, min_count nmasks is &, the subtract mask -.
 *      The result, in this order: (1) the maximal runs of kept bases, ascending, disjoint, never touching (normalize: intersecting
 *      or touching intervals are merged; empty intervals have no effect); (2) gaps closed as filterMask.d:124-147 does: a run is
 *      joined to the accumulated run before it iff it is on the same contig and acc.end + min_gap >= begin -- a gap of exactly
 *      min_gap is closed, joining cascades; (3) what is shorter than min_interval is dropped (:150-159), a size equal to it stays.
 *      Threshold and subtraction come first, so a closed gap may cover subtracted bases again.
 *   Tandem rule.  dh_la_tandem_mask does what tools/TANmask does on the host: a record counts iff aread == bread and
 *      DH_FLAG_COMP is not set; its interval is [min(abpos, bbpos), max(aepos, bepos)) on read aread - first_read and counts only
 *      if it is at least min_len long (and not empty); the union is taken, touching intervals merged; the result is indexed by
 *      read, read_off[nreads + 1] in the role of contig_off.  The records need no order.
 *   Refusals, all made on the host before anything is launched, naming the lowest offending mask ("subtract mask" for that one),
 *      contig or interval: DH_EINVAL "bad argument" for a NULL pointer, nmasks < 1 or a negative count; DH_EINVAL for
 *      min_count < 1, min_count > nmasks, a negative min_gap or min_interval; a contig longer than 2^31 - 1 or a contig_off that
 *      decreases; a ptr that does not start at 0 or decreases; begin < 0, begin > end, end behind the contig's end; tandem only: a
 *      counted record whose aread lies outside [first_read, first_read + nreads) or whose interval runs past the read's end.
 *      DH_EOVERFLOW for 2^30 intervals (records) or more, or when masks x contigs x the longest contig do not fit a 64-bit key.
 *      No interval at all is no error: an empty set, no launch.
 *   How.  Per launch group (whole contigs, as many as DH_MASKOPS_CHUNK_MB hold; one contig always fits; dh_la_tandem_mask is
 *      one group): one lane per interval writes two 64-bit keys contig << (posbits + 2) | pos << 2 | is_subtract << 1 | is_end
 *      (posbits from the group's longest contig); a device-wide stable LSD radix sort, 8-bit digits, only the digits in use
 *      (histogram per tile, one scan, scatter by a rank from wave ballots -- no atomic decides an order); a device-wide sweep:
 *      two scans give coverage and subtract depth behind every event, the last event of each distinct (contig, pos) is a
 *      boundary, boundaries are compacted, a run begins where kept turns on and ends where it turns off; head flags, a scan and
 *      compaction close the gaps, a size flag, a scan and compaction drop the short runs; one lane per contig finds its first
 *      run by a binary search.  With min_count > 1 every mask is normalised on its own first: the same sort and sweep over
 *      keys with mask * contigs + contig in front, min_count 1, whose runs are the events of the second sweep.  No step is
 *      organised per contig: the cost does not depend on how the intervals are spread over the contigs.  The result does not
 *      depend on the knobs and is the same from run to run.  Development knobs (tests): DH_MASKOPS_TILE_KEYS, 256 .. 2048 keys
 *      per workgroup tile of the sort (default 2048); DH_MASKOPS_CHUNK_MB, a decimal number of MiB (default 1024).
 *   Result.  ptr[ncontigs + 1], (begin, end) pairs, their number.  Counters (tests): events = twice the non-empty intervals
 *      given (subtract mask included); sort_passes = the radix passes run, over all groups and both sorts; launch groups (those
 *      that launched).
 *   Unpinned.  Nothing: every interval is pinned to the restatement tests/maskops_ref.py, which is pinned to the reference's
 *      own unit vectors (tests/golden/region_cases.json). */
typedef struct dh_mask_opts {
    int32_t min_count, min_gap, min_interval, pad_;
} dh_mask_opts;
void dh_default_mask_opts(dh_mask_opts *o); /* 1, 0, 0 */
typedef struct dh_mask_set dh_mask_set;
int dh_mask_combine(dh_ctx *ctx, const int64_t *const *ptr, const int32_t *const *iv, int32_t nmasks, const int64_t *sub_ptr,
                    const int32_t *sub_iv, const int64_t *contig_off, int32_t ncontigs, const dh_mask_opts *opts, dh_mask_set **out);
int dh_la_tandem_mask(dh_ctx *ctx, const dh_la *las, int64_t n, const int64_t *read_off, int32_t nreads, int32_t first_read,
                      int32_t min_len, dh_mask_set **out);
void dh_mask_set_destroy(dh_mask_set *s);
const int64_t *dh_mask_set_ptr(const dh_mask_set *s);      /* ncontigs + 1 */
const int32_t *dh_mask_set_iv(const dh_mask_set *s);       /* (begin, end) pairs */
int64_t dh_mask_set_count(const dh_mask_set *s);
int64_t dh_mask_set_events(const dh_mask_set *s);          /* keys written (tests) */
int64_t dh_mask_set_sort_passes(const dh_mask_set *s);     /* radix passes (tests) */
int64_t dh_mask_set_groups(const dh_mask_set *s);          /* launch groups (tests) */

/* ---- gap analysis of `dentist check-results` on the device (commands/checkResults.d: analyzeGaps :822-907, getGapState and
 *      isGap* :909-982, getInsertionMapping :984-1009, inputGapSize :1037-1046, computeInsertionAlignment :1270-1291,
 *      resultSubseqString :1355-1385, addDustAnalysis :1387-1462, StretcherAlignment.cropReference :1986-2011, the early return
 *      of stretcher :2081-2089): every gap of a batch of input contigs classified, and the inserted sequence of every closed or
 *      partially closed gap aligned to the true one, in one call.  tools/check-results is the drop-in of a subset of the
 *      command.  Kernels: csrc/dh_checkgaps.hip; lane code: csrc/dh_checkgaps.h.
 *   Input.  true_db / result_db: the true assembly and the result (contig c of the reference is sequence c - 1).  mapped: n_input
 *      triples (true contig 1-based or 0, begin, end), the mapped interval of every input contig.  maps: nmaps mappings in any
 *      order, the mappings of the input contigs cropped by `crop` on both sides.  result_gap[c - 1]: the N-run behind result
 *      contig c (0: none).  dust_ptr (true contigs + 1) / dust_iv: the dust mask in the layout of dh_dazz_read_mask, both NULL
 *      for none.  scoring NULL: 5/-4/16/4.  Gap i of the call, 0 <= i < count, lies between input contigs first_contig + i and
 *      first_contig + i + 1 (1-based, so first_contig >= 1; an input contig behind the last has the empty interval).
 *   Output, one dh_gap_summary per gap:
 *      state            the reference's GapState, values 0..5.  DH_GAP_IGNORED unless both mapped intervals lie on the same true
 *                       contig with id > 0; DH_GAP_UNKOWN unless each side has exactly one mapping with duplicate == 0.
 *      gap_length       rhs.begin - lhs.end (0 for an ignored gap);  lhs_map / rhs_map: indices into maps, or -1
 *      align_status     DH_CG_NONE (no attempt: the state is neither closed nor partially closed), DH_CG_OK, DH_CG_EMPTY (a side
 *                       is empty or the query is all n: the reference returns before it runs stretcher), DH_CG_BAND_EXCEEDED
 *                       (dh_nw_affine_batch's), DH_CG_TOO_LONG (a side over DH_NWA_MAX_LEN).  The last two keep the state; no
 *                       alignment is invented.
 *      complement       lhs mapping's; the query was reverse-complemented (n stays n)
 *      true_contig, true_begin, true_end    [lhs.end - crop, rhs.begin + crop) of the true contig
 *      result_begin_contig, result_begin, result_end_contig, result_end    the query: from the end of the left mapping to the
 *                       begin of the right one, both chosen after the complement swap; across two result contigs the left flank,
 *                       result_gap times n (code 4), the right flank
 *      col_begin, col_end   the columns cropReference keeps (crop 0: all); identity = matches / (col_end - col_begin)
 *      reference_length, query_length   crop 0: the bases of both sides (n included); crop > 0: the bases (codes 0..3) inside the
 *                       kept columns -- 0 when there is no alignment, as cropReference of an alignment without lines gives
 *      matches          '|' columns among the kept
 *      dust_ops, dust_matches, none_dust_ops, none_dust_matches   DH_GAP_CLOSED with a dust mask and DH_CG_OK only, else 0
 *      dh_gap_report_paths: a dh_edit_paths of one entry per gap (every accessor and formatter applies) with the uncropped ops
 *      of the DH_CG_OK gaps; score = the alignment score.
 *   Refusals, made on the host before anything is launched, naming the lowest offender: DH_EINVAL "bad argument" for a NULL
 *      pointer, a negative count or crop; first_contig < 1 or first_contig + count - 1 > n_input; a mapped interval with a contig id
 *      out of range, outside its contig, or -- a deviation: the reference's mask would merge them silently -- not behind the
 *      interval before it on the same true contig with at least one base between them; a true interval
 *      [lhs.end - crop, rhs.begin + crop) outside its contig; a mapping with an id out of range, outside its result contig, or
 *      whose ref_contig_length is not the contig's; a dust mask that is not sorted and disjoint or leaves its contig; a scoring
 *      dh_nw_affine_batch refuses.  count == 0: an empty report, no launch.  DH_EOVERFLOW for 2^30 bases of pairs or more is the one
 *      refusal behind a launch: the pair lengths are known once k_cg_bind has run. */
typedef struct {
    int32_t ref_contig, ref_begin, ref_end; /* ContigMapping.reference: result contig (1-based), [begin, end) */
    int32_t ref_contig_length;
    int32_t query_contig;                   /* input contig, 1-based */
    int32_t duplicate, complement;
    float alignment_error;                  /* carried, not read */
} dh_contig_mapping;                        /* 32 bytes */
typedef struct {
    int32_t state, gap_length, lhs_map, rhs_map, align_status, complement;
    int32_t true_contig, true_begin, true_end;
    int32_t result_begin_contig, result_begin, result_end_contig, result_end;
    int32_t col_begin, col_end;
    int32_t reference_length, query_length, matches;
    int32_t dust_ops, dust_matches, none_dust_ops, none_dust_matches;
} dh_gap_summary;                           /* 88 bytes */
#define DH_GAP_UNKOWN 0
#define DH_GAP_BROKEN 1
#define DH_GAP_UNCLOSED 2
#define DH_GAP_PARTIALLY_CLOSED 3
#define DH_GAP_CLOSED 4
#define DH_GAP_IGNORED 5
#define DH_CG_NONE 0
#define DH_CG_OK 1
#define DH_CG_EMPTY 2
#define DH_CG_BAND_EXCEEDED 3
#define DH_CG_TOO_LONG 4
typedef struct dh_gap_report dh_gap_report;
int dh_check_gaps(dh_ctx *ctx, dh_db *true_db, dh_db *result_db, const int32_t *mapped /* 3 x n_input */, int32_t n_input,
                  const dh_contig_mapping *maps, int32_t nmaps, const int32_t *result_gap /* per result contig */,
                  const int64_t *dust_ptr, const int32_t *dust_iv, int32_t crop, const dh_nw_scoring *scoring /* NULL: the default */,
                  int32_t first_contig, int32_t count, dh_gap_report **out);
void dh_gap_report_destroy(dh_gap_report *r);
int64_t dh_gap_report_count(const dh_gap_report *r);
const dh_gap_summary *dh_gap_report_summaries(const dh_gap_report *r);
const dh_edit_paths *dh_gap_report_paths(const dh_gap_report *r); /* owned by the report */
int64_t dh_gap_report_aligned(const dh_gap_report *r);            /* pairs handed to the aligner (tests) */
int64_t dh_gap_report_groups(const dh_gap_report *r);             /* the aligner's launch groups (tests) */

/* ---- gap-closed assembly writer (host only): the linear-scaffold subset of `dentist output`
 *      (source/dentist/commands/output.d:743-925): header "<id>\tscaffold-<first contig id>", contig
 *      slices lower case, insertions upper case (highlight != 0), unclosed gaps as 'n' runs, lines
 *      wrapped at line_width (commandline.d:1699, default 50); optional closed-gaps BED
 *      (output.d:879-891).  scaffold_of[c]: input scaffold of contig c (contigs of a scaffold are
 *      consecutive); headers[s]: its FASTA header without '>'; gap_len[c]: gap after contig c.
 *      Splice coordinates are dh_insertion.left_aepos / right_abpos / ins_begin / ins_end
 *      (common/insertions.d:110-146).  Pinned by the md5 of tests/test-commands.sh:62-65. */
int dh_output_fasta(const char *fasta_path, const char *bed_path, const uint8_t *contig_bases,
                    const int64_t *contig_off, int32_t ncontigs, const int32_t *scaffold_of,
                    const char *const *headers, const int32_t *gap_len, const dh_insertion *ins,
                    int32_t nins, const uint8_t *ins_bases, int32_t line_width, int32_t highlight);
/* `dentist output` with its graph step and all three writers (output.d:305-348 buildAssemblyGraph with
 * enforceJoinPolicy common/scaffold.d:642-723, normalizeUnkownJoins :373-451, fixCropping :931-1003; scaffoldStarts +
 * linearWalk scaffold.d:1021-1295; FASTA :782-925; AGP :454-573; BED :879-891 with every read id of the pile-up) for
 * insertions of any join (dh_insertion.join: gaps between any two contig ends, extensions).  join_policy: 0
 * scaffoldGaps (gap joins that do not sit on a gap of an input scaffold are dropped, *dropped counts them), 1 scaffolds
 * (they come back where both contig ends are still free), 2 contigs (all stay).  agp_dazzler: component ids are contig numbers / "reads-<ids>"; otherwise scaffold header ids and
 * read_names[id - 1]; agp_skip_read_ids: "<n> reads".  read_ids / read_ids_off[nins + 1]: 0-based read ids of
 * every insertion's pile-up, offsets int32 exactly as dh_insertions_read_ids_off returns them (NULL: the reference read
 * alone); nreads = length of read_names, every id is checked against it (-1: unknown, only without a name table). */
typedef struct {
    int32_t line_width, highlight, join_policy, agp_dazzler, agp_skip_read_ids;
    int32_t only;                 /* --only (commandline.d:2230-2250): 1 spanning (default; 0 means the same), 2 extending, 3 both */
    const char *agp_version, *tool, *input_assembly;
    int32_t min_extension_length; /* --min-extension-length (commandline.d:2098-2100, default 100): shorter extensions are skipped */
    int32_t pad;
} dh_output_opts;
void dh_default_output_opts(dh_output_opts *o);
/* Test surface of the writer's graph code (normalizeUnkownJoins common/scaffold.d:373-451, linearWalk :1021-1170,
 * scaffoldStarts :1209-1295 -- the reference's unit vectors run against it): the default edges of `ncontigs` contigs plus
 * joins4 = (contig0, part0, contig1, part1) per join, parts 0 pre, 1 begin, 2 end, 3 post, contigs 0-based; normalize != 0
 * runs normalizeUnkownJoins.  Out (each optional, `cap` entries each): the edges, the scaffold starts as (contig, part), and
 * the linear walk from walk_start2 (through the join walk_first4 when not NULL) as node pairs in walking direction. */
int dh_scaffold_graph_probe(int32_t ncontigs, const int32_t *joins4, int32_t njoins, int32_t normalize, int32_t *edges4,
                            int32_t *nedges, int32_t *starts2, int32_t *nstarts, const int32_t *walk_start2,
                            const int32_t *walk_first4, int32_t *walk4, int32_t *walk_len, int32_t *cyclic, int32_t cap);
int dh_output_assembly(const char *fasta_path, const char *bed_path, const char *agp_path,
                       const uint8_t *contig_bases, const int64_t *contig_off, int32_t ncontigs,
                       const int32_t *scaffold_of, const char *const *headers, const int32_t *gap_len,
                       const dh_insertion *ins, int32_t nins, const uint8_t *ins_bases, const int32_t *read_ids,
                       const int32_t *read_ids_off, int32_t nreads, const char *const *read_names,
                       const dh_output_opts *opts, int32_t *dropped);
/* dh_output_assembly with the FASTA text formatted on the device (dh_outfmt.h, dh_outfmt.hip: every byte of the file is a
 * function of its position; one lane formats 16 consecutive bytes) for contigs that are a dh_db and insertions that are a
 * dh_insertions (of dh_process_pileups or dh_insertions_from_db).  Replaces the host writer's fputc per base
 * (dh_output.cpp LineWriter); AGP and BED stay on the host.  All three files are byte-identical to dh_output_assembly's.
 * fasta_path NULL: stdout.  The other arguments as for dh_output_assembly.  filter (NULL: none) acts on the insertions before
 * the graph is built: an insertion with an overlap whose diffs / covered A bases exceeds max_insertion_error_ppm
 * (ensureHighQualityConsensus, output.d:388-410; averageErrorRate, base.d:695-698) and a gap insertion whose contig pair is
 * listed (removeBlacklisted, scaffold.d:735-768) are left out; they are not counted in *dropped.  The file goes through
 * chunks of DH_OUT_CHUNK_MB (a decimal number of MiB, default 256; a multiple of 16 bytes, at least 64): two device and two
 * page-locked host buffers of that size; the result does not depend on it.  No CPU route: ctx NULL is DH_EINVAL. */
typedef struct {
    int32_t max_insertion_error_ppm;  /* --max-insertion-error, commandline.d:1989-1999 (100 000); <= 0: no cut */
    int32_t nskip;                    /* --skip-gaps / --skip-gaps-file: pairs of 0-based contig ids, first < second */
    const int32_t *skip_gaps2;
} dh_output_filter;
int dh_output_db(dh_ctx *ctx, dh_db *contigs, const char *fasta_path, const char *bed_path, const char *agp_path,
                 const int32_t *scaffold_of, const char *const *headers, const int32_t *gap_len,
                 const dh_insertions *ins, int32_t nreads, const char *const *read_names,
                 const dh_output_opts *opts, const dh_output_filter *filter /* NULL: none */, int32_t *dropped);
/* Test surface of dh_output_db's plan (host only, nothing written): the walk of dh_output_assembly on the same arrays leaves
 * one plan per call -- per FASTA record its header bytes, its byte offset in the file and its body as segments (dh_outfmt.h
 * states the layout).  dh_out_plan_array: which = 0 rec_off, 1 hdr_off, 2 seg_first, 3 seg_base, 4 seg_src (int64), 5 seg_flags
 * (uint32), 6 header bytes; *n = entries.  ins_bases_len bounds the consensus slices. */
typedef struct dh_out_plan dh_out_plan;
int dh_output_plan(const int64_t *contig_off, int32_t ncontigs, const int32_t *scaffold_of, const char *const *headers,
                   const int32_t *gap_len, const dh_insertion *ins, int32_t nins, int64_t ins_bases_len,
                   const dh_output_opts *opts, dh_out_plan **out);
void dh_out_plan_destroy(dh_out_plan *p);
const void *dh_out_plan_array(const dh_out_plan *p, int32_t which, int64_t *n);
/* the last dh_output_db of the context, ms: kernels, copies back, fwrite, the whole formatting (plan upload to last write) */
int dh_get_output_stats(dh_ctx *ctx, double *ms4);

/* ---- DAZZ_DB files on disk (.db / .dam stub + hidden .idx / .bps / .hdr), host only.
 *      Replaces what DENTIST obtains by spawning fasta2DB / fasta2DAM / DBsplit
 *      (source/dentist/dazzler.d:6233-6330) and what the aligners open themselves.  The .idx, .bps
 *      and .hdr images are byte-identical to DAZZ_DB's (pinned by tests/test-commands.sh:54-61). */
typedef struct dh_dazz dh_dazz;
int dh_dazz_create_dam(const char *path, const char *fasta_text, int64_t n); /* fasta2DAM -i */
int dh_dazz_create_db(const char *path, const char *fasta_text, int64_t n);  /* fasta2DB -i  */
int dh_dazz_split(const char *path, int32_t cutoff, int32_t all, int64_t size_mb); /* DBsplit -x -a -s */
/* path may name a block ("reads.3"); the trimmed view is returned (ids are trimmed ids) */
int dh_dazz_open(const char *path, dh_dazz **out);
void dh_dazz_close(dh_dazz *db);
/* ---- sparse packed read loader: selected reads of a DAZZ_DB from disk to the device without the host unpack of dh_dazz_open
 *      (which reads the whole .bps and unpacks it base by base on one host thread; `dentist process --batch` touches a few
 *      thousand reads of a DB with a million, processPileUps/package.d:96-159).  Kernel: csrc/dh_bpsload.hip.
 *   Contract.  ids[n] are ascending, distinct ids of the view dh_dazz_open(db_path) would return (trimmed; a block path is
 *      allowed).  *out is an ungrouped DB of n sequences in that order, the DB dh_db_create would build from the matching
 *      slices of dh_dazz_bases.  n < 1, unsorted ids, duplicate ids and ids outside the view are DH_EINVAL.
 *   How.  Only the stub and the .idx are read whole.  The reads' packed byte ranges [boff, boff + ceil(rlen / 4)) are merged
 *      into runs where they touch in the file; not a byte of the .bps outside the runs is read.  The runs go chunk by chunk
 *      (DH_LOAD_CHUNK_MB packed MiB, a decimal number, default 64, at least one read; the result does not depend on it) through
 *      two page-locked buffers; a chunk is uploaded and unpacked on the context's stream while the next one is read.  The packed
 *      copies and the index of the DB stay lazy, as for any other DB.
 *   dh_get_load_stats: the context's last call -- ms4 = file reads, uploads, kernels, the whole call; counts4 = packed bytes
 *      read, bases written, runs, chunks.
 *   dh_db_get_bases: the bases (codes) of sequences [first, first + count) of any DB, device -> host; cap = bytes of `out`.
 *   dh_db_get_offsets: off[dh_db_nreads + 1] of any DB. */
int dh_dazz_load_reads(dh_ctx *ctx, const char *db_path, const int32_t *ids, int32_t n, dh_db **out);
int dh_get_load_stats(dh_ctx *ctx, double *ms4, int64_t *counts4);
int dh_db_get_bases(dh_db *db, int32_t first, int32_t count, uint8_t *out, int64_t cap);
int dh_db_get_offsets(const dh_db *db, int64_t *off);
int32_t dh_dazz_nreads(const dh_dazz *db);
int32_t dh_dazz_first_id(const dh_dazz *db);         /* trimmed id of the first read of the block */
const uint8_t *dh_dazz_bases(const dh_dazz *db);      /* base codes 0..3, concatenated              */
const int64_t *dh_dazz_offsets(const dh_dazz *db);    /* nreads + 1                                 */
const int32_t *dh_dazz_origin(const dh_dazz *db);     /* well (DB) / contig number in scaffold (DAM)*/
const int32_t *dh_dazz_fpulse(const dh_dazz *db);     /* first pulse (DB) / contig start (DAM)      */
const int32_t *dh_dazz_flags(const dh_dazz *db);      /* DAZZ_READ.flags: low 10 bits = RQ * 1000 (DB) */
const char *dh_dazz_header(const dh_dazz *db, int32_t i); /* DAM: scaffold header of contig i; DB: prolog */
/* mask tracks `<dir>/.<db>.<name>.anno/.data` (source/dentist/dazzler.d:4870-5170): .anno = int32
 * nreads, int32 size (0), int64 byte offsets[nreads + 1]; .data = int32 (begin, end) pairs.
 * read: intervals of the opened (trimmed) view, ptr has nreads + 1 entries; returns the number of
 * intervals or a negative error; iv may be NULL to size.  write: for the whole trimmed DB. */
int64_t dh_dazz_read_mask(const dh_dazz *db, const char *db_path, const char *name, int64_t *ptr, int32_t *iv,
                          int64_t iv_cap);
int dh_dazz_write_mask(const char *db_path, const char *name, int32_t nreads, const int64_t *ptr,
                       const int32_t *iv);
/* track extras (source/dentist/dazzler.d:5173-5344): named vectors of int64 or double stored behind the nreads + 1 pointers
 * of a mask's .anno, any number of them -- int32 vtype (DH_EXTRA_INT64 / DH_EXTRA_DOUBLE), int32 length, int32 accum
 * (DH_ACCUM_EXACT / DH_ACCUM_SUM: how Catrack would combine block tracks), int32 name length, the name without a NUL, `length`
 * values of 8 bytes.  Host only.  No reader of a mask looks behind the pointers; dh_dazz_write_mask truncates the .anno, so
 * rewriting a mask drops its extras (the reference does the same).
 *   read: the first extra called `name`, the ones before it skipped by their lengths.  *vtype on entry is the type asked for
 *      (-1: either), on return the type stored; *accum (may be NULL) the stored mode.  data may be NULL to size, cap counts
 *      elements; returns the element count.  DH_ENOTFOUND: the track has no extra of that name -- no error for a caller to whom
 *      extras are optional.  DH_EINVAL naming the file and the index of the extra: a file that ends inside an extra's header,
 *      name or data, another vtype than the one asked for, an unknown vtype or mode.  DH_EIO: no such track.
 *   write: appends, whatever the file holds already (a second extra of one name is never found by read). */
#define DH_ENOTFOUND (-7)
#define DH_EXTRA_INT64 0
#define DH_EXTRA_DOUBLE 1
#define DH_ACCUM_EXACT 0
#define DH_ACCUM_SUM 1
int64_t dh_dazz_read_extra(const char *db_path, const char *mask, const char *name, int32_t *vtype, int32_t *accum, void *data,
                           int64_t cap);
int dh_dazz_write_extra(const char *db_path, const char *mask, const char *name, int32_t vtype, int32_t accum, const void *data,
                        int64_t n);

/* ---- BED -> mask (host only): `dentist bed2mask` (source/dentist/commands/bed2mask.d:92-287), the intervals of a BED file in
 *      scaffold coordinates as a mask of the contigs of the opened .dam, with the contig pair and the read ids a data comment
 *      (`contigs-<a>-<b>|reads-<id>-<id>...`, column 4 as dh_output_assembly writes it to --closed-gaps-bed) gives every line.
 *   Input.  db: the whole opened .dam; its scaffolds are the runs of contigs under one header with ascending contig numbers,
 *      keyed by the header without '>' up to the first tab, a contig covering [fpulse, fpulse + length) of its scaffold.
 *      bed[n]: the text; bed_name: what messages call it.  data_comments 0: column 4 is not looked at.
 *   Rules.  Empty lines are skipped; columns are split at tabs; columns 2 and 3 are begin and end.  A line gives one interval
 *      per contig of its scaffold left after dropping the leading contigs with end <= begin and the trailing ones with begin >=
 *      end, clipped to the contig and shifted to its coordinates; every interval of a line carries the line's ids.  Data
 *      comment: parts split at '|', fields at '-'; `contigs` needs exactly two ids, `reads` takes any number, other parts are
 *      ignored, a later part of a name overwrites an earlier one; ids are plain decimal digits up to 2^32 - 1.  All errors of a
 *      line come together: "ill-formatted data comment in BED file <name>:<line>:" and one "  - " line each.
 *   Result.  The mask in the layout of dh_dazz_read_mask (ptr[ncontigs + 1], (begin, end) pairs in file order), per interval
 *      the contig-id pair (contig_ids[2 * i], [2 * i + 1]; 0 0 without data comments) and the read ids read_ids[read_off[i] ..
 *      read_off[i + 1]).  Nothing is sorted or merged: the ids are positional.
 *   Refusals beyond the reference, DH_EINVAL naming <name>:<line>: an unknown scaffold, fewer than three columns, a coordinate
 *      that is not a decimal number below 2^31, begin > end, an interval that overlaps no contig, an interval that sorts before
 *      the one in front of it by (contig, begin, end) (the reference sorts the mask but not the ids), and with data_comments a
 *      line without a `contigs` part. */
typedef struct dh_bed_mask dh_bed_mask;
int dh_bed_to_mask(const dh_dazz *db, const char *bed, int64_t n, const char *bed_name, int32_t data_comments, dh_bed_mask **out);
void dh_bed_mask_destroy(dh_bed_mask *m);
int32_t dh_bed_mask_ncontigs(const dh_bed_mask *m);
int64_t dh_bed_mask_count(const dh_bed_mask *m);
const int64_t *dh_bed_mask_ptr(const dh_bed_mask *m);        /* ncontigs + 1 */
const int32_t *dh_bed_mask_iv(const dh_bed_mask *m);         /* 2 x count (never NULL) */
const int64_t *dh_bed_mask_contig_ids(const dh_bed_mask *m); /* 2 x count */
const int64_t *dh_bed_mask_read_off(const dh_bed_mask *m);   /* count + 1 */
const int64_t *dh_bed_mask_read_ids(const dh_bed_mask *m);   /* read_off[count] (never NULL) */

/* ---- the binary containers between DENTIST's commands (host only):
 *      pile-ups.db (collect -> process, source/dentist/common/binio/pileupdb.d:400-897) and
 *      insertions.db (process -> output, binio/insertiondb.d:738-1031), byte-compatible with the D
 *      structs on x86-64.  Flat description used on both sides of the ABI:
 *        dh_seeded    one SeededAlignment: alignment chain (id, contig A = reference contig, contig B =
 *                     read, DENTIST flag bits 1 complement 2 disabled 4 alternateChain 8 chainContinuation
 *                     16 unchained), trace spacing, seed (0 front, 1 back), nla local alignments
 *        dh_chain_la  one LocalAlignment with ntp trace points
 *        tp           (numDiffs, numBasePairs) u16 pairs of all local alignments, in order
 *      pile-ups.db: npiles pile-ups of nra_of_pile[p] read alignments of nsa_of_ra[r] (1 or 2) seeded
 *      alignments.  insertions.db: nins insertions, each with its sequence (codes a,c,g,t = 0..3,
 *      stored 4 per byte as a=0 c=1 t=2 g=3), noverlaps seeded alignments and nread_ids read ids. */
typedef struct {
    int64_t id;
    uint32_t contig_a_id, contig_a_len, contig_b_id, contig_b_len;
    uint8_t flags, seed;
    uint16_t tspace;
    int32_t nla;
} dh_seeded;
typedef struct {
    uint32_t a_begin, a_end, b_begin, b_end, diffs;
    int32_t ntp;
} dh_chain_la;
typedef struct {
    int64_t start_contig, end_contig; /* ContigNode.contigId (1-based contig ids)                         */
    uint8_t start_part, end_part;     /* ContigPart: 0 pre, 1 begin, 2 end, 3 post (scaffold.d:77-90)     */
    uint8_t pad[6];
    int64_t seq_len, contig_len;
    int32_t noverlaps, nread_ids;
} dh_insertion_rec;
typedef struct dh_chaindb dh_chaindb; /* a parsed container, owned by the library */
int dh_pileupdb_write(const char *path, int32_t npiles, const int32_t *nra_of_pile, const int32_t *nsa_of_ra,
                      const dh_seeded *sa, const dh_chain_la *la, const uint16_t *tp);
int dh_pileupdb_read(const char *path, dh_chaindb **out);
int dh_insertiondb_write(const char *path, int32_t nins, const dh_insertion_rec *ins, const uint8_t *bases,
                         const uint32_t *read_ids, const dh_seeded *sa, const dh_chain_la *la, const uint16_t *tp);
int dh_insertiondb_read(const char *path, dh_chaindb **out);
/* `dentist merge-insertions` (commands/mergeInsertions.d:42-164): the insertions.db files of the process batches
 * (snakemake/Snakefile:1315-1334) merged into one file, ordered by (start contig, start part, end contig, end
 * part) like Insertion.opCmp (util/math.d:527-545); an unsorted input is sorted first (:66-72), equal keys keep
 * the order of the inputs (:120-138).  *ntotal (may be NULL) = insertions written. */
int dh_insertiondb_merge(const char *const *paths, int32_t npaths, const char *out_path, int64_t *ntotal);
/* pile-ups.db of a collect result (collectPileUps/package.d:88-96): every read of a pile-up becomes a
 * ReadAlignment of two SeededAlignments (left contig seeded at the back, right contig at the front) */
int dh_pileups_write_db(const dh_pileups *p, const dh_la *las, int64_t n, const uint16_t *trace,
                        const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                        int32_t tspace, const char *path);
/* insertions.db of a process result (processPileUps/package.d:156-158, 789-805): one insertion per
 * closed gap = (left contig, end) -> (right contig, begin), the whole consensus, its two flank overlaps
 * with trace points (tspace = dh_process_opts.tspace_pile) and the sorted 1-based read ids */
int dh_insertions_write_db(const dh_insertions *r, const int64_t *contig_off, int32_t ncontigs, int32_t tspace,
                           const char *path);
/* insertions.db back into the records the writers below take (`dentist output` reads the file the same way, output.d:309-319;
 * inverse of dh_insertions_write_db, dh_insertions.cpp:41-59): for a file of dh_insertions_write_db, of tools/merge-insertions
 * or of the D binary.  contig_left / contig_right / join from the insertion's nodes (makeJoin, base.d:2680-2722); left_aepos /
 * right_abpos = getCroppingPosition!"contigA" (common/insertions.d:110-119: front seed: the FIRST local alignment's A begin, back
 * seed: the LAST one's A end -- an overlap may be a chain); ins_begin / ins_end / comp from getCroppingPosition!"contigB" and
 * getInfoForNewSequenceInsertion (:122-140, :228-284) in the frame the writers expect; left_diffs / right_diffs summed over
 * the chain; the consensus (codes 0..3), the read ids 0-based with their offsets; status = DH_PILE_OK.  DH_EINVAL with a
 * message naming the insertion: a contig id outside [1, ncontigs], a contig_a_len that contradicts contig_off, more than two
 * overlaps, nodes that are neither a gap join nor an extension, a contig_b_len that differs from the sequence length. */
int dh_insertions_from_db(const char *path, const int64_t *contig_off, int32_t ncontigs, dh_insertions **out);
/* pile-ups.db back into pile-ups (`dentist process` reads the file the same way, processPileUps/package.d:96-118; inverse of
 * dh_pileups_write_db): for a file of that function, of tools/collect or of the D binary.  Pile-ups [first, first + count) of the
 * file are taken (count -1: to the end; --batch counts in file order, so the selection comes before any ordering).
 *   Records.  Every SeededAlignment becomes the consecutive records of one chain in *set: aread / bread the 0-based contig_a_id - 1
 *      / contig_b_id - 1, DH_FLAG_COMP from the chain's flag, trace values copied, tspace the file's.  The members of a chain
 *      (nla > 1) follow their first record in file order with the chain flags of a chained .las (first: DH_FLAG_START |
 *      DH_FLAG_BEST, others: DH_FLAG_NEXT; dazzler.d:1728-1758); a chain of one record carries neither.
 *   Pile-ups.  The nodes (contig0, seed0, contig1, seed1) of a pile-up come from its entries with two seeded alignments,
 *      normalised to contig0 < contig1 (the entry's sides are exchanged where needed); a pile-up whose entries all have one is
 *      an extension pile-up; a one-alignment entry of a gap pile-up is matched to its flank by (contig, seed).  Triples are
 *      (read id, index of the chain's first record on flank 0 or -1, the same on flank 1).  *piles is ordered by node, as
 *      dh_pileups_create_joins wants it; (*file_index)[i] (file_index may be NULL; release with dh_shard_free) = where pile-up i
 *      of *piles stood in the file.
 *   DH_EINVAL, the message naming the pile-up's index in the file: entries that disagree about the nodes, a contig joined with
 *      itself, a contig id outside [1, ncontigs], a contig_a_len that contradicts contig_off, a trace that does not sum to the
 *      record's A and B extents (points on the multiples of tspace inside [a_begin, a_end), B parts summing to b_end - b_begin);
 *      also first or count outside the file.  Host only. */
int dh_pileups_from_db(const char *path, int32_t first, int32_t count, const int64_t *contig_off, int32_t ncontigs,
                       dh_pileups **piles, dh_la_set **set, int32_t **file_index);
/* `dentist process --batch` on files (processPileUps/package.d:96-159): dh_pileups_from_db, the sorted distinct read ids of the
 * triples through dh_dazz_load_reads (the reads DB is never opened whole), every contig_b_len checked against the loaded read
 * (DH_EINVAL), read ids renumbered to positions in the sparse DB (a monotone map: every tie broken by read id falls as before),
 * dh_process_pileups_masked with tspace_map = the file's tspace, ref_read_id and dh_insertions_read_ids translated back to ids
 * of the whole DB.  The result is bit-identical to dh_process_pileups_masked on the whole reads DB with the same pile-ups
 * (records in node order).  An empty selection returns an empty result and does not touch the device (ctx may be NULL then).
 * dh_process_pileups_db_batches: the batches of the command (pileUpBatches, commandline.d:1174-1281) as ONE such call -- the
 * pile-ups [ranges2[2 k], ranges2[2 k + 1]) of the file for every k in the order given (an end of -1: the end of the file;
 * ranges that intersect are DH_EINVAL).  only: 0 both, 1 spanning (gap pile-ups), 2 extending (extension pile-ups), applied to
 * the loaded pile-ups first.  sorted != 0: the records in the order of Insertion.opCmp (processPileUps/package.d:156) instead
 * of node order.  *file_index = per record its pile-up's index in the file, *skipped[*nskipped] = the file indices `only` kept
 * out (each may be NULL; release with dh_shard_free). */
int dh_process_pileups_db(dh_ctx *ctx, dh_db *contigs, const char *reads_db_path, const char *pileups_path, int32_t first,
                          int32_t count, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                          dh_insertions **out);
int dh_process_pileups_db_batches(dh_ctx *ctx, dh_db *contigs, const char *reads_db_path, const char *pileups_path,
                                  const int32_t *ranges2, int32_t nranges, const int64_t *rep_ptr, const int32_t *rep_iv,
                                  const dh_process_opts *opts, int32_t only, int32_t sorted, dh_insertions **out,
                                  int32_t **file_index, int32_t **skipped, int32_t *nskipped);
void dh_chaindb_destroy(dh_chaindb *d);
int32_t dh_chaindb_npiles(const dh_chaindb *d);
const int32_t *dh_chaindb_pile_counts(const dh_chaindb *d);
int32_t dh_chaindb_nread_alignments(const dh_chaindb *d);
const int32_t *dh_chaindb_read_alignment_counts(const dh_chaindb *d);
int64_t dh_chaindb_nseeded(const dh_chaindb *d);
const dh_seeded *dh_chaindb_seeded(const dh_chaindb *d);
int64_t dh_chaindb_nlas(const dh_chaindb *d);
const dh_chain_la *dh_chaindb_las(const dh_chaindb *d);
int64_t dh_chaindb_ntrace(const dh_chaindb *d); /* number of u16 values = 2 x trace points */
const uint16_t *dh_chaindb_trace(const dh_chaindb *d);
int32_t dh_chaindb_ninsertions(const dh_chaindb *d);
const dh_insertion_rec *dh_chaindb_insertions(const dh_chaindb *d);
const uint8_t *dh_chaindb_bases(const dh_chaindb *d);
const uint32_t *dh_chaindb_read_ids(const dh_chaindb *d);

/* byte tracks `<dir>/.<db>.<name>.anno/.data` (the `qual` / `inqual` intrinsic-QV tracks DASqv and
 * computeintrinsicqv write and `DBdump -i` shows, dazzler.d:2877-2897, 6142-6183): .anno = int32 nreads,
 * int32 8, int64 byte offsets[nreads + 1]; .data = the bytes (one QV per trace tile).  read: bytes of the
 * opened (trimmed) view, ptr has nreads + 1 entries, data may be NULL to size; returns the byte count. */
int dh_dazz_write_track(const char *db_path, const char *name, int32_t nreads, const int64_t *ptr,
                        const uint8_t *data);
int64_t dh_dazz_read_track(const dh_dazz *db, const char *db_path, const char *name, int64_t *ptr, uint8_t *data,
                           int64_t cap);
/* DBrm (dazzler.d:216, 6115-6119): removes the stub and every hidden file of the DB */
int dh_dazz_remove(const char *db_path);

#ifdef __cplusplus
}
#endif
#endif
