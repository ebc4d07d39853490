// dh_process.h -- what the host files of the pile-up consensus path share (dh_pileups.cpp, dh_tracepoint.cpp, dh_rounds.cpp,
// dh_crop.cpp, dh_batch.cpp, dh_shard.cpp, dh_process.cpp): the two containers behind the C handles, and in namespace dhp
// the trace-point arithmetic of the cropper, the chaining of a pair, the consensus rounds and the small helpers of a
// process call.  What one file alone uses stays in that file.
#ifndef DH_PROCESS_H
#define DH_PROCESS_H

#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "dh_internal.h"

#define SEG_MAX 250 /* B bases of a consensus tile, and the upper limit of a trace spacing, that the vote kernel takes */

// pile-ups of a collector (dh_pileups.cpp)
struct dh_pileups {
    std::vector<int32_t> contig_left;
    std::vector<std::vector<int32_t>> triples;  // read, left LA, right LA
    // general joins (dh_pileups_create_joins): (contig0, seed0, contig1, seed1) per pile-up, contig1 = -1 for an
    // extension pile-up; empty = every pile-up is the gap (contig_left, BACK) -> (contig_left + 1, FRONT)
    std::vector<std::array<int32_t, 4>> join;
    std::array<int32_t, 4> join_of(size_t i) const
    {
        return join.empty() ? std::array<int32_t, 4>{contig_left[i], DH_SEED_BACK, contig_left[i] + 1, DH_SEED_FRONT} : join[i];
    }
};
// DH_EINVAL for pile-ups of general joins, in the name of the entry point `who` (the sharded glue handles plain gaps only)
int dh_refuse_general(const dh_pileups *p, const char *who);

// What `dentist process` holds after cropPileUp (cropper.d:113-175): per pile-up the common trace
// points, per cropped read its pile-up, its position in the pile-up's read list, its read id and
// its bases ([support patch] + read slice + [support patch]).  The bases live on the device
// (`dev`, an ungrouped DB in (pile, entry) order) and/or on the host.
struct dh_cropped {
    dh_ctx *ctx = nullptr;
    std::vector<dh_insertion> rec;
    std::vector<int32_t> pile, entry, read_id;
    std::vector<uint8_t> kind;  // per cropped read, bits 0-1: 0 = alignments on both flanks (spans the gap), 1 = on flank 0 only, 2 = on flank 1 only;
                                // bit 2 / 3: its alignment on flank 0 / 1 is a complement one
    std::vector<int64_t> off{0};
    // page-locked and not zero-filled on resize(): the cropped reads travel device -> host -> (collective) -> host -> device
    // in the sharded path, 21 MB per rank at N = 8
    std::vector<uint8_t, PinnedAlloc<uint8_t>> bases;
    bool host_valid = false;
    bool comp_known = true;  // false: made without kinds (dh_cropped_create): the complement bits are not there
    int32_t batch_most = 0;  // largest pile-up of the batch this crop is a part of (dh_process_pileups splits a batch): the
                             // record slots of the pile-up alignment are sized by it, so that the split does not show
    dh_db *dev = nullptr;
    float ms_crop = 0;
};

namespace dhp {

// ---- dh_tracepoint.cpp
// Alignment chains (base.d:306-421) in the cropper: an entry names the FIRST record of its chain, the members follow it
// (dh_continues_chain).  to!(ReferenceRegion, "contigA") of a chain = the union of its members' A intervals
// (common/package.d:228-241); the common alignment region of a flank = the intersection of the entries' regions.
typedef std::vector<std::pair<int32_t, int32_t>> Region;
void intersect_chain(Region &reg, const dh_la *las, int64_t n, int64_t i);
// the first member of the chain at record i that covers apos (AlignmentChain.translateTracePoint, base.d:866-880)
int64_t covering_member(const dh_la *las, int64_t n, int64_t i, int32_t apos);
// getCommonTracePoint (cropper.d:446-500); mask: sorted disjoint (begin, end) pairs of this contig, nmask of them (may be 0 / NULL)
int32_t common_trace_point(const Region &reg, int32_t contig_len, int32_t ts, bool seed_front, const int32_t *mask = nullptr,
                           int64_t nmask = 0);
// Trace.translateTracePoint!"contigA"(pos, mode), base.d:185-203; translate_floor_b: the B coordinate with mode 0
void translate_trace_point(const dh_la &la, const uint16_t *tr, int32_t ts, int32_t apos, int32_t mode, int32_t *outa,
                           int32_t *outb);
int32_t translate_floor_b(const dh_la &la, const uint16_t *tr, int32_t ts, int32_t apos);
// isValidPileUpAlignment (flat), dazzler.d:4126-4141
bool valid_pileup_alignment(const dh_la &la, bool same, int32_t alen, int32_t blen, int32_t allow);
// chainLocalAlignments on the records [first, last) of one (aread, bread) pair; dups: see the definition
struct ChainDup {
    size_t i;
    uint32_t flags;
};
void chain_pair(LaVec &la, size_t first, size_t last, int32_t min_score, double min_rel_score, std::vector<ChainDup> &dups);

// ---- dh_crop.cpp: one part of a cropped read as k_gather_parts takes it (src 0: the reads DB, 1: the contigs DB)
struct PartDescH {
    int32_t src, sidx, sbeg, len, rc, pad;
    int64_t dst;
};

// ---- dh_process.cpp: times, counters and work of the last process call of a thread (dh_get_process_stats / _work)
struct ProcStats {
    float ms[7] = {0, 0, 0, 0, 0, 0, 0};
    int64_t counters[3] = {0, 0, 0};
    // the work of the call: [0] pile-ups processed, [1] their entries (cropped reads), [2] cropped bases,
    // [3] algorithmic bytes = sum over pile-ups of (n^2 + 2) L, n entries of mean cropped length L
    int64_t work[4] = {0, 0, 0, 0};
};
// this thread's instance: written by dh_process_cropped, copied out by the worker threads of a batch, folded by its driver
ProcStats &dh_proc_stats();

// ---- the guards, the timer and the alignment options of a process call
struct DbGuard {
    std::vector<dh_db *> dbs;
    ~DbGuard()
    {
        for (dh_db *d : dbs) dh_db_destroy(d);
    }
};
struct SetGuard {
    std::vector<dh_la_set *> sets;
    ~SetGuard()
    {
        for (dh_la_set *s : sets) dh_la_set_destroy(s);
    }
};

// The events a dh_process_cropped call times its stages with (0 / 1: around a stage; 2 / 3: the device funnel, inside the
// span of the pile-up alignment) and the DH_TRACE laps of the host's wall clock between the stages.
struct ProcTimer {
    hipStream_t st = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool trace = false;
    double tmark = 0;
    ~ProcTimer()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    static double now_ms()
    {
        return (double)std::chrono::duration_cast<std::chrono::microseconds>(
                   std::chrono::steady_clock::now().time_since_epoch()).count() / 1e3;
    }
    int init(hipStream_t s)
    {
        st = s;
        for (auto &e : ev) HIPCHK(hipEventCreate(&e));
        trace = getenv("DH_TRACE") != nullptr;
        tmark = now_ms();
        return DH_OK;
    }
    hipError_t mark(int i) { return hipEventRecord(ev[i], st); }
    int add_elapsed(int a, int b, float &acc)
    {
        float t = 0;
        HIPCHK(hipEventSynchronize(ev[b]));
        HIPCHK(hipEventElapsedTime(&t, ev[a], ev[b]));
        acc += t;
        return DH_OK;
    }
    void lap(const char *what)
    {
        const double t = now_ms();
        if (trace) fprintf(stderr, "[dh_process] %-28s %.2f ms\n", what, t - tmark);
        tmark = t;
    }
};

// the alignment calls of the pile-up path differ in the shortest overlap and in the record / candidate slots per item
dh_align_opts pile_align_opts(int32_t tspace, int32_t min_len, int32_t max_la, int32_t max_cand);

// ---- dh_rounds.cpp
// One voting + emission round.  T: templates (one per active pile-up), R: pile-up reads.
// las: overlaps with A = a template coordinate system; tmpl_of[i] = template of LA i or -1.
int consensus_round(dh_ctx *ctx, dh_db *T, dh_db *R, const LaVec &las, const TraceVec &trace, const std::vector<int32_t> &tmpl_of,
                    int32_t ts, dh_db **newT, int64_t *nseg_out, int64_t *ncell_out);
// One re-alignment + vote round (see the definition)
int realign_round(dh_ctx *ctx, dh_db *R, const dh_align_opts &ro, const std::vector<uint8_t> *active_ok, DbGuard &dbg, SetGuard &sg,
                  ProcTimer *tm, ProcStats *ps, dh_db **T);

}  // namespace dhp

#endif
