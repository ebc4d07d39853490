// dh_scaffold_blob.cpp -- the join blobs of the sharded collector: every rank turns the alignments of ITS reads into raw
// joins (a per-read computation, dh_shard_read_joins), the joins are all-gathered in rank order (= read order), and every
// rank builds the same scaffold from them (dh_scaffold_from_join_blobs, called by dh_shard_graph_plan_create).
#include <atomic>
#include <cstring>

#include "dh_scaffold.h"
#include "dh_parallel.h"

using namespace dh_scaffold_detail;

namespace {
// blob of the sharded collector (dh_shard_read_joins): JoinHead, then one JoinRec per raw join with copies of the FIRST
// record of the alignment chain of each flank, then the other members of those chains (x0 of flank 0, then x1 of flank 1,
// join by join) -- an entry of a pile-up names the first record of its chain and the cropper finds the members behind it
#pragma pack(push, 1)
struct JoinHead {
    int64_t njoins, nextra;
};
struct JoinRec {
    Node s, e;
    int32_t read;
    uint8_t seed0, seed1, n, pad;
    int32_t x0, x1;  // chain members after the first, per flank
    dh_la la0, la1;  // la1 zeroed for an extension
};
#pragma pack(pop)
static_assert(sizeof(JoinRec) == 32 + 2 * sizeof(dh_la) && sizeof(JoinHead) == 16, "join blob layout");

inline bool well_formed(const JoinRec &j) { return j.x0 >= 0 && j.x1 >= 0 && (j.n == 1 || j.n == 2); }

// one rank's blob, its head checked against its size
struct BlobView {
    const JoinRec *recs;
    const dh_la *extras;
    int64_t njoins, nextra;
};

// where the records of the joins go in the gathered record array: pos0 / pos1 (blob-relative, pos1 = -1 for an extension)
// and the first extra record (xoff) per join, the blobs' first records (nrec, summed up) and separators
struct Layout {
    std::vector<int32_t> pos0, pos1;
    std::vector<int64_t> xoff, nrec;
    std::vector<std::vector<int32_t>> seps;  // where a blob's separator records go (blob-relative)
};
}  // namespace

extern "C" int dh_shard_read_joins(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                                   const int64_t *read_off, int32_t read_first, int32_t nreads, uint8_t **blob, int64_t *nbytes)
{
    if ((n > 0 && !las) || !contig_off || !read_off || !blob || !nbytes || ncontigs < 0 || nreads < 0 || n < 0 || n >= (1ll << 31) ||
        read_first < 0)
        return dh_fail(DH_EINVAL, "dh_shard_read_joins: bad argument");
    // alignment chains are the unit, as in dh_scaffold_pileups: the joins are collected on one pseudo record per chain,
    // the blob carries every member (a read with a long indel next to a gap is cropped through the member that covers
    // the crop point, dh_crop_pileups)
    dh_chain_view cv;
    dh_chain_view_build(las, n, cv);
    const dh_la *u = cv.trivial ? las : cv.unit.data();
    const int64_t nu = cv.trivial ? n : (int64_t)cv.unit.size();
    auto mfirst = [&](int32_t ci) { return cv.trivial ? (int64_t)ci : cv.first[(size_t)ci]; };
    auto mrest = [&](int32_t ci) { return cv.trivial || ci < 0 ? (int64_t)0 : cv.first[(size_t)ci + 1] - cv.first[(size_t)ci] - 1; };  // members after the first
    std::vector<std::vector<RawJoin>> raws;
    if (int rc = collect_raw_joins("dh_shard_read_joins", u, nu, contig_off, ncontigs, read_off, read_first, nreads, &raws)) return rc;
    size_t tot = 0, totx = 0;
    std::vector<size_t> at(raws.size()), atx(raws.size());
    for (size_t i = 0; i < raws.size(); i++) {
        at[i] = tot;
        atx[i] = totx;
        tot += raws[i].size();
        if (!cv.trivial)
            for (const RawJoin &r : raws[i]) totx += (size_t)(mrest(r.ra.la0) + mrest(r.ra.la1));
    }
    const size_t bytes = sizeof(JoinHead) + tot * sizeof(JoinRec) + totx * sizeof(dh_la);
    uint8_t *blk = (uint8_t *)malloc(bytes);
    if (!blk) return dh_fail(DH_EINVAL, "dh_shard_read_joins: out of memory");
    JoinHead *head = (JoinHead *)blk;
    head->njoins = (int64_t)tot;
    head->nextra = (int64_t)totx;
    JoinRec *out = (JoinRec *)(blk + sizeof(JoinHead));
    dh_la *extra = (dh_la *)(blk + sizeof(JoinHead) + tot * sizeof(JoinRec));
    dh_parallel_for((int64_t)raws.size(), 1, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            size_t xat = atx[(size_t)i];
            for (size_t x = 0; x < raws[(size_t)i].size(); x++) {
                const RawJoin &r = raws[(size_t)i][x];
                JoinRec &j = out[at[(size_t)i] + x];
                memset(&j, 0, sizeof(j));  // (la1 of an extension stays zero)
                j.s = r.s;
                j.e = r.e;
                j.read = r.ra.read;
                j.seed0 = r.ra.seed0;
                j.seed1 = r.ra.seed1;
                j.n = r.ra.n;
                j.x0 = (int32_t)mrest(r.ra.la0);
                j.x1 = (int32_t)mrest(r.ra.la1);
                j.la0 = las[mfirst(r.ra.la0)];
                if (r.ra.la1 >= 0) j.la1 = las[mfirst(r.ra.la1)];
                for (int32_t m = 1; m <= j.x0; m++) extra[xat++] = las[mfirst(r.ra.la0) + m];
                for (int32_t m = 1; m <= j.x1; m++) extra[xat++] = las[mfirst(r.ra.la1) + m];
            }
        }
    });
    *blob = blk;
    *nbytes = (int64_t)bytes;
    return DH_OK;
}

namespace {
// the heads of the gathered blobs against their sizes; start[r] = joins in front of blob r
int parse_blobs(const uint8_t *const *blobs, const int64_t *sizes, int32_t world, std::vector<BlobView> &views, std::vector<int64_t> &start)
{
    views.resize((size_t)world);
    start.assign((size_t)world + 1, 0);
    for (int32_t r = 0; r < world; r++) {
        if (sizes[r] < (int64_t)sizeof(JoinHead) || !blobs[r]) return dh_fail(DH_EINVAL, "dh_shard_graph_plan_create: blob size");
        JoinHead h;
        memcpy(&h, blobs[r], sizeof(h));
        if (h.njoins < 0 || h.nextra < 0 || h.njoins > sizes[r] / (int64_t)sizeof(JoinRec) || h.nextra > sizes[r] / (int64_t)sizeof(dh_la) ||
            (int64_t)sizeof(JoinHead) + h.njoins * (int64_t)sizeof(JoinRec) + h.nextra * (int64_t)sizeof(dh_la) != sizes[r])
            return dh_fail(DH_EINVAL, "dh_shard_graph_plan_create: blob size");
        views[(size_t)r] = BlobView{(const JoinRec *)(blobs[r] + sizeof(JoinHead)),
                                    (const dh_la *)(blobs[r] + sizeof(JoinHead) + h.njoins * sizeof(JoinRec)), h.njoins, h.nextra};
        start[(size_t)r + 1] = start[(size_t)r] + h.njoins;
    }
    return DH_OK;
}

// the last record of a blob as the layout places it, nullptr: no joins (or a tail its own pass reports as malformed)
const dh_la *last_record(const BlobView &b)
{
    if (!b.njoins) return nullptr;
    const JoinRec &j = b.recs[b.njoins - 1];
    const int32_t tail = j.n == 2 ? j.x1 : j.x0;
    const int64_t last = j.n == 2 ? b.nextra - 1 : b.nextra - 1 - j.x1;
    if (!well_formed(j) || (tail > 0 && (last < 0 || last >= b.nextra))) return nullptr;
    return tail ? &b.extras[last] : (j.n == 2 ? &j.la1 : &j.la0);
}

// where the records of every join go: the members of a chain behind its first record (la0 chain, then la1 chain).  Two
// copies that would read as one chain (a record flagged NEXT without START behind a copy of its own read on the same
// contig) are kept apart by a separator record that continues nothing.  One host thread per rank's blob lays its
// records out from zero (the record in front of a blob's first one is the last record of the nearest non-empty blob
// before it); the blobs' sizes are then summed up
int lay_out_records(const std::vector<BlobView> &views, const std::vector<int64_t> &start, Layout &lo)
{
    const int32_t world = (int32_t)views.size();
    const size_t tot = (size_t)start[(size_t)world];
    lo.pos0.resize(tot);
    lo.pos1.resize(tot);
    lo.xoff.resize(tot);
    lo.nrec.assign((size_t)world + 1, 0);
    lo.seps.assign((size_t)world, {});
    std::atomic<int> malformed{0};
    dh_parallel_for(world, 1, [&](int64_t rlo, int64_t rhi) {
        auto may_continue = [](const dh_la &x) { return (x.flags & DH_FLAG_NEXT) && !(x.flags & DH_FLAG_START); };
        for (int32_t r = (int32_t)rlo; r < (int32_t)rhi; r++) {
            const BlobView &b = views[(size_t)r];
            const dh_la *prev = nullptr;  // the record that will precede the next one placed
            for (int32_t q = r - 1; q >= 0 && !prev; q--) prev = last_record(views[(size_t)q]);
            int64_t xr = 0, cur = 0;
            int64_t at = start[(size_t)r];
            bool bad = false;
            for (int64_t i = 0; i < b.njoins; i++, at++) {
                const JoinRec &j = b.recs[i];
                if (!well_formed(j) || xr + j.x0 + j.x1 > b.nextra) {
                    bad = true;
                    break;
                }
                lo.xoff[(size_t)at] = xr;
                if (prev && may_continue(j.la0) && dh_continues_chain(*prev, j.la0)) lo.seps[(size_t)r].push_back((int32_t)cur++);
                lo.pos0[(size_t)at] = (int32_t)cur;
                cur += 1 + j.x0;
                prev = j.x0 ? &b.extras[xr + j.x0 - 1] : &j.la0;
                if (j.n == 2) {
                    if (may_continue(j.la1) && dh_continues_chain(*prev, j.la1)) lo.seps[(size_t)r].push_back((int32_t)cur++);
                    lo.pos1[(size_t)at] = (int32_t)cur;
                    cur += 1 + j.x1;
                    prev = j.x1 ? &b.extras[xr + j.x0 + j.x1 - 1] : &j.la1;
                } else
                    lo.pos1[(size_t)at] = -1;
                xr += j.x0 + j.x1;
            }
            if (bad || xr != b.nextra) malformed = 1;
            lo.nrec[(size_t)r + 1] = cur;
        }
    });
    if (malformed) return dh_fail(DH_EINVAL, "dh_shard_graph_plan_create: malformed join record");
    for (int32_t r = 0; r < world; r++) lo.nrec[(size_t)r + 1] += lo.nrec[(size_t)r];
    return DH_OK;
}

// the records of every join into glas and its raw join, which names them, into the runs of the concatenation (rank
// order = read order), as in the single-rank builder
int fill_records(const std::vector<BlobView> &views, const std::vector<int64_t> &start, const Layout &lo, int32_t ncontigs,
                 dh_la_vec &glas, std::vector<std::vector<RawJoin>> &found)
{
    const int64_t tot = start.back(), grain = 4096, nruns = (tot + grain - 1) / grain;
    found.assign((size_t)std::max<int64_t>(nruns, 1), {});
    std::atomic<int> bad{0};
    dh_parallel_for(nruns, 1, [&](int64_t rlo, int64_t rhi) {
        for (int64_t run = rlo; run < rhi; run++) {
            std::vector<RawJoin> &raw = found[(size_t)run];
            const int64_t a0 = run * grain, a1 = std::min(tot, a0 + grain);
            raw.resize((size_t)(a1 - a0));
            int32_t r = (int32_t)(std::upper_bound(start.begin(), start.end(), a0) - start.begin()) - 1;
            for (int64_t at = a0; at < a1; at++) {
                while (at >= start[(size_t)r + 1]) r++;
                const JoinRec &j = views[(size_t)r].recs[at - start[(size_t)r]];
                if (j.s.contig < 0 || j.s.contig >= ncontigs || j.e.contig < 0 || j.e.contig >= ncontigs || j.s.part < 0 || j.s.part > 3 ||
                    j.e.part < 0 || j.e.part > 3)
                    bad = 1;
                const dh_la *x = views[(size_t)r].extras + lo.xoff[(size_t)at];
                const size_t p0 = (size_t)(lo.nrec[(size_t)r] + lo.pos0[(size_t)at]), p1 = j.n == 2 ? (size_t)(lo.nrec[(size_t)r] + lo.pos1[(size_t)at]) : 0;
                glas[p0] = j.la0;
                for (int32_t m = 0; m < j.x0; m++) glas[p0 + 1 + (size_t)m] = x[m];
                if (j.n == 2) {
                    glas[p1] = j.la1;
                    for (int32_t m = 0; m < j.x1; m++) glas[p1 + 1 + (size_t)m] = x[j.x0 + m];
                }
                raw[(size_t)(at - a0)] = RawJoin{j.s, j.e, dh_read_alignment{j.read, (int32_t)p0, j.n == 2 ? (int32_t)p1 : -1, j.seed0, j.seed1, j.n, 0}};
            }
        }
    });
    return bad ? dh_fail(DH_EINVAL, "dh_shard_graph_plan_create: malformed join record") : DH_OK;
}
}  // namespace

int dh_scaffold_from_join_blobs(const uint8_t *const *blobs, const int64_t *sizes, int32_t world, int32_t ncontigs, const int32_t *input_gaps,
                                int32_t ngaps, const dh_scaffold_opts *opts, dh_la_vec &glas, dh_scaffold **out)
{
    if (!blobs || !sizes || world < 1 || !opts || !out || ncontigs < 0 || (ngaps > 0 && !input_gaps) || ngaps < 0)
        return dh_fail(DH_EINVAL, "dh_shard_graph_plan_create: bad argument");
    dh_lap_timer lap{"[scaffold]", 24};
    std::vector<BlobView> views;
    std::vector<int64_t> start;
    if (int rc = parse_blobs(blobs, sizes, world, views, start)) return rc;
    int64_t totx = 0;
    for (const BlobView &b : views) totx += b.nextra;
    if (4 * start.back() + totx >= (1ll << 31)) return dh_fail(DH_EINVAL, "dh_shard_graph_plan_create: too many joins");
    if (int rc = check_input_gaps("dh_shard_graph_plan_create", input_gaps, ngaps, ncontigs)) return rc;
    Layout lo;
    if (int rc = lay_out_records(views, start, lo)) return rc;
    lap("blobs: positions");
    dh_la sep;
    memset(&sep, 0, sizeof(sep));
    sep.aread = sep.bread = -1;
    sep.flags = DH_FLAG_DISABLED;
    glas.resize((size_t)lo.nrec[(size_t)world]);  // (unwritten: every record is stored below, by the thread that touches its page first)
    for (int32_t r = 0; r < world; r++)
        for (int32_t x : lo.seps[(size_t)r]) glas[(size_t)(lo.nrec[(size_t)r] + x)] = sep;
    lap("blobs: records array");
    std::vector<std::vector<RawJoin>> found;
    if (int rc = fill_records(views, start, lo, ncontigs, glas, found)) return rc;
    lap("blobs: records, raw joins");
    return scaffold_from_runs(found, ncontigs, input_gaps, ngaps, opts, out);
}
