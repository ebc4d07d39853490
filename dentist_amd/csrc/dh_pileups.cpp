// dh_pileups.cpp -- the dh_pileups container and what fills it on the host: the spanning-read collector
// (collect_candidates, dh_collect_spanning), the min / max reads cut (select_pile, dh_pileups_select), the creators and
// accessors, pile-ups.db (dh_pileups_write_db), and the re-mapping of the reads of a join that skips contigs
// (dh_remap_skipping_reads: the collector's bubble resolution).
#include <array>
#include <atomic>
#include <cstring>
#include <map>

#include "dh_process.h"
#include "dh_parallel.h"

// ------------------------------------------------------------------------------------ collect

int dh_refuse_general(const dh_pileups *p, const char *who)
{
    return p && !p->join.empty() ? dh_fail(DH_EINVAL, std::string(who) + ": pile-ups of general joins are not handled here") : DH_OK;
}

// Candidates: for every read and every gap the read spans, ONE (read, left LA, right LA) entry --
// the qualifying pair with the longest anchors (ties: lowest LA indices) -- grouped by gap, ordered
// by read id.  No min/max-reads cut yet (the sharded path applies it after the exchange).
static int collect_candidates(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                              const dh_process_opts &o, dh_pileups **out)
{
    if (n >= (1ll << 31)) return dh_fail(DH_EINVAL, "dh_collect_spanning: more than 2^31 - 1 local alignments");
    // the enabled LAs (dh_collect_filter leaves most of a mapping disabled) as (read, LA index), listed
    // by the host threads over runs of the input and grouped by read with a counting sort that keeps
    // the LA order inside a read
    const int64_t lgrain = 1 << 16, lchunks = (n + lgrain - 1) / lgrain;
    std::vector<std::vector<std::pair<int32_t, int32_t>>> live((size_t)std::max<int64_t>(lchunks, 1));
    std::atomic<int> bad{0};
    dh_parallel_for(lchunks, 1, [&](int64_t clo, int64_t chi) {
        for (int64_t c = clo; c < chi; c++) {
            auto &v = live[(size_t)c];
            const int64_t i1 = std::min(n, (c + 1) * lgrain);
            for (int64_t i = c * lgrain; i < i1; i++) {
                if (las[i].bread < 0 || las[i].aread < 0 || las[i].aread >= ncontigs) bad = 1;
                else if (!(las[i].flags & DH_FLAG_DISABLED)) v.emplace_back(las[i].bread, (int32_t)i);
            }
        }
    });
    if (bad) return dh_fail(DH_EINVAL, "dh_collect_spanning: read or contig id out of range");
    int32_t nreads = 0;
    int64_t nlive = 0;
    for (const auto &v : live) {
        nlive += (int64_t)v.size();
        for (const auto &e : v) nreads = std::max(nreads, e.first + 1);
    }
    std::vector<int64_t> first((size_t)nreads + 1, 0), order((size_t)nlive);
    for (const auto &v : live)
        for (const auto &e : v) first[(size_t)e.first + 1]++;
    for (int32_t r = 0; r < nreads; r++) first[(size_t)r + 1] += first[(size_t)r];
    {
        std::vector<int64_t> cur(first.begin(), first.end() - 1);
        for (const auto &v : live)
            for (const auto &e : v) order[(size_t)cur[(size_t)e.first]++] = e.second;
    }
    live.clear();
    // reads are independent: host threads take runs of reads and list their entries (gap, read, iL,
    // iR) in read order; the runs are concatenated in order and split by gap afterwards
    struct Ent {
        int32_t gap, rd, iL, iR;
    };
    const int64_t grain = 16384, nchunks = ((int64_t)nreads + grain - 1) / grain;
    std::vector<std::vector<Ent>> found((size_t)std::max<int64_t>(nchunks, 1));
    dh_parallel_for(nchunks, 1, [&](int64_t clo, int64_t chi) {
        for (int64_t c = clo; c < chi; c++) {
            std::vector<Ent> &out_c = found[(size_t)c];
            const int32_t r1 = (int32_t)std::min<int64_t>(nreads, (c + 1) * grain);
            std::vector<std::pair<int32_t, std::pair<int64_t, std::pair<int64_t, int64_t>>>> best;  // gap -> (anchors, (iL, iR))
            for (int32_t rd = (int32_t)(c * grain); rd < r1; rd++) {
                const int64_t *idx = order.data() + first[(size_t)rd], cnt = first[(size_t)rd + 1] - first[(size_t)rd];
                if (cnt < 2) continue;
                best.clear();
                for (int64_t x = 0; x < cnt; x++) {
                    const int64_t iL = idx[x];
                    const dh_la &L = las[iL];
                    if (L.flags & DH_FLAG_DISABLED) continue;  // dropped by dh_collect_filter
                    if (L.aread + 1 >= ncontigs) continue;
                    const int64_t cl = contig_off[L.aread + 1] - contig_off[L.aread];
                    if (L.aepos + o.allowance < cl || L.aepos - L.abpos < o.min_anchor) continue;
                    for (int64_t y = 0; y < cnt; y++) {
                        const int64_t iR = idx[y];
                        const dh_la &R = las[iR];
                        if (R.flags & DH_FLAG_DISABLED) continue;
                        if (R.aread != L.aread + 1 || (R.flags & DH_FLAG_COMP) != (L.flags & DH_FLAG_COMP)) continue;
                        if (R.abpos > o.allowance || R.aepos - R.abpos < o.min_anchor) continue;
                        if (R.bbpos + o.allowance < L.bepos - o.allowance) continue;
                        const int64_t anchors = (int64_t)(L.aepos - L.abpos) + (R.aepos - R.abpos);
                        size_t k = 0;
                        while (k < best.size() && best[k].first != L.aread) k++;
                        if (k == best.size()) best.push_back(std::make_pair(L.aread, std::make_pair((int64_t)-1, std::make_pair(iL, iR))));
                        if (anchors > best[k].second.first) best[k].second = std::make_pair(anchors, std::make_pair(iL, iR));
                    }
                }
                for (auto &b : best)
                    out_c.push_back(Ent{b.first, rd, (int32_t)b.second.second.first, (int32_t)b.second.second.second});
            }
        }
    });
    std::map<int32_t, std::vector<int32_t>> piles;
    for (const std::vector<Ent> &v : found)
        for (const Ent &e : v) {
            std::vector<int32_t> &t = piles[e.gap];
            t.push_back(e.rd);
            t.push_back(e.iL);
            t.push_back(e.iR);
        }
    dh_pileups *p = new dh_pileups();
    for (auto &kv : piles) {
        p->contig_left.push_back(kv.first);
        p->triples.push_back(std::move(kv.second));
    }
    *out = p;
    return DH_OK;
}

// min-reads / max-reads cut of one candidate list (ordered by read id): fewer than min_reads
// distinct reads -> dropped; more than max_reads -> the max_reads entries with the lowest error
// rate of their two anchoring LAs stay (ties: lower read id), still ordered by read id.
static bool select_pile(std::vector<int32_t> &v, const dh_la *las, const dh_process_opts &o)
{
    const int32_t cnt = (int32_t)v.size() / 3;
    if (cnt < o.min_reads) return false;
    if (o.max_reads <= 0 || cnt <= o.max_reads) return true;  // max_reads 0 = no cap (the reference has none)
    // key = (class, error rate, entry); class = 2 x (extension entry) + (a further entry of its read).  A spanning read that opens with an extension enters the
    // pile-up as TWO extension entries (pileups.d:870) cropped from the same bases -- read[cropL, end) and read[0, cropR)
    // overlap in the gap -- so both of them in the vote count that read's errors twice.  With more entries than the cap
    // there are enough distinct reads: a read's second entry is considered only after every read's best one
    // (configs[2]: consensus error 0.091 % -> the spanning collector's level with the same 60 entries).
    std::vector<std::array<int64_t, 3>> key((size_t)cnt);
    for (int32_t e = 0; e < cnt; e++) {
        // an extension entry (one index is -1) is judged by the one alignment it has
        const int32_t iL = v[(size_t)e * 3 + 1], iR = v[(size_t)e * 3 + 2];
        int64_t len = 0, diffs = 0;
        if (iL >= 0) {
            len += las[iL].aepos - las[iL].abpos;
            diffs += las[iL].diffs;
        }
        if (iR >= 0) {
            len += las[iR].aepos - las[iR].abpos;
            diffs += las[iR].diffs;
        }
        key[(size_t)e] = {0, diffs * 1000000 / std::max<int64_t>(len, 1), e};
    }
    for (int32_t e = 0; e < cnt;) {  // entries of one read are adjacent: all but its best one rank behind
        int32_t f = e + 1, best = e;
        while (f < cnt && v[(size_t)f * 3] == v[(size_t)e * 3]) f++;
        for (int32_t x = e + 1; x < f; x++)
            if (key[(size_t)x][1] < key[(size_t)best][1]) best = x;
        for (int32_t x = e; x < f; x++) key[(size_t)x][0] = x == best ? 0 : 1;
        // ... and an extension entry (it covers the gap as far as its read goes) only after the reads that span the gap
        for (int32_t x = e; x < f; x++)
            if (v[(size_t)x * 3 + 1] < 0 || v[(size_t)x * 3 + 2] < 0) key[(size_t)x][0] += 2;
        e = f;
    }
    std::sort(key.begin(), key.end());  // entries are in read-id order, so e breaks ties by read id
    std::vector<int32_t> keep((size_t)o.max_reads);
    for (int32_t x = 0; x < o.max_reads; x++) keep[(size_t)x] = (int32_t)key[(size_t)x][2];
    std::sort(keep.begin(), keep.end());
    std::vector<int32_t> w;
    w.reserve((size_t)o.max_reads * 3);
    for (int32_t e : keep) w.insert(w.end(), v.begin() + (size_t)e * 3, v.begin() + (size_t)e * 3 + 3);
    v.swap(w);
    return true;
}

extern "C" int dh_collect_candidates(const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                                     const dh_process_opts *opts, dh_pileups **out)
{
    if ((n > 0 && !las) || !contig_off || !opts || !out || ncontigs < 0)
        return dh_fail(DH_EINVAL, "dh_collect_candidates: bad argument");
    return collect_candidates(las, n, contig_off, ncontigs, *opts, out);
}

extern "C" int dh_pileups_select(const dh_pileups *cands, const dh_la *las, int64_t n,
                                 const dh_process_opts *opts, dh_pileups **out)
{
    if (!cands || !opts || !out || (n > 0 && !las)) return dh_fail(DH_EINVAL, "dh_pileups_select: bad argument");
    // pile-ups are independent (the cut reads the anchoring LAs: cache misses into the mapping's records)
    const size_t np = cands->contig_left.size();
    std::vector<std::vector<int32_t>> sel(np);
    std::vector<char> keep(np, 0);
    std::atomic<int> bad{0};
    dh_parallel_for((int64_t)np, 4, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            std::vector<int32_t> v = cands->triples[(size_t)i];
            bool ok = true;
            for (size_t e = 0; e < v.size() && ok; e += 3)  // -1 = no alignment on that side (extension entry)
                ok = v[e + 1] >= -1 && v[e + 1] < n && v[e + 2] >= -1 && v[e + 2] < n && (v[e + 1] >= 0 || v[e + 2] >= 0);
            if (!ok) {
                bad = 1;
                continue;
            }
            if (!select_pile(v, las, *opts)) continue;
            keep[(size_t)i] = 1;
            sel[(size_t)i] = std::move(v);
        }
    });
    if (bad) return dh_fail(DH_EINVAL, "dh_pileups_select: LA index out of range");
    dh_pileups *p = new dh_pileups();
    for (size_t i = 0; i < np; i++)
        if (keep[i]) {
            p->contig_left.push_back(cands->contig_left[i]);
            if (!cands->join.empty()) p->join.push_back(cands->join[i]);
            p->triples.push_back(std::move(sel[i]));
        }
    *out = p;
    return DH_OK;
}

// internal helpers of dh_map_reads: LA indices shifted by a constant; pile-ups of several parts (ascending
// read ranges) concatenated gap by gap
void dh_pileups_shift(dh_pileups *p, int32_t by)
{
    for (auto &t : p->triples)
        for (size_t e = 0; e + 2 < t.size(); e += 3) {
            if (t[e + 1] >= 0) t[e + 1] += by;
            if (t[e + 2] >= 0) t[e + 2] += by;
        }
}
int dh_pileups_concat(dh_pileups *const *parts, int32_t nparts, dh_pileups **out)
{
    for (int32_t i = 0; i < nparts; i++)
        if (int rc = dh_refuse_general(parts[i], "dh_pileups_concat")) return rc;
    std::map<int32_t, std::vector<int32_t>> m;
    for (int32_t i = 0; i < nparts; i++) {
        if (!parts[i]) continue;
        for (size_t g = 0; g < parts[i]->contig_left.size(); g++) {
            std::vector<int32_t> &t = m[parts[i]->contig_left[g]];
            t.insert(t.end(), parts[i]->triples[g].begin(), parts[i]->triples[g].end());
        }
    }
    dh_pileups *p = new dh_pileups();
    for (auto &kv : m) {
        p->contig_left.push_back(kv.first);
        p->triples.push_back(std::move(kv.second));
    }
    *out = p;
    return DH_OK;
}

extern "C" int dh_pileups_create(const int32_t *contig_left, const int32_t *count, int32_t npiles,
                                 const int32_t *triples, dh_pileups **out)
{
    if (npiles < 0 || !out || (npiles > 0 && (!contig_left || !count || !triples)))
        return dh_fail(DH_EINVAL, "dh_pileups_create: bad argument");
    dh_pileups *p = new dh_pileups();
    int64_t at = 0;
    for (int32_t i = 0; i < npiles; i++) {
        if (count[i] < 0 || contig_left[i] < 0 || (i > 0 && contig_left[i] <= contig_left[i - 1])) {
            delete p;
            return dh_fail(DH_EINVAL, "dh_pileups_create: pile-ups must be ordered by contig and counts >= 0");
        }
        p->contig_left.push_back(contig_left[i]);
        p->triples.emplace_back(triples + at * 3, triples + (at + count[i]) * 3);
        at += count[i];
    }
    *out = p;
    return DH_OK;
}

extern "C" int dh_pileups_create_joins(const int32_t *nodes4, const int32_t *count, int32_t npiles, const int32_t *triples,
                                       dh_pileups **out)
{
    if (npiles < 0 || !out || (npiles > 0 && (!nodes4 || !count || !triples)))
        return dh_fail(DH_EINVAL, "dh_pileups_create_joins: bad argument");
    dh_pileups *p = new dh_pileups();
    int64_t at = 0;
    for (int32_t i = 0; i < npiles; i++) {
        const int32_t *q = nodes4 + 4 * (size_t)i;
        const bool ext = q[2] < 0;
        // node order of the scaffold graph: (contig, part) with begin < end, i.e. seed front < seed back
        auto key = [](const int32_t *x) { return std::array<int64_t, 4>{x[0], x[1], x[2] < 0 ? INT32_MAX : x[2], x[3]}; };
        if (count[i] < 0 || q[0] < 0 || (q[1] != DH_SEED_FRONT && q[1] != DH_SEED_BACK) || (!ext && (q[3] != DH_SEED_FRONT && q[3] != DH_SEED_BACK)) ||
            (!ext && q[2] <= q[0]) || (i > 0 && !(key(q - 4) < key(q)))) {
            delete p;
            return dh_fail(DH_EINVAL, "dh_pileups_create_joins: joins must be ordered by their nodes, contig0 < contig1, seeds 0 / 1, counts >= 0");
        }
        p->contig_left.push_back(q[0]);
        p->join.push_back({q[0], q[1], ext ? -1 : q[2], ext ? 0 : q[3]});
        p->triples.emplace_back(triples + at * 3, triples + (at + count[i]) * 3);
        at += count[i];
    }
    *out = p;
    return DH_OK;
}

extern "C" int dh_pileups_get_join(const dh_pileups *p, int32_t i, int32_t *nodes4)
{
    if (!p || !nodes4 || i < 0 || i >= (int32_t)p->contig_left.size()) return dh_fail(DH_EINVAL, "dh_pileups_get_join: bad argument");
    const std::array<int32_t, 4> j = p->join_of((size_t)i);
    memcpy(nodes4, j.data(), sizeof(int32_t) * 4);
    return DH_OK;
}

extern "C" int dh_collect_spanning(const dh_la *las, int64_t n, const int64_t *contig_off,
                                   int32_t ncontigs, const dh_process_opts *opts, dh_pileups **out)
{
    if ((n > 0 && !las) || !contig_off || !opts || !out || ncontigs < 0)
        return dh_fail(DH_EINVAL, "dh_collect_spanning: bad argument");
    dh_pileups *c = nullptr;
    if (int rc = collect_candidates(las, n, contig_off, ncontigs, *opts, &c)) return rc;
    const int rc = dh_pileups_select(c, las, n, opts, out);
    delete c;
    return rc;
}

// pile-ups.db of a collect result (what `dentist collect` hands to `dentist process`,
// collectPileUps/package.d:88-96 writePileUpsDb): every read of a pile-up is a ReadAlignment of two
// SeededAlignments -- its chain on the left contig seeded at the back, its chain on the right contig
// seeded at the front (pileups.d:821-888); chains hold one local alignment with its trace points.
extern "C" int dh_pileups_write_db(const dh_pileups *p, const dh_la *las, int64_t n, const uint16_t *trace,
                                   const int64_t *contig_off, int32_t ncontigs, const int64_t *read_off, int32_t nreads,
                                   int32_t tspace, const char *path)
{
    if (!p || !contig_off || !read_off || !path || (n > 0 && (!las || !trace)))
        return dh_fail(DH_EINVAL, "dh_pileups_write_db: bad argument");
    std::vector<int32_t> nra, nsa;
    std::vector<dh_seeded> sa;
    std::vector<dh_chain_la> la;
    std::vector<uint16_t> tp;
    for (size_t i = 0; i < p->contig_left.size(); i++) {
        const std::vector<int32_t> &t = p->triples[i];
        const std::array<int32_t, 4> jn = p->join_of(i);
        nra.push_back((int32_t)t.size() / 3);
        for (size_t e = 0; e + 2 < t.size(); e += 3) {
            nsa.push_back((t[e + 1] >= 0 ? 1 : 0) + (t[e + 2] >= 0 ? 1 : 0));
            for (int side = 0; side < 2; side++) {
                const int32_t li = t[e + 1 + (size_t)side];
                if (li == -1 && t[e + 2 - (size_t)side] >= 0) continue;  // extension entry: one seeded alignment
                if (li < 0 || li >= n) return dh_fail(DH_EINVAL, "dh_pileups_write_db: LA index out of range");
                const dh_la &x = las[li];
                if (x.aread < 0 || x.aread >= ncontigs || x.bread < 0 || x.bread >= nreads)
                    return dh_fail(DH_EINVAL, "dh_pileups_write_db: id out of range");
                dh_seeded s;
                memset(&s, 0, sizeof(s));
                s.id = li;
                s.contig_a_id = (uint32_t)(x.aread + 1);
                s.contig_a_len = (uint32_t)(contig_off[x.aread + 1] - contig_off[x.aread]);
                s.contig_b_id = (uint32_t)(x.bread + 1);
                s.contig_b_len = (uint32_t)(read_off[x.bread + 1] - read_off[x.bread]);
                s.flags = (x.flags & DH_FLAG_COMP) ? 1 : 0;
                s.seed = (uint8_t)jn[1 + 2 * (size_t)side];  // AlignmentLocationSeed of the flank (plain gap: back, front)
                s.tspace = (uint16_t)tspace;
                s.nla = 1;
                sa.push_back(s);
                la.push_back(dh_chain_la{(uint32_t)x.abpos, (uint32_t)x.aepos, (uint32_t)x.bbpos, (uint32_t)x.bepos,
                                         (uint32_t)x.diffs, x.tlen / 2});
                tp.insert(tp.end(), trace + x.toff, trace + x.toff + x.tlen);
            }
        }
    }
    return dh_pileupdb_write(path, (int32_t)nra.size(), nra.data(), nsa.data(), sa.data(), la.data(), tp.data());
}

// all pile-ups at once: contig_left[npiles], count[npiles], triples[3 * total]; arrays may be NULL to
// size; returns the total number of triples
extern "C" int64_t dh_pileups_flat(const dh_pileups *p, int32_t *contig_left, int32_t *count, int32_t *triples)
{
    if (!p) return 0;
    int64_t at = 0;
    for (size_t i = 0; i < p->contig_left.size(); i++) {
        const std::vector<int32_t> &t = p->triples[i];
        if (contig_left) contig_left[i] = p->contig_left[i];
        if (count) count[i] = (int32_t)t.size() / 3;
        if (triples && !t.empty()) memcpy(triples + 3 * at, t.data(), sizeof(int32_t) * t.size());
        at += (int64_t)t.size() / 3;
    }
    return at;
}

extern "C" void dh_pileups_destroy(dh_pileups *p) { delete p; }
extern "C" int32_t dh_pileups_count(const dh_pileups *p) { return p ? (int32_t)p->contig_left.size() : 0; }
extern "C" int32_t dh_pileups_get(const dh_pileups *p, int32_t i, int32_t *contig_left,
                                  const int32_t **triples)
{
    if (!p || i < 0 || i >= (int32_t)p->contig_left.size()) return -1;
    if (contig_left) *contig_left = p->contig_left[(size_t)i];
    if (triples) *triples = p->triples[(size_t)i].data();
    return (int32_t)p->triples[(size_t)i].size() / 3;
}

// ------------------------------------------------------------------------------------ bubbles
// getReadAlignmentsOnContigs of `resolveBubbles` (collectPileUps/pileups.d:1316-1385): the reads of a pile-up whose
// join skips contigs are mapped again, without any mask, onto just those intermediate contigs (the reference builds
// two DB subsets and spawns damapper on them, :1337-1366); chains that do not cover their contig completely within
// `allowance` (AlignmentChain.completelyCovers!"contigA", common/alignments/base.d:562-566) are disabled, ids are
// those of the full DBs again (:1373-1380).  The graph surgery around it (BubbleResolver) stays with the caller.
extern "C" int dh_remap_skipping_reads(dh_ctx *ctx, dh_db *contigs, dh_db *reads, const int32_t *contig_ids, int32_t ncontig_ids,
                                       const int32_t *read_ids, int32_t nread_ids, const dh_align_opts *opts, int32_t allowance,
                                       dh_la_set **out)
{
    if (!ctx || !contigs || !reads || !contig_ids || !read_ids || !opts || !out || ncontig_ids < 1 || nread_ids < 1 || allowance < 0)
        return dh_fail(DH_EINVAL, "dh_remap_skipping_reads: bad argument");
    auto subset = [&](dh_db *src, const int32_t *ids, int32_t n, dh_db **sub) -> int {
        std::vector<int32_t> sidx((size_t)n), sbeg((size_t)n, 0), slen((size_t)n);
        for (int32_t i = 0; i < n; i++) {
            if (ids[i] < 0 || ids[i] >= src->n || (i > 0 && ids[i] <= ids[i - 1]))
                return dh_fail(DH_EINVAL, "dh_remap_skipping_reads: ids must be ascending, distinct and inside the DB");
            sidx[(size_t)i] = ids[i];
            slen[(size_t)i] = (int32_t)(src->h_off[(size_t)ids[i] + 1] - src->h_off[(size_t)ids[i]]);
        }
        return dh_db_from_slices(ctx, src, sidx, sbeg, slen, {}, sub);  // no mask: "align without any mask"
    };
    dh_db *sa = nullptr, *sb = nullptr;
    if (int rc = subset(contigs, contig_ids, ncontig_ids, &sa)) return rc;
    if (int rc = subset(reads, read_ids, nread_ids, &sb)) {
        dh_db_destroy(sa);
        return rc;
    }
    dh_la_set *set = nullptr;
    const int rc = dh_align_db(ctx, sa, sb, opts, 1, &set);
    if (!rc) {
        // chains in file order: START, then its NEXT records (how the reference reads them, dazzler.d:1728-1758)
        LaVec &la = set->la;
        for (size_t i = 0; i < la.size();) {
            size_t j = i + 1;
            while (j < la.size() && (la[j].flags & DH_FLAG_NEXT) && !(la[j].flags & DH_FLAG_START)) j++;
            const int32_t alen = (int32_t)(sa->h_off[(size_t)la[i].aread + 1] - sa->h_off[(size_t)la[i].aread]);
            const bool covers = la[i].abpos <= allowance && la[j - 1].aepos >= alen - allowance;
            for (size_t x = i; x < j; x++) {
                if (!covers) la[x].flags |= DH_FLAG_DISABLED;
                la[x].aread = contig_ids[la[x].aread];
                la[x].bread = read_ids[la[x].bread];
            }
            i = j;
        }
        *out = set;
    }
    dh_db_destroy(sa);
    dh_db_destroy(sb);
    return rc;
}
