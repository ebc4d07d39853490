// dh_pileupsdb.cpp -- the file route of the process stage: pile-ups.db back into pile-ups and records (dh_pileups_from_db,
// the inverse of dh_pileups_write_db, dh_pileups.cpp) and dh_process_pileups_db, which processes a selection of a
// pile-ups.db with only the reads its pile-ups name loaded from the reads DB (dh_dazz_load_reads, dh_bpsload.cpp) -- what
// `dentist process --batch` does (commands/processPileUps/package.d:96-159).
#include <cstring>
#include <map>

#include "dh_process.h"

namespace {
std::string pile_name(int64_t f) { return "pile-up " + std::to_string(f); }

struct Flank {
    int32_t contig, seed;
    bool operator==(const Flank &o) const { return contig == o.contig && seed == o.seed; }
    bool operator!=(const Flank &o) const { return !(*this == o); }
};
}  // namespace

// pile-ups `sel` (indices into the file, each once) of the parsed container, see dh_pileups_from_db
static int piles_from_chaindb(const dh_chaindb *db, const std::vector<int32_t> &sel, const int64_t *contig_off, int32_t ncontigs,
                              dh_pileups **piles, dh_la_set **set, int32_t **file_index)
{
    const char *who = "dh_pileups_from_db: ";
    const int32_t npiles = dh_chaindb_npiles(db);
    const int32_t *nra_of_pile = dh_chaindb_pile_counts(db), *nsa_of_ra = dh_chaindb_read_alignment_counts(db);
    const dh_seeded *sa = dh_chaindb_seeded(db);
    const dh_chain_la *la = dh_chaindb_las(db);
    const uint16_t *tp = dh_chaindb_trace(db);
    // where every pile-up starts in the four levels below the pile-ups
    std::vector<int64_t> ra0((size_t)npiles + 1, 0), si0((size_t)npiles + 1, 0), li0((size_t)npiles + 1, 0), ti0((size_t)npiles + 1, 0);
    {
        int64_t ra = 0, si = 0, li = 0, ti = 0;
        for (int32_t p = 0; p < npiles; p++) {
            for (int32_t r = 0; r < nra_of_pile[p]; r++, ra++)
                for (int32_t s = 0; s < nsa_of_ra[ra]; s++, si++)
                    for (int32_t l = 0; l < sa[si].nla; l++, li++) ti += 2 * (int64_t)la[li].ntp;
            ra0[(size_t)p + 1] = ra, si0[(size_t)p + 1] = si, li0[(size_t)p + 1] = li, ti0[(size_t)p + 1] = ti;
        }
    }
    const int32_t count = (int32_t)sel.size();

    std::unique_ptr<dh_la_set> out(new dh_la_set());
    struct Pile {
        std::array<int32_t, 4> nodes;
        std::vector<int32_t> triples;
        int32_t file;
    };
    std::vector<Pile> got((size_t)count);
    int32_t tspace = 0;
    for (int32_t k = 0; k < count; k++) {
        const int32_t p = sel[(size_t)k];
        int64_t ra = ra0[(size_t)p], si = si0[(size_t)p], li = li0[(size_t)p], ti = ti0[(size_t)p];
        Pile &pl = got[(size_t)k];
        pl.file = p;
        const std::string name = std::string(who) + pile_name(p) + ": ";
        struct Entry {
            int32_t read, nsa;
            Flank fl[2];
            int32_t rec[2];
        };
        std::vector<Entry> entries;
        for (int32_t r = 0; r < nra_of_pile[p]; r++, ra++) {
            Entry e{-1, nsa_of_ra[ra], {{-1, 0}, {-1, 0}}, {-1, -1}};
            if (e.nsa < 1 || e.nsa > 2) return dh_fail(DH_EINVAL, name + "a read alignment with " + std::to_string(e.nsa) + " seeded alignments");
            for (int32_t s = 0; s < e.nsa; s++, si++) {
                const dh_seeded &x = sa[si];
                if (x.contig_a_id < 1 || (int64_t)x.contig_a_id > ncontigs)
                    return dh_fail(DH_EINVAL, name + "contig id " + std::to_string(x.contig_a_id) + " outside [1, " + std::to_string(ncontigs) + "]");
                const int64_t alen = contig_off[x.contig_a_id] - contig_off[x.contig_a_id - 1];
                if ((int64_t)x.contig_a_len != alen)
                    return dh_fail(DH_EINVAL, name + "contig " + std::to_string(x.contig_a_id) + " has " + std::to_string(alen) + " bases, the file says " +
                                                  std::to_string(x.contig_a_len));
                if (x.contig_b_id < 1 || x.contig_b_id > (uint32_t)INT32_MAX) return dh_fail(DH_EINVAL, name + "read id " + std::to_string(x.contig_b_id) + " is not a read id");
                if (x.seed > 1) return dh_fail(DH_EINVAL, name + "seed " + std::to_string(x.seed) + " is neither front nor back");
                if (x.nla < 1) return dh_fail(DH_EINVAL, name + "a seeded alignment without a local alignment");
                if (x.tspace < 1 || (tspace && x.tspace != tspace)) return dh_fail(DH_EINVAL, name + "trace spacing " + std::to_string(x.tspace) + " differs from the file's " + std::to_string(tspace));
                tspace = x.tspace;
                const int32_t rd = (int32_t)x.contig_b_id - 1;
                if (s == 1 && rd != e.read) return dh_fail(DH_EINVAL, name + "the two seeded alignments of a read alignment name different reads");
                e.read = rd;
                e.fl[s] = Flank{(int32_t)x.contig_a_id - 1, (int32_t)x.seed};
                if (out->la.size() + (size_t)x.nla > (size_t)INT32_MAX) return dh_fail(DH_EINVAL, name + "more than 2^31 records");
                e.rec[s] = (int32_t)out->la.size();
                for (int32_t l = 0; l < x.nla; l++, li++) {
                    const dh_chain_la &c = la[li];
                    if (c.ntp < 0 || c.a_end < c.a_begin || c.b_end < c.b_begin || c.a_end > x.contig_a_len || c.b_end > x.contig_b_len)
                        return dh_fail(DH_EINVAL, name + "a local alignment outside its sequences");
                    // the trace points of [a_begin, a_end) lie on the multiples of the spacing; their B parts sum to the B extent
                    const int64_t want = c.a_end > c.a_begin ? ((int64_t)c.a_end - 1) / tspace - (int64_t)c.a_begin / tspace + 1 : c.ntp;
                    int64_t bsum = 0;
                    for (int32_t t = 0; t < c.ntp; t++) bsum += tp[ti + 2 * (int64_t)t + 1];
                    if (c.ntp != want || bsum != (int64_t)c.b_end - c.b_begin)
                        return dh_fail(DH_EINVAL, name + "the trace of a local alignment (" + std::to_string(c.ntp) + " points, " + std::to_string(bsum) +
                                                      " B bases) does not sum to its extents [" + std::to_string(c.a_begin) + ", " + std::to_string(c.a_end) + ") x [" +
                                                      std::to_string(c.b_begin) + ", " + std::to_string(c.b_end) + ")");
                    dh_la rec;
                    memset(&rec, 0, sizeof(rec));
                    rec.tlen = 2 * c.ntp;
                    rec.diffs = (int32_t)c.diffs;
                    rec.abpos = (int32_t)c.a_begin;
                    rec.aepos = (int32_t)c.a_end;
                    rec.bbpos = (int32_t)c.b_begin;
                    rec.bepos = (int32_t)c.b_end;
                    rec.aread = (int32_t)x.contig_a_id - 1;
                    rec.bread = rd;
                    rec.flags = (x.flags & 1) ? DH_FLAG_COMP : 0u;
                    if (x.nla > 1) rec.flags |= l == 0 ? (DH_FLAG_START | DH_FLAG_BEST) : DH_FLAG_NEXT;  // as a chained .las holds them
                    rec.toff = (int64_t)out->trace.size();
                    out->trace.insert(out->trace.end(), tp + ti, tp + ti + 2 * (int64_t)c.ntp);
                    out->la.push_back(rec);
                    ti += 2 * (int64_t)c.ntp;
                }
            }
            entries.push_back(e);
        }
        // the nodes: from the entries with two seeded alignments, the smaller contig first; without one, an extension
        Flank f0{-1, 0}, f1{-1, 0};
        bool have = false;
        for (const Entry &e : entries) {
            if (e.nsa != 2) continue;
            if (e.fl[0].contig == e.fl[1].contig) return dh_fail(DH_EINVAL, name + "contig " + std::to_string(e.fl[0].contig + 1) + " is joined with itself");
            const bool swap = e.fl[0].contig > e.fl[1].contig;
            const Flank a = e.fl[swap ? 1 : 0], b = e.fl[swap ? 0 : 1];
            if (have && (a != f0 || b != f1)) return dh_fail(DH_EINVAL, name + "its entries disagree about its nodes");
            f0 = a;
            f1 = b;
            have = true;
        }
        if (!have) {
            for (const Entry &e : entries) {
                if (f0.contig >= 0 && e.fl[0] != f0) return dh_fail(DH_EINVAL, name + "its entries disagree about its nodes");
                f0 = e.fl[0];
            }
            if (entries.empty()) return dh_fail(DH_EINVAL, name + "has no entry");
        }
        pl.nodes = {f0.contig, f0.seed, f1.contig, f1.contig < 0 ? 0 : f1.seed};
        for (const Entry &e : entries) {
            int32_t on[2] = {-1, -1};
            for (int32_t s = 0; s < e.nsa; s++) {
                const int side = e.fl[s] == f0 ? 0 : (f1.contig >= 0 && e.fl[s] == f1 ? 1 : -1);
                if (side < 0 || on[side] >= 0) return dh_fail(DH_EINVAL, name + "its entries disagree about its nodes");
                on[side] = e.rec[s];
            }
            pl.triples.insert(pl.triples.end(), {e.read, on[0], on[1]});
        }
    }
    // dh_pileups_create_joins wants the pile-ups ordered by node
    auto key = [](const Pile &x) { return std::array<int64_t, 4>{x.nodes[0], x.nodes[1], x.nodes[2] < 0 ? INT32_MAX : x.nodes[2], x.nodes[3]}; };
    std::stable_sort(got.begin(), got.end(), [&](const Pile &x, const Pile &y) { return key(x) < key(y); });
    for (size_t i = 1; i < got.size(); i++)
        if (key(got[i - 1]) == key(got[i]))
            return dh_fail(DH_EINVAL, std::string(who) + pile_name(got[i].file) + ": has the nodes of " + pile_name(got[i - 1].file));
    std::vector<int32_t> nodes4, cnt, triples;
    for (const Pile &x : got) {
        nodes4.insert(nodes4.end(), x.nodes.begin(), x.nodes.end());
        cnt.push_back((int32_t)x.triples.size() / 3);
        triples.insert(triples.end(), x.triples.begin(), x.triples.end());
    }
    int32_t *fi = nullptr;
    if (file_index) {
        fi = (int32_t *)malloc(sizeof(int32_t) * std::max<size_t>(got.size(), 1));
        if (!fi) return dh_fail(DH_ENOMEM, std::string(who) + "out of memory");
        for (size_t i = 0; i < got.size(); i++) fi[i] = got[i].file;
    }
    out->tspace = tspace;
    const int32_t none = 0;
    if (int rc = dh_pileups_create_joins(nodes4.empty() ? &none : nodes4.data(), cnt.empty() ? &none : cnt.data(), (int32_t)got.size(),
                                         triples.empty() ? &none : triples.data(), piles)) {
        free(fi);
        return rc;
    }
    if (file_index) *file_index = fi;
    *set = out.release();
    return DH_OK;
}

// the file indices of [first, first + count) (count -1: to the end) behind `sel`, or DH_EINVAL
static int select_range(const dh_chaindb *db, int32_t first, int32_t count, std::vector<int32_t> &sel)
{
    const int32_t npiles = dh_chaindb_npiles(db);
    if (first < 0 || first > npiles || count < -1 || (count >= 0 && (int64_t)first + count > npiles))
        return dh_fail(DH_EINVAL, "dh_pileups_from_db: first " + std::to_string(first) + ", count " + std::to_string(count) + " outside the file's " +
                                      std::to_string(npiles) + " pile-ups");
    if (count < 0) count = npiles - first;
    for (int32_t p = first; p < first + count; p++) sel.push_back(p);
    return DH_OK;
}

struct ChainDbGuard {
    dh_chaindb *d;
    ~ChainDbGuard() { dh_chaindb_destroy(d); }
};

extern "C" int dh_pileups_from_db(const char *path, int32_t first, int32_t count, const int64_t *contig_off, int32_t ncontigs,
                                  dh_pileups **piles, dh_la_set **set, int32_t **file_index)
{
    if (!path || !contig_off || ncontigs < 0 || !piles || !set) return dh_fail(DH_EINVAL, "dh_pileups_from_db: bad argument");
    dh_chaindb *db = nullptr;
    if (int rc = dh_pileupdb_read(path, &db)) return rc;
    ChainDbGuard guard{db};
    std::vector<int32_t> sel;
    if (int rc = select_range(db, first, count, sel)) return rc;
    return piles_from_chaindb(db, sel, contig_off, ncontigs, piles, set, file_index);
}

// the pile-ups of `p` that `only` lets through (0 both, 1 spanning: gap pile-ups, 2 extending: extension pile-ups); `keep`
// gets their indices in p
static dh_pileups *filter_only(const dh_pileups *p, int32_t only, std::vector<int32_t> &keep)
{
    dh_pileups *q = new dh_pileups();
    for (size_t i = 0; i < p->contig_left.size(); i++) {
        const bool ext = p->join_of(i)[2] < 0;
        if (only == 0 || (only == 1 && !ext) || (only == 2 && ext)) {
            keep.push_back((int32_t)i);
            q->contig_left.push_back(p->contig_left[i]);
            q->join.push_back(p->join_of(i));
            q->triples.push_back(p->triples[i]);
        }
    }
    return q;
}

// Insertion.opCmp (util/math.d:527-545) on the nodes dh_insertions_write_db gives a record: (start contig, start part, end
// contig, end part) with pre < begin < end < post
static std::array<int64_t, 4> insertion_key(const dh_insertion &x)
{
    const bool ext = (x.join & DH_JOIN_EXTENSION) != 0, front0 = (x.join & DH_JOIN_FLANK0_FRONT) != 0, front1 = (x.join & DH_JOIN_FLANK1_BACK) == 0;
    if (ext) return {x.contig_left, front0 ? 0 : 2, x.contig_left, front0 ? 1 : 3};
    return {x.contig_left, front0 ? 1 : 2, x.join == 0 && x.contig_right == 0 ? x.contig_left + 1 : x.contig_right, front1 ? 1 : 2};
}

// The batches of `dentist process` (pileUpBatches, commandline.d:1174-1281): the pile-ups [ranges2[2 k], ranges2[2 k + 1]) of the
// file for every k, in the order given (an end of -1: the end of the file; ranges must not intersect), as ONE call of the route
// of dh_process_pileups_db.  only: 0 both, 1 spanning (gap pile-ups), 2 extending (extension pile-ups), applied to the loaded
// pile-ups first.  sorted != 0: the records in the order of Insertion.opCmp (processPileUps/package.d:156) instead of node
// order.  *file_index = per record its pile-up's index in the file, *skipped[*nskipped] = the file indices `only` kept out (each
// may be NULL; release with dh_shard_free).
extern "C" int dh_process_pileups_db_batches(dh_ctx *ctx, dh_db *contigs, const char *reads_db_path, const char *pileups_path,
                                             const int32_t *ranges2, int32_t nranges, const int64_t *rep_ptr, const int32_t *rep_iv,
                                             const dh_process_opts *opts, int32_t only, int32_t sorted, dh_insertions **out,
                                             int32_t **file_index, int32_t **skipped, int32_t *nskipped)
{
    const char *who = "dh_process_pileups_db: ";
    if (!contigs || !reads_db_path || !pileups_path || !opts || !out || only < 0 || only > 2 || nranges < 0 || (nranges > 0 && !ranges2))
        return dh_fail(DH_EINVAL, std::string(who) + "bad argument");
    dh_chaindb *db = nullptr;
    if (int rc = dh_pileupdb_read(pileups_path, &db)) return rc;
    ChainDbGuard db_guard{db};
    std::vector<int32_t> sel;
    for (int32_t k = 0; k < nranges; k++) {
        const int32_t a = ranges2[2 * k], b = ranges2[2 * k + 1];
        if (int rc = select_range(db, a, b < 0 ? -1 : (b >= a ? b - a : -2), sel)) return rc;
    }
    {
        std::vector<int32_t> seen(sel);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) return dh_fail(DH_EINVAL, std::string(who) + "the batches intersect");
    }
    dh_pileups *all = nullptr;
    dh_la_set *set = nullptr;
    int32_t *fidx = nullptr;
    if (int rc = piles_from_chaindb(db, sel, contigs->h_off.data(), contigs->n, &all, &set, &fidx)) return rc;
    std::vector<int32_t> keep;
    std::unique_ptr<dh_pileups> piles(filter_only(all, only, keep));
    std::unique_ptr<dh_la_set> set_guard(set);
    std::vector<int32_t> kept_file, skip_file;
    {
        size_t k = 0;
        for (size_t i = 0; i < all->contig_left.size(); i++)
            if (k < keep.size() && keep[k] == (int32_t)i) {
                kept_file.push_back(fidx[i]);
                k++;
            } else
                skip_file.push_back(fidx[i]);
    }
    free(fidx);
    dh_pileups_destroy(all);
    auto give = [](const std::vector<int32_t> &v, int32_t **dst) -> bool {
        if (!dst) return true;
        *dst = (int32_t *)malloc(sizeof(int32_t) * std::max<size_t>(v.size(), 1));
        if (!*dst) return false;
        if (!v.empty()) memcpy(*dst, v.data(), sizeof(int32_t) * v.size());
        return true;
    };
    if (nskipped) *nskipped = (int32_t)skip_file.size();
    if (piles->contig_left.empty()) {  // an empty selection: an empty result, and the device is not touched
        if (!give(kept_file, file_index) || !give(skip_file, skipped)) return dh_fail(DH_ENOMEM, std::string(who) + "out of memory");
        *out = new dh_insertions();
        return DH_OK;
    }
    if (!ctx) return dh_fail(DH_EINVAL, std::string(who) + "needs a context with a device (there is no CPU route)");
    // the sorted distinct read ids of the triples, and what the file says about the length of every one
    std::map<int32_t, int64_t> blen;
    for (const auto &t : piles->triples)
        for (size_t e = 0; e + 2 < t.size(); e += 3) blen[t[e]] = -1;
    {
        const dh_seeded *sa = dh_chaindb_seeded(db);
        for (int64_t s = 0; s < dh_chaindb_nseeded(db); s++) {
            auto it = blen.find((int32_t)sa[s].contig_b_id - 1);
            if (it == blen.end()) continue;
            if (it->second >= 0 && it->second != (int64_t)sa[s].contig_b_len)
                return dh_fail(DH_EINVAL, std::string(who) + "read " + std::to_string(sa[s].contig_b_id) + " has two lengths in " + pileups_path);
            it->second = sa[s].contig_b_len;
        }
    }
    std::vector<int32_t> ids;
    for (const auto &kv : blen) ids.push_back(kv.first);
    dh_db *reads = nullptr;
    if (int rc = dh_dazz_load_reads(ctx, reads_db_path, ids.data(), (int32_t)ids.size(), &reads)) return rc;
    struct ReadsGuard {
        dh_db *d;
        ~ReadsGuard() { dh_db_destroy(d); }
    } reads_guard{reads};
    for (size_t k = 0; k < ids.size(); k++) {
        const int64_t have = reads->h_off[k + 1] - reads->h_off[k];
        if (blen[ids[k]] != have)
            return dh_fail(DH_EINVAL, std::string(who) + "read " + std::to_string(ids[k] + 1) + " has " + std::to_string(have) + " bases in " + reads_db_path +
                                          ", the pile-ups say " + std::to_string(blen[ids[k]]));
    }
    // ids of the whole DB -> positions in the sparse DB: monotone, so every tie broken by read id falls as before (records of
    // pile-ups that `only` kept out name reads that were not loaded: nothing reads them)
    auto pos_of = [&](int32_t id) {
        const auto it = std::lower_bound(ids.begin(), ids.end(), id);
        return it != ids.end() && *it == id ? (int32_t)(it - ids.begin()) : -1;
    };
    for (auto &t : piles->triples)
        for (size_t e = 0; e + 2 < t.size(); e += 3) t[e] = pos_of(t[e]);
    for (dh_la &l : set->la) {
        const int32_t at = pos_of(l.bread);
        l.bread = at >= 0 ? at : 0;
        if (at < 0) l.flags |= DH_FLAG_DISABLED;
    }
    dh_process_opts o = *opts;
    o.tspace_map = set->tspace;
    dh_insertions *res = nullptr;
    if (int rc = dh_process_pileups_masked(ctx, contigs, reads, set->la.data(), (int64_t)set->la.size(), set->trace.data(), piles.get(), rep_ptr, rep_iv,
                                           &o, &res))
        return rc;
    std::unique_ptr<dh_insertions> res_guard(res);
    if (res->rec.size() != kept_file.size() || res->ids_off.size() != res->rec.size() + 1 || res->flank_of.size() != res->rec.size())
        return dh_fail(DH_EINVAL, std::string(who) + "the result has " + std::to_string(res->rec.size()) + " records for " + std::to_string(kept_file.size()) + " pile-ups");
    for (dh_insertion &r : res->rec)
        if (r.ref_read_id >= 0 && (size_t)r.ref_read_id < ids.size()) r.ref_read_id = ids[(size_t)r.ref_read_id];
    for (int32_t &id : res->ids)
        if (id >= 0 && (size_t)id < ids.size()) id = ids[(size_t)id];
    if (sorted) {
        const size_t n = res->rec.size();
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; i++) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return insertion_key(res->rec[x]) < insertion_key(res->rec[y]); });
        std::vector<dh_insertion> rec(n);
        std::vector<int32_t> flank_of(n), ids_off{0}, rids, kf(n);
        for (size_t i = 0; i < n; i++) {
            const size_t j = order[i];
            rec[i] = res->rec[j];
            flank_of[i] = res->flank_of[j];
            kf[i] = kept_file[j];
            rids.insert(rids.end(), res->ids.begin() + res->ids_off[j], res->ids.begin() + res->ids_off[j + 1]);
            ids_off.push_back((int32_t)rids.size());
        }
        res->rec.swap(rec);
        res->flank_of.swap(flank_of);
        res->ids.swap(rids);
        res->ids_off.swap(ids_off);
        kept_file.swap(kf);
    }
    if (!give(kept_file, file_index) || !give(skip_file, skipped)) return dh_fail(DH_ENOMEM, std::string(who) + "out of memory");
    *out = res_guard.release();
    return DH_OK;
}

extern "C" int dh_process_pileups_db(dh_ctx *ctx, dh_db *contigs, const char *reads_db_path, const char *pileups_path, int32_t first,
                                     int32_t count, const int64_t *rep_ptr, const int32_t *rep_iv, const dh_process_opts *opts,
                                     dh_insertions **out)
{
    if (first < 0 || count < -1) return dh_fail(DH_EINVAL, "dh_pileups_from_db: first " + std::to_string(first) + ", count " + std::to_string(count) + " outside the file");
    const int32_t range[2] = {first, count < 0 ? -1 : first + count};
    return dh_process_pileups_db_batches(ctx, contigs, reads_db_path, pileups_path, range, 1, rep_ptr, rep_iv, opts, 0, 0, out, nullptr, nullptr, nullptr);
}
