// dh_insertions.cpp -- the result of the process stage on the host: the accessors of a dh_insertions (the struct itself:
// dh_internal.h) and insertions.db (dh_insertions_write_db).
#include <cstring>

#include "dh_internal.h"

// ------------------------------------------------------------------------------------ results

// (struct dh_insertions: dh_internal.h)

extern "C" void dh_insertions_destroy(dh_insertions *r) { delete r; }
extern "C" int32_t dh_insertions_count(const dh_insertions *r) { return r ? (int32_t)r->rec.size() : 0; }
extern "C" const dh_insertion *dh_insertions_records(const dh_insertions *r) { return r ? r->rec.data() : nullptr; }
extern "C" const uint8_t *dh_insertions_bases(const dh_insertions *r) { return r ? r->bases.data() : nullptr; }
extern "C" int64_t dh_insertions_bases_len(const dh_insertions *r) { return r ? (int64_t)r->bases.size() : 0; }
// read ids (0-based) of every record's pile-up: ids[off[i] .. off[i + 1]); off has count + 1 entries (all 0 when the
// result carries no ids)
extern "C" const int32_t *dh_insertions_read_ids(const dh_insertions *r) { return r ? r->ids.data() : nullptr; }
extern "C" const int32_t *dh_insertions_read_ids_off(const dh_insertions *r)
{
    return r && r->ids_off.size() == r->rec.size() + 1 ? r->ids_off.data() : nullptr;
}

// insertions.db of a result (what `dentist process` hands to `dentist output`,
// processPileUps/package.d:156-158, 789-805): one insertion per closed gap -- start = (left contig,
// end), end = (right contig, begin), the whole consensus as sequence, the two flank overlaps
// (contig = A, consensus = B, seeds back / front) and the sorted 1-based read ids of the pile-up.
extern "C" int dh_insertions_write_db(const dh_insertions *r, const int64_t *contig_off, int32_t ncontigs,
                                      int32_t tspace, const char *path)
{
    if (!r || !contig_off || !path || ncontigs < 0) return dh_fail(DH_EINVAL, "dh_insertions_write_db: bad argument");
    std::vector<dh_insertion_rec> ins;
    std::vector<uint8_t> bases;
    std::vector<uint32_t> ids;
    std::vector<dh_seeded> sa;
    std::vector<dh_chain_la> la;
    std::vector<uint16_t> tp;
    for (size_t i = 0; i < r->rec.size(); i++) {
        const dh_insertion &x = r->rec[i];
        if (x.status != DH_PILE_OK || r->flank_of[i] < 0) continue;
        const bool ext = (x.join & DH_JOIN_EXTENSION) != 0;
        const int32_t nf = ext ? 1 : 2;
        const int32_t fcontig[2] = {x.contig_left, ext ? x.contig_left : (x.join == 0 && x.contig_right == 0 ? x.contig_left + 1 : x.contig_right)};
        const bool front[2] = {(x.join & DH_JOIN_FLANK0_FRONT) != 0, (x.join & DH_JOIN_FLANK1_BACK) == 0};
        if (fcontig[0] < 0 || fcontig[0] >= ncontigs || fcontig[1] < 0 || fcontig[1] >= ncontigs)
            return dh_fail(DH_EINVAL, "dh_insertions_write_db: gap outside the contigs");
        dh_insertion_rec q;
        memset(&q, 0, sizeof(q));
        // makeJoin (base.d:2680-2722): a gap joins the seeded parts of its two contigs (begin = 1, end = 2); a front
        // extension is (contig, pre = 0) -> (contig, begin), a back extension (contig, end) -> (contig, post = 3)
        q.start_contig = fcontig[0] + 1;
        q.end_contig = fcontig[1] + 1;
        if (ext) {
            q.start_part = front[0] ? 0 : 2;
            q.end_part = front[0] ? 1 : 3;
        } else {
            q.start_part = front[0] ? 1 : 2;
            q.end_part = front[1] ? 1 : 2;
        }
        q.seq_len = x.cons_len;
        q.contig_len = 0;
        q.noverlaps = nf;
        q.nread_ids = r->ids_off[i + 1] - r->ids_off[i];
        ins.push_back(q);
        bases.insert(bases.end(), r->bases.begin() + x.cons_off, r->bases.begin() + x.cons_off + x.cons_len);
        std::vector<uint32_t> my(r->ids.begin() + r->ids_off[i], r->ids.begin() + r->ids_off[i + 1]);
        for (uint32_t &v : my) v += 1;
        std::sort(my.begin(), my.end());
        ids.insert(ids.end(), my.begin(), my.end());
        for (int side = 0; side < nf; side++) {
            const dh_la &f = r->flank[(size_t)r->flank_of[i] + (size_t)side];
            const int32_t c = fcontig[side];
            dh_seeded s;
            memset(&s, 0, sizeof(s));
            s.id = (int64_t)sa.size();
            s.contig_a_id = (uint32_t)(c + 1);
            s.contig_a_len = (uint32_t)(contig_off[c + 1] - contig_off[c]);
            s.contig_b_id = 1;
            s.contig_b_len = (uint32_t)x.cons_len;
            s.flags = (f.flags & DH_FLAG_COMP) ? 1 : 0;
            s.seed = front[side] ? 0 : 1;  // AlignmentLocationSeed: front = 0, back = 1 (plain gap: the back of the left contig, the front of the right one)
            s.tspace = (uint16_t)tspace;
            s.nla = 1;
            sa.push_back(s);
            la.push_back(dh_chain_la{(uint32_t)f.abpos, (uint32_t)f.aepos, (uint32_t)f.bbpos, (uint32_t)f.bepos, (uint32_t)f.diffs, f.tlen / 2});
            tp.insert(tp.end(), r->flank_tr.begin() + f.toff, r->flank_tr.begin() + f.toff + f.tlen);
        }
    }
    return dh_insertiondb_write(path, (int32_t)ins.size(), ins.data(), bases.data(), ids.data(), sa.data(), la.data(), tp.data());
}
