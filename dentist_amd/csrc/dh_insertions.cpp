// dh_insertions.cpp -- the result of the process stage on the host: the accessors of a dh_insertions (the struct itself:
// dh_internal.h) and insertions.db (dh_insertions_write_db, dh_insertions_from_db).
#include <climits>
#include <cstring>
#include <memory>

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

// insertions.db back into the records dh_output_assembly / dh_output_db take (what `dentist output` does with the file,
// output.d:309-319): the inverse of dh_insertions_write_db for a file of this library, of tools/merge-insertions or of the D
// binary.  Per insertion: the join from its two nodes (makeJoin, base.d:2680-2722), the splice sites on the contigs
// (getCroppingPosition!"contigA", common/insertions.d:110-119: a front seed gives the FIRST local alignment's A begin, a back
// seed the LAST one's A end), the slice of the consensus (getCroppingPosition!"contigB" :122-140 and
// getInfoForNewSequenceInsertion :228-284) in the frame of the flank-0 overlap as make_insertion (dh_process.cpp) leaves it,
// the diffs summed over the overlap's local alignments.  `flank` gets one pseudo record per overlap, flank_cov its covered A bases.
extern "C" int dh_insertions_from_db(const char *path, const int64_t *contig_off, int32_t ncontigs, dh_insertions **out)
{
    if (!path || !contig_off || ncontigs < 0 || !out) return dh_fail(DH_EINVAL, "dh_insertions_from_db: bad argument");
    dh_chaindb *db = nullptr;
    if (int rc = dh_insertiondb_read(path, &db)) return rc;
    struct Guard {
        dh_chaindb *d;
        ~Guard() { dh_chaindb_destroy(d); }
    } guard{db};
    const int32_t n = dh_chaindb_ninsertions(db);
    const dh_insertion_rec *q = dh_chaindb_insertions(db);
    const dh_seeded *sa = dh_chaindb_seeded(db);
    const dh_chain_la *la = dh_chaindb_las(db);
    const uint8_t *bases = dh_chaindb_bases(db);
    const uint32_t *ids = dh_chaindb_read_ids(db);
    const int64_t nsa = dh_chaindb_nseeded(db), nla = dh_chaindb_nlas(db);
    std::unique_ptr<dh_insertions> r(new dh_insertions());
    r->ids_off.push_back(0);
    int64_t at_sa = 0, at_la = 0, at_base = 0, at_id = 0;
    for (int32_t i = 0; i < n; i++) {
        const dh_insertion_rec &x = q[i];
        const std::string who = "dh_insertions_from_db: insertion " + std::to_string(i) + " of " + path + ": ";
        auto bad = [&](const std::string &m) { return dh_fail(DH_EINVAL, who + m); };
        if (x.noverlaps > 2) return bad("more than two overlaps");
        if (x.noverlaps < 1 || x.seq_len < 0 || x.seq_len > INT32_MAX || x.nread_ids < 0 || at_sa + x.noverlaps > nsa) return bad("malformed record");
        if (x.start_contig < 1 || x.start_contig > ncontigs || x.end_contig < 1 || x.end_contig > ncontigs)
            return bad("contig id outside [1, " + std::to_string(ncontigs) + "]");
        dh_insertion rec;
        memset(&rec, 0, sizeof(rec));
        const int32_t sp = x.start_part, ep = x.end_part;
        const bool same = x.start_contig == x.end_contig;
        const bool ext = same && ((sp == 0 && ep == 1) || (sp == 2 && ep == 3));
        const bool gap = !same && (sp == 1 || sp == 2) && (ep == 1 || ep == 2);
        if (!ext && !gap) return bad("its nodes are neither a gap join nor an extension");
        if (x.noverlaps != (ext ? 1 : 2)) return bad(ext ? "an extension needs one overlap" : "a gap join needs two overlaps");
        // flank 0 is the contig with the smaller id (Insertion edges are stored with ordered nodes; be safe about it)
        const bool swapped = gap && x.start_contig > x.end_contig;
        const int64_t c0 = swapped ? x.end_contig : x.start_contig, c1 = swapped ? x.start_contig : x.end_contig;
        const int32_t p0 = swapped ? ep : sp, p1 = swapped ? sp : ep;
        rec.contig_left = (int32_t)c0 - 1;
        rec.contig_right = ext ? -1 : (int32_t)c1 - 1;
        bool front[2] = {false, true};
        if (ext) {
            front[0] = sp == 0;
            rec.join = DH_JOIN_EXTENSION | (front[0] ? DH_JOIN_FLANK0_FRONT : 0);
        } else {
            front[0] = p0 == 1;
            front[1] = p1 == 1;
            rec.join = (front[0] ? DH_JOIN_FLANK0_FRONT : 0) | (front[1] ? 0 : DH_JOIN_FLANK1_BACK);
        }
        // the overlaps: the one on flank 0 is the one whose contig A is contig_left
        const dh_seeded *ov[2] = {nullptr, nullptr};
        const dh_chain_la *first[2] = {nullptr, nullptr}, *last[2] = {nullptr, nullptr};
        int64_t diffs[2] = {0, 0}, cov[2] = {0, 0};
        for (int32_t k = 0; k < x.noverlaps; k++) {
            const dh_seeded &s = sa[at_sa + k];
            if (s.nla < 1 || at_la + s.nla > nla) return bad("an overlap without local alignments");
            if (s.contig_a_id < 1 || (int64_t)s.contig_a_id > ncontigs) return bad("contig id outside [1, " + std::to_string(ncontigs) + "]");
            if ((int64_t)s.contig_a_len != contig_off[s.contig_a_id] - contig_off[s.contig_a_id - 1])
                return bad("contig_a_len " + std::to_string(s.contig_a_len) + " contradicts the length of contig " + std::to_string(s.contig_a_id));
            if ((int64_t)s.contig_b_len != x.seq_len)
                return bad("contig_b_len " + std::to_string(s.contig_b_len) + " differs from the sequence length " + std::to_string(x.seq_len));
            int32_t side;
            if (ext)
                side = 0;
            else if ((int64_t)s.contig_a_id == c0 && !ov[0] && (s.seed == 0) == front[0])
                side = 0;
            else if ((int64_t)s.contig_a_id == c1 && !ov[1] && (s.seed == 0) == front[1])
                side = 1;
            else
                return bad("an overlap that belongs to neither node");
            if (ext && ((int64_t)s.contig_a_id != c0 || (s.seed == 0) != front[0])) return bad("an overlap that belongs to neither node");
            ov[side] = &s;
            first[side] = la + at_la;
            last[side] = la + at_la + s.nla - 1;
            for (int32_t l = 0; l < s.nla; l++) {
                const dh_chain_la &a = la[at_la + l];
                if (a.a_end < a.a_begin || a.a_end > s.contig_a_len || a.b_end < a.b_begin || a.b_end > s.contig_b_len) return bad("a local alignment outside its sequences");
                diffs[side] += a.diffs;
                cov[side] += (int64_t)a.a_end - a.a_begin;
            }
            at_la += s.nla;
        }
        at_sa += x.noverlaps;
        const int32_t clen = (int32_t)x.seq_len;
        const dh_seeded *L = ov[0], *R = ov[1];
        rec.status = DH_PILE_OK;
        rec.ref_read = -1;
        rec.ref_read_id = x.nread_ids > 0 ? (int32_t)ids[at_id] - 1 : -1;
        rec.nreads = x.nread_ids;
        rec.crop_left = rec.crop_right = -1;
        rec.cons_len = clen;
        rec.cons_off = (int64_t)r->bases.size();
        rec.comp = (L->flags & 1) ? 1 : 0;
        rec.left_diffs = (int32_t)diffs[0];
        rec.right_diffs = (int32_t)diffs[1];
        rec.left_aepos = (int32_t)(front[0] ? first[0]->a_begin : last[0]->a_end);
        const int32_t b0 = (int32_t)(front[0] ? first[0]->b_begin : last[0]->b_end);
        if (!ext) {
            rec.right_abpos = (int32_t)(front[1] ? first[1]->a_begin : last[1]->a_end);
            int32_t b1 = (int32_t)(front[1] ? first[1]->b_begin : last[1]->b_end);
            if ((R->flags & 1) != (L->flags & 1)) b1 = clen - b1;
            rec.ins_begin = front[0] ? b1 : b0;
            rec.ins_end = front[0] ? b0 : b1;
            if (rec.ins_end < rec.ins_begin) std::swap(rec.ins_begin, rec.ins_end);  // insertions.d:266-267
        } else {
            rec.right_abpos = -1;
            rec.ins_begin = front[0] ? 0 : b0;
            rec.ins_end = front[0] ? b0 : clen;
        }
        for (int32_t side = 0; side < (ext ? 1 : 2); side++) {
            dh_la f;
            memset(&f, 0, sizeof(f));
            f.abpos = (int32_t)first[side]->a_begin;
            f.aepos = (int32_t)last[side]->a_end;
            f.bbpos = (int32_t)first[side]->b_begin;
            f.bepos = (int32_t)last[side]->b_end;
            f.diffs = (int32_t)diffs[side];
            f.flags = (ov[side]->flags & 1) ? DH_FLAG_COMP : 0;
            f.aread = (int32_t)ov[side]->contig_a_id - 1;
            if (side == 0) r->flank_of.push_back((int32_t)r->flank.size());
            r->flank.push_back(f);
            r->flank_cov.push_back(cov[side]);
        }
        r->rec.push_back(rec);
        r->bases.insert(r->bases.end(), bases + at_base, bases + at_base + x.seq_len);
        at_base += x.seq_len;
        for (int32_t k = 0; k < x.nread_ids; k++) {
            if (ids[at_id + k] < 1) return bad("read id 0 (ids are 1-based)");
            r->ids.push_back((int32_t)ids[at_id + k] - 1);
        }
        at_id += x.nread_ids;
        r->ids_off.push_back((int32_t)r->ids.size());
    }
    *out = r.release();
    return DH_OK;
}
