// dh_bedmask.cpp -- dh_bed_to_mask: the intervals of a BED file in scaffold coordinates as a mask of the contigs of a .dam,
// with the contig pair and the read ids of every line's data comment (`dentist bed2mask`, commands/bed2mask.d:92-287).
// Host only, and on purpose: a closed-gaps BED has one line per closed gap, so there is nothing here a device could speed up.
// Only the public accessors of an opened DB are used.
#include <algorithm>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/dentist_hip.h"

int dh_fail(int code, const std::string &msg);

struct dh_bed_mask {
    int32_t ncontigs = 0;
    std::vector<int64_t> ptr, contig_ids, read_off, read_ids;
    std::vector<int32_t> iv;
};

namespace {

struct Contig {
    int32_t id;          // index in the opened view
    int64_t begin, end;  // in scaffold coordinates
};

// the fields of `s` between the separators: "a--b" has an empty one, "" is one empty field
std::vector<std::string> split(const std::string &s, char sep)
{
    std::vector<std::string> out;
    size_t at = 0;
    for (;;) {
        const size_t e = s.find(sep, at);
        out.push_back(s.substr(at, e == std::string::npos ? std::string::npos : e - at));
        if (e == std::string::npos) return out;
        at = e + 1;
    }
}

// plain decimal digits, at least one, value <= limit (the reference's to!uint also takes a sign and more: not reproduced)
bool parse_number(const std::string &s, uint64_t limit, int64_t *out)
{
    if (s.empty()) return false;
    uint64_t v = 0;
    for (char c : s) {
        if (c < '0' || c > '9') return false;
        v = v * 10 + (uint64_t)(c - '0');
        if (v > limit) return false;
    }
    *out = (int64_t)v;
    return true;
}

// parseDataComment (bed2mask.d:229-287): the errors of the comment, `contigs` (two ids or none) and `reads`
std::vector<std::string> parse_data_comment(const std::string &comment, std::vector<int64_t> &contigs, std::vector<int64_t> &reads)
{
    std::vector<std::string> errors;
    auto parse_fields = [&](std::vector<int64_t> &dest, const std::vector<std::string> &fields) {
        dest.clear();
        for (size_t i = 1; i < fields.size(); i++) {
            int64_t v = 0;
            if (!parse_number(fields[i], UINT32_MAX, &v)) {
                dest.clear();
                errors.push_back("could not parse uint in " + fields[0]);
                return;
            }
            dest.push_back(v);
        }
    };
    for (const std::string &part : split(comment, '|')) {
        const std::vector<std::string> fields = split(part, '-');
        if (fields[0] == "contigs") {
            if (fields.size() == 3)
                parse_fields(contigs, fields);
            else
                errors.push_back("contigs must have exactly two entries");
        } else if (fields[0] == "reads")
            parse_fields(reads, fields);
    }
    return errors;
}

}  // namespace

extern "C" int dh_bed_to_mask(const dh_dazz *db, const char *bed, int64_t n, const char *bed_name, int32_t data_comments, dh_bed_mask **out)
{
    if (!db || (!bed && n > 0) || n < 0 || !out) return dh_fail(DH_EINVAL, "dh_bed_to_mask: bad argument");
    const std::string file = bed_name ? bed_name : "-";
    const int32_t ncontigs = dh_dazz_nreads(db);
    const int64_t *off = dh_dazz_offsets(db);
    const int32_t *origin = dh_dazz_origin(db), *fpulse = dh_dazz_fpulse(db);
    // getContigsByScaffold (:92-105): a later scaffold of the same name replaces an earlier one
    std::map<std::string, std::vector<Contig>> by_scaffold;
    std::vector<Contig> *cur = nullptr;
    for (int32_t c = 0; c < ncontigs; c++) {
        const char *h = dh_dazz_header(db, c);
        if (c == 0 || origin[c] <= origin[c - 1] || strcmp(h, dh_dazz_header(db, c - 1)) != 0) {
            std::string key = h[0] == '>' ? h + 1 : h;
            key.resize(std::min(key.find('\t'), key.size()));
            cur = &by_scaffold[key];
            cur->clear();
        }
        cur->push_back(Contig{c, fpulse[c], (int64_t)fpulse[c] + (off[c + 1] - off[c])});
    }
    struct Interval {
        int32_t contig, begin, end;
        size_t line;  // index into the per-line ids
    };
    std::vector<Interval> intervals;
    std::vector<std::vector<int64_t>> line_contigs, line_reads;
    int64_t at = 0, line_no = 0;
    while (at < n) {
        const char *nl = (const char *)memchr(bed + at, '\n', (size_t)(n - at));
        const int64_t e = nl ? nl - bed : n;
        const std::string line(bed + at, (size_t)(e - at));
        at = e + 1;
        line_no++;
        if (line.empty()) continue;
        const std::string where = file + ":" + std::to_string(line_no);
        const std::vector<std::string> fields = split(line, '\t');
        if (fields.size() < 3) return dh_fail(DH_EINVAL, "BED file " + where + ": fewer than three columns");
        int64_t begin = 0, end = 0;
        if (!parse_number(fields[1], INT32_MAX, &begin) || !parse_number(fields[2], INT32_MAX, &end))
            return dh_fail(DH_EINVAL, "BED file " + where + ": begin and end must be decimal numbers below 2^31");
        if (begin > end) return dh_fail(DH_EINVAL, "BED file " + where + ": begin > end");
        const auto sc = by_scaffold.find(fields[0]);
        if (sc == by_scaffold.end()) return dh_fail(DH_EINVAL, "BED file " + where + ": unknown scaffold " + fields[0]);
        // getOverlappingContigs (:188-203), which runs off the array where nothing is left
        const std::vector<Contig> &cs = sc->second;
        size_t lo = 0, hi = cs.size();
        while (lo < hi && cs[lo].end <= begin) lo++;
        while (hi > lo && cs[hi - 1].begin >= end) hi--;
        if (lo == hi) return dh_fail(DH_EINVAL, "BED file " + where + ": the interval overlaps no contig of " + fields[0]);
        std::vector<int64_t> contigs, reads;
        if (data_comments) {
            const std::vector<std::string> errors = fields.size() >= 4 ? parse_data_comment(fields[3], contigs, reads) : std::vector<std::string>();
            if (!errors.empty()) {
                std::string msg = "ill-formatted data comment in BED file " + where + ":";
                for (const std::string &err : errors) msg += "\n  - " + err;
                return dh_fail(DH_EINVAL, msg);
            }
            if (contigs.size() != 2) return dh_fail(DH_EINVAL, "BED file " + where + ": the data comment has no contigs part");
        }
        line_contigs.push_back(contigs);
        line_reads.push_back(reads);
        for (size_t k = lo; k < hi; k++) {
            const Interval x{cs[k].id, (int32_t)(std::max(begin, cs[k].begin) - cs[k].begin), (int32_t)(std::min(end, cs[k].end) - cs[k].begin),
                             line_contigs.size() - 1};
            if (!intervals.empty()) {
                const Interval &p = intervals.back();
                if (std::make_tuple(x.contig, x.begin, x.end) < std::make_tuple(p.contig, p.begin, p.end))
                    return dh_fail(DH_EINVAL, "BED file " + where + ": the interval on contig " + std::to_string(x.contig + 1) +
                                                  " sorts before the one in front of it; intervals must ascend by contig and position");
            }
            intervals.push_back(x);
        }
    }
    dh_bed_mask *m = new dh_bed_mask();
    m->ncontigs = ncontigs;
    m->ptr.assign((size_t)ncontigs + 1, 0);
    m->read_off.push_back(0);
    for (const Interval &x : intervals) {
        m->ptr[(size_t)x.contig + 1]++;
        m->iv.push_back(x.begin);
        m->iv.push_back(x.end);
        const std::vector<int64_t> &c = line_contigs[x.line], &r = line_reads[x.line];
        m->contig_ids.push_back(c.size() == 2 ? c[0] : 0);
        m->contig_ids.push_back(c.size() == 2 ? c[1] : 0);
        m->read_ids.insert(m->read_ids.end(), r.begin(), r.end());
        m->read_off.push_back((int64_t)m->read_ids.size());
    }
    for (int32_t c = 0; c < ncontigs; c++) m->ptr[(size_t)c + 1] += m->ptr[(size_t)c];
    // (never an empty array behind an accessor)
    m->iv.resize(m->iv.size() + 2, 0);
    m->contig_ids.resize(m->contig_ids.size() + 2, 0);
    m->read_ids.push_back(0);
    *out = m;
    return DH_OK;
}

extern "C" void dh_bed_mask_destroy(dh_bed_mask *m) { delete m; }
extern "C" int32_t dh_bed_mask_ncontigs(const dh_bed_mask *m) { return m ? m->ncontigs : 0; }
extern "C" int64_t dh_bed_mask_count(const dh_bed_mask *m) { return m ? (int64_t)m->read_off.size() - 1 : 0; }
extern "C" const int64_t *dh_bed_mask_ptr(const dh_bed_mask *m) { return m ? m->ptr.data() : nullptr; }
extern "C" const int32_t *dh_bed_mask_iv(const dh_bed_mask *m) { return m ? m->iv.data() : nullptr; }
extern "C" const int64_t *dh_bed_mask_contig_ids(const dh_bed_mask *m) { return m ? m->contig_ids.data() : nullptr; }
extern "C" const int64_t *dh_bed_mask_read_off(const dh_bed_mask *m) { return m ? m->read_off.data() : nullptr; }
extern "C" const int64_t *dh_bed_mask_read_ids(const dh_bed_mask *m) { return m ? m->read_ids.data() : nullptr; }
