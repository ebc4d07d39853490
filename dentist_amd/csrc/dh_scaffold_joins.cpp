// dh_scaffold_joins.cpp -- the per-read join collector of the scaffold-graph pile-up builder: read alignments of every
// read (pileups.d:821-888 collectReadAlignments over base.d:1964-2050 SeededAlignment), one join per read alignment
// (base.d:2680-2722 makeJoin).  Host code: per-read work runs on the thread pool.
#include <atomic>
#include <tuple>

#include "dh_scaffold.h"
#include "dh_parallel.h"

namespace dh_scaffold_detail {
// collectReadAlignments for the enabled LAs idx[0..cnt) of one read, appended to `out` as raw joins
// (sa, on return: the seeded alignments of the read in read order -- what the bubble resolver checks against the skipped path)
void read_joins(const Ctx &c, const int64_t *idx, int64_t cnt, std::vector<RawJoin> &out, std::vector<SA> &sa, std::vector<std::pair<size_t, size_t>> &sl)
{
    sa.clear();
    for (int64_t x = 0; x < cnt; x++) {
        const dh_la &l = c.L(idx[x]);
        const bool comp = (l.flags & DH_FLAG_COMP) != 0;
        const int32_t bl = c.blen(l);
        const int32_t b = comp ? bl - l.bepos : l.bbpos, e = comp ? bl - l.bbpos : l.bepos;
        if (l.bbpos > l.abpos) sa.push_back(SA{idx[x], FRONT, b, e, comp ? -FRONT : FRONT});                 // isFrontExtension
        if (bl - l.bepos > c.alen(l) - l.aepos) sa.push_back(SA{idx[x], BACK, b, e, comp ? -BACK : BACK});  // isBackExtension
    }
    if (sa.empty()) return;
    std::stable_sort(sa.begin(), sa.end(), [](const SA &p, const SA &q) { return std::tie(p.b, p.e, p.srel) < std::tie(q.b, q.e, q.srel); });
    for (size_t i = 0; i + 1 < sa.size(); i++)
        if (sa[i].e > sa[i + 1].b && !(sa[i].la == sa[i + 1].la && sa[i].seed != sa[i + 1].seed)) return;  // a region of the read used twice
    const bool start_ext = sa[0].b > 0;
    // slices [0,1) if the read starts with an extension, then pairs
    sl.clear();
    if (start_ext) sl.emplace_back(0, 1);
    for (size_t i = start_ext ? 1 : 0; i < sa.size(); i += 2) sl.emplace_back(i, std::min(i + 2, sa.size()));
    for (auto &p : sl)  // one invalid read alignment discards the read
        if (p.second - p.first == 2 && c.L(sa[p.first].la).aread == c.L(sa[p.first + 1].la).aread) return;
    for (auto &p : sl) {
        dh_read_alignment ra;  // (read, la0, la1, seed0, seed1, n, pad)
        Edge e;
        if (p.second - p.first == 2) {
            SA a = sa[p.first], b = sa[p.first + 1];
            if (!(c.L(a.la).aread < c.L(b.la).aread)) std::swap(a, b);  // getInOrder
            ra = dh_read_alignment{c.L(a.la).bread, (int32_t)a.la, (int32_t)b.la, (uint8_t)a.seed, (uint8_t)b.seed, 2, 0};
            e = make_edge(Node{c.L(a.la).aread, a.seed == FRONT ? BEGIN : END}, Node{c.L(b.la).aread, b.seed == FRONT ? BEGIN : END});
        } else {
            const SA a = sa[p.first];
            const int32_t ct = c.L(a.la).aread;
            ra = dh_read_alignment{c.L(a.la).bread, (int32_t)a.la, -1, (uint8_t)a.seed, 0, 1, 0};
            e = a.seed == FRONT ? make_edge(Node{ct, PRE}, Node{ct, BEGIN}) : make_edge(Node{ct, END}, Node{ct, POST});
        }
        out.push_back(RawJoin{e.s, e.e, ra});
    }
}

namespace {
typedef std::vector<std::vector<std::pair<int32_t, int32_t>>> Live;  // per chunk of the input: (read - read_first, LA) of the enabled LAs

int live_records(const char *who, const dh_la *las, int64_t n, int32_t ncontigs, int32_t read_first, int32_t nreads, Live &live)
{
    std::atomic<int> bad{0};
    const int64_t lgrain = 1 << 14, lchunks = (n + lgrain - 1) / lgrain;  // (a mapping of configs[2]: 70 runs for up to 64 threads)
    live.assign((size_t)std::max<int64_t>(lchunks, 1), {});
    dh_parallel_for(lchunks, 1, [&](int64_t clo, int64_t chi) {
        for (int64_t ch = clo; ch < chi; ch++) {
            auto &v = live[(size_t)ch];
            const int64_t i1 = std::min(n, (ch + 1) * lgrain);
            for (int64_t i = ch * lgrain; i < i1; i++) {
                const int64_t rd = (int64_t)las[i].bread - read_first;
                if (rd < 0 || rd >= nreads || las[i].aread < 0 || las[i].aread >= ncontigs) bad = 1;
                else if (!(las[i].flags & DH_FLAG_DISABLED)) v.emplace_back((int32_t)rd, (int32_t)i);
            }
        }
    });
    return bad ? dh_fail(DH_EINVAL, std::string(who) + ": read or contig id out of range") : DH_OK;
}

// the live records grouped by read, input order inside a read: order[first[r] .. first[r + 1]) = the LAs of read r
void group_by_read(const dh_la *las, int32_t read_first, int32_t nreads, const Live &live, std::vector<int64_t> &order, std::vector<int64_t> &first)
{
    first.assign((size_t)nreads + 1, 0);
    std::vector<int64_t> loff(live.size() + 1, 0);
    for (size_t ch = 0; ch < live.size(); ch++) loff[ch + 1] = loff[ch] + (int64_t)live[ch].size();
    const int64_t nlive = loff.back();
    order.resize((size_t)nlive);
    // records in read order (a mapping as the device hands it over, or LAsort order inside one contig): the live
    // records are already grouped -- offsets by a merge walk per run of reads instead of a serial counting sort
    std::atomic<int> unsorted{0};
    dh_parallel_for((int64_t)live.size(), 1, [&](int64_t clo, int64_t chi) {
        for (int64_t ch = clo; ch < chi; ch++) {
            const auto &v = live[(size_t)ch];
            // (the last live record before this chunk: the nearest earlier chunk that has one -- a run of 16 384 disabled
            // records, e.g. a fully filtered repeat contig in A-major input, must not hide a descent in read id)
            int32_t prev = -1;
            for (int64_t pc = ch - 1; pc >= 0 && prev < 0; pc--)
                if (!live[(size_t)pc].empty()) prev = live[(size_t)pc].back().first;
            for (size_t k = 0; k < v.size(); k++) {
                if (v[k].first < prev) unsorted = 1;
                prev = v[k].first;
                order[(size_t)loff[(size_t)ch] + k] = v[k].second;
            }
        }
    });
    if (!unsorted.load()) {
        const int64_t rgrain = 1 << 13, rchunks = ((int64_t)nreads + 1 + rgrain - 1) / rgrain;
        dh_parallel_for(rchunks, 1, [&](int64_t clo, int64_t chi) {
            for (int64_t ch = clo; ch < chi; ch++) {
                const int64_t r0 = ch * rgrain, r1 = std::min<int64_t>((int64_t)nreads + 1, r0 + rgrain);
                int64_t lo = std::partition_point(order.begin(), order.end(), [&](int64_t i) { return (int64_t)las[i].bread - read_first < r0; }) -
                             order.begin();  // first live record of a read >= r0
                for (int64_t r = r0; r < r1; r++) {
                    while (lo < nlive && (int64_t)las[order[(size_t)lo]].bread - read_first < r) lo++;
                    first[(size_t)r] = lo;
                }
            }
        });
    } else {
        for (const auto &v : live)
            for (const auto &e : v) first[(size_t)e.first + 1]++;
        for (int32_t r = 0; r < nreads; r++) first[(size_t)r + 1] += first[(size_t)r];
        std::vector<int64_t> cur(first.begin(), first.end() - 1);
        for (const auto &v : live)
            for (const auto &e : v) order[(size_t)cur[(size_t)e.first]++] = e.second;
    }
}
}  // namespace

// The raw joins of the reads [read_first, read_first + nreads) named by `las` (bread = global read id), in read
// order: one flat array per run of reads (a run per host thread).
int collect_raw_joins(const char *who, const dh_la *las, int64_t n, const int64_t *contig_off, int32_t ncontigs,
                      const int64_t *read_off, int32_t read_first, int32_t nreads, std::vector<std::vector<RawJoin>> *raws)
{
    Ctx c{las, contig_off, read_off - read_first};
    dh_lap_timer lap{"[scaffold]", 24};
    // ---- the enabled LAs grouped by read, input order inside a read
    std::vector<int64_t> order, first;
    {
        Live live;
        if (int rc = live_records(who, las, n, ncontigs, read_first, nreads, live)) return rc;
        group_by_read(las, read_first, nreads, live, order, first);
    }
    lap("group by read");
    // ---- raw joins of the reads, in read order (collectScaffoldJoins, pileups.d:650-667)
    // (64 runs: with 16 the step ran on 16 of the host's cores; the runs stay raw -- scaffold_from_runs sorts them by
    // edge, all runs at once)
    const int64_t grain = std::max<int64_t>(4096, ((int64_t)nreads + 63) / 64), nchunks = ((int64_t)nreads + grain - 1) / grain;
    raws->assign((size_t)std::max<int64_t>(nchunks, 1), {});
    dh_parallel_for(nchunks, 1, [&](int64_t clo, int64_t chi) {
        std::vector<SA> sa;
        std::vector<std::pair<size_t, size_t>> sl;
        for (int64_t ch = clo; ch < chi; ch++) {
            std::vector<RawJoin> &raw = (*raws)[(size_t)ch];
            const int32_t r1 = (int32_t)std::min<int64_t>(nreads, (ch + 1) * grain);
            raw.clear();
            for (int32_t rd = (int32_t)(ch * grain); rd < r1; rd++) {
                const int64_t cnt = first[(size_t)rd + 1] - first[(size_t)rd];
                if (cnt > 0) read_joins(c, order.data() + first[(size_t)rd], cnt, raw, sa, sl);
            }
        }
    });
    lap("read joins");
    return DH_OK;
}
}  // namespace dh_scaffold_detail
