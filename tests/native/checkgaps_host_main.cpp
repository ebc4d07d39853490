// A stand-alone run of the gap analysis' CPU harness (checkgaps_host.cpp) for the sanitizers: `make tests/native/checkgaps_host_san`
// builds both with -fsanitize=address,undefined; the program exits 0 when every scene agrees and no report was printed.
// The scenes: a true contig with 2..80 input contigs; every gap closed by a sequence derived from the true one through random ops
// (so the alignment is known by construction: runs of insertions and deletions, also in the first and last columns, 1..300 columns),
// left open behind an N-run, or partially filled; the result as it is or reverse-complemented as a whole; crop 0..15; a random dust
// mask or none; batches that start anywhere and run past the last contig.  Against the contract written out here column by column
// on the three lines of the alignment.  The harness keeps every device buffer in a heap block of exactly its size.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dentist_hip.h"

extern "C" int32_t checkgaps_host(const uint8_t *true_bases, const int64_t *true_off, int32_t n_true, const uint8_t *res_bases, const int64_t *res_off,
                                  int32_t n_res, const int32_t *mapped, int32_t n_input, const dh_contig_mapping *maps, int32_t nmaps,
                                  const int32_t *result_gap, const int64_t *dust_ptr, const int32_t *dust_iv, int32_t crop, int32_t first_contig,
                                  int32_t count, int32_t run_check, const uint8_t *given_up, const int64_t *op_off, const uint8_t *ops,
                                  dh_gap_summary *out, int32_t *out_len, uint8_t *out_ref, uint8_t *out_qry, int64_t cap, char *msg, int32_t msg_cap);

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

typedef std::vector<uint8_t> Seq;

static Seq revcomp(const Seq &s)
{
    Seq r(s.rbegin(), s.rend());
    for (auto &b : r)
        if (b < 4) b = (uint8_t)(3 - b);
    return r;
}

struct Gap {
    int kind;  // 0 closed, 1 unclosed, 2 partial
    std::vector<uint8_t> ops;  // closed: over [lhs.end - crop, rhs.begin + crop)
    Seq query;                 // closed: what the ops make of the true interval
};

// ops over `ref` whose first and last `crop` columns are matches (the mappings are exact), and the query they produce
static void random_ops(const Seq &ref, int32_t crop, std::vector<uint8_t> &ops, Seq &qry)
{
    const int32_t R = (int32_t)ref.size();
    int32_t i = 0;
    auto ins = [&](int32_t n) {
        for (int32_t k = 0; k < n; k++) ops.push_back(2), qry.push_back((uint8_t)rnd_in(0, rnd() % 9 == 0 ? 4 : 3));
    };
    for (; i < crop; i++) ops.push_back(0), qry.push_back(ref[(size_t)i]);
    if (rnd() % 3 == 0) ins(rnd_in(1, 70));
    while (i < R - crop) {
        const uint32_t x = rnd() % 16;
        if (x == 0)
            ins(rnd_in(1, 5));
        else if (x == 1)
            ops.push_back(1), i++;
        else if (x == 2)
            ops.push_back(3), qry.push_back((uint8_t)((ref[(size_t)i] + 1) & 3)), i++;
        else
            ops.push_back(0), qry.push_back(ref[(size_t)i]), i++;
    }
    if (rnd() % 3 == 0) ins(rnd_in(1, 70));
    for (; i < R; i++) ops.push_back(0), qry.push_back(ref[(size_t)i]);
}

static int fail(const char *what, int scene, int g, long long got, long long exp)
{
    fprintf(stderr, "scene %d gap %d: %s %lld, expected %lld\n", scene, g, what, got, exp);
    return 1;
}

static int run_scene(int scene)
{
    const int32_t crop = rnd() % 3 == 0 ? 0 : rnd_in(1, 15), n_input = rnd_in(2, scene % 7 == 0 ? 80 : 9);
    const bool complement = rnd() % 2 == 0, with_dust = rnd() % 3 != 0;
    // ---- the true contig and its input contigs
    std::vector<int32_t> mapped;
    int32_t at = rnd_in(crop, crop + 40);
    for (int32_t c = 0; c < n_input; c++) {
        const int32_t len = rnd_in(2 * crop + 1, 2 * crop + 120);
        mapped.insert(mapped.end(), {1, at, at + len});
        at += len + rnd_in(1, 300);
    }
    const int32_t T = at + crop + rnd_in(0, 30);
    Seq tr((size_t)T);
    for (auto &b : tr) b = (uint8_t)rnd_in(0, 3);
    // ---- the result, contig by contig
    std::vector<Gap> gaps((size_t)n_input - 1);
    std::vector<Seq> res(1);
    std::vector<int32_t> result_gap;
    std::vector<dh_contig_mapping> maps;
    for (int32_t c = 0; c < n_input; c++) {
        const int32_t b = mapped[3 * c + 1], e = mapped[3 * c + 2];
        Seq &cur = res.back();
        // (the crop bases behind the contig before it are in the result already when its gap was closed)
        const bool joined = c > 0 && gaps[(size_t)c - 1].kind == 0;
        const int32_t pos = (int32_t)cur.size() - (joined ? crop : 0);
        cur.insert(cur.end(), tr.begin() + b + (joined ? crop : 0), tr.begin() + e);
        maps.push_back(dh_contig_mapping{(int32_t)res.size(), pos + crop, pos + (e - b) - crop, 0, c + 1, 0, 0, 0.0f});
        if (c == n_input - 1) break;
        Gap &g = gaps[(size_t)c];
        const int32_t nb = mapped[3 * (c + 1) + 1];
        g.kind = rnd() % 5 == 0 ? rnd_in(1, 2) : 0;
        if (g.kind == 2 && nb - e < 2) g.kind = 1;
        if (g.kind == 0) {
            const Seq ref(tr.begin() + e - crop, tr.begin() + nb + crop);
            random_ops(ref, crop, g.ops, g.query);
            cur.resize(cur.size() - (size_t)crop);  // the query brings its own crop bases
            cur.insert(cur.end(), g.query.begin(), g.query.end());
        } else {
            const int32_t hole = nb - e, left = g.kind == 2 ? rnd_in(0, hole / 2) : 0, right = g.kind == 2 ? rnd_in(left ? 0 : 1, hole / 2) : 0;
            cur.insert(cur.end(), tr.begin() + e, tr.begin() + e + left);
            result_gap.push_back(rnd_in(1, 40));
            res.emplace_back(tr.begin() + nb - right, tr.begin() + nb);
            if (g.kind == 2 && left + right == 0) g.kind = 1;
        }
    }
    result_gap.push_back(0);
    const int32_t n_res = (int32_t)res.size();
    if (complement) {  // the scaffold's other strand
        std::reverse(res.begin(), res.end());
        std::reverse(result_gap.begin(), result_gap.end() - 1);
        for (auto &s : res) s = revcomp(s);
        for (auto &m : maps) {
            m.ref_contig = n_res + 1 - m.ref_contig;
            const int32_t len = (int32_t)res[(size_t)m.ref_contig - 1].size(), b = m.ref_begin;
            m.ref_begin = len - m.ref_end, m.ref_end = len - b, m.complement = 1;
        }
    }
    Seq rbases;
    std::vector<int64_t> roff{0};
    for (auto &s : res) rbases.insert(rbases.end(), s.begin(), s.end()), roff.push_back((int64_t)rbases.size());
    for (auto &m : maps) m.ref_contig_length = (int32_t)(roff[(size_t)m.ref_contig] - roff[(size_t)m.ref_contig - 1]);
    const int64_t toff[2] = {0, T};
    std::vector<int64_t> dptr{0};
    std::vector<int32_t> div;
    for (int32_t p = rnd_in(0, 200); with_dust && p < T;) {
        const int32_t e = std::min(T, p + rnd_in(0, 150));
        div.insert(div.end(), {p, e});
        p = e + rnd_in(0, 250);
    }
    dptr.push_back((int64_t)div.size() / 2);
    div.insert(div.end(), {0, 0});
    // ---- the batch and its ops
    const int32_t first = rnd_in(1, n_input), count = n_input - first + 1;
    std::vector<int64_t> op_off{0};
    std::vector<uint8_t> ops;
    for (int32_t g = 0; g < count; g++) {
        const int32_t c = first + g - 1;
        if (c < n_input - 1 && gaps[(size_t)c].kind == 0 && !gaps[(size_t)c].query.empty())
            ops.insert(ops.end(), gaps[(size_t)c].ops.begin(), gaps[(size_t)c].ops.end());
        op_off.push_back((int64_t)ops.size());
    }
    ops.push_back(0);
    std::vector<uint8_t> given_up((size_t)count, 0);
    std::vector<dh_gap_summary> out((size_t)count);
    std::vector<int32_t> lens(2 * (size_t)count);
    const int64_t cap = 1 << 20;
    std::vector<uint8_t> oref((size_t)cap), oqry((size_t)cap);
    char msg[256] = "";
    const int32_t rc = checkgaps_host(tr.data(), toff, 1, rbases.data(), roff.data(), n_res, mapped.data(), n_input, maps.data(), (int32_t)maps.size(),
                                      result_gap.data(), with_dust ? dptr.data() : nullptr, with_dust ? div.data() : nullptr, crop, first, count, 1,
                                      given_up.data(), op_off.data(), ops.data(), out.data(), lens.data(), oref.data(), oqry.data(), cap, msg, 256);
    if (rc) {
        fprintf(stderr, "scene %d: refused (%d): %s\n", scene, rc, msg);
        return 1;
    }
    // ---- the contract, column by column
    int64_t rat = 0, qat = 0;
    for (int32_t g = 0; g < count; g++) {
        const int32_t c = first + g - 1;
        const dh_gap_summary &s = out[(size_t)g];
        if (c == n_input - 1) {
            if (s.state != DH_GAP_IGNORED) return fail("state", scene, g, s.state, DH_GAP_IGNORED);
            continue;
        }
        const Gap &gp = gaps[(size_t)c];
        const int32_t e = mapped[3 * c + 2], nb = mapped[3 * (c + 1) + 1];
        const int32_t want = gp.kind == 0 ? DH_GAP_CLOSED : (gp.kind == 1 ? DH_GAP_UNCLOSED : DH_GAP_PARTIALLY_CLOSED);
        if (s.state != want) return fail("state", scene, g, s.state, want);
        if (s.gap_length != nb - e) return fail("gap_length", scene, g, s.gap_length, nb - e);
        if (s.lhs_map != c || s.rhs_map != c + 1) return fail("lhs_map", scene, g, s.lhs_map, c);
        if (gp.kind == 1) {
            if (s.align_status != DH_CG_NONE) return fail("align_status", scene, g, s.align_status, DH_CG_NONE);
            continue;
        }
        if (s.complement != (complement ? 1 : 0)) return fail("complement", scene, g, s.complement, complement);
        if (s.true_begin != e - crop || s.true_end != nb + crop) return fail("true_begin", scene, g, s.true_begin, e - crop);
        const int32_t rl = lens[2 * (size_t)g], ql = lens[2 * (size_t)g + 1];
        if (gp.kind == 2) {  // the pair only: left flank, the run, right flank
            if (rl != nb - e + 2 * crop) return fail("partial reference length", scene, g, rl, nb - e + 2 * crop);
            if (memcmp(oref.data() + rat, tr.data() + e - crop, (size_t)rl)) return fail("partial reference bytes", scene, g, 0, 0);
            int32_t nn = 0;
            for (int32_t k = 0; k < ql; k++) nn += oqry[(size_t)(qat + k)] == 4;
            if (nn < 1 || nn > 40) return fail("partial query's run", scene, g, nn, 1);
            rat += rl, qat += ql;
            continue;
        }
        if (gp.query.empty()) {
            if (s.align_status != DH_CG_EMPTY) return fail("align_status", scene, g, s.align_status, DH_CG_EMPTY);
            continue;
        }
        if (s.align_status != DH_CG_OK) return fail("align_status", scene, g, s.align_status, DH_CG_OK);
        if (rl != nb - e + 2 * crop || ql != (int32_t)gp.query.size()) return fail("query length", scene, g, ql, (long long)gp.query.size());
        if (memcmp(oref.data() + rat, tr.data() + e - crop, (size_t)rl) || memcmp(oqry.data() + qat, gp.query.data(), (size_t)ql))
            return fail("gathered bytes", scene, g, 0, 0);
        rat += rl, qat += ql;
        // the three lines
        std::string rline, qline;
        int32_t i = 0, j = 0;
        for (uint8_t op : gp.ops) {
            rline += op == 2 ? '-' : "acgtn"[tr[(size_t)(e - crop + i++)]];
            qline += op == 1 ? '-' : "acgtn"[gp.query[(size_t)j++]];
        }
        const int32_t n = (int32_t)gp.ops.size();
        int32_t cb = 0, ce = n;
        if (crop > 0) {
            int32_t seen = 0, k;
            for (k = 0; k < n && !((seen += rline[(size_t)k] != '-' && rline[(size_t)k] != 'n') == crop); k++) {}
            cb = k < n ? k + 1 : 0;
            for (seen = 0, k = n - 1; k >= 0 && !((seen += rline[(size_t)k] != '-' && rline[(size_t)k] != 'n') == crop); k--) {}
            ce = k >= 0 ? k : n;
        }
        int32_t m = 0, rlen = 0, qlen = 0, d[4] = {0, 0, 0, 0};
        int64_t ref_pos = e;
        auto dust = [&](int64_t p) {
            if (p < e || p >= nb) return false;
            for (size_t k = 0; k + 2 < div.size(); k += 2)
                if (div[k] <= p && p < div[k + 1]) return true;
            return false;
        };
        for (int32_t k = cb; k < ce; k++) {
            const uint8_t op = gp.ops[(size_t)k];
            m += op == 0;
            rlen += rline[(size_t)k] != '-' && rline[(size_t)k] != 'n';
            qlen += qline[(size_t)k] != '-' && qline[(size_t)k] != 'n';
            if (with_dust) {
                const bool du = dust(ref_pos) || (rline[(size_t)k] == '-' && (dust(ref_pos - 1) || dust(ref_pos + 1)));
                d[du ? 0 : 2]++, d[du ? 1 : 3] += op == 0;
            }
            if (op == 0 || op == 3 || (rline[(size_t)k] != '-' && rline[(size_t)k] != 'n')) ref_pos++;
        }
        if (crop == 0) rlen = rl, qlen = ql;
        if (s.col_begin != cb || s.col_end != ce) return fail("col_begin", scene, g, s.col_begin, cb);
        if (s.matches != m) return fail("matches", scene, g, s.matches, m);
        if (s.reference_length != rlen || s.query_length != qlen) return fail("query_length", scene, g, s.query_length, qlen);
        if (s.dust_ops != d[0] || s.dust_matches != d[1] || s.none_dust_ops != d[2] || s.none_dust_matches != d[3])
            return fail("dust_ops", scene, g, s.dust_ops, d[0]);
    }
    return 0;
}

int main()
{
    for (int scene = 0; scene < 400; scene++)
        if (run_scene(scene)) return 1;
    printf("checkgaps_host: 400 scenes agree\n");
    return 0;
}
