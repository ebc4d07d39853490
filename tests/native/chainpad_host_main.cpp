// A stand-alone run of the chain padder's CPU harness (chainpad_host.cpp) for the sanitizers: `make
// tests/native/chainpad_host_san` builds both with -fsanitize=address,undefined; the program exits 0 when every check holds
// and no report was printed.  The cases: random chains of 1..12 records with random cuts, overlaps, gaps and B shifts, their
// records and trace values in buffers of exactly their size, so that a read behind them is a report.  Checked: a chain that is
// not NESTED consumes A and B without a hole -- every segment starts where the one before it ended -- from the first record's
// begin to the last record's end; both runs (count, then write into a buffer of exactly the count) agree.
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../../dentist_amd/csrc/dh_chainpad.h"

extern "C" int32_t chainpad_host_plan(const CpRec *recs, int64_t nrec, const uint16_t *tr, int32_t ts, int32_t *rows, int64_t cap,
                                      int64_t *nrows);
extern "C" int32_t chainpad_host_generated_op(const uint8_t *a, const uint8_t *b, int32_t la, int32_t lb, int32_t p);

static uint64_t g_state = 88172645463325252ull;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return (uint32_t)(g_state >> 11);
}
static int32_t rnd_in(int32_t lo, int32_t hi) { return lo + (int32_t)(rnd() % (uint32_t)(hi - lo + 1)); }

int main()
{
    int bad = 0, nested = 0, ok = 0;
    for (int it = 0; it < 4000 && !bad; it++) {
        const int32_t ts = it % 3 == 0 ? 100 : (it % 3 == 1 ? 37 : 250);
        const int n = rnd_in(1, 12);
        std::vector<CpRec> recs;
        std::vector<uint16_t> tr;
        int32_t ab = rnd_in(0, 500), bb = rnd_in(0, 500);
        for (int k = 0; k < n; k++) {
            CpRec r = {};
            r.abpos = ab;
            r.aepos = ab + rnd_in(1, 900);
            r.nt = (r.aepos + ts - 1) / ts - r.abpos / ts;
            r.toff = (int64_t)tr.size();
            r.bbpos = bb;
            int32_t b = bb;
            for (int32_t t = 0; t < r.nt; t++) {
                const int32_t a0 = t == 0 ? r.abpos : (r.abpos / ts + t) * ts, a1 = t + 1 == r.nt ? r.aepos : (r.abpos / ts + t + 1) * ts;
                const int32_t nb = std::max(0, a1 - a0 + rnd_in(-5, 5));
                tr.push_back((uint16_t)rnd_in(0, 20));
                tr.push_back((uint16_t)nb);
                b += nb;
            }
            r.bepos = b;
            recs.push_back(r);
            const uint32_t kind = rnd() % 10;
            ab = kind < 4 ? r.aepos + rnd_in(0, 300) : std::max(r.abpos, r.aepos - rnd_in(1, 400));
            bb = std::max(0, (kind & 1) ? r.bepos + rnd_in(0, 300) : r.bepos - rnd_in(0, 400));
        }
        int64_t cnt = 0, cnt2 = 0;
        const int32_t st = chainpad_host_plan(recs.data(), n, tr.data(), ts, nullptr, 0, &cnt);
        std::vector<int32_t> rows((size_t)cnt * 6);
        const int32_t st2 = chainpad_host_plan(recs.data(), n, tr.data(), ts, rows.data(), cnt, &cnt2);
        if (st != st2 || cnt != cnt2) bad = 1;
        if (st == CP_NESTED) {
            nested++;
            continue;
        }
        ok++;
        int32_t a = recs[0].abpos, b = recs[0].bbpos;
        for (int64_t s = 0; s < cnt && !bad; s++) {
            const int32_t *r = rows.data() + 6 * s;
            if (r[0] == CP_SEG_TILES) {
                const CpRec &rc = recs[(size_t)r[1]];
                if (r[2] < 0 || r[3] > rc.nt || r[2] >= r[3]) bad = 2;
                const cp::Point p0 = cp::point_at(rc, tr.data(), ts, r[2]), p1 = cp::point_at(rc, tr.data(), ts, r[3]);
                if (p0.a != a || p0.b != b) bad = 3;
                a = p1.a, b = p1.b;
            } else {
                if (r[2] != a || r[4] != b || r[3] < r[2] || r[5] < r[4]) bad = 4;
                a = r[3], b = r[5];
            }
        }
        if (!bad && (a != recs.back().aepos || b != recs.back().bepos)) bad = 5;
        if (bad) printf("case %d: check %d failed\n", it, bad);
    }
    // the generated filler reads exactly its two ranges
    for (int it = 0; it < 200 && !bad; it++) {
        const int32_t la = rnd_in(0, 40), lb = rnd_in(0, 40);
        std::vector<uint8_t> a((size_t)la), b((size_t)lb);
        for (auto &x : a) x = (uint8_t)(rnd() & 3);
        for (auto &x : b) x = (uint8_t)(rnd() & 3);
        int32_t ca = 0, cb = 0;
        for (int32_t p = 0; p < std::max(la, lb); p++) {
            const int32_t op = chainpad_host_generated_op(a.data(), b.data(), la, lb, p);
            ca += op != 2;
            cb += op != 1;
        }
        if (ca != la || cb != lb) bad = 6;
    }
    printf("chainpad_host_san: %d chains walked, %d nested, %s\n", ok, nested, bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
