"""Inputs of the extension-stage tests (dh_extend_candidates against oz.extend_candidates): sequences and PLANTED candidates
that put the rules of the candidate loop, of the acceptance and of the two extensions (DESIGN.md "Algorithm DH-1", "DH-2";
oracle/align.c: extend_cands, extend, extend_tiled) on both sides of their boundaries.  Simulated reads never put a
candidate 64 or 65 diagonals from a finished region or an alignment exactly at min_len; these do.  Everything is seeded and
small: sequences of one base to a few thousand, a handful of items per case.

A case is a dict:
  name     id of the case (the suffix names the configuration: -dh1w62, -dh2w64, ...)
  rule     the rule of the list in LABNOTES.md it belongs to
  claim    what the case claims about itself, in words
  A, B     sim.SeqDb; B is A itself (the same object) for skip_self 2 and 3
  kw       the alignment options that differ from the oracle's defaults
  cand, ncand   oz.CAND_DTYPE[nitems, max_cand], int32[nitems]: the planted candidates, item = 2 * read + strand
  expect   {(item, slot): set of attempt states} the oracle's attempts log has to show (COVERED, ATTEMPTED, ...)
  check    optional callable(result) -> None asserting further claims on the oracle's result (boxes, counts)
  pair     name of the case on the other side of the rule: the two must differ in records or counters
  transposed  True: the call also asks for the transposed file (DH-2 mapping)
  overflow    True: more records than max_la slots (symmetric DH-1): the device returns a subset and reports the items
  pflags      True: A (= B) carries per-sequence flags saying which records of a symmetric DH-2 call are wanted (A.pflags)

A builder only builds.  Where a position depends on what an earlier attempt did (a region's box or its diagonal excursion),
the builder reads it from the ORACLE's attempts log; where a rule has no closed form on a constructed input (the x-drop that
just lets an extension pass, the longest indel a wave of `width` diagonals crosses) it searches the oracle's parameter or
input for the flip.  Nothing here looks at the code under test; tests/test_extend_cases.py asserts every claim on the
oracle."""
import functools

import numpy as np

from dentist_amd import sim
from oracle import pyoracle as oz

NOT_REACHED, COVERED, REJECTED, ACCEPTED = {0}, {1}, {2}, {3}
ATTEMPTED = {2, 3}
ATT = {n: i for i, n in enumerate(oz.ATT_FIELDS)}
CONFIGS = ((1, 64), (1, 32), (0, 62), (0, 30), (0, 14))   # (algo, width): k_tile 64 / 32, k_wave, k_wave2<32>, k_wave2<16>
BASE_KW = dict(k=14, min_len=40, max_cand=8, max_la=8, tspace=100)


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def differ(x):
    return np.uint8((int(x) + 1) % 4)


def subs(seq, positions):
    """a copy of seq with the bases at `positions` substituted"""
    s = np.array(seq, dtype=np.uint8)
    for p in positions:
        s[p] = differ(s[p])
    return s


def cat(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts])


def db(seqs):
    return sim.SeqDb.from_list([np.asarray(s, dtype=np.uint8) for s in seqs])


def tag(algo, width):
    return f"dh{2 if algo else 1}w{width}"


def case(name, rule, claim, A, B, kw, plants, expect=None, check=None, pair=None, transposed=False, overflow=False, pflags=False):
    """plants: {item: [(aseq, apos, bpos), ...]} in the order the extension takes them"""
    kw = dict(BASE_KW, **kw)
    need = max([len(v) for v in plants.values()] + [1])
    kw["max_cand"] = max(kw["max_cand"], need)
    nitems = 2 * B.n
    cand = np.zeros((nitems, kw["max_cand"]), dtype=oz.CAND_DTYPE)
    ncand = np.zeros(nitems, dtype=np.int32)
    for it, lst in plants.items():
        ncand[it] = len(lst)
        for c, (aseq, apos, bpos) in enumerate(lst):
            cand[it][c] = (100, aseq, apos, bpos, 0)
    return dict(name=name, rule=rule, claim=claim, A=A, B=B, kw=kw, cand=cand, ncand=ncand, expect=expect or {}, check=check,
                pair=pair, transposed=transposed, overflow=overflow, pflags=pflags)


class Result:
    """the oracle's answer to a case: records in item and slot order, trace, stats[4], attempts[nitems, max_cand, 9]"""

    def __init__(self, las, trace, stats, att, las2=None, trace2=None):
        self.las, self.trace, self.stats, self.att, self.las2, self.trace2 = las, trace, stats, att, las2, trace2

    def a(self, item, slot, field):
        return int(self.att[item][slot][ATT[field]])

    def box(self, item, slot):
        return tuple(self.a(item, slot, f) for f in ("abpos", "aepos", "bbpos", "bepos"))


def oracle_opts(kw):
    return oz.default_opts(**kw)


def run_oracle(c):
    out = oz.extend_candidates(c["A"], c["B"], oracle_opts(c["kw"]), c["cand"], c["ncand"], transposed=c["transposed"])
    if c["transposed"]:
        las, trace, stats, att, (las2, trace2) = out
        return Result(las, trace, stats, att, las2, trace2)
    return Result(*out)


_ORACLE = {}


def oracle(c):
    """the oracle's result of a case, computed once and shared by every test that needs it (never modified)"""
    if c["name"] not in _ORACLE:
        _ORACLE[c["name"]] = run_oracle(c)
    return _ORACLE[c["name"]]


def merged(x, y):
    z = dict(x)
    z.update(y)
    return z


def paired(lo, hi):
    lo["pair"], hi["pair"] = hi["name"], lo["name"]
    return [lo, hi]


# ------------------------------------------------------------------------------------------------ the covered rule
def island(seed, alen=1200, lo=200, hi=1000, flank=60, every=97):
    """a[lo:hi] with a substitution every `every` bases between two random flanks: one alignment of about hi - lo bases on
    diagonal lo - flank, through the seed ((lo + hi) / 2, flank + (hi - lo) / 2)"""
    a = rnd(seed, alen)
    b = cat(rnd(seed + 1, flank), subs(a[lo:hi], range(50, hi - lo, every)), rnd(seed + 2, flank))
    return a, b


def bulged(seed, g1, g2):
    """the island with two bulges: g1 bases of A missing in B at a = 350 and g1 extra at a = 500 (left of the seed: the path
    leaves the seed diagonal by +g1 in the REVERSE extension only and is back on it before it ends), g2 extra at a = 700
    and g2 missing at a = 850 (right: -g2 in the forward extension, between two trace points)"""
    a = rnd(seed, 1200)
    b = cat(rnd(seed + 1, 60), a[200:350], a[350 + g1:500], rnd(seed + 3, g1), a[500:700], rnd(seed + 4, g2), a[700:850],
            a[850 + g2:1000], rnd(seed + 2, 60))
    return a, b


def region_edges(algo, width, name, rule, a, b, extra_check=None):
    """one region, then a second candidate on either side of every face of the covered rule"""
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    A, B = db([a, a.copy()]), db([b])
    first = (0, 600, 460)
    base = case(f"{name}-first-{t}", rule, "the region of the first candidate, alone", A, B, kw, {0: [first]}, {(0, 0): ACCEPTED},
                check=extra_check)
    r = run_oracle(base)
    ab, ae, bb, be = r.box(0, 0)
    dlo, dhi = r.a(0, 0, "dlo"), r.a(0, 0, "dhi")
    out = [base]

    def edge(what, inside, outside):
        out.extend(paired(
            case(f"{name}-{what}-in-{t}", rule, f"second candidate {inside}: covered", A, B, kw, {0: [first, inside]},
                 {(0, 0): ACCEPTED, (0, 1): COVERED}),
            case(f"{name}-{what}-out-{t}", rule, f"second candidate {outside}: attempted", A, B, kw, {0: [first, outside]},
                 {(0, 0): ACCEPTED, (0, 1): ATTEMPTED})))

    edge("abpos", (0, ab, bb + 20), (0, ab - 1, bb + 20))
    edge("aepos", (0, ae - 1, be - 20), (0, ae, be - 20))
    edge("bbpos", (0, ab + 20, bb), (0, ab + 20, bb - 1))
    edge("bepos", (0, ae - 20, be - 1), (0, ae - 20, be))
    edge("dlo", (0, 600, 600 - (dlo - 64)), (0, 600, 600 - (dlo - 65)))
    edge("dhi", (0, 600, 600 - (dhi + 64)), (0, 600, 600 - (dhi + 65)))
    edge("aseq", (0, 650, 510), (1, 650, 510))
    return out


def covered_rule(algo, width):
    a, b = island(11)
    out = region_edges(algo, width, "cov", "covered rule: box and diagonal range", a, b)
    g1, g2 = (8, 10) if width >= 30 else (3, 4)   # (what a wave of 14 diagonals still follows)
    a, b = bulged(21, g1, g2)

    def excursion(r):
        ab, ae, bb, be = r.box(0, 0)
        assert abs(ab - bb - 140) < min(g1, g2) and abs(ae - be - 140) < min(g1, g2), "both ends on the seed diagonal (or a few random matches off it)"
        assert r.a(0, 0, "dhi") >= 140 + g1 and r.a(0, 0, "dlo") <= 140 - g2, "the extremes lie inside the path, not at its ends"
        assert ab < 340 and ae > 870, "the path runs through both bulges"

    out += region_edges(algo, width, "bulge", "covered rule: excursion of the reverse half / at trace points only", a, b, excursion)
    return out


def kth_region(algo, width):
    """k - 1 rejected attempts on k - 1 other A sequences, then the region, then a candidate only that region covers"""
    t = tag(algo, width)
    a, b = island(31)
    out = []
    for k in (1, 16, 17, 32, 33, 63, 64):
        junk = [rnd(1000 + j, 40) for j in range(k - 1)]
        A, B = db([a] + junk), db([b])
        head = [(1 + j, 20, 20 + j) for j in range(k - 1)] + [(0, 600, 460)]
        kw = dict(algo=algo, width=width, max_cand=80)
        exp = {(0, j): REJECTED for j in range(k - 1)}
        exp[(0, k - 1)] = ACCEPTED
        rule = "covered rule: the k-th region (slot boundaries 16 | 17, 32 | 33, 63 | 64)"
        if k == 64:
            out.append(case(f"region{k}-{t}", rule, "the 64th attempt is the last: the candidate behind it is not looked at", A, B, kw,
                            {0: head + [(0, 650, 510)]}, merged(exp, {(0, k): NOT_REACHED}),
                            check=lambda r: (_eq(r.stats[2], 64), _eq(len(r.las), 1))))
            continue
        out += paired(case(f"region{k}-in-{t}", rule, f"covered by region {k} alone", A, B, kw, {0: head + [(0, 650, 510)]},
                           merged(exp, {(0, k): COVERED})),
                      case(f"region{k}-out-{t}", rule, f"just behind region {k}'s A end: attempted", A, B, kw,
                           {0: head + [(0, run_oracle(case("x", "", "", A, B, kw, {0: [(0, 600, 460)]})).box(0, 0)[1], 900)]},
                           merged(exp, {(0, k): ATTEMPTED})))
    return out


def _eq(x, y):
    assert int(x) == int(y), (int(x), int(y))


# ------------------------------------------------------------------------------------------- attempt cap and max_la
def pieces(seed, n, step=20, ln=50):
    """B = one read, A = n exact copies of `ln` bases of it, `step` apart; candidate j = (j, ln / 2, step * j + ln / 2)"""
    b = rnd(seed, step * n + ln + 40)
    A = [b[step * j:step * j + ln] for j in range(n)]
    good = [(j, ln // 2, step * j + ln // 2) for j in range(n)]
    return A, b, good


def caps(algo, width):
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    rule = "attempt cap and max_la"
    out = []
    A, b, good = pieces(41, 70)
    dA, dB = db(A), db([b, rnd(42, 90), b])   # (read 1 has no candidate at all)
    out.append(case(f"cap70-{t}", rule, "70 acceptable candidates on 70 sequences: 64 attempted, 64 records", dA, dB,
                    dict(kw, max_cand=80, max_la=100), {0: good},
                    merged({(0, j): ACCEPTED for j in range(64)}, {(0, j): NOT_REACHED for j in range(64, 70)}),
                    check=lambda r: (_eq(r.stats[2], 64), _eq(len(r.las), 64))))
    out.append(case(f"cap63-{t}", rule, "63 candidates: all attempted (the other side of the cap)", dA, dB,
                    dict(kw, max_cand=80, max_la=100), {0: good[:63], 4: good[60:]},
                    {(0, j): ACCEPTED for j in range(63)}, check=lambda r: (_eq(r.stats[2], 73), _eq(len(r.las), 73))))
    paired(out[-2], out[-1])
    # rejected attempts count towards the 64, not towards max_la
    wrong = [(j, 25, (20 * j + 700) % 1300 + 30) for j in range(62)]
    out.append(case(f"cap-rejected-{t}", rule, "62 rejected attempts, then acceptable ones: two fit under the cap, max_la 4 is not reached",
                    dA, dB, dict(kw, max_cand=80, max_la=4), {0: wrong + good[62:]},
                    merged({(0, j): REJECTED for j in range(62)}, {(0, 62): ACCEPTED, (0, 63): ACCEPTED, (0, 64): NOT_REACHED}),
                    check=lambda r: (_eq(r.stats[2], 64), _eq(len(r.las), 2))))
    # covered candidates count towards neither
    cov = [(0, 20 + j, 20 + j) for j in range(10)]
    plan = [good[0]] + cov + [(1, 25, 600)] + good[2:6]
    exp = {(0, 0): ACCEPTED, (0, 11): REJECTED, (0, 12): ACCEPTED, (0, 13): ACCEPTED, (0, 14): NOT_REACHED, (0, 15): NOT_REACHED}
    exp.update({(0, 1 + j): COVERED for j in range(10)})
    out.append(case(f"cap-covered-{t}", rule, "covered and rejected candidates do not use up max_la = 3", dA, dB,
                    dict(kw, max_cand=80, max_la=3), {0: plan}, exp, check=lambda r: (_eq(r.stats[2], 4), _eq(len(r.las), 3))))
    for m in (1, 2, 3):
        exp = {(0, j): ACCEPTED if j < m else NOT_REACHED for j in range(5)}
        out.append(case(f"maxla{m}-{t}", rule, f"max_la = {m}: {m} records, the acceptable rest is not reached", dA, dB,
                        dict(kw, max_la=m), {0: good[:5], 5: []}, exp, check=lambda r, m=m: (_eq(r.stats[2], m), _eq(len(r.las), m))))
    paired(out[-3], out[-2])   # (max_la 1 | 2; max_la 3 stands by its counts)
    out.append(case(f"all-covered-{t}", rule, "every candidate behind the first is covered by it", dA, dB, kw, {4: [good[3]] + [(3, 10 + 5 * j, 70 + 5 * j) for j in range(6)]},
                    merged({(4, 0): ACCEPTED}, {(4, 1 + j): COVERED for j in range(6)}), check=lambda r: _eq(r.stats[2], 1)))
    return out


# ------------------------------------------------------------------------------------------------------- acceptance
def acceptance(algo, width):
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    out = []
    b = rnd(51, 400)
    rule = "acceptance: min_len"
    for ln, st in ((49, REJECTED), (50, ACCEPTED)):
        out.append(case(f"minlen-{ln}-{t}", rule, f"a whole A sequence of {ln} bases at min_len 50", db([b[100:100 + ln], rnd(52, 64)]), db([b]),
                        dict(kw, min_len=50), {0: [(0, 20, 120)]}, {(0, 0): st},
                        check=lambda r, ln=ln: _eq(r.a(0, 0, "aepos") - r.a(0, 0, "abpos"), ln)))
    paired(out[-2], out[-1])
    rule = "acceptance: error bound"
    for nd, pos, st in ((5, (5, 14, 23, 32, 41), ACCEPTED), (6, (5, 14, 23, 32, 37, 42), REJECTED)):
        def chk(r, nd=nd):
            ab, ae, bb, be = r.box(0, 0)
            assert (ae - ab, be - bb, r.a(0, 0, "diffs")) == (50, 50, nd)
        out.append(case(f"err-{nd}-{t}", rule, f"2 * {nd} * 10^6 against 100000 * (50 + 50)", db([subs(b[100:150], pos), rnd(52, 64)]), db([b]),
                        dict(kw, max_err_ppm=100000), {0: [(0, 27, 127)]}, {(0, 0): st}, check=chk))
    paired(out[-2], out[-1])

    def empty(r):
        assert r.a(0, 0, "aepos") == r.a(0, 0, "abpos") and len(r.las) == 1 and r.las[0]["aepos"] == r.las[0]["abpos"]
    out.append(case(f"minlen0-empty-{t}", "acceptance: min_len 0, both extensions empty", "a candidate between sequences that share no base: the zero-length record is kept",
                    db([np.zeros(120, np.uint8), rnd(52, 64)]), db([np.ones(120, np.uint8)]), dict(kw, min_len=0), {0: [(0, 60, 60)]},
                    {(0, 0): ACCEPTED}, check=empty))
    return out


# ---------------------------------------------------------------------------------------------------- sequence ends
def sequence_ends(algo, width):
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    rule = "sequence ends"
    a = rnd(61, 300)
    same = subs(a, (100, 200))
    inside = cat(rnd(62, 50), a, rnd(63, 50))
    A = db([a])
    B = db([same, same, inside, inside, a[100:]])

    def chk(r):
        assert r.box(0, 0) == (0, 300, 0, 300) and r.box(2, 0) == (0, 300, 0, 300)
        assert r.box(4, 0) == (0, 300, 50, 350) and r.box(8, 0) == (100, 300, 0, 200)
        assert r.a(6, 0, "aepos") == 300   # (nothing lies behind the end of A)
    out = [case(f"ends-{t}", rule, "candidates at (0, 0), (alen, blen), (alen, x) on and off the match, (x, 0)", A, B, kw,
                {0: [(0, 0, 0)], 2: [(0, 300, 300)], 4: [(0, 300, 350)], 6: [(0, 300, 200)], 8: [(0, 100, 0)]},
                {(0, 0): ACCEPTED, (2, 0): ACCEPTED, (4, 0): ACCEPTED, (6, 0): REJECTED, (8, 0): ACCEPTED}, check=chk)]
    # one base, seven bases, ten bases (fewer than W / 2); B ending inside a tile, A ending inside the first tile
    s7, s10 = np.array([1, 2, 3, 0, 1, 2, 3], np.uint8), rnd(64, 10)
    A = db([[2], s7, s10, rnd(65, 64)])
    B = db([[2], cat(rnd(66, 20), s7, rnd(67, 20)), s10, cat(rnd(68, 30), [2], rnd(69, 30))])

    def tiny(r):
        assert r.box(0, 0) == (0, 1, 0, 1) and r.box(2, 0)[:2] == (0, 7) and r.box(4, 0) == (0, 10, 0, 10)
        assert r.box(6, 0)[:2] == (0, 1) and r.box(2, 1)[1] <= 1
    out.append(case(f"tiny-{t}", rule, "sequences of 1, 7 and 10 bases, whole and inside a longer read", A, B, dict(kw, min_len=1),
                    {0: [(0, 0, 0)], 2: [(1, 3, 23), (0, 0, 5)], 4: [(2, 5, 5)], 6: [(0, 0, 30)]},
                    {(0, 0): ACCEPTED, (2, 0): ACCEPTED, (4, 0): ACCEPTED, (6, 0): ACCEPTED}, check=tiny))
    return out


def neighbours(algo, width):
    """A = [filler, X, Y], B = [filler, XY]: the alignment on X ends with X although the DB goes on with Y, which B matches as
    well, and the one on Y begins with Y.  The fillers put X, Y and the read on every 2-bit phase and around the edges of
    the 32-base plane words"""
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    out = []
    for fa, fb, lx in ((32, 32, 150), (33, 34, 150), (34, 35, 160), (35, 33, 150), (63, 32, 160), (32, 63, 150), (64, 65, 128), (65, 64, 150)):
        x, y = rnd(70 + fa, lx), rnd(71 + fb, 160)
        A = db([rnd(72, fa), x, y])
        B = db([rnd(73, fb), subs(cat(x, y), (40, lx + 100))])

        def chk(r, lx=lx):
            assert r.box(2, 0) == (0, lx, 0, lx) and r.box(2, 1) == (0, 160, lx, lx + 160)
        out.append(case(f"neighbour-{fa}-{fb}-{lx}-{t}", "sequence ends: the neighbour in the DB continues the match; packed phases",
                        f"A starts at base {fa}, B at {fb}: the alignments stop at the ends of X ({lx} bases) and Y", A, B, kw,
                        {2: [(1, 75, 75), (2, 80, lx + 80)]}, {(2, 0): ACCEPTED, (2, 1): ACCEPTED}, check=chk))
    return out


def match_runs(algo, width):
    """exact runs of 31 ... 65 matches from the seed on: ending at a mismatch, and ending with the sequence while the next
    sequence of the DB continues the match; a leading filler moves the whole DB through the four 2-bit phases"""
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    runs = (31, 32, 33, 63, 64, 65)
    out = []
    for f in range(4):
        As, Bs, As2, Bs2, plants, plants2 = [rnd(80, 32 + f)], [rnd(81, 35 - f)], [rnd(80, 32 + f)], [rnd(81, 35 - f)], {}, {}
        for j, n in enumerate(runs):
            s = rnd(82 + j, 40 + n + 61)
            As.append(s)
            Bs.append(subs(s, (40 + n,)))
            plants[2 * (1 + j)] = [(1 + j, 40, 40)]
            nxt = rnd(90 + j, 60)
            As2 += [s[:40 + n], nxt]
            Bs2.append(cat(s[:40 + n], nxt))
            plants2[2 * (1 + j)] = [(1 + 2 * j, 40, 40)]

        def chk(r):
            for j, n in enumerate(runs):
                assert r.box(2 * (1 + j), 0) == (0, 40 + n + 61, 0, 40 + n + 61) and r.a(2 * (1 + j), 0, "diffs") == 1

        def chk2(r):
            for j, n in enumerate(runs):
                assert r.box(2 * (1 + j), 0) == (0, 40 + n, 0, 40 + n) and r.a(2 * (1 + j), 0, "diffs") == 0
        out.append(case(f"runs-mismatch-{f}-{t}", "packed phases and run lengths", "runs of 31 ... 65 matches ending at one mismatch", db(As), db(Bs), kw,
                        plants, {(it, 0): ACCEPTED for it in plants}, check=chk))
        out.append(case(f"runs-seqend-{f}-{t}", "packed phases and run lengths", "runs of 31 ... 65 matches ending with the A sequence", db(As2), db(Bs2), kw,
                        plants2, {(it, 0): ACCEPTED for it in plants2}, check=chk2))
    return out


# -------------------------------------------------------------------------------------------------------- trace grid
def trace_grid(algo, width):
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    rule = "trace grid"
    a, b = island(101)
    out = [case(f"grid-apos-{t}", rule, "apos mod tspace = 0, 1, tspace - 1", db([a]), db([b, b, b]), kw,
                {0: [(0, 600, 460)], 2: [(0, 601, 461)], 4: [(0, 599, 459)]}, {(0, 0): ACCEPTED, (2, 0): ACCEPTED, (4, 0): ACCEPTED})]
    read = cat(rnd(102, 30), a[:301], rnd(103, 30))
    out.append(case(f"grid-alen-{t}", rule, "alen = 3 tspace - 1, 3 tspace, 3 tspace + 1", db([a[:299], a[:300], a[:301]]), db([read] * 3), kw,
                    {0: [(0, 150, 180)], 2: [(1, 150, 180)], 4: [(2, 150, 180)]}, {(0, 0): ACCEPTED, (2, 0): ACCEPTED, (4, 0): ACCEPTED},
                    check=lambda r: [_eq(r.box(2 * j, 0)[1], 299 + j) for j in range(3)]))
    for ts in (16, 128):
        out.append(case(f"grid-tspace{ts}-{t}", rule, f"tspace = {ts}", db([a]), db([b, sim.revcomp(b)]), dict(kw, tspace=ts),
                        {0: [(0, 600, 460)], 3: [(0, 601, 461)]}, {(0, 0): ACCEPTED, (3, 0): ACCEPTED}))
    if algo == 0:
        out.append(case(f"grid-tspace-long-{t}", rule, "DH-1: tspace larger than both sequences", db([a[:300]]), db([read]), dict(kw, tspace=1000),
                        {0: [(0, 150, 180)]}, {(0, 0): ACCEPTED}, check=lambda r: _eq(r.las[0]["tlen"], 2)))
    out.append(case(f"grid-strand1-{t}", rule, "items of strand 1 (the read is the reverse complement of what matches)", db([a]),
                    db([sim.revcomp(b), sim.revcomp(b[:843])]), kw, {1: [(0, 600, 460)], 3: [(0, 600, 460)]},
                    {(1, 0): ACCEPTED, (3, 0): ACCEPTED}))
    return out


# ------------------------------------------------------------------------------------------------------------ x-drop
def xdrop_cases(algo, width):
    t = tag(algo, width)
    kw = dict(algo=algo, width=width)
    rule = "x-drop"
    m = 70 if algo else 12
    a = rnd(111, 200 + m + 300)
    b = subs(a, range(200, 200 + m))
    A, B = db([a]), db([b])

    def passes(x):
        return run_oracle(case("x", "", "", A, B, dict(kw, xdrop=x), {0: [(0, 100, 100)]})).box(0, 0)[1] == len(a)
    lo, hi = 0, 600   # the smallest x-drop at which the extension survives the bad stretch (passes() is monotone in x)
    assert not passes(lo) and passes(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if passes(mid) else (mid, hi)
    out = paired(case(f"xdrop-pass-{t}", rule, f"{m} mismatches in a row: at xdrop {hi} the score falls to best - xdrop and the extension goes on",
                      A, B, dict(kw, xdrop=hi), {0: [(0, 100, 100)]}, {(0, 0): ACCEPTED}, check=lambda r: _eq(r.box(0, 0)[1], len(a))),
                 case(f"xdrop-stop-{t}", rule, f"the same at xdrop {lo}: one below, the extension stops at the best point", A, B,
                      dict(kw, xdrop=lo), {0: [(0, 100, 100)]}, {(0, 0): ACCEPTED}, check=lambda r: _eq(r.box(0, 0)[1], 200)))
    ia, ib = island(112)
    out.append(case(f"xdrop0-{t}", rule, "xdrop = 0", db([ia]), db([ib]), dict(kw, xdrop=0), {0: [(0, 600, 460)]}, {(0, 0): ATTEMPTED}))
    if algo == 1:
        # an end point inside the last tile against the best boundary (at a = 200): equal (it stays), one more, two more
        s = rnd(113, 204)
        s[200:204] = (0, 1, 2, 3)   # (no two neighbours alike: the rows next to the end point do not tie with it)
        q = np.uint8(3)
        ends = (("equal", s[:203], cat(subs(s[:203], (200,)), rnd(114, 20)), 200),
                ("one-more", s[:203], cat(s[:201], [q], s[201:203]), 203),
                ("two-more", s[:204], cat(subs(s[:204], (200,)), rnd(114, 20)), 204))
        got = []
        for name, sa, sb, ae in ends:
            got.append(case(f"endpoint-{name}-{t}", "x-drop: DH-2 end point inside the last tile", f"the end point scores {name} than / to the best boundary: aepos {ae}",
                            db([sa]), db([sb]), kw, {0: [(0, 100, 100)]}, {(0, 0): ACCEPTED}, check=lambda r, ae=ae: _eq(r.box(0, 0)[1], ae)))
        out += paired(got[0], got[1]) + [got[2]]
    return out


# -------------------------------------------------------------------------------------------------------- DH-1 only
def dh1_only():
    out = []
    rule = "DH-1: dmax"
    a = rnd(121, 200)
    for nd, pos in ((5, (110, 125, 140, 155, 170)), (6, (110, 125, 140, 155, 170, 185))):
        def chk(r, nd=nd):
            assert r.box(0, 0)[1] == (200 if nd == 5 else 185) and r.a(0, 0, "diffs") == 5
        out.append(case(f"dmax5-{nd}diffs", rule, f"an extension that needs {nd} differences at dmax 5", db([a]), db([subs(a, pos)]),
                        dict(algo=0, width=62, dmax=5), {0: [(0, 50, 50)]}, {(0, 0): ACCEPTED}, check=chk))
    paired(out[-2], out[-1])
    # the longest run of extra bases a wave of `width` diagonals crosses, and one base more: extra bases in B need the
    # diagonals below the seed's, extra bases in A those above; when the window is cut at equal edge scores the LOW edge
    # goes, so the two directions differ
    rule = "DH-1: width (14 | 15 and 30 | 31 switch the kernel) and the edge that goes at equal scores"
    p, q = rnd(122, 150), rnd(123, 250)
    for w in (1, 2, 5, 14, 15, 30, 31, 62):
        for side in ("ins", "del"):
            def build(g, w=w, side=side):
                extra = rnd(124, g)
                sa, sb = (cat(p, q), cat(p, extra, q)) if side == "ins" else (cat(p, extra, q), cat(p, q))
                return case(f"width{w}-{side}{g}", rule, f"{g} extra bases in {'B' if side == 'ins' else 'A'} at width {w}", db([sa]), db([sb]),
                            dict(algo=0, width=w, xdrop=2000), {0: [(0, 75, 75)]}, {(0, 0): ACCEPTED})

            def crosses(c):
                r = run_oracle(c)
                return r.box(0, 0)[1] == c["A"].length(0) and r.box(0, 0)[3] == c["B"].length(0)
            g = 0
            while g <= 72 and crosses(build(g)):
                g += 1
            if 1 <= g <= 72:
                lo, hi = build(g - 1), build(g)
                lo["check"] = lambda r, c=lo: _eq(r.box(0, 0)[1], c["A"].length(0))
                hi["check"] = lambda r, c=hi: _eq(r.box(0, 0)[1] < c["A"].length(0) or r.box(0, 0)[3] < c["B"].length(0), 1)
                out += paired(lo, hi)
    rule = "DH-1: N against N and N against a base (byte path)"
    a = rnd(125, 300)
    an = a.copy()
    an[150] = 4
    out += paired(case("n-n", rule, "code 4 in both sequences: equal codes match", db([an]), db([an.copy()]), dict(algo=0, width=62), {0: [(0, 100, 100)]},
                       {(0, 0): ACCEPTED}, check=lambda r: _eq(r.a(0, 0, "diffs"), 0)),
                  case("n-base", rule, "code 4 against a base: a difference", db([an]), db([a]), dict(algo=0, width=62), {0: [(0, 100, 100)]},
                       {(0, 0): ACCEPTED}, check=lambda r: _eq(r.a(0, 0, "diffs"), 1)))
    return out


# -------------------------------------------------------------------------------------------------------- DH-2 only
def dh2_only(width):
    t = tag(1, width)
    kw = dict(algo=1, width=width)
    h = width // 2
    out = []
    rule = "DH-2: one indel of W/2 - 1 | W/2 | W/2 + 1 bases inside a tile"
    p, q = rnd(131, 205), rnd(132, 295)   # (early in its tile: the true path stays cheaper than a random one)
    for side in ("ins", "del"):
        got = []
        for g in (h - 1, h, h + 1):
            extra = rnd(133, g)
            sa, sb = (cat(p, q), cat(p, extra, q)) if side == "ins" else (cat(p, extra, q), cat(p, q))
            c = case(f"indel-{side}{g}-{t}", rule, f"{g} extra bases in {'B' if side == 'ins' else 'A'} inside the third tile", db([sa]), db([sb]), kw,
                     {0: [(0, 50, 50)]}, {(0, 0): ATTEMPTED})
            r = run_oracle(c)
            got.append((c, (r.box(0, 0)[1] == len(sa) and r.box(0, 0)[3] == len(sb), r.a(0, 0, "diffs") == g)))
        for (c0, f0), (c1, f1) in zip(got, got[1:]):
            if f0 != f1 and c0["pair"] is None and c1["pair"] is None:
                paired(c0, c1)
        out += [c for c, _ in got]
    a, g = rnd(134, 700), h - 4
    b = cat(a[:130], a[130 + g:230], a[230 + g:330], a[330 + g:430], a[430 + g:])

    def drift(r):
        assert r.box(0, 0)[:2] == (0, 700) and r.a(0, 0, "dhi") - r.a(0, 0, "dlo") >= 4 * g > h
    out.append(case(f"drift-{t}", "DH-2: drift that fits because the band re-centres at each tile", f"{g} bases of A missing in B in each of four tiles in a row",
                    db([a]), db([b]), kw, {0: [(0, 50, 50)]}, {(0, 0): ACCEPTED}, check=drift))
    A = db([np.zeros(300, np.uint8), np.tile(np.array([0, 1], np.uint8), 150)])
    B = db([np.zeros(250, np.uint8), np.tile(np.array([1, 0], np.uint8), 140)])
    out.append(case(f"ties-{t}", "DH-2: last-column ties on homopolymer and dinucleotide sequences", "every row of the last column ties", A, B, kw,
                    {0: [(0, 120, 100), (0, 10, 240)], 2: [(1, 121, 100), (1, 290, 3)]}, {(0, 0): ACCEPTED, (2, 0): ACCEPTED}))
    # tandem: a read against itself below the main diagonal
    units = (1, h - 1, h, h + 1)
    reads = [np.tile(rnd(135 + u, u), 400 // u + 1)[:400] for u in units]
    T = db(reads)
    out.append(case(f"tandem-{t}", "tandem (skip_self 3): apos - bpos = 1, W/2 - 1, W/2, W/2 + 1", "repeats of period 1, W/2 - 1, W/2, W/2 + 1 against themselves",
                    T, T, dict(kw, skip_self=3, strands=1), {2 * j: [(j, 150 + u, 150)] for j, u in enumerate(units)},
                    {(2 * j, 0): ATTEMPTED for j in range(4)}))
    # the transposed file of a mapping
    ia, ib = island(136)
    out.append(case(f"transposed-{t}", "transposed file", "a mapping with its second file: both strands, a read whose length is no multiple of tspace",
                    db([ia]), db([ib, sim.revcomp(ib[:843]), ib]), kw, {0: [(0, 600, 460)], 3: [(0, 600, 460)], 4: [(0, 300, 160), (0, 900, 760)]},
                    {(0, 0): ACCEPTED, (3, 0): ACCEPTED, (4, 0): ACCEPTED, (4, 1): COVERED}, transposed=True,
                    check=lambda r: _eq(len(r.las2), 3)))
    return out


# -------------------------------------------------------------------------------------------------------- symmetric
def symmetric(algo, width):
    t = tag(algo, width)
    kw = dict(algo=algo, width=width, skip_self=2, max_la=100)
    out = []
    g = rnd(141, 800)
    R = db([subs(g[0:400], (250, 330)), g[200:600], sim.revcomp(g[300:730])])
    out.append(case(f"sym-strands-{t}", "symmetric: the mirrored record of a strand-1 candidate", "three overlapping reads, one of them complemented", R, R, kw,
                    {2: [(0, 300, 100)], 5: [(0, 350, 50), (1, 200, 100), (1, 210, 110)]},
                    {(2, 0): ACCEPTED, (5, 0): ACCEPTED, (5, 1): ACCEPTED, (5, 2): COVERED}, check=lambda r: _eq(len(r.las), 6)))
    if algo == 1:
        # pflags: bit 0 = records with the sequence as A read are wanted, bit 1 = it may be the B read of a wanted record.
        # Read 1 carries one bit only: of every pair it belongs to exactly one record is wanted, the other of the two in the
        # other case; the attempts are the same (an unwanted record is not written, its alignment is not made)
        rule = "symmetric: pflags with bit 0 / bit 1 set on one side only (DH-2)"
        got = []
        for bit, wanted in ((2, {(0, 1), (2, 1), (0, 2), (2, 0)}), (1, {(1, 0), (1, 2), (0, 2), (2, 0)})):
            Rp = db([R.seq(i) for i in range(3)])
            Rp.pflags = np.array([3, bit, 3], dtype=np.uint8)

            def chk(r, wanted=wanted):
                assert {(int(x["aread"]), int(x["bread"])) for x in r.las} == wanted and len(r.las) == 4 and r.stats[2] == 3
            got.append(case(f"sym-pflags-bit{bit >> 1}-{t}", rule, f"read 1 has pflags {bit}: the records {sorted(wanted)} and no other", Rp, Rp, kw,
                            {2: [(0, 300, 100)], 5: [(0, 350, 50), (1, 200, 100), (1, 210, 110)]},
                            {(2, 0): ACCEPTED, (5, 0): ACCEPTED, (5, 1): ACCEPTED, (5, 2): COVERED}, check=chk, pflags=True))
        out += paired(got[0], got[1])
    s = rnd(142, 50)
    longer = np.insert(s, [8, 16, 24, 32, 40, 46], [differ(s[8]), differ(s[16]), differ(s[24]), differ(s[32]), differ(s[40]), differ(s[46])])
    P = db([longer, s, rnd(143, 64)])
    out.append(case(f"sym-one-passes-{t}", "symmetric: a pair of which one record passes acceptance (DH-2)", "56 bases against 50 at min_len 53: the transposed pair is accepted on its own in DH-2",
                    P, P, dict(kw, min_len=53), {2: [(0, 28, 25)]}, {(2, 0): ACCEPTED}, check=lambda r: _eq(len(r.las), 1 if algo else 2)))
    # a hub read with 65 partners; the candidates of the partners 0 and 62 are two each, the latter at the indices 63 and 64
    hub = rnd(144, 30 * 65 + 60)
    parts = [hub[30 * j:30 * j + 50] for j in range(65)]
    H = db(parts + [hub])
    plan = [(0, 10, 10), (0, 40, 40)] + [(j, 25, 30 * j + 25) for j in range(1, 62)] + [(62, 25, 30 * 62 + 25), (62, 5, 100)] + \
           [(63, 25, 30 * 63 + 25), (64, 25, 30 * 64 + 25)]
    exp = {(130, 0): ACCEPTED, (130, 1): COVERED, (130, 63): ACCEPTED, (130, 64): REJECTED, (130, 65): NOT_REACHED, (130, 66): NOT_REACHED}
    out.append(case(f"sym-hub-{t}", "symmetric: an item with 65 partners, two candidates of one partner at the indices 63 and 64",
                    "the 64th attempt is the second candidate of partner 62", H, H, dict(kw, max_cand=80), {130: plan}, exp,
                    check=lambda r: (_eq(r.stats[2], 64), _eq(len(r.las), 126))))
    if algo == 0:
        out.append(case(f"sym-overflow-{t}", "symmetric: DH-1 with fewer slots than records", "the hub gets 10 records at max_la 4: a subset, the items reported",
                        H, H, dict(kw, max_la=4, max_cand=80), {130: [(j, 25, 30 * j + 25) for j in range(10)]},
                        {(130, j): ACCEPTED for j in range(10)}, overflow=True))
    return out


# ------------------------------------------------------------------------------------------------------------- all
@functools.lru_cache(maxsize=None)
def all_cases():
    out = []
    for algo, width in CONFIGS:
        for build in (covered_rule, kth_region, caps, acceptance, sequence_ends, neighbours, match_runs, trace_grid, xdrop_cases, symmetric):
            out += build(algo, width)
        if algo == 1:
            out += dh2_only(width)
    out += dh1_only()
    names = [c["name"] for c in out]
    assert len(names) == len(set(names)), "case names are unique"
    return tuple(out)


def by_name():
    return {c["name"]: c for c in all_cases()}
