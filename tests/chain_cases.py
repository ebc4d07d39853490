"""The shapes the chaining tests share (CPU harness, reference restatement, GPU parity, tool), seeded.

random_case(): pairs of a forward run and a shorter complement run whose successors are abutting with an indel up to +-1 100
(both sides of max_indel), overlapping by 5-50 % (both sides of 0.3), starting where their predecessor starts (ties), or
jumping 9-14 kb (both sides of max_chain_gap: new components); 5 % more records are disabled; the records of a pair are
shuffled; several bread share an aread.  SIZES are enabled records per pair.

HAND: cases small enough to work out on paper; their expected chains are written out, not computed."""
import numpy as np

LA_DTYPE = np.dtype([("tlen", "<i4"), ("diffs", "<i4"), ("abpos", "<i4"), ("bbpos", "<i4"), ("aepos", "<i4"), ("bepos", "<i4"),
                     ("flags", "<u4"), ("aread", "<i4"), ("bread", "<i4"), ("pad", "<i4"), ("toff", "<i8")])
COMP, START, NEXT, BEST, DISABLED = 0x1, 0x4, 0x8, 0x10, 0x20
TSPACE = 100
SIZES = (1, 2, 3, 9, 63, 64, 65, 200)
# (min_relative_score, min_score)
OPTION_SETS = ((1.0, 100), (0.5, 100), (0.0, 100), (0.8, 2500))


def opts_of(rel, min_score):
    return dict(min_relative_score=rel, min_score=min_score)


def _run(rng, n, comp):
    """n records of one strand: (abpos, aepos, bbpos, bepos, flags)"""
    out = []
    ab, bb = int(rng.integers(0, 3000)), int(rng.integers(5000, 9000))
    la = int(rng.integers(600, 3000))
    lb = la + int(rng.integers(-30, 31))
    out.append((ab, ab + la, bb, bb + lb))
    for _ in range(n - 1):
        pab, pae, pbb, pbe = out[-1]
        la = int(rng.integers(600, 3000))
        lb = la + int(rng.integers(-30, 31))
        kind = rng.choice(4, p=[0.45, 0.25, 0.15, 0.15])
        if kind == 0:    # abutting, an indel on B
            g = int(rng.integers(0, 200))
            ab, bb = pae + g, max(pbb + 1, pbe + g + int(rng.integers(-1100, 1101)))
        elif kind == 1:  # overlapping
            f = rng.uniform(0.05, 0.5)
            ab = pae - int(f * min(pae - pab, la))
            bb = pbe - int(f * min(pbe - pbb, lb))
        elif kind == 2:  # the same start: a tie in the node order but for the index
            ab, bb = pab, pbb
        else:            # a jump
            g = int(rng.integers(9000, 14001))
            ab, bb = pae + g, pbe + g + int(rng.integers(-50, 51))
        out.append((ab, ab + la, bb, bb + lb))
    return [(a, b, c, d, comp) for a, b, c, d in out]


def make_pair(rng, aread, bread, size):
    """`size` enabled records (a forward run, a complement run of a third) and about 5 % disabled ones, shuffled"""
    ncomp = size // 3
    recs = _run(rng, size - ncomp, 0) + (_run(rng, ncomp, COMP) if ncomp else [])
    for _ in range(int(rng.binomial(size, 0.05)) + (1 if size == 1 else 0)):
        a, b, c, d, f = recs[int(rng.integers(0, size))]
        recs.append((a + 10, b + 10, c + 10, d + 10, f | DISABLED))
    rng.shuffle(recs)
    las = np.zeros(len(recs), dtype=LA_DTYPE)
    for i, (a, b, c, d, f) in enumerate(recs):
        las[i]["abpos"], las[i]["aepos"], las[i]["bbpos"], las[i]["bepos"], las[i]["flags"] = a, b, c, d, f
        las[i]["aread"], las[i]["bread"] = aread, bread
        las[i]["diffs"] = int(rng.integers(0, (b - a) // 5 + 1))
    return las


def random_case(seed=1, sizes=SIZES, reps=2):
    """pairs of every size, `reps` of each, three bread per aread, in (aread, bread) order"""
    rng = np.random.default_rng(seed)
    todo = [s for s in sizes for _ in range(reps)]
    rng.shuffle(todo)
    parts = [make_pair(rng, i // 3, 7 * (i % 3) + 1, s) for i, s in enumerate(todo)]
    return np.concatenate(parts)


def with_traces(las, seed=2):
    """tlen / toff and a trace array (values below 256) that fits the A intervals at TSPACE"""
    rng = np.random.default_rng(seed)
    las = las.copy()
    at = 0
    for la in las:
        ntp = -(-int(la["aepos"]) // TSPACE) - int(la["abpos"]) // TSPACE
        la["tlen"], la["toff"] = 2 * ntp, at
        at += 2 * ntp
    return las, rng.integers(0, 200, at).astype(np.uint16)


def _las(recs, aread=3, bread=5):
    las = np.zeros(len(recs), dtype=LA_DTYPE)
    for i, (a, b, c, d, f) in enumerate(recs):
        las[i]["abpos"], las[i]["aepos"], las[i]["bbpos"], las[i]["bepos"], las[i]["flags"] = a, b, c, d, f
        las[i]["aread"], las[i]["bread"] = aread, bread
    return las


SB, S, N = START | BEST, START, NEXT
assert 0.3 * 1000 == 300.0  # the overlap case below sits exactly on the bound

# name -> (records, options, expected chains as (record indices, flags, score))
HAND = {
    # r0 -> r2 chain (gap 100 on both: edge = 0 + 100 / 10 - 1000, distance -1990); r1 lies on the other strand
    "two chain, one on the other strand": (
        _las([(0, 1000, 0, 1000, 0), (500, 1500, 500, 1500, COMP), (1100, 2100, 1100, 2100, 0)]), {},
        [([0, 2], [SB, N], 1990)]),
    # ... at 0.5 the pair's threshold is 995 and the complement record's own chain (1000) is accepted too
    "the other strand at 0.5": (
        _las([(0, 1000, 0, 1000, 0), (500, 1500, 500, 1500, COMP), (1100, 2100, 1100, 2100, 0)]), dict(min_relative_score=0.5),
        [([0, 2], [SB, N], 1990), ([1], [SB | COMP], 1000)]),
    # r0 -> r1 (gap 100) and r0 -> r2 (gap 105) both cost 10 and weigh 1000: distance -1990 twice.  r1 comes first in the
    # node order and takes r0; r2's path runs into r0: an alternate chain of its whole path.  Order: last.aepos 2100 < 2105
    "a fork whose branches tie": (
        _las([(0, 1000, 0, 1000, 0), (1100, 2100, 1100, 2100, 0), (1105, 2105, 1105, 2105, 0)]), {},
        [([0, 1], [SB, N], 1990), ([0, 2], [S, N], 1990)]),
    # overlap 300 = 0.3 x 1000: chainable (<=); edge = 0 + 300 / 10 - 1000
    "overlap of exactly 0.3": (
        _las([(0, 1000, 0, 1000, 0), (700, 1700, 700, 1700, 0)]), {},
        [([0, 1], [SB, N], 1970)]),
    "overlap of 0.3 and one base": (
        _las([(0, 1000, 0, 1000, 0), (699, 1699, 699, 1699, 0)]), {},
        [([0], [SB], 1000), ([1], [SB], 1000)]),
    # gaps 100 and 1100: indel 1000 = max_indel; edge = 1000 + 1100 / 10 - 3000 = -1890
    "indel of exactly max_indel": (
        _las([(0, 3000, 0, 3000, 0), (3100, 6100, 4100, 7100, 0)]), {},
        [([0, 1], [SB, N], 4890)]),
    "indel of max_indel + 1": (
        _las([(0, 3000, 0, 3000, 0), (3100, 6100, 4101, 7101, 0)]), {},
        [([0], [SB], 3000), ([1], [SB], 3000)]),
    "the only record scores min_score - 1": (
        _las([(0, 99, 0, 99, 0)]), {},
        []),
}
