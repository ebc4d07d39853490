"""Constructed pile-ups for one consensus round (dh_consensus(..., rounds=1) / oracle.pyoracle.consensus /
consensus_ref.consensus): the generator of self-consistent records and trace pairs, the named cases and seeded random piles.

A spec describes one overlap of the template (read 0 of the pile): spec(read, a0, a1, ...).  pile() aligns every spec's
template interval to its read interval once with oz.nw, cuts the path at the multiples of the trace spacing and writes the
record and the trace pairs a local aligner could have reported for that path.

CASES: (id, family, function returning (template, specs, trace spacing)).  Only numpy, dentist_amd.sim and oracle.pyoracle
are used: no GPU."""
import functools

import numpy as np

from dentist_amd import sim
from oracle import pyoracle as oz

LA_DTYPE = oz.LA_DTYPE
COMP, DISABLED = 0x1, 0x20
MAXINS = oz.MAXINS
SEG_MAX = 250
TSPACES = (16, 100, 102, 103, 126, 127, 128, 250)
BLOCK_TILES = 64   # tiles per block of the fills and of the vote pass


# ---------------------------------------------------------------- generator
def overlap(tmpl, a0, a1, read, b0, b1, ts, ins_side="next", slack=0, comp=0, pairs=None):
    """One overlap of tmpl[a0:a1] with read[b0:b1] (`read` in the orientation of the overlap): (record, trace pairs,
    the read as the DB stores it).  ins_side: the tile that gets insertions lying exactly on an inner tile boundary -- "next":
    slot 0 of the following tile, "prev": the slot behind the last column of the preceding one.  slack: added to every
    tile's diffs (a trace's diffs are an upper bound of the tile's distance only).  comp: the DB holds the reverse complement
    and the record carries the COMP flag.  pairs: trace pairs to use as they are, unchecked (for the one malformed input)."""
    tmpl, read = np.asarray(tmpl, dtype=np.uint8), np.asarray(read, dtype=np.uint8)
    assert 0 <= a0 < a1 <= len(tmpl) and 0 <= b0 <= b1 <= len(read) and ins_side in ("next", "prev")
    first, ntile = a0 // ts, (a1 - 1) // ts - a0 // ts + 1
    if pairs is None:
        _, ops = oz.nw(tmpl[a0:a1], read[b0:b1])
        diffs, bb = [0] * ntile, [0] * ntile
        x, y = a0, b0
        for op in ops:
            if op == 2:
                t = min(x, a1 - 1) // ts
                if ins_side == "prev" and x % ts == 0 and a0 < x < a1:
                    t -= 1
                diffs[t - first] += 1
                bb[t - first] += 1
                y += 1
                continue
            t = x // ts - first
            if op == 0:
                diffs[t] += int(tmpl[x] != read[y])
                bb[t] += 1
                y += 1
            else:
                diffs[t] += 1
            x += 1
        assert x == a1 and y == b1
        pairs = np.asarray([[min(d + slack, 65535), b] for d, b in zip(diffs, bb)], dtype=np.uint16)
        # self-consistent: the B bases of the tiles are the read interval, the diffs bound every tile's distance from above
        assert int(pairs[:, 1].sum()) == b1 - b0
        for e in range(ntile):
            alen = min((first + e + 1) * ts, a1) - max((first + e) * ts, a0)
            assert int(pairs[e, 0]) >= abs(alen - int(pairs[e, 1]))
    else:
        pairs = np.asarray(pairs, dtype=np.uint16).reshape(-1, 2)
        assert len(pairs) == ntile
    la = np.zeros(1, dtype=LA_DTYPE)
    la["abpos"], la["aepos"], la["bbpos"], la["bepos"] = a0, a1, b0, b1
    la["tlen"], la["diffs"], la["flags"] = 2 * ntile, int(pairs[:, 0].astype(np.int64).sum()), COMP if comp else 0
    return la, pairs, (sim.revcomp(read) if comp else read)


def spec(read, a0, a1, b0=0, b1=None, ins_side="next", slack=0, comp=0, disabled=0, aread=0, pairs=None):
    read = np.asarray(read, dtype=np.uint8)
    return dict(read=read, a0=a0, a1=a1, b0=b0, b1=len(read) if b1 is None else b1, ins_side=ins_side, slack=slack, comp=comp,
                disabled=disabled, aread=aread, pairs=pairs)


def pile(tmpl, specs, ts):
    """(SeqDb with the template as read 0 and the read of spec i as read i + 1, records, trace) -- records in the order of
    the specs, aread 0 unless the spec says otherwise (such records are aligned to the template all the same)."""
    tmpl = np.asarray(tmpl, dtype=np.uint8)
    seqs, recs, tr = [tmpl], [], []
    toff = 0
    for i, s in enumerate(specs):
        la, pairs, stored = overlap(tmpl, s["a0"], s["a1"], s["read"], s["b0"], s["b1"], ts, s["ins_side"], s["slack"], s["comp"],
                                    s["pairs"])
        la["aread"], la["bread"], la["toff"] = s["aread"], i + 1, toff
        if s["disabled"]:
            la["flags"] |= DISABLED
        assert 0 <= la["bbpos"][0] <= la["bepos"][0] <= len(stored)
        seqs.append(stored)
        recs.append(la)
        tr.append(pairs.reshape(-1))
        toff += pairs.size
    las = np.ascontiguousarray(np.concatenate(recs)) if recs else np.zeros(0, dtype=LA_DTYPE)
    trace = np.ascontiguousarray(np.concatenate(tr)) if tr else np.zeros(0, dtype=np.uint16)
    return sim.SeqDb.from_list(seqs), las, trace


def voting(las, trace, aidx=0):
    """The records that take part in the vote of template `aidx`."""
    keep = []
    for i, la in enumerate(las):
        t = trace[la["toff"]:la["toff"] + la["tlen"]]
        if la["aread"] == aidx and not la["flags"] & DISABLED and (len(t) == 0 or t[1::2].max() <= SEG_MAX):
            keep.append(i)
    return keep


def band_classes(las, trace):
    """Tiles per fill, as the host sorts the voting overlaps: [bit-parallel one word, two words, scalar] by the largest
    tile diffs + 1 being at most 31, at most 63, or more."""
    n = [0, 0, 0]
    for i in voting(las, trace):
        la = las[i]
        dmax = int(trace[la["toff"]:la["toff"] + la["tlen"]][0::2].max())
        n[0 if dmax + 1 <= 31 else (1 if dmax + 1 <= 63 else 2)] += int(la["tlen"]) // 2
    return n


def vote_kernel(ts):
    """The k_seg_vote2 instantiation of a trace spacing: column sets of 13 or 16 words of eight columns, or 0 = byte-wise."""
    nw8 = ((ts + 2 + 7) & ~7) // 8
    return 13 if nw8 <= 13 else (16 if nw8 <= 16 else 0)


# ---------------------------------------------------------------- building blocks
def rnd(seed, n, alphabet=4):
    return np.random.default_rng(seed).integers(0, alphabet, n).astype(np.uint8)


def no_runs(seed, n):
    """Random bases without two equal neighbours."""
    s = rnd(seed, n)
    for i in range(1, n):
        if s[i] == s[i - 1]:
            s[i] = (s[i] + 1) % 4
    return s


def low_complexity(seed, n):
    """Homopolymer runs of 1 .. 9 bases, mostly of two letters."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        c = int(rng.integers(0, 2)) if rng.random() < 0.8 else int(rng.integers(0, 4))
        if out and out[-1] == c:
            c = (c + 1) % 4
        out += [c] * int(rng.integers(1, 10))
    return np.asarray(out[:n], dtype=np.uint8)


def noisy(rng, s, sub=0.04, ins=0.05, dele=0.04):
    out = []
    for b in s:
        x = rng.random()
        while x < ins:
            out.append(int(rng.integers(0, 4)))
            x = rng.random()
        x = rng.random()
        if x < dele:
            continue
        out.append(int((b + rng.integers(1, 4)) % 4) if x < dele + sub and b < 4 else int(b))
    return np.asarray(out, dtype=np.uint8)


def edited(tmpl, a0, a1, edits):
    """tmpl[a0:a1] with edits in template coordinates: (x, "s", base), (x, "d", columns), (x, "i", bases before column x)."""
    out = [[int(c)] for c in tmpl[a0:a1]] + [[]]
    pre = [[] for _ in range(a1 - a0 + 1)]
    for x, kind, arg in edits:
        assert a0 <= x <= a1
        if kind == "s":
            out[x - a0] = [int(arg)]
        elif kind == "d":
            for k in range(arg):
                out[x - a0 + k] = []
        else:
            pre[x - a0] = pre[x - a0] + [int(c) for c in arg]
    return np.asarray([c for p, o in zip(pre, out) for c in p + o], dtype=np.uint8)


def carriers(tmpl, edits, k, d, a0=0, a1=None, **kw):
    """d overlaps of tmpl[a0:a1]: k carry the edits, d - k are exact."""
    a1 = len(tmpl) if a1 is None else a1
    return [spec(edited(tmpl, a0, a1, edits if i < k else []), a0, a1, **kw) for i in range(d)]


def other(c, k=1):
    return (int(c) + k) % 4


# ---------------------------------------------------------------- the named cases
CASES = []


def case(family, cid, fn, *args, **kw):
    CASES.append((cid, family, functools.partial(fn, *args, **kw)))


# --- band classes: the same overlap at slack values that put its largest tile diffs on either side of the class borders
def _band_overlap():
    tmpl = rnd(101, 520)
    return tmpl, noisy(np.random.default_rng(102), tmpl, 0.04, 0.05, 0.04)


def band_case(target):
    """The noisy read twice, nothing else: two of two win every vote, so the consensus shows the whole alignment."""
    tmpl, read = _band_overlap()
    _, pairs, _ = overlap(tmpl, 0, len(tmpl), read, 0, len(read), 100)
    top = int(pairs[:, 0].max())
    assert top <= 29
    return tmpl, [spec(read, 0, len(tmpl), slack=target - top, comp=c) for c in (0, 1)], 100


def band_mixed():
    tmpl, _ = _band_overlap()
    rng = np.random.default_rng(103)
    specs = [spec(noisy(rng, tmpl[a0:a1], 0.04, 0.05, 0.04), a0, a1, slack=s, comp=c, ins_side=side)
             for a0, a1, s, c, side in ((0, 520, 0, 0, "next"), (37, 480, 30, 1, "prev"), (100, 520, 200, 0, "next"),
                                        (0, 301, 45, 0, "prev"), (199, 401, 5, 1, "next"), (3, 517, 60, 0, "next"))]
    return tmpl, specs, 100


def band_edge_case(kind, n, sub=0):
    """Three reads that differ from the template in the tile [100, 200) only: a block of n - sub deleted columns or inserted
    bases at its start (and one substitution near its end if sub = 1).  The tile's diffs are n and its optimal path runs
    n - sub cells off the diagonal through most of the tile: with sub = 0 as far out as a path of n diffs can go, the last
    cells the band of n + 1 is there for."""
    tmpl = rnd(104, 300)
    m = n - sub
    tmpl[95:125 + (m if kind == "del" else 0)] = 0
    block = 1 + rnd(105, m, 3)   # c / g / t among a's: the block pairs with nothing around it
    if kind == "del":
        tmpl[105:105 + m] = block
        e = [(105, "d", m)]
    else:
        e = [(105, "i", block)]
    return tmpl, carriers(tmpl, e + ([(197, "s", other(tmpl[197]))] if sub else []), 3, 3), 100


for _t in (29, 30, 31, 61, 62, 63, 240):
    case("band", f"band-dmax{_t}", band_case, _t)
for _k in ("del", "ins"):
    for _n in (30, 31, 62, 63, 90):
        case("band", f"band-edge-{_k}{_n}", band_edge_case, _k, _n)
        case("band", f"band-edge-{_k}{_n}-sub", band_edge_case, _k, _n, 1)
case("band", "band-mixed", band_mixed)


# --- launch edges: the tiles of one fill total 1, 63, 64, 65 (blocks of BLOCK_TILES)
def launch_parts(ntiles):
    """(template without runs, edits, tiles of the pair of reads): a substitution in every tile and a deleted column in every
    third one; with an odd number of tiles the last tile belongs to a read of its own that lacks one column."""
    ts = 16
    half = ntiles // 2
    tmpl = no_runs(110 + ntiles, ts * (half + ntiles % 2))
    edits = [(ts * t + 8, "s", other(tmpl[ts * t + 8])) for t in range(half)] + [(ts * t + 3, "d", 1) for t in range(0, half, 3)]
    return tmpl, edits + ([(ts * half + 5, "d", 1)] if ntiles % 2 else []), half


def launch_case(ntiles, slack):
    """Tiles in launch order: the pair's first read, its second read (complement), then the single read's tile.  Two of two
    reads win every vote and one read of one wins a deletion, so every tile's edit shows in the consensus: with 64 and 65
    tiles the last tile of the first block, with 65 the only tile of the second block."""
    ts = 16
    tmpl, edits, half = launch_parts(ntiles)
    specs = [spec(edited(tmpl, 0, ts * half, edits[:-1] if ntiles % 2 else edits), 0, ts * half, slack=slack, comp=c)
             for c in (0, 1)] if half else []
    if ntiles % 2:
        specs.append(spec(edited(tmpl, ts * half, len(tmpl), edits[-1:]), ts * half, len(tmpl), slack=slack))
    return tmpl, specs, ts


for _n in (1, 63, 64, 65):
    for _c, _s in enumerate((0, 40, 80)):
        case("launch", f"launch-{_n}tiles-class{_c}", launch_case, _n, _s)


# --- tile sides
def side_one_column(where):
    """Three overlaps whose first / last tile is one column wide, that column substituted in all of them."""
    tmpl = no_runs(120, 400)
    a0, a1, x = {"begin": (99, 250, 99), "end": (50, 201, 200), "first": (0, 1, 0), "last": (399, 400, 399)}[where]
    return tmpl, carriers(tmpl, [(x, "s", other(tmpl[x]))], 3, 3, a0, a1), 100


def side_empty_b():
    """Three reads that lack the whole tile [100, 200)."""
    # a / c outside the tile, g / t inside: a tile column paired with a read base is a mismatch, so every optimal alignment
    # deletes exactly the tile's columns
    tmpl = rnd(121, 400, 2)
    tmpl[100:200] = 2 + (np.arange(100) & 1)
    return tmpl, carriers(tmpl, [(100, "d", 100)], 3, 3) + carriers(tmpl, [], 0, 1), 100


def side_long_b(nb):
    """Three reads with nb B bases in the tile [126, 252) (a block of foreign bases in its middle) beside one exact read:
    at 251 they take no part and the exact read decides alone."""
    tmpl = rnd(122, 378)
    block = rnd(123, nb - 126)
    return tmpl, carriers(tmpl, [(189, "i", block)], 3, 3, 126, 252) + carriers(tmpl, [(40, "s", other(tmpl[40]))], 1, 1), 126


for _w in ("begin", "end", "first", "last"):
    case("sides", f"sides-one-column-{_w}", side_one_column, _w)
case("sides", "sides-empty-b", side_empty_b)
case("sides", "sides-b250", side_long_b, 250)
case("sides", "sides-b251", side_long_b, 251)


# --- trace spacings: the three vote kernels and their borders
def tspace_case(ts):
    """Homopolymer runs over the columns 60 .. 67 of the first and of the second tile (columns 63, 64, 65 inside: the border
    of the first column-set word) and over the last two columns of a full tile, shortened or lengthened in four of six
    reads; the other two are noisy partial overlaps."""
    n = max(3 * ts + 7, 135)
    tmpl = no_runs(130 + ts, n)
    runs = [(60, 68), (ts - 2, ts), (2 * ts - 2, 2 * ts)] + ([(ts + 60, ts + 68)] if ts >= 70 else [])
    for k, (r0, r1) in enumerate(runs):
        if r1 < n:
            tmpl[r0:r1] = other(tmpl[r0 - 1], 1 + (other(tmpl[r0 - 1]) == tmpl[r1]))
    # (as many columns deleted as bases inserted in the second tile, one deleted in the third, which gets the base inserted
    # on its border with "next": no tile has more B bases than columns, SEG_MAX at 250)
    edits = [(63, "d", 1), (ts - 1, "d", 1), (ts + 5, "d", 1), (2 * ts - 1, "i", [tmpl[2 * ts - 1]]), (2 * ts + 5, "d", 1)]
    if ts >= 70:
        edits += [(ts + 10, "d", 2), (ts + 65, "i", [tmpl[ts + 65]] * 2)]
    rng = np.random.default_rng(131 + ts)
    specs = carriers(tmpl, edits, 2, 2) + carriers(tmpl, edits, 2, 2, ins_side="prev", slack=33)
    rates = (0.04, 0.02, 0.06) if ts == SEG_MAX else (0.04, 0.05, 0.04)
    specs.append(spec(noisy(rng, tmpl[5:n - 3], *rates), 5, n - 3, comp=1))
    specs.append(spec(noisy(rng, tmpl[ts - 1:2 * ts + 1], *rates), ts - 1, 2 * ts + 1, slack=70))
    return tmpl, specs, ts


def tspace_pair_case(ts, seed=0):
    """A low-complexity template and noisy reads that are each there twice and share no column with another pair: two of two
    reads win every vote, so the consensus shows every column and slot of every tile as the passes left it.  The two copies
    differ in their diffs only (the one-word bit-parallel fill and the scalar one)."""
    n = max(3 * ts + 7, 135)
    tmpl = low_complexity(230 + ts + 1000 * seed, n)
    rng = np.random.default_rng(231 + ts + 1000 * seed)
    specs = []
    for a0, a1, comp, side in ((0, 2 * ts, 0, "next"), (2 * ts, n, 1, "prev")):
        read = noisy(rng, tmpl[a0:a1], 0.04, 0.01 if ts == SEG_MAX else 0.04, 0.07 if ts == SEG_MAX else 0.04)   # (B sides within SEG_MAX)
        specs += [spec(read, a0, a1, comp=comp, ins_side=side, slack=sl) for sl in (0, 70)]
    return tmpl, specs, ts


for _t in TSPACES:
    case("tspace", f"tspace-{_t}", tspace_case, _t)
    for _s in range(3):
        case("tspace", f"tspace-pair{_s}-{_t}", tspace_pair_case, _t, _s)


# --- insertions
def ins_case(n, kind, place, side, ts=100):
    """Three of three reads insert n bases: copies of the run's base, of the previous run's base, or foreign and mixed; at slot
    0 of a tile, behind a tile's last column (an overlap that ends there), or behind the template's last column."""
    end = 3 * ts
    tmpl = no_runs(140, end)
    x = {"slot0": ts, "tile-end": 2 * ts, "template-end": end}[place]
    a0, a1 = {"slot0": (0, end), "tile-end": (40, 2 * ts), "template-end": (ts + 20, end)}[place]
    if kind == "run":
        bases = [tmpl[x] if x < end else tmpl[x - 1]] * n
    elif kind == "prev":
        bases = [tmpl[x - 1]] * n
    else:
        avoid = {int(tmpl[x - 1]), int(tmpl[min(x, end - 1)])}
        pool = [c for c in range(4) if c not in avoid]
        bases = [pool[t % 2] for t in range(n)]
    return tmpl, carriers(tmpl, [(x, "i", bases)], 3, 3, a0, a1, ins_side=side), ts


for _n in (1, 4, 5, 9):
    for _k in ("run", "prev", "foreign"):
        for _p in ("slot0", "tile-end", "template-end"):
            for _s in ("next", "prev"):
                case("ins", f"ins-{_n}-{_k}-{_p}-{_s}", ins_case, _n, _k, _p, _s)
# ... and the foreign ones at trace spacings of the other two vote kernels
for _t in (126, 128):
    for _n in (1, 4, 5):
        for _p in ("slot0", "tile-end", "template-end"):
            for _s in ("next", "prev"):
                case("ins", f"ins-{_n}-foreign-{_p}-{_s}-ts{_t}", ins_case, _n, "foreign", _p, _s, _t)


def ins_leading(side):
    """Overlaps that begin with inserted copies of the base in front of them: votes for the previous run's base in the slot of
    a run's first column, which belong to the previous run's length."""
    tmpl = no_runs(141, 300)
    specs = [spec(np.concatenate([[tmpl[99]], tmpl[100:300]]), 100, 300, ins_side=side) for _ in range(3)]
    return tmpl, specs + carriers(tmpl, [], 0, 3), 100


for _s in ("next", "prev"):
    case("ins", f"ins-leading-prev-base-{_s}", ins_leading, _s)


# --- homopolymers
def homo_parts(kind, delta, ts=100):
    """(template with the run, the edit that changes the run's length by delta)"""
    end = 3 * ts + 30
    tmpl = no_runs(150, end)
    if kind == "boundary":          # a run of 8 over the first tile boundary
        r0, r1 = ts - 4, ts + 4
    elif kind == "long":            # a run longer than a tile
        r0, r1 = ts - 10, 2 * ts + 15
    elif kind == "first":
        r0, r1 = 0, 6
    elif kind == "last":
        r0, r1 = end - 6, end
    else:                           # the template is one run
        r0, r1 = 0, end
    c = other(tmpl[r0 - 1] if r0 else tmpl[r1 % end], 1)
    if r1 < end and c == tmpl[r1]:
        c = other(c)
    tmpl[r0:r1] = c
    mid = (r0 + r1) // 2
    return tmpl, [(mid, "d", -delta)] if delta < 0 else [(mid, "i", [c] * delta)]


def homo_case(kind, delta, ts=100):
    """Four of five reads change the run's length by delta."""
    tmpl, e = homo_parts(kind, delta, ts)
    return tmpl, carriers(tmpl, e, 3, 4) + carriers(tmpl, e, 1, 1, ins_side="prev", comp=1), ts


for _d in (-2, -1, 1, 2):
    case("homo", f"homo-boundary{_d:+d}", homo_case, "boundary", _d)
for _k, _d in (("long", -2), ("long", 3), ("first", -1), ("first", 2), ("last", -1), ("last", 2), ("boundary", 6), ("long", 7),
               ("single", -3), ("single", 2), ("single", 6)):
    case("homo", f"homo-{_k}{_d:+d}", homo_case, _k, _d)
for _t in (126, 128):
    for _k, _d in (("boundary", -2), ("boundary", 1), ("long", -2), ("long", 3), ("last", 2), ("single", -3)):
        case("homo", f"homo-{_k}{_d:+d}-ts{_t}", homo_case, _k, _d, _t)


# --- ties and depth
def tie_none():
    return rnd(160, 230), [], 100


def tie_parts(kind, d, k):
    tmpl = no_runs(161, 230)
    x = 100 if (d + k) % 2 else 57
    return tmpl, {"sub": (x, "s", other(tmpl[x])), "del": (x, "d", 1),
                  "ins": (x, "i", [next(c for c in range(4) if c not in (tmpl[x - 1], tmpl[x]))])}[kind]


def tie_ladder(kind, d, k):
    """k of d reads carry one substitution / one-base deletion / one-base foreign insertion, the others are exact."""
    tmpl, e = tie_parts(kind, d, k)
    return tmpl, carriers(tmpl, [e], k, d), 100


def tie_run_half():
    """Three reads cover a run of 6, two of them lack one base: 2 * net = cover + 1."""
    tmpl = no_runs(162, 230)
    tmpl[60:66] = other(tmpl[59], 1 + (other(tmpl[59]) == tmpl[66]))
    return tmpl, carriers(tmpl, [(62, "d", 1)], 2, 3), 100


def tie_run_half_longer():
    tmpl, specs, ts = tie_run_half()
    return tmpl, carriers(tmpl, [(62, "i", [tmpl[62]])], 2, 3), ts


case("ties", "ties-no-overlap", tie_none)
for _kind in ("sub", "del", "ins"):
    for _d in range(1, 6):
        for _k in range(0, _d + 1):
            case("ties", f"ties-{_kind}-{_k}of{_d}", tie_ladder, _kind, _d, _k)
case("ties", "ties-run-half-shorter", tie_run_half)
case("ties", "ties-run-half-longer", tie_run_half_longer)


# --- codes: N (4) in the template, in reads, aligned to each other, next to an indel
def codes_case(kind, ts=100):
    tmpl = no_runs(170, 260)
    rng = np.random.default_rng(171)
    if kind in ("template", "both", "indel"):
        tmpl[[0, 63, 64, ts - 1, ts, 180, 259]] = 4
        tmpl[130:134] = 4
    reads = []
    for i in range(4):
        r = [int(c) for c in tmpl]
        if kind == "template":
            r = [c if c < 4 else int(rng.integers(0, 4)) for c in r]
        if kind == "reads":
            for x in (0, 50, 64, ts - 1, ts, ts + 1, 259):
                r[x] = 4
        if kind == "indel":
            e = [(63, "d", 1), (ts, "i", [2]), (131, "d", 1), (181, "i", [4]), (200, "i", [4, 4]), (220, "s", 4), (221, "d", 1)]
            r = list(edited(tmpl, 0, 260, e if i < 3 else []))
            r = [c if c < 4 or i != 1 else 0 for c in r]
        reads.append(np.asarray(r, dtype=np.uint8))
    return tmpl, [spec(r, 0, 260, comp=i == 2, ins_side=("next", "prev")[i & 1]) for i, r in enumerate(reads)], ts


for _t in (100, 126, 128):
    for _k in ("template", "reads", "both", "indel"):
        case("codes", f"codes-n-{_k}-ts{_t}", codes_case, _k, _t)


# --- records to ignore, interleaved with the voting ones
def ignore_case(order):
    tmpl = no_runs(180, 250)
    good = carriers(tmpl, [(70, "s", other(tmpl[70])), (150, "d", 1)], 3, 3)
    bad = [(99, "s", other(tmpl[99])), (120, "d", 2), (30, "i", [other(tmpl[30], 2)])]
    off = carriers(tmpl, bad, 4, 4, disabled=1) + carriers(tmpl, bad, 4, 4, aread=1) + carriers(tmpl, bad, 1, 1, aread=2, disabled=1)
    specs = good + off
    return tmpl, [specs[i] for i in np.random.default_rng(181 + order).permutation(len(specs))], 100


for _o in range(3):
    case("ignore", f"ignore-order{_o}", ignore_case, _o)


# --- vote-space sizes: the pack kernel's chunk of 256 columns, the scan's blocks of 2 048 slots over length + 3
def space_case(n):
    ts = 126
    tmpl = rnd(190 + n, n)
    rng = np.random.default_rng(191 + n)
    edge = 256 if n < 1000 else 2045
    ends = [(0, n), (edge - 20, n), (0, max(edge - 3, 1)), (max(n - 1, 0), n), (edge - 140, min(edge + 1, n)), (max(edge - 300, 0), n - 1),
            (0, n)]
    specs = []
    for i, (a0, a1) in enumerate(ends):
        a0, a1 = max(a0, 0), min(a1, n)
        specs.append(spec(noisy(rng, tmpl[a0:a1], 0.05, 0.04, 0.04), a0, a1, comp=i & 1, ins_side=("next", "prev")[(i >> 1) & 1]))
    # the last columns: substituted, deleted and followed by an insertion in a majority
    e = [(n - 1, "s", other(tmpl[n - 1])), (n - 3, "d", 1), (n, "i", [1, 2])]
    return tmpl, specs + carriers(tmpl, e, 9, 9, max(n - 130, 0), n), ts


for _n in (255, 256, 257, 2044, 2045, 2046):
    case("space", f"space-{_n}", space_case, _n)


# --- seeded random piles
def random_case(seed):
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(1, 701))
    tmpl = low_complexity(9500 + seed, n) if seed % 3 == 0 else rnd(9500 + seed, n)
    if seed % 7 == 0:
        tmpl[rng.integers(0, n, 1 + n // 100)] = 4
    ts = int(rng.choice(TSPACES))
    specs = []
    twice = seed % 4 == 1   # every read twice, a few of them: a read's every edit wins its vote and shows in the consensus
    for _ in range(int(rng.integers(0, 4 if twice else 13))):
        a0 = int(rng.integers(0, n)) if rng.random() < 0.6 else 0
        a1 = int(rng.integers(a0 + 1, n + 1)) if rng.random() < 0.6 else n
        rates = rng.uniform(0, 0.15, 3)
        read = noisy(rng, tmpl[a0:a1], *rates)
        lead, tail = rnd(int(rng.integers(1 << 30)), int(rng.integers(0, 20))), rnd(int(rng.integers(1 << 30)), int(rng.integers(0, 20)))
        specs.append(spec(np.concatenate([lead, read, tail]), a0, a1, len(lead), len(lead) + len(read), comp=int(rng.integers(0, 2)),
                          ins_side=("next", "prev")[int(rng.integers(0, 2))], slack=int(rng.choice([0, 0, 1, 10, 40, 90, 250])),
                          disabled=int(rng.random() < 0.05)))
        if twice:
            specs.append(dict(specs[-1], slack=int(rng.choice([0, 40, 90]))))
    return tmpl, specs, ts


NRANDOM = 150
for _s in range(NRANDOM):
    case("random", f"random-{_s}", random_case, _s)

FAMILIES = tuple(dict.fromkeys(f for _, f, _ in CASES))


def refusal_case():
    """The one malformed input: a single overlap whose only tile claims 0 diffs for three more B bases than columns."""
    tmpl = rnd(200, 60)
    read = np.concatenate([tmpl[:30], rnd(201, 3), tmpl[30:]])
    return tmpl, [spec(read, 0, 60, pairs=[[0, 63]])], 100


@functools.lru_cache(maxsize=None)
def built(cid):
    """(template, db, records, trace, trace spacing) of a case, built once per process; treat as read-only."""
    fn = next(fn for i, _, fn in CASES if i == cid)
    tmpl, specs, ts = fn()
    db, las, trace = pile(tmpl, specs, ts)
    return np.asarray(tmpl, dtype=np.uint8), db, las, trace, ts


@functools.lru_cache(maxsize=None)
def expected(cid):
    """(consensus bases, vote table) of a case by the oracle, computed once per process; treat as read-only."""
    tmpl, db, las, trace, ts = built(cid)
    return oz.consensus(tmpl, db, las, trace, 0, ts, want_votes=True)


def ids_of(*families):
    return [cid for cid, fam, _ in CASES if fam in families]
