"""Inputs of the mask-propagation tests (dh_la_propagate_mask): hand-worked cases with their expected intervals written out,
and seeded shapes -- every combination of trace tiles and intersecting intervals per record around the sizes of a chunk of
tiles and a batch of intervals (64), destination lengths around the words of the bitmap, long records, a destination that
collects many raw intervals, a destination laid out for several ranges, and a volume case.  A case is a dict: las, trace,
tspace, mask = (ptr, iv), ncontigs, read_off."""
import numpy as np

LA_DTYPE = np.dtype([("tlen", "<i4"), ("diffs", "<i4"), ("abpos", "<i4"), ("bbpos", "<i4"), ("aepos", "<i4"), ("bepos", "<i4"),
                     ("flags", "<u4"), ("aread", "<i4"), ("bread", "<i4"), ("pad", "<i4"), ("toff", "<i8")])
COMP = 0x1

TILES = (1, 2, 63, 64, 65, 129, 700)
INTERVALS = (0, 1, 2, 63, 64, 65, 200)
EDGE_LENGTHS = (1, 31, 32, 33, 63, 64, 65)


class Builder:
    """records with their trace values, the mask per contig, the reads' lengths"""

    def __init__(self, tspace):
        self.tspace, self.rows, self.trace, self.mask, self.read_len = tspace, [], [], {}, {}

    def record(self, aread, bread, abpos, aepos, bbpos, bbases, comp=False, tail=0):
        ts = self.tspace
        assert len(bbases) == (aepos + ts - 1) // ts - abpos // ts
        bepos = bbpos + int(sum(bbases))
        self.rows.append((2 * len(bbases), 0, abpos, bbpos, aepos, bepos, COMP if comp else 0, aread, bread, 0, len(self.trace)))
        for b in bbases:
            self.trace += [0, int(b)]
        self.read_len[bread] = max(self.read_len.get(bread, 0), bepos + tail)

    def case(self, ncontigs=None, nreads=None):
        las = np.array(self.rows, dtype=LA_DTYPE) if self.rows else np.zeros(0, dtype=LA_DTYPE)
        ncontigs = ncontigs if ncontigs is not None else 1 + max([r[7] for r in self.rows] + list(self.mask) + [0])
        nreads = nreads if nreads is not None else 1 + max(list(self.read_len) + [0])
        ptr, iv = [0], []
        for c in range(ncontigs):
            iv += self.mask.get(c, [])
            ptr.append(len(iv))
        read_off = np.concatenate([[0], np.cumsum([self.read_len.get(r, 0) for r in range(nreads)])]).astype(np.int64)
        return dict(las=las, trace=np.asarray(self.trace, dtype=np.uint16), tspace=self.tspace,
                    mask=(np.asarray(ptr, dtype=np.int64), np.asarray(iv, dtype=np.int32).reshape(-1, 2)), ncontigs=ncontigs,
                    read_off=read_off)


def read_len(case):
    return np.diff(case["read_off"])


# ---------------------------------------------------------------------------------------------------------- hand-worked
def _hand():
    out = {}
    # the example of the header: tspace 100, [150, 420) on A, four tiles of 48, 103, 97 and 21 b-bases from 1000.  [0, 160) is
    # cut to [150, 160): begin at trace point 0, end rounded up to trace point 1 (A 200) -> [1000, 1048); [250, 260) lies in
    # the tile [200, 300) -> [1048, 1151); [405, 500) is cut to [405, 420): down to A 400 (1000 + 48 + 103 + 97), up to 420
    b = Builder(100)
    b.record(0, 0, 150, 420, 1000, [48, 103, 97, 21], tail=731)
    b.mask[0] = [(0, 160), (250, 260), (405, 500)]
    out["header_example"] = (b.case(), {0: [(1000, 1151), (1248, 1269)]})
    # the same on the complement strand of a read of 2000 bases: [b, e) -> [2000 - e, 2000 - b)
    b = Builder(100)
    b.record(0, 0, 150, 420, 1000, [48, 103, 97, 21], comp=True, tail=731)
    b.mask[0] = [(0, 160), (250, 260), (405, 500)]
    out["header_example_complement"] = (b.case(), {0: [(731, 752), (849, 1000)]})
    # tspace 126, [126, 378) on A: two tiles of 130 and 0 b-bases from 10.  [126, 127) begins at abpos (trace point 0) and
    # ends at trace point 1 -> [10, 140); [300, 378) lies in the second tile, which has no b-bases: [140, 140) vanishes.
    # Read 1 gets nothing, contig 1 has no mask
    b = Builder(126)
    b.record(0, 0, 126, 378, 10, [130, 0], tail=5)
    b.record(1, 1, 0, 100, 0, [90])
    b.mask[0] = [(126, 127), (300, 378)]
    out["zero_tile"] = (b.case(), {0: [(10, 140)]})
    # two records on one read whose results touch ([0, 50) and [50, 120)) are one interval; a third further on stays apart
    b = Builder(100)
    b.record(0, 0, 0, 100, 0, [50])
    b.record(0, 0, 100, 200, 50, [70])
    b.record(0, 0, 300, 400, 200, [99], tail=1)
    b.mask[0] = [(0, 400)]
    out["touching_results_merge"] = (b.case(), {0: [(0, 120), (200, 299)]})
    return out


HAND = _hand()


# ---------------------------------------------------------------------------------------------------------- trace shapes
def _intervals_in(rng, abpos, aepos, k, ts, variant):
    """k disjoint intervals that all intersect [abpos, aepos): the first is cut at abpos or begins there, the last is cut at
    aepos or ends there, some end on a tile boundary; when they are dense they are single bases that touch"""
    span = aepos - abpos
    assert 0 < k <= span
    if 2 * k > span + 1:
        starts = np.sort(rng.choice(np.arange(abpos, aepos), size=k, replace=False)).tolist()
        iv = [[s, s + 1] for s in starts]
    else:
        pts = np.sort(rng.choice(np.arange(abpos, aepos + 1), size=2 * k, replace=False)).tolist()
        iv = [[pts[2 * j], pts[2 * j + 1]] for j in range(k)]
        for j in range(k):  # an end on a tile boundary where one lies in reach
            nxt = iv[j + 1][0] if j + 1 < k else aepos
            t = (iv[j][0] // ts + 1) * ts
            if t <= nxt and rng.random() < 0.3:
                iv[j][1] = t
    if variant % 2 == 0:
        iv[0][0] = max(0, abpos - 7)
        iv[-1][1] = aepos + 9
    else:
        iv[0][0] = abpos
        iv[-1][1] = aepos
    return [tuple(x) for x in iv]


def trace_shapes(tspace, seed=1):
    """every (tiles, intervals) of TILES x INTERVALS twice, once per strand; a record of one tile has tspace bases at most, so
    (1, 200) takes the tspace intervals that fit.  Reads 0..11 collect the records (several each), reads 12..14 have none;
    the contigs of the (tiles, 0) shapes have no mask or only intervals outside the record"""
    rng = np.random.default_rng(seed)
    b = Builder(tspace)
    ts, contig = tspace, 0
    shapes = {}
    for tiles in TILES:
        for k in INTERVALS:
            for comp in (False, True):
                loose = (2 * ts + 37, (2 + tiles) * ts - 11)
                abpos, aepos = loose if 2 * k <= loose[1] - loose[0] else (2 * ts, (2 + tiles) * ts)
                kk = min(k, aepos - abpos)
                bbases = rng.integers(ts - 12, ts + 13, tiles)
                bbases[rng.random(tiles) < 0.1] = 0
                if tiles > 2:
                    bbases[1] = 0
                bread = int(rng.integers(0, 12))
                b.record(contig, bread, abpos, aepos, int(rng.integers(0, 3000)), bbases.tolist(), comp=comp, tail=int(rng.integers(0, 40)))
                if kk:
                    iv = _intervals_in(rng, abpos, aepos, kk, ts, contig // 2)
                    if iv[0][0] == abpos and abpos >= 20:
                        iv = [(abpos - 20, abpos - 9), (abpos - 3, abpos)] + iv  # end at abpos: no intersection
                    if iv[-1][1] == aepos:
                        iv = iv + [(aepos, aepos + 4), (aepos + 50, aepos + 60)]  # begin at aepos: no intersection
                    b.mask[contig] = iv
                elif contig % 4 == 0:
                    b.mask[contig] = [(0, abpos), (aepos, aepos + 10)]
                shapes[contig] = (tiles, kk)
                contig += 1
    case = b.case(nreads=15)
    case["shapes"] = shapes
    return case


# ---------------------------------------------------------------------------------------------------------- bitmap edges
def _exact(b, contig, bread, blen, results, comp=False):
    """one record on a contig of its own whose tiles end where the results begin and end, and the mask that selects them"""
    ts = b.tspace
    cuts = sorted({0, blen} | {x for r in results for x in r})
    if comp:
        cuts = sorted(blen - x for x in cuts)
        results = [(blen - e, blen - s) for s, e in results]
    bbases = [cuts[i + 1] - cuts[i] for i in range(len(cuts) - 1)]
    b.record(contig, bread, 0, ts * len(bbases), 0, bbases, comp=comp)
    b.read_len[bread] = blen
    b.mask[contig] = sorted((ts * cuts.index(s), ts * cuts.index(e)) for s, e in results)


def bitmap_edges():
    """(case, expected) with the expected intervals written by the construction: per destination length two neighbouring
    reads masked in full, then a read with a result at 0 and one that ends at the length, results that end on a word boundary,
    lie inside one word, span three words, and two records whose results touch; a read of 300 bases takes the wide painter"""
    b = Builder(100)
    expected, contig, read = {}, 0, 0

    def add(blen, per_record, merged, comp=False):
        nonlocal contig, read
        for results in per_record:
            _exact(b, contig, read, blen, results, comp)
            contig += 1
        expected[read] = merged
        read += 1
    for n in EDGE_LENGTHS:
        add(n, [[(0, n)]], [(0, n)])
        add(n, [[(0, n)]], [(0, n)], comp=True)
        if n >= 3:
            add(n, [[(0, 1), (n - 1, n)]], [(0, 1), (n - 1, n)], comp=n % 2 == 0)
        if n >= 31:
            add(n, [[(2, 10)], [(10, 20)], [(25, 26)]], [(2, 20), (25, 26)])
        if n >= 33:
            add(n, [[(5, 32)]], [(5, 32)])
            add(n, [[(31, 33)]], [(31, 33)], comp=True)
        if n >= 63:
            add(n, [[(33, 35), (36, 37), (40, 63)]], [(33, 35), (36, 37), (40, 63)])
        if n >= 65:
            add(n, [[(31, 65)]], [(31, 65)])
            add(n, [[(0, 32)], [(32, 64)], [(64, 65)]], [(0, 65)])
    add(300, [[(3, 290)], [(100, 299)]], [(3, 299)])
    return b.case(), expected


# ---------------------------------------------------------------------------------------------------------- long shapes
def long_record(seed=3, tiles=20000, k=3000, tspace=100):
    """one record of `tiles` tiles whose contig has k intersecting intervals, and a second short one on the same read"""
    rng = np.random.default_rng(seed)
    b = Builder(tspace)
    abpos, aepos = 2 * tspace + 37, (2 + tiles) * tspace - 11
    bb = rng.integers(tspace - 12, tspace + 13, tiles)
    bb[rng.random(tiles) < 0.05] = 0
    b.record(0, 0, abpos, aepos, 17, bb.tolist(), tail=23)
    b.record(0, 0, 5 * tspace, 9 * tspace, 300, [90, 110, 100, 95], comp=True)
    b.mask[0] = _intervals_in(rng, abpos, aepos, k, tspace, 0)
    return b.case()


def many_into_one(seed=4, nrec=5000, per=20, tspace=100):
    """the reads -> reference direction: nrec records of 8 tiles with `per` intersecting intervals each, all into one sequence"""
    rng = np.random.default_rng(seed)
    b = Builder(tspace)
    for i in range(nrec):
        abpos, aepos = 2 * tspace + 37, 10 * tspace - 11
        b.record(i, 0, abpos, aepos, int(rng.integers(0, 3_000_000)), rng.integers(tspace - 12, tspace + 13, 8).tolist(), comp=bool(i & 1))
        b.mask[i] = _intervals_in(rng, abpos, aepos, per, tspace, i)
    return b.case()


def wide_destination(nreads=6, blen=5_000_000, tspace=100):
    """reads of 5 Mbp each (0.6 MB of bitmap): with a bitmap of 1 MB every read is a destination range of its own"""
    b = Builder(tspace)
    for r in range(nreads):
        for k in range(3):
            b.record(r % 2, r, 100 * k, 100 * k + 300, 1_000_000 * (k + 1) + 1000 * r, [100, 90 + k, 110], comp=bool(r & 1))
        b.read_len[r] = blen
    b.mask[0] = [(50, 150), (250, 420)]
    b.mask[1] = [(0, 10), (120, 130), (300, 301)]
    return b.case()


def volume(seed=6, nrec=200_000, ncontigs=50, contig_len=1_000_000, nreads=50_000, tspace=100):
    """nrec records of 10..40 tiles against a sparse mask (40 intervals of 100..500 bases per contig); built with numpy"""
    rng = np.random.default_rng(seed)
    ts = tspace
    tiles = rng.integers(10, 41, nrec)
    q = rng.integers(0, contig_len // ts - 45, nrec)
    las = np.zeros(nrec, dtype=LA_DTYPE)
    las["aread"] = rng.integers(0, ncontigs, nrec)
    las["bread"] = rng.integers(0, nreads, nrec)
    las["abpos"] = q * ts + rng.integers(0, ts, nrec)
    las["aepos"] = (q + tiles) * ts - rng.integers(0, ts - 1, nrec)
    las["flags"] = rng.integers(0, 2, nrec) * COMP
    las["tlen"] = 2 * tiles
    las["toff"] = 2 * (np.cumsum(tiles) - tiles)
    trace = np.zeros(2 * int(tiles.sum()), dtype=np.uint16)
    trace[1::2] = rng.integers(ts - 10, ts + 11, int(tiles.sum()))
    bsum = np.add.reduceat(trace[1::2].astype(np.int64), (las["toff"] // 2).astype(np.int64))
    las["bbpos"] = rng.integers(0, 500, nrec)
    las["bepos"] = las["bbpos"] + bsum
    rl = np.zeros(nreads, dtype=np.int64)
    np.maximum.at(rl, las["bread"], las["bepos"].astype(np.int64) + 3)
    ptr, iv = [0], []
    for c in range(ncontigs):
        cuts = np.sort(rng.choice(np.arange(1, contig_len // 600), size=40, replace=False)) * 600
        for s in cuts:
            iv.append((int(s), int(s + rng.integers(100, 501))))
        ptr.append(len(iv))
    return dict(las=las, trace=trace, tspace=ts, mask=(np.asarray(ptr, dtype=np.int64), np.asarray(iv, dtype=np.int32)), ncontigs=ncontigs,
                read_off=np.concatenate([[0], np.cumsum(rl)]).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------- refusals
def refusals():
    """[(name, case, what the message names)]: one malformed input per line of the contract's list; the base is a good case"""
    good = HAND["header_example"][0]

    def variant(**rec):
        c = dict(good)
        c["las"] = good["las"].copy()
        c["las"] = np.concatenate([c["las"], c["las"]])  # the fault sits in record 1
        for k, v in rec.items():
            c["las"][1][k] = v
        return c

    def masked(iv, ptr=(0, 3)):
        c = dict(good)
        c["ncontigs"] = len(ptr)
        c["mask"] = (np.asarray((0,) + tuple(ptr), dtype=np.int64), np.asarray(iv, dtype=np.int32).reshape(-1, 2))
        c["las"] = good["las"].copy()
        return c
    past = dict(good)  # four tiles whose b-bases sum to 1269 - 1000 in a read of 2000 bases: raise one to run past its end
    past["las"] = np.concatenate([good["las"], good["las"]])
    past["las"][1]["toff"] = len(good["trace"])
    tr2 = good["trace"].copy()
    tr2[7] = 60000
    past["trace"] = np.concatenate([good["trace"], tr2])
    cut = dict(good)
    cut["las"] = np.concatenate([good["las"], good["las"]])
    cut["las"][1]["toff"] = 2
    return [
        ("aread_out_of_range", variant(aread=1), "record 1"),
        ("bread_out_of_range", variant(bread=-1), "record 1"),
        ("abpos_negative", variant(abpos=-50, tlen=10), "record 1"),
        ("abpos_behind_aepos", variant(abpos=430, tlen=0), "record 1"),
        ("tlen_negative", variant(tlen=-2), "record 1"),
        ("tlen_odd", variant(tlen=7), "record 1"),
        ("tlen_does_not_fit", variant(tlen=6), "record 1"),
        ("trace_behind_the_array", cut, "record 1"),
        ("trace_runs_past_the_read", past, "record 1"),
        ("mask_not_sorted", masked([(250, 260), (0, 160), (405, 500)], ptr=(0, 3)), "contig 1"),
        ("mask_overlaps", masked([(0, 160), (150, 260), (405, 500)], ptr=(0, 3)), "contig 1"),
        ("mask_empty_interval", masked([(0, 160), (250, 250), (405, 500)], ptr=(0, 3)), "contig 1"),
        ("mask_negative_begin", masked([(-5, 160), (250, 260), (405, 500)], ptr=(0, 3)), "contig 1"),
    ]
