"""Inputs of the region-validation tests (dh_la_validate_regions): hand-worked cases with their expected results written out,
and seeded shapes, each the smallest at which one piece of the device path can go wrong -- the window geometry, records at the
edges of a region and of a window, pair and spanning counts around a wavefront (64), weak runs that fuse or just do not, a
weak run across the chunks of the scan (256 window starts), regions that nest, repeat and overlap in shuffled order, regions on
contigs the records do not reach, a region around the cap of the LDS tier, regions that each fill a launch group, and many
regions on one contig.  A case is a dict: las, contig_off, regions [(contig, begin, end)], min_cov, min_span, context, window."""
import numpy as np

LA_DTYPE = np.dtype([("tlen", "<i4"), ("diffs", "<i4"), ("abpos", "<i4"), ("bbpos", "<i4"), ("aepos", "<i4"), ("bepos", "<i4"),
                     ("flags", "<u4"), ("aread", "<i4"), ("bread", "<i4"), ("pad", "<i4"), ("toff", "<i8")])
CHUNK = 256         # window starts per chunk of the region scan (VR_BLOCK)
LOW_CAP = 300       # DH_VREG_LDS_WINDOWS of the tier tests


def case(rows, lens, regions, min_cov=1, min_span=1, context=10, window=5):
    """rows: (contig, abpos, aepos, bread) in any order; the records are sorted by contig alone (stable)"""
    rows = sorted(rows, key=lambda r: r[0])
    las = np.zeros(len(rows), dtype=LA_DTYPE)
    for i, (c, b, e, rd) in enumerate(rows):
        las[i]["aread"], las[i]["abpos"], las[i]["aepos"], las[i]["bread"] = c, b, e, rd
    return dict(las=las, contig_off=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), regions=[tuple(int(x) for x in r) for r in regions],
                min_cov=min_cov, min_span=min_span, context=context, window=window)


def args(c):
    """the arguments of validate_regions behind las, contig_off, regions"""
    return dict(min_coverage_reads=c["min_cov"], min_spanning_reads=c["min_span"], region_context=c["context"],
                weak_coverage_window=c["window"])


# ---------------------------------------------------------------------------------------------------------- hand-worked
# one contig of 100 bases, region (0, 40, 50), context 10: cb = 30, ce = 60; W = 5: window starts 30 .. 55; min coverage 1,
# min spanning 1.  Expected: spanning ids, weak (contig, begin, end), weak_bp, is_valid
def _hand():
    out = {}
    region = [(0, 40, 50)]
    # [0, 60) covers every window but does not span: ce < aepos is 60 < 60
    out["covers_but_ends_at_ce"] = (case([(0, 0, 60, 7)], [100], region), dict(span=[], weak=[], weak_bp=0, valid=False))
    # [29, 61) does: 29 < 30 and 60 < 61
    out["one_spanning_read"] = (case([(0, 0, 60, 7), (0, 29, 61, 3)], [100], region), dict(span=[3], weak=[], weak_bp=0, valid=True))
    # [35, 52) spans the windows that start at 35 .. 47: starts 30 .. 34 are weak -> [30, 39), starts 48 .. 55 -> [48, 60)
    out["two_weak_intervals"] = (case([(0, 35, 52, 1)], [100], region),
                                 dict(span=[], weak=[(0, 30, 39), (0, 48, 60)], weak_bp=21, valid=False))
    # [33, 38) spans the window at 33 alone: the weak runs 30 .. 32 ([30, 37)) and 34 .. 55 (from 34 <= 37) fuse
    out["runs_fuse_through_a_spanned_window"] = (case([(0, 33, 38, 1)], [100], region),
                                                 dict(span=[], weak=[(0, 30, 60)], weak_bp=30, valid=False))
    return out


HAND = _hand()


# --------------------------------------------------------------------------------------------------------------- shapes
def _piled(n_pairs, n_span, seed):
    """one region (0, 1000, 1100), context 100 (cb 900, ce 1200) with n_pairs records that touch it, n_span of them spanning;
    record indices shuffled against bread"""
    rng = np.random.default_rng(seed)
    rows = [(0, int(rng.integers(0, 900)), int(rng.integers(1201, 3000))) for _ in range(n_span)]
    while len(rows) < n_pairs:
        b = int(rng.integers(890, 1199))
        rows.append((0, b, min(1200, b + int(rng.integers(11, 200)))))  # ends behind cb and at ce at the latest: never spanning
    rows += [(0, int(rng.integers(0, 800)), 900), (0, 1200, 1300), (1, 0, 500)]  # touch it from outside: no pairs
    order = rng.permutation(len(rows))
    breads = rng.permutation(len(rows)) + 10
    return case([rows[k] + (int(breads[k]),) for k in order], [3000, 600], [(0, 1000, 1100)], min_cov=2, min_span=2, context=100, window=50)


def _gap_between_runs(gap):
    """a record that spans exactly `gap` consecutive window starts in the middle of a region: the weak run behind it begins
    gap + 1 starts after the end of the one in front.  window 5: gap 4 -> exactly wlen apart (fuse), gap 5 -> wlen + 1 (two)"""
    return case([(0, 120, 120 + gap - 1 + 5, 0)], [400], [(0, 110, 150)], context=10, window=5)


def tier_case(entries):
    """one region whose difference array has `entries` entries (window starts + 1), window 5, with weak and covered stretches"""
    length = entries + 3  # nw = length - 5 + 1
    rows = [(0, 20, 20 + length // 3, 0), (0, 10 + length // 2, 15 + length, 1), (0, 0, 40 + length, 2), (0, 25, 60, 3)]
    return case(rows, [length + 100], [(0, 20, 20 + length)], min_cov=2, min_span=1, context=0, window=5)


def _chunks():
    """a region of 3 chunks and a bit; the covered stretches end one start before, at and one behind a chunk boundary, and a
    weak run lies across the second boundary"""
    rows = [(0, 100, 100 + CHUNK - 1 + 4, 0), (0, 100, 100 + CHUNK + 4, 1), (0, 100, 100 + CHUNK + 1 + 4, 2),
            (0, 100 + 2 * CHUNK + 40, 100 + 3 * CHUNK + 80, 3), (0, 90, 100 + 3 * CHUNK + 60, 4)]
    return case(rows, [2000], [(0, 100, 100 + 3 * CHUNK + 50)], min_cov=2, min_span=1, context=0, window=5)


def _regions_shuffled(seed):
    """three contigs with records; regions that repeat, nest and overlap, on all of them and in shuffled order"""
    rng = np.random.default_rng(seed)
    lens = [5000, 300, 8000]
    rows = []
    for c, n in enumerate(lens):
        for _ in range(60):
            b = int(rng.integers(0, n))
            rows.append((c, b, int(min(n, b + rng.integers(1, 2500))), len(rows)))
    regions = [(0, 1000, 1200), (0, 1000, 1200), (0, 900, 2500), (0, 1100, 1150), (0, 1150, 1400), (0, 0, 5000), (0, 4990, 5000),
               (1, 0, 10), (1, 100, 300), (1, 120, 130), (2, 3000, 3001), (2, 2500, 6000), (2, 2600, 2700), (2, 5900, 6100), (2, 7999, 8000)]
    regions = [regions[k] for k in rng.permutation(len(regions))]
    return case(rows, lens, regions, min_cov=3, min_span=2, context=150, window=60)


def _outside_the_file():
    """records on contigs 1 and 2 only; regions on contigs 0 and 3 as well"""
    rows = [(1, 0, 400, 5), (1, 50, 390, 6), (2, 100, 900, 7), (2, 0, 1000, 8)]
    return case(rows, [500, 400, 1000, 700], [(3, 100, 200), (1, 100, 200), (0, 0, 500), (2, 300, 400), (3, 690, 700)], context=50,
                window=20)


def group_case():
    """four regions of about 270 000 window starts each: each takes more than 1 MB of the slab, so a launch group of its own
    at DH_VREG_SLAB_MB=1; few records, so that the literal loop stays quick"""
    n = 270_000
    lens = [4 * n + 1000]
    rows, regions = [], []
    for k in range(4):
        b = 500 + k * n
        regions.append((0, b, b + n - 300))
        rows += [(0, b - 10, b + 1000 + 7 * k, 4 * k), (0, b + 5000, b + n - 400, 4 * k + 1), (0, b - 200, b + n, 4 * k + 2)]
    return case(rows, lens, regions, min_cov=2, min_span=1, context=100, window=500)


def many_regions():
    """1 000 regions on one contig with 100 000 records: the shape of a gap-closed scaffold"""
    rng = np.random.default_rng(77)
    n = 10_000_000
    b = rng.integers(0, n - 200, 100_000)
    e = np.minimum(n, b + rng.integers(1000, 12000, 100_000))
    rows = [(0, int(x), int(y), int(k)) for k, (x, y) in enumerate(zip(b, e))]
    rb = np.sort(rng.integers(0, n - 6000, 1000))
    regions = [(0, int(x), int(x + rng.integers(50, 5000))) for x in rb]
    regions = [regions[k] for k in rng.permutation(len(regions))]
    return case(rows, [n], regions, min_cov=45, min_span=3, context=1000, window=500)


def _shapes():
    s = {}
    cover = [(0, 0, 300, 0), (0, 95, 135, 1), (0, 100, 101, 2)]
    s["window_of_one_base"] = case(cover + [(0, 110, 112, 3)], [300], [(0, 100, 120)], min_cov=2, context=5, window=1)
    s["region_shorter_than_the_window"] = case(cover, [300], [(0, 100, 120)], min_cov=2, context=5, window=500)
    s["region_shorter_than_the_window_weak"] = case(cover, [300], [(0, 100, 120)], min_cov=3, context=5, window=500)
    s["empty_extended_region"] = case(cover, [300], [(0, 100, 100)], context=0, window=5)
    s["region_behind_the_contig"] = case(cover, [300], [(0, 400, 410)], context=20, window=5)
    s["context_clipped_at_the_start"] = case([(0, 0, 50, 0), (0, 3, 80, 1)], [300], [(0, 5, 30)], context=10, window=5)
    s["context_clipped_at_the_end"] = case([(0, 250, 300, 0), (0, 200, 299, 1)], [300], [(0, 280, 295)], context=10, window=5)
    s["contig_without_records"] = case([(0, 0, 100, 0)], [100, 200], [(1, 50, 60)], context=10, window=5)
    s["no_records"] = case([], [100, 200], [(1, 50, 60), (0, 0, 100)], context=10, window=5)
    s["no_regions"] = case([(0, 0, 100, 0)], [100], [], context=10, window=5)
    s["record_shorter_than_the_window"] = case([(0, 40, 44, 0), (0, 0, 100, 1)], [100], [(0, 40, 50)], min_cov=2)
    s["record_ends_at_a_window_end"] = case([(0, 30, 45, 0), (0, 32, 60, 1), (0, 30, 35, 2)], [100], [(0, 40, 50)])
    s["abpos_at_cb_and_aepos_at_ce"] = case([(0, 30, 70, 0), (0, 20, 60, 1), (0, 29, 61, 2)], [100], [(0, 40, 50)])
    for k in (0, 1, 63, 64, 65):
        s[f"pairs_{k}"] = _piled(k, 0, 100 + k)
    for k in (1, 64, 65):
        s[f"spanning_{k}"] = _piled(k + 9, k, 200 + k)
    s["runs_exactly_wlen_apart"] = _gap_between_runs(4)
    s["runs_wlen_plus_one_apart"] = _gap_between_runs(5)
    s["weak_run_across_chunks"] = _chunks()
    s["regions_shuffled"] = _regions_shuffled(31)
    s["regions_outside_the_file"] = _outside_the_file()
    for k in (-1, 0, 1):
        s[f"tier_cap{k:+d}"] = tier_case(LOW_CAP + k)
    return s


SHAPES = _shapes()


def refusals():
    """(name, case, the words dh_last_error must hold)"""
    good = HAND["one_spanning_read"][0]

    def with_las(**fields):
        c = dict(good)
        c["las"] = good["las"].copy()
        for k, v in fields.items():
            c["las"][1][k] = v
        return c
    out = [("aread_out_of_range", with_las(aread=1), "record 1"), ("negative_abpos", with_las(abpos=-1), "record 1"),
           ("abpos_behind_aepos", with_las(abpos=62), "record 1"), ("aepos_behind_the_contig", with_las(aepos=101), "record 1")]
    c = case([(1, 0, 50, 0), (0, 0, 60, 1), (0, 0, 70, 2)], [100, 100], [(0, 40, 50)])
    c["las"] = c["las"][[0, 2, 1]]  # contigs 0, 1, 0
    out.append(("not_sorted", c, "record 2: reads-alignment must be sorted at least by a-read ID"))
    for name, region in (("region_contig", (1, 40, 50)), ("region_negative_begin", (0, -1, 50)), ("region_end_before_begin", (0, 40, 39))):
        c = dict(good)
        c["regions"] = [(0, 40, 50), region, (5, 0, 0)]
        out.append((name, c, "region 1"))
    c = dict(good)
    c["window"] = 0
    out.append(("window_of_zero", c, "bad argument"))
    c = dict(good)
    c["context"] = -1
    out.append(("negative_context", c, "bad argument"))
    return out
