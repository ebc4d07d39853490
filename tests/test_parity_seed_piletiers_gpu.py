"""The segment-fed 8 192- and 16 384-entry tiers of k_seed -- the pile-up all-vs-all's -- against the oracle's seed stage,
item by item as tests/test_parity_seedstage_gpu.py compares: nhits, ncand and every candidate field in stored order.  What
is checked here is what these two tiers do differently from the others: the band heads in a table behind the read's own hits
in LDS (reads whose table does not fit keep the slab of global scratch; DH_SEED_SLAB_BANDS=1 sends every read there), and
a lane group for every long range of a candidate band pair instead of for the first 64.  Every case runs both ways and the
counter dh_get_seed_band_counts tells which way its reads went.  Inputs: tests/seed_piletier_cases.py; what a case claims
about its input is asserted on the oracle's figures before the device is touched -- a precondition that does not hold
fails the test."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from oracle import pyoracle as oz
import seed_piletier_cases as pc
from test_parity_map_gpu import both_opts

pytestmark = pytest.mark.gpu

FIELDS = ("score", "aseq", "apos", "bpos")
K = 14


def where(it):
    return f"item {it} (read {it // 2}, strand {it & 1})"


def assert_same_seeds(got, exp, what):
    """ncand, nhits and the first ncand candidates of every item, field by field in stored order"""
    cand, ncand, nhits = got
    ecand, encand, enhits = exp
    assert len(ncand) == len(encand), what
    for name, a, b in (("nhits", nhits, enhits), ("ncand", ncand, encand)):
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{what}: {where(int(bad[0]))} {name} {a[bad[0]]}, oracle {b[bad[0]]} ({len(bad)} items differ)"
    live = np.arange(cand.shape[1])[None, :] < ncand[:, None]
    for f in FIELDS:
        bad = np.argwhere(live & (cand[f] != ecand[f][:, :cand.shape[1]]))
        if len(bad):
            it, r = int(bad[0][0]), int(bad[0][1])
            raise AssertionError(f"{what}: {where(it)} rank {r} field {f}: {cand[it][r][f]}, oracle {ecand[it][r][f]} "
                                 f"({len(bad)} candidates differ in {f})")


def oracle_seeds(db, **kw):
    _, o = both_opts(**kw)
    return oz.seed_candidates_all(db, db, o, with_nhits=True)


def per_read(x):
    return x[0::2].astype(np.int64) + x[1::2]


def gpu_seeds(ctx, db, **kw):
    g, _ = both_opts(**kw)
    d = ctx.db(db)
    try:
        return ctx.seed_candidates(d, d, g)
    finally:
        d.close()


def both_ways(ctx, monkeypatch, db, exp, what, cap, **kw):
    """The call with the head table and with DH_SEED_SLAB_BANDS=1, each against the oracle, the pile-up join feeding the
    tier DH_SEED_CAP names.  Returns the counter (reads by the table, reads by the slab) of the first."""
    monkeypatch.setenv("DH_SEED_CAP", str(cap))
    ctx.join_counts(reset=True)
    ctx.seed_band_counts(reset=True)
    got = gpu_seeds(ctx, db, **kw)
    assert_same_seeds(got, exp, f"{what}, cap {cap}")
    assert ctx.join_counts()[0] >= 1, "the pile-up join did not run"
    counts = ctx.seed_band_counts(reset=True)
    monkeypatch.setenv("DH_SEED_SLAB_BANDS", "1")
    slab = gpu_seeds(ctx, db, **kw)
    monkeypatch.delenv("DH_SEED_SLAB_BANDS")
    assert_same_seeds(slab, exp, f"{what}, cap {cap}, DH_SEED_SLAB_BANDS=1")
    for a, b in zip(got, slab):
        live = np.arange(got[0].shape[1])[None, :] < got[1][:, None] if a.ndim == 2 else np.ones(a.shape, dtype=bool)
        assert np.array_equal(a[live], b[live]), what
    by_slab = ctx.seed_band_counts(reset=True)
    assert by_slab[0] == 0 and by_slab[1] == sum(counts), (counts, by_slab)
    return counts


@pytest.fixture(scope="module")
def ctx():
    c = dentist_amd.Context(0)
    yield c
    c.close()


# -------------------------------------------------------------------------------------------------- 260 x 1 kb locus
def locus_kw(algo, max_cand=48):
    return dict(pc.PILE_KW, algo=algo, width=64 if algo else 30, max_cand=max_cand)


@pytest.fixture(scope="module")
def locus():
    """the 260 x 1 kb locus at 9 % error, the oracle's seeds per algo, and the uncut candidates"""
    db = pc.deep_locus(err=0.09)
    uncut = oracle_seeds(db, **locus_kw(1, max_cand=256))
    return db, {algo: oracle_seeds(db, **locus_kw(algo)) for algo in (0, 1)}, uncut


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("cap", [8192, 16384])
def test_deep_locus(ctx, monkeypatch, locus, cap, algo):
    """A band pair that covers P bases holds at least P / k hits (a hit covers at most k bases of its own), so a candidate
    of score above 16 k has a range above 16 hits whatever else lies in it: at least 20 items have more than 64 of those
    -- what went to the serial walk before -- and their reads fit the 16 384-entry tier.  At DH_SEED_CAP=8192 the reads up to
    8 192 hits are the 8 192-entry tier's and the others are redone from the list by the 16 384-entry tier."""
    db, exp, uncut = locus
    ucand, uncand, unhits = uncut
    assert uncand.max() < 256  # nothing cut, no item given up: the candidates are the band pairs
    live = np.arange(ucand.shape[1])[None, :] < uncand[:, None]
    long_ranges = (live & (ucand["score"] > 16 * K)).sum(axis=1)
    hits = per_read(unhits)
    many = np.flatnonzero((long_ranges > 64) & (hits[np.arange(len(long_ranges)) // 2] <= 16384))
    assert len(many) >= 20, len(many)
    assert (hits <= 8192).sum() >= 20 and ((hits > 8192) & (hits <= 16384)).sum() >= 100
    counts = both_ways(ctx, monkeypatch, db, exp[algo], f"260 x 1 kb locus, algo {algo}", cap, **locus_kw(algo))
    # every read with hits inside the LDS tiers went through one of the two (once: a read redone from the list is counted
    # by the tier that held it)
    assert sum(counts) == int(((hits > 0) & (hits <= 16384)).sum()) and counts[0] > 0, counts


def test_deep_locus_inside_the_8192_entry_tier(ctx, monkeypatch):
    """the same locus at 13 % error (the reads of the seed-stage module's deep pile-up): every read within 8 192 hits, 200
    and more items with over 64 band pairs -- the 8 192-entry instantiation with more long ranges than the 64 slots held"""
    db = pc.deep_locus(err=0.13)
    kw = locus_kw(1)
    exp = oracle_seeds(db, **kw)
    uncut = oracle_seeds(db, **dict(kw, max_cand=256))
    hits = per_read(uncut[2])
    assert (uncut[1] > 64).sum() >= 200 and uncut[1].max() < 256 and 2048 < hits.max() <= 8192
    counts = both_ways(ctx, monkeypatch, db, exp, "260 x 1 kb locus at 13 % error", 8192, **kw)
    assert sum(counts) == int((hits > 0).sum()) and counts[0] > 0, counts


# ---------------------------------------------------------------------------------------------------- slab fall-back
@pytest.mark.parametrize("cap", [8192, 16384])
def test_slab_fall_back(ctx, monkeypatch, cap):
    """Reads on both sides of the table's limit (n hits and a table of nheads + 1 entries -- two per 8-byte word at 8 192,
    one at 16 384 -- within `cap` words): a table never holds more heads than hits, so a read of at most cap / 2 hits
    certainly takes it; a read within a few hundred hits of the capacity does not when its hits lie in some hundreds of
    bands.  Bands of 8 diagonals (band_shift 3) make heads of most runs."""
    db = pc.near_capacity(cap)
    kw = dict(pc.PILE_KW, algo=1, width=64, max_cand=48, band_shift=3)
    exp = oracle_seeds(db, **kw)
    uncut = oracle_seeds(db, **dict(kw, max_cand=256))
    assert uncut[1].max() < 256
    hits = per_read(exp[2])
    near = int(((hits > 3 * cap // 4) & (hits <= cap)).sum())
    assert near >= 10 and int(((hits > cap - 400) & (hits <= cap)).sum()) >= 5, (near, np.sort(hits)[-40:])
    assert int(((hits > 0) & (hits <= cap // 2)).sum()) >= 10
    table, slab = both_ways(ctx, monkeypatch, db, exp, "reads near the capacity", cap, **kw)
    print("head table", table, "slab", slab)
    assert table >= 10 and slab >= 1, (table, slab)


# ------------------------------------------------------------------------------------------- head-table field limits
def test_coverage_field_of_the_narrow_entry(ctx, monkeypatch):
    """The 8 192-entry tier's table entry keeps the coverage before a head in 18 bits.  The candidate band pairs of a read
    are disjoint (a candidate b scores above b + 1, so b + 1 is none), hence the coverage summed over a read's hits --
    the last entry of its table -- is at least the sum of its uncut candidates' scores: at least one read that fits the tier
    brings that above 2^13.5, three quarters of the field's bits."""
    db = pc.covered_deep()
    kw = dict(pc.PILE_KW, algo=1, width=64, max_cand=48)
    exp = oracle_seeds(db, **kw)
    ucand, uncand, unhits = oracle_seeds(db, **dict(kw, max_cand=256))
    assert uncand.max() < 256
    live = np.arange(ucand.shape[1])[None, :] < uncand[:, None]
    covered = per_read((ucand["score"] * live).sum(axis=1))
    hits = per_read(unhits)
    assert hits.max() <= 8192, hits.max()  # the oracle's hits stay within the tier
    assert covered.max() >= 2 ** 13.5, covered.max()
    counts = both_ways(ctx, monkeypatch, db, exp, "low-error pile-up", 8192, **kw)
    assert counts[0] > 0


# ------------------------------------------------------------------------------------------ runs of a ranged candidate
@pytest.mark.parametrize("cap", [8192, 16384])
def test_runs_of_a_ranged_candidate(ctx, monkeypatch, cap):
    """two runs of equal coverage (the earliest wins) and a best run across the edges of the 16-hit groups, on both strands"""
    c = pc.ranged_runs()
    exp = oracle_seeds(c["A"], **c["kw"])
    assert sorted(np.flatnonzero(exp[1]).tolist()) == sorted(c["expect"])
    counts = both_ways(ctx, monkeypatch, c["A"], exp, c["name"], cap, **c["kw"])
    assert counts == (4, 0)  # the four reads with hits


# ------------------------------------------------------------------------------------------------ whole process stage
def test_process_stage_with_a_160_deep_pile_up(ctx, monkeypatch):
    """`process_pileups` over some thirty pile-ups of ~10 reads and one of more than 160: records and consensus bases are
    the same with the head table and with DH_SEED_SLAB_BANDS=1, and the deep pile-up's reads went through these tiers"""
    w = sim.Workload(1_200_000, 30, 2400, 6000, seed=131, spacing=30000, gap_max=900)
    gb, ge = int(w.gap_begin[7]), int(w.gap_end[7])
    lo = gb - 3200
    extra, _ = sim.reads(133, w.truth[lo:ge + 3200], 170, 6000, 0, min_len=6000)
    reads = sim.SeqDb.from_list([w.reads.seq(i) for i in range(w.reads.n)] + [extra.seq(i) for i in range(extra.n)])
    mo = dentist_amd.default_align_opts(kmer_mod=4, k=20, width=64, xdrop=60, algo=1)
    po = dentist_amd.default_process_opts(algo=1, max_reads=0, rounds=2)
    A, B = ctx.db(w.contigs), ctx.db(reads)
    try:
        las, trace, _, cands = ctx.map_reads(A, B, mo, po, sorted=False, candidates=True)
        piles = cands.select(las, po)
        sizes = [len(piles.get(i)[1]) for i in range(len(piles))]
        assert len(piles) >= 24 and max(sizes) >= 160, (len(piles), max(sizes))
        ctx.seed_band_counts(reset=True)
        rec, bases = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po)
        counts = ctx.seed_band_counts(reset=True)
        monkeypatch.setenv("DH_SEED_SLAB_BANDS", "1")
        rec2, bases2 = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po)
        by_slab = ctx.seed_band_counts(reset=True)
    finally:
        A.close()
        B.close()
    assert counts[0] >= 160 and by_slab[0] == 0 and by_slab[1] == sum(counts), (counts, by_slab)
    assert (rec["status"] == 0).sum() >= 20
    for f in rec.dtype.names:
        if f not in ("cons_off", "pad"):
            assert np.array_equal(rec[f], rec2[f]), f
    for a, b in zip(rec, rec2):
        assert np.array_equal(bases[a["cons_off"]:a["cons_off"] + a["cons_len"]], bases2[b["cons_off"]:b["cons_off"] + b["cons_len"]])
