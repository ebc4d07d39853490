"""The mask layer of a DB on the device -- dh_db_dust (k_dust<16|32|64>), dh_db_mask_coverage (k_cov_events, the scan,
k_cov_mask_at), dh_db_set_mask and their recomposition (k_or_words), read back by dh_db_get_mask -- against the plain
restatements of tests/mask_ref.py on the constructed cases of tests/mask_cases.py, and the k-mers that a masked base takes out
of the seeding against the oracle's counter.  ptr and iv are compared for equality; a failure names the first sequence that
differs."""
import numpy as np
import pytest

import dentist_amd
from oracle import pyoracle as oz

import mask_cases as cases
import mask_ref as mr

pytestmark = pytest.mark.gpu

DUST_CASES = {
    "repeats": cases.dust_repeats,
    "thresholds": cases.dust_thresholds,
    "nonbase": cases.dust_nonbase,
    "borders_16383": lambda: cases.dust_borders(16383),
    "borders_16384": lambda: cases.dust_borders(16384),
    "borders_140000": lambda: cases.dust_borders(140000),
}


def assert_same_mask(got, exp, what=""):
    gptr, giv = np.asarray(got[0]), np.asarray(got[1]).reshape(-1)
    eptr, eiv = np.asarray(exp[0]), np.asarray(exp[1]).reshape(-1)
    if np.array_equal(gptr, eptr) and np.array_equal(giv, eiv):
        return
    assert len(gptr) == len(eptr), what
    for s in range(len(eptr) - 1):
        g, e = cases.per_seq(gptr, giv, s), cases.per_seq(eptr, eiv, s)
        assert g == e, f"{what}: sequence {s} of {len(eptr) - 1}: device {g[:6]}, expected {e[:6]}"
    raise AssertionError(what)


def zero_db(ctx, lens):
    return ctx.db(cases.sim.SeqDb.from_list([np.zeros(int(n), dtype=np.uint8) for n in lens]))


@pytest.fixture(scope="module")
def short():
    """the 70 000-sequence DB with its reference dust mask and the coverage case on it, built once"""
    return dict(db=cases.short_db()["db"], dust=cases.short_dust(), cov=cases.coverage_short())


@pytest.mark.parametrize("name", list(DUST_CASES))
def test_dust(gpu_ctx, name):
    db = DUST_CASES[name]()["db"]
    d = gpu_ctx.db(db)
    d.dust()
    assert_same_mask(d.get_mask(), mr.dust_mask(db.bases, db.off), name)


def test_dust_70000_short_sequences(gpu_ctx, short):
    d = gpu_ctx.db(short["db"])
    d.dust()
    assert_same_mask(d.get_mask(), short["dust"], "short_70000")


@pytest.mark.parametrize("t", range(5), ids=["0_1", "1_3", "0_69999", "0_70000", "2_max"])
def test_coverage_70000_short_sequences(gpu_ctx, short, t):
    """two launches of the classification (65 535 sequences each at most), more than one block sum per thread at the top of
    the scan, a sequence covered 70 000 deep"""
    c = short["cov"]
    lower, upper = c["thresholds"][t]
    d = gpu_ctx.db(short["db"])
    d.mask_coverage(c["las"], lower, upper)
    assert_same_mask(d.get_mask(), mr.coverage_mask(c["lens"], c["intervals"], lower, upper), f"limits ({lower}, {upper})")


@pytest.mark.parametrize("lower,upper", cases.coverage_tiny()["thresholds"])
def test_coverage_tiny_sequences(gpu_ctx, lower, upper):
    c = cases.coverage_tiny()
    d = zero_db(gpu_ctx, c["lens"])
    d.mask_coverage(c["las"], lower, upper)
    assert_same_mask(d.get_mask(), mr.coverage_mask(c["lens"], c["intervals"], lower, upper), f"limits ({lower}, {upper})")


def test_coverage_without_alignments_and_with_empty_ones(gpu_ctx):
    c = cases.coverage_tiny()
    d = zero_db(gpu_ctx, c["lens"])
    d.mask_coverage(np.zeros(0, dtype=dentist_amd.LA_DTYPE), 1, 2)
    assert d.get_mask()[0][-1] == 0                       # no alignment at all: no mask
    only_empty = np.asarray([(2, 3, 3)])
    d.mask_coverage(cases.las_of(only_empty), 1, 2)       # an alignment that covers nothing: coverage 0 everywhere
    assert_same_mask(d.get_mask(), mr.coverage_mask(c["lens"], only_empty, 1, 2), "one empty alignment")


def test_coverage_reference_vectors(gpu_ctx):
    from test_maskcov import ALIGNMENTS, CONTIGS
    lens = [e - b for _, b, e in CONTIGS]
    iv = np.asarray([(c - 1, b, e) for c, b, e in ALIGNMENTS])
    for lower, upper in [(3, 5), (0, 0), (1, 7), (7, 7), (0, 6), (4, 4)]:
        d = zero_db(gpu_ctx, lens)
        d.mask_coverage(cases.las_of(iv), lower, upper)
        assert_same_mask(d.get_mask(), mr.coverage_mask(lens, iv, lower, upper), f"limits ({lower}, {upper})")


@pytest.mark.parametrize("allowance", [0, 7])
@pytest.mark.parametrize("lower,upper", cases.improper_cases()["thresholds"])
def test_improper_only_at_the_allowance(gpu_ctx, lower, upper, allowance):
    c = cases.improper_cases()
    d = zero_db(gpu_ctx, c["lens"])
    d.mask_coverage(c["las"], lower, upper, read_off=c["read_off"], improper_only=True, allowance=allowance)
    exp = mr.coverage_mask(c["lens"], cases.improper_intervals(c, allowance), lower, upper)
    assert_same_mask(d.get_mask(), exp, f"allowance {allowance}, limits ({lower}, {upper})")


def test_layers_recompose_at_word_edges(gpu_ctx):
    c = cases.layers()
    db, lens, off = c["db"], c["lens"], c["db"].off
    u1, u2 = mr.flags_of(*c["user1"], off), mr.flags_of(*c["user2"], off)
    dust = mr.dust_flags(db.bases, off)
    c1, c2 = (mr.coverage_flags(lens, c["intervals"], *c[k]) for k in ("cov1", "cov2"))
    d = gpu_ctx.db(db)

    def check(flags, step):
        assert_same_mask(d.get_mask(), mr.intervals_of(flags, off), step)
    d.set_mask(*c["user1"])
    check(u1, "user track")
    d.dust()
    check(u1 | dust, "user track, dust")
    d.mask_coverage(c["las"], *c["cov1"])
    check(u1 | dust | c1, "user track, dust, coverage")
    d.set_mask(*c["user2"])
    check(u2 | dust | c1, "second user track replaces the first")
    d.set_mask(np.zeros(db.n + 1, dtype=np.int64), np.zeros(0, dtype=np.int32))
    check(dust | c1, "empty user track leaves the derived layer")
    d.mask_coverage(c["las"], *c["cov2"])
    check(dust | c1 | c2, "second coverage mask joins the first")
    d.set_mask(*c["user1"])
    check(u1 | dust | c1 | c2, "user track over both coverage masks")
    d.set_mask(None, None)
    check(np.zeros(len(u1), dtype=bool), "cleared")
    d.mask_coverage(c["las"], *c["cov2"])
    check(c2, "coverage after clearing")


def _hits(ctx, c, a_iv, b_iv):
    """(hits of the device, hits of the oracle) with [b, e) masked on A, on B or on both"""
    from test_parity_map_gpu import both_opts
    g, o = both_opts(k=c["k"], kmer_mod=1)
    A, B = ctx.db(cases.masked_db(c["seq"], None)), ctx.db(cases.masked_db(c["seq"], None))
    for d, iv in ((A, a_iv), (B, b_iv)):
        if iv is not None:
            d.set_mask(np.array([0, 1], dtype=np.int64), np.array(iv, dtype=np.int32))
    ctx.align_db(A, B, g)
    exp = oz.align_db(cases.masked_db(c["seq"], a_iv), cases.masked_db(c["seq"], b_iv), o)
    return int(ctx.align_stats().hits), int(exp[2][0])


@pytest.fixture(scope="module")
def unmasked_hits(gpu_ctx):
    return _hits(gpu_ctx, cases.kmer_edges(), None, None)


@pytest.mark.parametrize("side", ["A", "B", "both"])
@pytest.mark.parametrize("name", list(cases.kmer_edges()["masks"]))
def test_masked_base_takes_out_the_kmers_that_touch_it(gpu_ctx, unmasked_hits, name, side):
    c = cases.kmer_edges()
    iv = c["masks"][name]
    plain, exp_plain = unmasked_hits
    assert plain == exp_plain == c["starts"]
    got, exp = _hits(gpu_ctx, c, iv if side in ("A", "both") else None, iv if side in ("B", "both") else None)
    assert got == exp
    assert plain - got == cases.kmer_drop(c, *iv)
