"""The restatements of the mask layer (tests/mask_ref.py) against their independent witnesses on every case of
tests/mask_cases.py: dust_mask against the oracle's sliding-window DUST (oracle/dust.c), coverage_mask against the oracle's
event machine (oracle/maskcov.py) and the reference's own vectors, the masked k-mer edges against the oracle's seed counter.
Building a case runs the assertions the builder makes about it.  Every comparison is equality.  No GPU needed."""
import numpy as np
import pytest

from oracle import maskcov as mc
from oracle import pyoracle as oz

import mask_cases as cases
import mask_ref as mr
from test_maskcov import ALIGNMENTS, CONTIGS, MASK_3_5

DUST_CASES = {
    "repeats": cases.dust_repeats,
    "thresholds": cases.dust_thresholds,
    "nonbase": cases.dust_nonbase,
    "borders_16383": lambda: cases.dust_borders(16383),
    "borders_16384": lambda: cases.dust_borders(16384),
    "borders_140000": lambda: cases.dust_borders(140000),
    "short_70000": cases.short_db,
}


def same_mask(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(np.asarray(got[1]).reshape(-1), np.asarray(exp[1]).reshape(-1))


def oracle_coverage(lens, intervals, lower, upper):
    """oracle.maskcov.bad_coverage_mask as (ptr, iv)"""
    rows = [(int(s) + 1, int(b), int(e)) for s, b, e in np.asarray(intervals).reshape(-1, 3).tolist()]
    out = mc.bad_coverage_mask(rows, [(s + 1, 0, int(n)) for s, n in enumerate(lens)], lower, upper)
    assert out == sorted(out)
    ptr = np.searchsorted(np.asarray([c for c, _, _ in out], dtype=np.int64), np.arange(1, len(lens) + 2)).astype(np.int64)
    return ptr, np.asarray([(b, e) for _, b, e in out], dtype=np.int32).reshape(-1)


@pytest.mark.parametrize("name", list(DUST_CASES))
def test_dust_restatement_equals_the_oracle(name):
    db = DUST_CASES[name]()["db"]
    got = cases.short_dust() if name == "short_70000" else mr.dust_mask(db.bases, db.off)
    assert same_mask(got, oz.dust(db))
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32


def test_dust_cases_hold_what_they_are_named_for():
    assert cases.dust_borders(16383)["chunk"] == 64 and cases.dust_borders(16384)["chunk"] == 512
    assert cases.dust_borders(140000)["chunk"] == 512 and cases.dust_borders(140000)["db"].length(1) > 256 * 512
    want = cases.dust_thresholds()["want"]
    assert [(L, t) for L, t, _ in want] == [(16, 27), (16, 26), (32, 59), (32, 58), (64, 123), (64, 122)]
    short = cases.short_db()
    ptr, iv = cases.short_dust()
    masked = np.diff(ptr) > 0
    # repeats of 20 to 31 bases of a three-base unit stay clear (26 = 2 (16 - 3)); the other repeats are masked
    assert masked[short["low"]].mean() > 0.7 and masked[~short["low"]].mean() < 0.01 and masked[cases.SLAB:].any()


@pytest.mark.parametrize("t", range(5))
def test_coverage_restatement_equals_the_oracle_on_70000_sequences(t):
    c = cases.coverage_short()
    lower, upper = c["thresholds"][t]
    got = mr.coverage_mask(c["lens"], c["intervals"], lower, upper)
    assert same_mask(got, oracle_coverage(c["lens"], c["intervals"], lower, upper))
    assert got[1].size > 0


def test_coverage_restatement_equals_the_oracle_on_tiny_sequences():
    c = cases.coverage_tiny()
    for lower, upper in c["thresholds"]:
        assert same_mask(mr.coverage_mask(c["lens"], c["intervals"], lower, upper),
                         oracle_coverage(c["lens"], c["intervals"], lower, upper)), (lower, upper)
    none = np.zeros((0, 3), dtype=np.int64)
    assert mr.coverage_mask(c["lens"], none, 1, 2)[0][-1] == 0 and oracle_coverage(c["lens"], none, 1, 2)[0][-1] == 0
    only_empty = np.asarray([(2, 3, 3)])   # an alignment, but an empty one: coverage 0 everywhere, below lower
    got = mr.coverage_mask(c["lens"], only_empty, 1, 2)
    assert same_mask(got, oracle_coverage(c["lens"], only_empty, 1, 2)) and got[0][-1] == np.count_nonzero(c["lens"])


def test_coverage_restatement_on_the_reference_vectors():
    lens = [e - b for _, b, e in CONTIGS]
    iv = [(c - 1, b, e) for c, b, e in ALIGNMENTS]
    ptr, m = mr.coverage_mask(lens, iv, 3, 5)
    assert [(s + 1,) + x for s in range(len(lens)) for x in cases.per_seq(ptr, m, s)] == MASK_3_5
    assert mr.coverage_mask(lens, [], 3, 5)[0][-1] == 0
    for lower, upper in [(0, 0), (1, 7), (7, 7), (0, 6), (4, 4)]:
        assert same_mask(mr.coverage_mask(lens, iv, lower, upper), oracle_coverage(lens, iv, lower, upper))


@pytest.mark.parametrize("allowance", [0, 7])
def test_improper_rule_at_the_allowance(allowance):
    c = cases.improper_cases()
    iv = cases.improper_intervals(c, allowance)
    assert len(iv) == (28 if allowance == 0 else 12)
    for lower, upper in c["thresholds"]:
        got = mr.coverage_mask(c["lens"], iv, lower, upper)
        assert same_mask(got, oracle_coverage(c["lens"], iv, lower, upper))
    # with limits (0, 0) a contig is masked exactly where its improper record lies
    ptr, m = mr.coverage_mask(c["lens"], iv, 0, 0)
    assert {s: cases.per_seq(ptr, m, s) for s in range(len(c["lens"])) if ptr[s + 1] > ptr[s]} == {int(s): [(int(b), int(e))] for s, b, e in iv}
    # the rule of the existing test (tests/test_maskcov.py) in its own words
    for la in c["las"]:
        alen, blen = int(c["lens"][la["aread"]]), int(c["read_len"][la["bread"]])
        proper = (la["abpos"] <= allowance or la["bbpos"] <= allowance) and (la["aepos"] >= alen - allowance or la["bepos"] >= blen - allowance)
        assert mr.improper(la, alen, blen, allowance) == (not proper)


def test_layers_case_and_interval_round_trip():
    c = cases.layers()
    off = c["db"].off
    for track in (c["user1"], c["user2"]):
        assert same_mask(mr.intervals_of(mr.flags_of(*track, off), off), track)
    # two sequences masked whole stay two intervals; an empty sequence between them gets none
    ptr, iv = mr.intervals_of(np.ones(5, dtype=bool), np.array([0, 3, 3, 5]))
    assert ptr.tolist() == [0, 1, 1, 2] and iv.tolist() == [0, 3, 0, 2]


def oracle_hits(c, a_iv, b_iv):
    o = oz.default_opts(k=c["k"], kmer_mod=1)
    return int(oz.align_db(cases.masked_db(c["seq"], a_iv), cases.masked_db(c["seq"], b_iv), o)[2][0])


def test_masked_kmer_edges_against_the_oracle_counter():
    c = cases.kmer_edges()
    base = oracle_hits(c, None, None)
    assert base == c["starts"] == 587
    drops = {}
    for name, (b, e) in c["masks"].items():
        drops[name] = cases.kmer_drop(c, b, e)
        for a_iv, b_iv in (((b, e), None), (None, (b, e)), ((b, e), (b, e))):
            assert oracle_hits(c, a_iv, b_iv) == base - drops[name], (name, a_iv, b_iv)
    k = c["k"]
    assert drops == {"first": 1, "second": 2, "k-1": k, "k": k, "len-k-1": k, "len-k": k, "last": 1, "tail": 5}
