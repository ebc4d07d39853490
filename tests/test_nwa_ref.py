"""tests/nwa_ref.py, the restatement every affine-gap test compares with, pinned on its own (no GPU, no library): the
optimal score against every alignment there is for short sequences, the vectorised matrices against the cell-by-cell
definition, the unit-cost reduction against oracle/nw.c op for op, and the property affine gaps exist for."""
import itertools

import numpy as np
import pytest

import nw_ref as nr
import nwa_ref as ar

SCORINGS = [ar.DEFAULT, (1, -1, 2, 1), (0, -1, 0, 1), (2, -3, 0, 2), (5, -4, 12, 4)]


def every_alignment(rl, ql):
    """all op sequences (diagonal 'd', deletion 1, insertion 2) that consume rl and ql bases"""
    if rl == 0 and ql == 0:
        yield ()
        return
    if rl and ql:
        for rest in every_alignment(rl - 1, ql - 1):
            yield ("d",) + rest
    if rl:
        for rest in every_alignment(rl - 1, ql):
            yield (1,) + rest
    if ql:
        for rest in every_alignment(rl, ql - 1):
            yield (2,) + rest


def best_by_enumeration(r, q, sc):
    best = None
    for al in every_alignment(len(r), len(q)):
        i = j = 0
        ops = []
        for o in al:
            if o == "d":
                ops.append(0 if r[i] == q[j] else 3)
                i, j = i + 1, j + 1
            else:
                ops.append(o)
                i, j = i + (o == 1), j + (o == 2)
        s = ar.score_of_ops(r, q, ops, sc)
        best = s if best is None or s > best else best
    return best


@pytest.mark.parametrize("sc", SCORINGS, ids=str)
def test_optimal_score_against_exhaustive_enumeration(sc):
    rng = np.random.default_rng(sum(abs(x) for x in sc))
    shapes = list(itertools.product(range(0, 6), repeat=2))
    for rl, ql in shapes:
        for _ in range(3 if rl + ql >= 8 else 2):
            r, q = rng.integers(0, 3, rl).astype(np.uint8), rng.integers(0, 3, ql).astype(np.uint8)
            score, cost, ops = ar.align(r, q, sc)
            assert score == best_by_enumeration(r, q, sc), (rl, ql, r, q)
            assert ar.score_of_ops(r, q, ops, sc) == score  # the walk is an alignment of that score


@pytest.mark.parametrize("sc", SCORINGS, ids=str)
def test_vectorised_matrices_equal_the_definition(sc):
    rng = np.random.default_rng(7)
    for _ in range(60):
        r, q = ar.pair_of(rng, int(rng.integers(1, 30)), int(rng.integers(1, 30)), 0.3, ncodes=5)
        for a, b in zip(ar.matrices(r, q, sc), ar.gotoh_plain(r, q, sc)):
            assert np.array_equal(np.minimum(a, ar.INF), np.minimum(b, ar.INF))


def test_unit_costs_reduce_to_find_alignment():
    """{0, -1, 0, 1}: ops equal oracle/nw.c (through nw_ref) op for op, score = -cost"""
    rng = np.random.default_rng(11)
    for it in range(150):
        rl, ql = int(rng.integers(0, 60)), int(rng.integers(0, 60))
        r, q = nr.pair_of(rng, rl, ql, [0.0, 0.1, 0.4][it % 3], ncodes=5)
        escore, eops = nr.oracle(r, q, 0)
        score, cost, ops = ar.align(r, q, (0, -1, 0, 1))
        assert score == -escore and cost == 2 * escore
        assert np.array_equal(ops, eops), (rl, ql)


def test_a_long_deletion_is_one_gap():
    rng = np.random.default_rng(13)
    r = rng.integers(0, 4, 400).astype(np.uint8)
    q = np.concatenate([r[:170], r[230:]])
    score, cost, ops = ar.align(r, q)
    dels = np.flatnonzero(ops == 1)
    assert len(dels) == 60 and dels[-1] - dels[0] == 59  # one run
    assert np.count_nonzero(ops == 2) == 0
    assert score == 5 * 340 - (16 + 4 * 60)
    # unit costs scatter nothing here either, but they do not prefer the single gap: same number of edits for any split
    assert ar.align(r, q, (0, -1, 0, 1))[0] == -60


def test_policy_restatement():
    assert ar.costs(ar.DEFAULT) == (18, 13, 32)
    assert ar.costs((1, 2, 0, 1)) is None and ar.costs((0, -1, 0, 0)) is None and ar.costs((1, -1, -1, 1)) is None
    assert ar.band(100, 130, 10) == (-10, 40, False) and ar.band(5, 5, 10) == (-5, 5, True)
    assert ar.accepted(130, 10, 13, False) and not ar.accepted(131, 10, 13, False) and ar.accepted(10 ** 6, 1, 13, True)
    assert ar.band_class(256) == (4, 1) and ar.band_class(257) == (8, 1) and ar.band_class(1025) == (16, 2)
    assert ar.next_w(3000, 3000, 0, 64, 2048) == 64 and ar.next_w(3000, 3000, 512, 64, 2048) == 1023
    assert ar.next_w(3000, 3000, 1023, 64, 2048) == -1
    assert ar.expected_attempts(3000, 3000, 13 * 64, 13, 2048) == (0, 1, 64)
    assert ar.expected_attempts(3000, 3000, 13 * 64 + 1, 13, 2048) == (0, 2, 128)
    assert ar.expected_attempts(3000, 3000, 13 * 1024, 13, 2048) == (1, 5, 0)
