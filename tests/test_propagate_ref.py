"""The restatement of the mask-propagation contract (tests/propagate_ref.py) against its two independent witnesses, the
oracle's propagate_mask and the library's host function dh_propagate_mask, on every case of tests/propagate_cases.py, and
against the written-out values of the hand-worked cases.  Every comparison is equality.  No GPU needed."""
import numpy as np
import pytest

import dentist_amd
from oracle import maskcov as mc

import propagate_cases as pc
import propagate_ref as pr


def restated(case):
    return pr.propagate(case["las"], case["trace"], case["tspace"], case["mask"][0], case["mask"][1], pc.read_len(case))


def check_witnesses(case):
    exp, stats = restated(case)
    nreads = len(case["read_off"]) - 1
    ptr, iv = dentist_amd.propagate_mask(case["las"], case["trace"], case["tspace"], case["mask"], case["ncontigs"], case["read_off"])
    eptr, eiv = pr.arrays(exp, nreads)
    assert np.array_equal(ptr, eptr) and np.array_equal(iv, eiv) and ptr.dtype == eptr.dtype and iv.dtype == eiv.dtype
    assert pr.as_dict(ptr, iv) == exp
    assert mc.propagate_mask(case["las"], case["trace"], case["tspace"], case["mask"][0], case["mask"][1], pc.read_len(case)) == exp
    return exp, stats


@pytest.mark.parametrize("name", list(pc.HAND))
def test_hand_worked_cases_equal_their_written_values(name):
    case, expected = pc.HAND[name]
    exp, _ = check_witnesses(case)
    assert exp == expected


@pytest.mark.parametrize("tspace", [100, 126])
def test_trace_shapes(tspace):
    case = pc.trace_shapes(tspace)
    exp, stats = check_witnesses(case)
    count = sum(len(v) for v in exp.values())
    assert stats["raw"] > count > 0 and stats["empty"] > 0
    # every combination is there, on both strands; (1, 200) holds the tspace intervals one tile has room for
    want = sorted((t, min(k, tspace) if t == 1 else k) for t in pc.TILES for k in pc.INTERVALS for _ in range(2))
    assert sorted(case["shapes"].values()) == want
    assert set(range(12, 15)).isdisjoint(exp) and int(np.count_nonzero(np.diff(case["mask"][0]) == 0)) > 0
    assert {int(f) & 1 for f in case["las"]["flags"]} == {0, 1}


def test_bitmap_edges_equal_their_construction():
    case, expected = pc.bitmap_edges()
    exp, _ = check_witnesses(case)
    assert exp == expected
    lens = pc.read_len(case).tolist()
    assert set(pc.EDGE_LENGTHS) <= set(lens)
    full = [r for r in expected if expected[r] == [(0, lens[r])]]
    assert any(r + 1 in full for r in full)  # two neighbouring reads masked in full stay two intervals


def test_long_shapes():
    case = pc.long_record()
    exp, stats = check_witnesses(case)
    alone = pr.raw_intervals(case["las"][:1], case["trace"], case["tspace"], case["mask"][0], case["mask"][1], pc.read_len(case))[0]
    assert int(case["las"][0]["tlen"]) == 40_000 and len(alone) == 3000 and stats["raw"] > len(exp[0]) > 0
    case = pc.many_into_one()
    exp, stats = check_witnesses(case)
    assert stats["raw"] + stats["empty"] == 100_000 and list(exp) == [0]


def test_wide_destination_and_volume():
    exp, stats = check_witnesses(pc.wide_destination())
    assert len(exp) == 6
    case = pc.volume()
    exp, stats = check_witnesses(case)
    assert 0 < stats["hit"] < len(case["las"]) // 4 and len(case["las"]) == 200_000
