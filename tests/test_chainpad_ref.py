"""Invariants of the chain padder's restatement (tests/chainpad_ref.py) on every constructed case (tests/chainpad_cases.py):
replaying a chain's ops over A [a0, a1) yields exactly B [b0, b1), the score is the number of non-zero ops, a chain without
junction trouble costs no more than its records' tiles plus its fillers' lengths, and the statuses are as constructed.  No GPU
needed."""
import numpy as np
import pytest

import chainpad_cases as cc
import chainpad_ref as cr
from dentist_amd import sim

NAMES = list(cc.cases().keys())


@pytest.fixture(scope="module")
def results():
    return {n: cr.run(c) for n, c in cc.cases().items()}


def frames(case, ch):
    a = case["A"].seq(int(ch[0]["aread"]))
    b = case["B"].seq(int(ch[0]["bread"]))
    return a, (sim.revcomp(b) if ch[0]["flags"] & 1 else b)


@pytest.mark.parametrize("name", NAMES)
def test_replay_score_and_status(results, name):
    case = cc.cases()[name]
    op_off, ops, score, status, fillers = results[name]
    off = cr.chains_of(case["las"])
    assert len(score) == len(off) - 1 == len(case["expect"])
    for i in range(len(off) - 1):
        ch = case["las"][off[i]:off[i + 1]]
        o = ops[op_off[i]:op_off[i + 1]]
        assert status[i] == case["expect"][i]
        if status[i] == cr.NESTED:
            assert len(o) == 0 and score[i] == -1
            continue
        a, b = frames(case, ch)
        assert cr.replay(o, a[ch[0]["abpos"]:ch[-1]["aepos"]], b[ch[0]["bbpos"]:ch[-1]["bepos"]])
        assert score[i] == np.count_nonzero(o)
    assert (fillers > 0) == case["fillers"]


@pytest.mark.parametrize("name", NAMES)
def test_score_bounded_by_tiles_and_fillers(results, name):
    case = cc.cases()[name]
    _, _, score, status, _ = results[name]
    off = cr.chains_of(case["las"])
    for i in range(len(off) - 1):
        if status[i] != cr.OK:
            continue
        ch = case["las"][off[i]:off[i + 1]]
        a, b = frames(case, ch)
        st, segs = cr.segments(ch, case["trace"], case["ts"])
        bound = 0
        for k, la in enumerate(ch):
            pts = cr.points(la, case["trace"], case["ts"])
            bound += sum(cr.nw_ref.oracle(a[p[0]:q[0]], b[p[1]:q[1]], False)[0] for p, q in zip(pts[:-1], pts[1:]))
        bound += sum((s[3] - s[2]) + (s[5] - s[4]) for s in segs if s[0] == "f")
        assert score[i] <= bound


def test_the_single_record_is_its_tiles(results):
    case = cc.cases()["single"]
    la = case["las"][0]
    pts = cr.points(la, case["trace"], case["ts"])
    a, b = frames(case, case["las"][:1])
    exp = np.concatenate([cr.tile_ops(a[p[0]:q[0]], b[p[1]:q[1]]) for p, q in zip(pts[:-1], pts[1:])])
    assert np.array_equal(results["single"][1], exp)


def test_junction_picks():
    c = cc.cases()
    ts = cc.TS
    seg = lambda n: cr.segments(c[n]["las"], c[n]["trace"], ts)
    bm = cc.Script(7, 3000).bm
    # clean gap: p whole, the gap, q whole
    assert seg("gap_both") == (cr.OK, [("t", 0, 0, 9), ("f", 0, 1000, 1130, int(bm[1000]), int(bm[1130])), ("t", 1, 0, 14)])
    assert seg("gap_none") == (cr.OK, [("t", 0, 0, 9), ("t", 1, 0, 15)])
    # overlap cut mid-tile: p ends at floor(1130) = 1100, q starts at ceil(1250) = 1300
    assert seg("overlap_both_mid_tile") == (cr.OK, [("t", 0, 0, 10), ("f", 0, 1100, 1300, int(bm[1100]), int(bm[1300])), ("t", 1, 2, 14)])
    # ... and on the grid: no rounding
    assert seg("overlap_both_on_grid") == (cr.OK, [("t", 0, 0, 10), ("f", 0, 1100, 1200, int(bm[1100]), int(bm[1200])), ("t", 1, 1, 14)])
    # the B resolution reaches further back on p and further on q than the A resolution does
    st, s = seg("overlap_both_picks_differ")
    assert st == cr.OK and s[1][0] == "f" and (s[1][2] < 1100 or s[1][3] > 1300)
    assert seg("zero_tiles_of_p")[1][2:4] == [("f", 1, 1000, 1100, int(bm[1000]), int(bm[1100])), ("t", 2, 1, 10)]
    assert seg("nested") == (cr.NESTED, [])
    assert len(seg("short_records_200")[1]) > 64 * 4
