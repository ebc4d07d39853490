"""The lane code of k_nwa (dh_nwa.h: Gotoh's three states in diagonal-band coordinates, the 4-bit decisions, the traceback,
the acceptance predicate and the doubling of the half-width) compiled for the CPU and played as a 64-lane wavefront
(tests/native/nwa_host.cpp), against the full matrix of tests/nwa_ref.py op for op and score for score (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nwa_ref as ar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCORINGS = [ar.DEFAULT, (1, -1, 2, 1), (0, -1, 0, 1)]


@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "tests", "native", "libdh_nwa_host.so")
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libdh_nwa_host.so"], check=True)
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.nwa_host_attempt.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, vp]
    L.nwa_host_attempt.restype = i32
    L.nwa_host_align.argtypes = [vp, i32, vp, i32, vp, i32, vp, i32, vp]
    L.nwa_host_align.restype = i32
    L.nwa_host_costs.argtypes = [vp, vp]
    L.nwa_host_costs.restype = i32
    L.nwa_host_limits.argtypes = [vp]
    lim = np.zeros(2, np.int32)
    L.nwa_host_limits(lim.ctypes.data)
    L.max_w, L.max_len = int(lim[0]), int(lim[1])
    return L


def _sc(sc):
    return np.asarray(sc, dtype=np.int32)


def align(L, r, q, sc, w0=ar.W0):
    """the whole policy: (status, cost, attempts, last w, score, ops)"""
    ops = np.zeros(len(r) + len(q) + 8, np.uint8)
    out = np.zeros(5, np.int32)
    s = _sc(sc)
    n = L.nwa_host_align(r.ctypes.data, len(r), q.ctypes.data, len(q), s.ctypes.data, w0, ops.ctypes.data, len(ops), out.ctypes.data)
    assert n >= 0, n
    return int(out[0]), int(out[1]), int(out[2]), int(out[3]), int(out[4]), ops[:n].copy()


def attempt(L, r, q, sc, w):
    """one band: dict of the harness's report and the ops of its walk"""
    ops = np.zeros(len(r) + len(q) + 8, np.uint8)
    info = np.zeros(8, np.int32)
    s = _sc(sc)
    n = L.nwa_host_attempt(r.ctypes.data, len(r), q.ctypes.data, len(q), s.ctypes.data, w, ops.ctypes.data, len(ops), info.ctypes.data)
    assert n >= 0, n
    keys = ("cost", "accepted", "left_band", "lo", "hi", "corner", "cpl", "ns")
    d = dict(zip(keys, (int(v) for v in info)))
    d["ops"] = ops[:n].copy()
    return d


def check_pair(L, r, q, sc, w0=ar.W0):
    """the policy's answer equals the full matrix's, after exactly the attempts the restatement of the policy predicts"""
    r, q = np.ascontiguousarray(r, np.uint8), np.ascontiguousarray(q, np.uint8)
    score, cost, ops = ar.align(r, q, sc)
    st, c, att, w, s, got = align(L, r, q, sc, w0)
    est, eatt, ew = ar.expected_attempts(len(r), len(q), cost, ar.costs(sc)[1], L.max_w, w0)
    assert (st, att) == (est, eatt), (len(r), len(q), cost, st, att, w)
    if st == 0:
        assert (c, s, w) == (cost, score, ew)
        assert np.array_equal(got, ops), (len(r), len(q), sc)
    else:
        assert c == -1 and len(got) == 0
    return att, w


def test_cost_form_and_refusals(host):
    cost = np.zeros(3, np.int32)
    for sc in SCORINGS + [(2, -3, 0, 2)]:
        assert host.nwa_host_costs(_sc(sc).ctypes.data, cost.ctypes.data) == 1
        assert tuple(int(x) for x in cost) == ar.costs(sc)
    for bad in ((1, 2, 0, 1), (0, -1, 0, 0), (-2, -3, 0, 1), (1, -1, -1, 1),      # cm < 0, ce <= 0 (twice), co < 0
                (5, -4, 16, 10 ** 6), (5, -4, 2 ** 30, 4), (10 ** 5, -4, 16, 4), (5, -2 ** 30, 16, 4)):  # could overflow
        assert host.nwa_host_costs(_sc(bad).ctypes.data, cost.ctypes.data) == 0, bad


@pytest.mark.parametrize("sc", SCORINGS, ids=str)
@pytest.mark.parametrize("w0", [1, 3, 64])
def test_random_short_pairs(host, sc, w0):
    """1 200 pairs of 1-40 bases, five codes; small first half-widths so that most pairs go through rejected bands first"""
    rng = np.random.default_rng(100 * w0 + sum(abs(x) for x in sc))
    attempts = 0
    for it in range(1200):
        rl, ql = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if it % 2:
            r, q = ar.pair_of(rng, rl, ql, [0.0, 0.1, 0.3][it % 3], ncodes=5)
        else:
            r, q = rng.integers(0, 5, rl).astype(np.uint8), rng.integers(0, 5, ql).astype(np.uint8)
        attempts += check_pair(host, r, q, sc, w0)[0]
    assert attempts > 1200 or w0 == 64  # rejected bands really occurred


@pytest.mark.parametrize("sc", SCORINGS, ids=str)
def test_one_base_sides(host, sc):
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 300):
        s = rng.integers(0, 4, n).astype(np.uint8)
        for one in ([s[n // 2]], [(s[0] + 1) % 4], [4]):
            check_pair(host, s, np.asarray(one, np.uint8), sc)
            check_pair(host, np.asarray(one, np.uint8), s, sc)


# (d = ql - rl, w) whose band is exactly W wide when nothing is clipped: W = |d| + 2 w + 1; lengths around 64 * CPL per class
SEAMS = [(1, 127, 256, 4, 1), (0, 128, 257, 8, 1), (1, 255, 512, 8, 1), (0, 256, 513, 16, 1), (1, 511, 1024, 16, 1),
         (0, 512, 1025, 16, 2), (1, 1023, 2048, 16, 2)]


@pytest.mark.parametrize("d,w,W,cpl,ns", SEAMS, ids=[f"W{s[2]}" for s in SEAMS])
def test_band_of_one_strip_and_one_cell_more(host, d, w, W, cpl, ns):
    """band widths on both sides of every class boundary; the sequences are as long as the band is wide, so that the band
    is clipped at the start and at the end and free in between"""
    assert W <= host.max_w
    rng = np.random.default_rng(W)
    rl = 64 * cpl * ns + 70
    r, q = ar.pair_of(rng, rl, rl + d, 0.03)
    score, cost, ops = ar.align(r, q)
    a = attempt(host, r, q, ar.DEFAULT, w)
    assert (a["cpl"], a["ns"]) == (cpl, ns) and a["hi"] - a["lo"] + 1 == min(W, 2 * rl + d + 1)
    assert cost <= 13 * w and a["accepted"] == 1 and a["cost"] == cost == a["corner"]
    assert np.array_equal(a["ops"], ops)


@pytest.mark.parametrize("n", [255, 256, 257, 511, 512, 513, 1023, 1024, 1025])
def test_lengths_around_a_strip_in_the_full_rectangle(host, n):
    """64 * CPL - 1, 64 * CPL and one more base on both sides, the band as wide as the rectangle allows"""
    rng = np.random.default_rng(n)
    r, q = ar.pair_of(rng, n, n - 3, 0.1)
    score, cost, ops = ar.align(r, q, (1, -1, 2, 1))
    w = (host.max_w - 4) // 2
    a = attempt(host, r, q, (1, -1, 2, 1), w)
    assert a["left_band"] == 0 and a["accepted"] == 1 and a["cost"] == cost == a["corner"] and np.array_equal(a["ops"], ops)
    assert a["hi"] - a["lo"] + 1 == min(2 * n - 3 + 1, 2 * w + 3 + 1)


def test_a_long_deletion_needs_a_wider_band_and_stays_one_gap(host):
    rng = np.random.default_rng(13)
    r = rng.integers(0, 4, 400).astype(np.uint8)
    q = np.concatenate([r[:170], r[230:]])
    att, w = check_pair(host, r, q, ar.DEFAULT)
    st, c, att, w, score, ops = align(host, r, q, ar.DEFAULT)
    assert c == 32 + 13 * 60 and score == 5 * 340 - (16 + 4 * 60) and att == 1
    assert ops.tolist() == [0] * 170 + [1] * 60 + [0] * 170


def test_band_exceeded(host):
    rng = np.random.default_rng(19)
    r, q = rng.integers(0, 4, 30).astype(np.uint8), rng.integers(0, 4, host.max_w + 100).astype(np.uint8)
    st, c, att, w, score, ops = align(host, r, q, ar.DEFAULT)  # ql - rl alone is wider than the widest band
    assert (st, c, att, len(ops)) == (1, -1, 0, 0)
    r, q = rng.integers(0, 4, 3000).astype(np.uint8), rng.integers(0, 4, 3000).astype(np.uint8)
    st, c, att, w, score, ops = align(host, r, q, ar.DEFAULT)  # unrelated: no band proves the result
    assert (st, c, len(ops)) == (1, -1, 0) and att >= 5


@pytest.mark.parametrize("sc", SCORINGS, ids=str)
def test_the_acceptance_predicate_against_the_full_matrix(host, sc):
    """The exactness argument on its own: whatever a band of ANY half-width computes, a result the predicate accepts is the
    full matrix's result in score and ops and its walk stayed in the band; a band the true cost does not allow is never
    accepted.  Among the rejected bands there are walks that differ from the full matrix's."""
    rng = np.random.default_rng(23 + sum(abs(x) for x in sc))
    ce = ar.costs(sc)[1]
    wrong_rejected = narrow = accepted = 0
    for it in range(1500):
        rl, ql = int(rng.integers(8, 41)), int(rng.integers(8, 41))
        r, q = ar.pair_of(rng, rl, ql, [0.03, 0.1, 0.3, 0.6][it % 4])
        score, cost, ops = ar.align(r, q, sc)
        for w in (1, 2, 4, 7):
            lo, hi, full = ar.band(rl, ql, w)
            a = attempt(host, r, q, sc, w)
            assert (a["lo"], a["hi"]) == (lo, hi)
            same = a["cost"] == cost and np.array_equal(a["ops"], ops) and not a["left_band"]
            if a["accepted"]:
                accepted += 1
                assert same and a["corner"] == cost, (it, w, rl, ql)
            elif not same:
                wrong_rejected += 1
            if not full and not ar.accepted(cost, w, ce, False):
                narrow += 1
                assert a["accepted"] == 0, (it, w, rl, ql)
    assert wrong_rejected > 100 and narrow > 1000 and accepted > 100  # each kind really occurred
