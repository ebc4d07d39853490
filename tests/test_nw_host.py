"""The lane code of k_nw (dh_nw.h: the banded fill in diagonal coordinates, the 2-bit decisions, the traceback, the
acceptance predicate and the doubling of the half-width) compiled for the CPU and played as a 64-lane wavefront
(tests/native/nw_host.cpp), against oracle/nw.c op for op and score for score, for both free_shift values (no GPU needed)."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import nw_ref as nr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [0, 1]


@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "tests", "native", "libdh_nw_host.so")
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libdh_nw_host.so"], check=True)
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.nw_host_attempt.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, vp]
    L.nw_host_attempt.restype = i32
    L.nw_host_align.argtypes = [vp, i32, vp, i32, i32, i32, vp, i32, vp]
    L.nw_host_align.restype = i32
    return L


def _bytes(x):
    return np.frombuffer(x.encode(), np.uint8) if isinstance(x, str) else np.ascontiguousarray(x, dtype=np.uint8)


def align(L, ref, qry, fs, w0=nr.W0):
    """the whole policy: (status, score, attempts, last w, ops)"""
    r, q = _bytes(ref), _bytes(qry)
    ops = np.zeros(len(r) + len(q) + 8, np.uint8)
    out = np.zeros(4, np.int32)
    n = L.nw_host_align(r.ctypes.data, len(r), q.ctypes.data, len(q), fs, w0, ops.ctypes.data, len(ops), out.ctypes.data)
    assert n >= 0, n
    return int(out[0]), int(out[1]), int(out[2]), int(out[3]), ops[:n].copy()


def attempt(L, ref, qry, fs, w):
    """one band: dict of the harness's report and the ops of its walk"""
    r, q = _bytes(ref), _bytes(qry)
    ops = np.zeros(len(r) + len(q) + 8, np.uint8)
    info = np.zeros(8, np.int32)
    n = L.nw_host_attempt(r.ctypes.data, len(r), q.ctypes.data, len(q), fs, w, ops.ctypes.data, len(ops), info.ctypes.data)
    assert n >= 0, n
    keys = ("cost", "accepted", "left_band", "lo", "hi", "corner", "cpl", "ns")
    d = dict(zip(keys, (int(v) for v in info)))
    d["ops"] = ops[:n].copy()
    return d


def check_pair(L, ref, qry, fs, w0=nr.W0):
    """the policy's answer equals the oracle's, after exactly the attempts the restatement of the policy predicts"""
    r, q = _bytes(ref), _bytes(qry)
    score, ops = nr.oracle(r, q, fs)
    st, sc, att, w, got = align(L, r, q, fs, w0)
    est, eatt, ew = nr.expected_attempts(len(r), len(q), fs, score, w0)
    assert (st, att) == (est, eatt), (len(r), len(q), fs, score, st, att, w)
    if st == 0:
        assert sc == score and w == ew
        assert np.array_equal(got, ops)
    else:
        assert sc == -1 and len(got) == 0
    return att, w


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "nw_cases.json")) as f:
        return [c for c in json.load(f)["cases"] if c["indel"] == 1]


def test_the_fixture_has_both_modes():
    assert sum(1 for c in _golden() if c["free_shift"]) >= 3 and sum(1 for c in _golden() if not c["free_shift"]) >= 3


@pytest.mark.parametrize("case", _golden(), ids=lambda c: f"string.d:{c['line']}")
@pytest.mark.parametrize("fs", MODES)
def test_golden_cases(host, case, fs):
    # both modes on every case; in the case's own mode the fixture's score pins the oracle as well
    check_pair(host, case["ref"], case["qry"], fs)
    if "score" in case and bool(fs) == case["free_shift"]:
        assert align(host, case["ref"], case["qry"], fs)[1] == case["score"]


@pytest.mark.parametrize("fs", MODES)
@pytest.mark.parametrize("w0", [1, 3, 64])
def test_random_short_pairs(host, fs, w0):
    """lengths 1-40 (an empty side never reaches the kernel: dh_nw_batch answers it), the four codes and n; small first
    half-widths so that most pairs go through rejected bands first"""
    rng = np.random.default_rng(100 * w0 + fs)
    attempts = 0
    for it in range(1200):
        rl, ql = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        if it % 2:
            r, q = nr.pair_of(rng, rl, ql, [0.0, 0.1, 0.3][it % 3], ncodes=5)
        else:
            r, q = rng.integers(0, 5, rl).astype(np.uint8), rng.integers(0, 5, ql).astype(np.uint8)
        attempts += check_pair(host, r, q, fs, w0)[0]
    assert attempts > 1200 or w0 == 64  # rejected bands really occurred


@pytest.mark.parametrize("fs", MODES)
def test_one_base_sides(host, fs):
    rng = np.random.default_rng(5)
    for n in (1, 2, 63, 64, 65, 300):
        s = rng.integers(0, 4, n).astype(np.uint8)
        for one in ([s[n // 2]], [(s[0] + 1) % 4], [4]):
            check_pair(host, s, np.asarray(one, np.uint8), fs)
            check_pair(host, np.asarray(one, np.uint8), s, fs)


# (d = ql - rl, w) whose band is exactly W wide when nothing is clipped: W = |d| + 2 w + 1
SEAMS = [(1, 127, 256, 4, 1), (0, 128, 257, 8, 1), (1, 255, 512, 8, 1), (0, 256, 513, 16, 1), (1, 511, 1024, 16, 1),
         (0, 512, 1025, 16, 2), (1, 1023, 2048, 16, 2), (0, 1024, 2049, 16, 4)]


@pytest.mark.parametrize("d,w,W,cpl,ns", SEAMS, ids=[f"W{s[2]}" for s in SEAMS])
def test_band_of_one_strip_and_one_cell_more(host, d, w, W, cpl, ns):
    """band widths on both sides of every class boundary: one strip of 64 x 4, 64 x 8, 64 x 16 cells, then two and four
    strips -- W = 1024 is exactly one strip of the widest lanes, 1025 one strip plus one cell"""
    rng = np.random.default_rng(W)
    rl = 1100
    r, q = nr.pair_of(rng, rl, rl + d, 0.03)
    score, ops = nr.oracle(r, q, 0)
    a = attempt(host, r, q, 0, w)
    assert a["hi"] - a["lo"] + 1 == W and (a["cpl"], a["ns"]) == (cpl, ns)
    assert score + 1 <= w and a["accepted"] == 1 and a["cost"] == score == a["corner"]
    assert np.array_equal(a["ops"], ops)


@pytest.mark.parametrize("fs", MODES)
def test_length_difference_above_the_first_half_width(host, fs):
    rng = np.random.default_rng(9)
    for rl, ql in ((100, 300), (300, 100), (500, 1300), (40, 1000)):
        assert abs(rl - ql) > nr.W0
        r, q = nr.pair_of(rng, rl, ql, 0.05)
        check_pair(host, r, q, fs)


@pytest.mark.parametrize("fs", MODES)
def test_rejected_then_accepted(host, fs):
    """90 spaced substitutions: the band of half-width 64 cannot prove them, the next one can (no free shift), the one after
    that with free shift"""
    rng = np.random.default_rng(11)
    r = rng.integers(0, 4, 1800).astype(np.uint8)
    q = r.copy()
    q[10::20] = (q[10::20] + 1) % 4
    score, _ = nr.oracle(r, q, fs)
    assert score == 90
    att, w = check_pair(host, r, q, fs)
    assert (att, w) == ((2, 128) if not fs else (3, 256))
    first = attempt(host, r, q, fs, 64)
    assert first["accepted"] == 0


@pytest.mark.parametrize("fs", MODES)
def test_accepted_at_the_exact_bound(host, fs):
    """c + 1 == w (2 (c + 1) == w with free shift) is accepted, one less is not"""
    rng = np.random.default_rng(13)
    r = rng.integers(0, 4, 400).astype(np.uint8)
    q = r.copy()
    q[15::40] = (q[15::40] + 2) % 4
    c, ops = nr.oracle(r, q, fs)
    assert c == 10
    w = 2 * (c + 1) if fs else c + 1
    a = attempt(host, r, q, fs, w)
    assert a["accepted"] == 1 and a["cost"] == c and np.array_equal(a["ops"], ops)
    b = attempt(host, r, q, fs, w - 1)
    assert b["accepted"] == 0 and b["left_band"] == 0
    st, sc, att, lw, got = align(host, r, q, fs, w0=w)  # the policy stops at that very band
    assert (st, sc, att, lw) == (0, c, 1, w) and np.array_equal(got, ops)


def test_free_shift_path_far_from_the_end_diagonal(host):
    """a stretch of the reference the query lacks: in front of the common part it is free (the path starts on the left
    border, on the end diagonal); behind it the path starts 60 diagonals away from the one it ends on and has to cross them"""
    rng = np.random.default_rng(17)
    core = rng.integers(0, 4, 200).astype(np.uint8)
    q = nr.mutate(rng, core, 0.03)
    att, _ = check_pair(host, np.concatenate([rng.integers(0, 4, 300).astype(np.uint8), core]), q, 1)
    assert att == 1
    for r2, q2 in ((np.concatenate([core, rng.integers(0, 4, 60).astype(np.uint8)]), q),
                   (q, np.concatenate([core, rng.integers(0, 4, 60).astype(np.uint8)]))):
        _, ops = nr.oracle(r2, q2, 1)
        lead = 0
        while lead < len(ops) and ops[lead] == ops[0] and ops[0] in (1, 2):
            lead += 1
        start = (lead if ops[0] == 2 else 0) - (lead if ops[0] == 1 else 0)  # diagonal j - i behind the leading padding
        assert abs(start - (len(q2) - len(r2))) >= 50
        att, w = check_pair(host, r2, q2, 1)
        assert att > 1 and w >= 2 * 51


def test_band_exceeded(host):
    rng = np.random.default_rng(19)
    r, q = rng.integers(0, 4, 30).astype(np.uint8), rng.integers(0, 4, 4200).astype(np.uint8)
    st, sc, att, w, ops = align(host, r, q, 0)  # ql - rl alone is wider than the widest band
    assert (st, sc, att, len(ops)) == (1, -1, 0, 0)


@pytest.mark.parametrize("fs", MODES)
def test_the_acceptance_predicate_rejects_too_narrow_bands(host, fs):
    """The exactness argument on its own: whatever a band of ANY half-width computes, a result the predicate accepts is the
    full matrix's result, and a band below the bound is never accepted.  Among the rejected bands there are walks that
    differ from the reference's -- the predicate is what keeps them out."""
    rng = np.random.default_rng(23 + fs)
    wrong_rejected = narrow = 0
    for it in range(1500):
        rl, ql = int(rng.integers(8, 41)), int(rng.integers(8, 41))
        r, q = nr.pair_of(rng, rl, ql, [0.1, 0.3, 0.6][it % 3])
        score, ops = nr.oracle(r, q, fs)
        for w in (1, 2, 4, 7):
            lo, hi, full = nr.band(rl, ql, w, fs)
            a = attempt(host, r, q, fs, w)
            assert (a["lo"], a["hi"]) == (lo, hi)
            same = a["cost"] == score and np.array_equal(a["ops"], ops) and not a["left_band"]
            if a["accepted"]:
                assert same, (it, w, rl, ql)
            elif not same:
                wrong_rejected += 1
            if not full and not nr.accepted(score, w, fs, False):
                narrow += 1
                assert a["accepted"] == 0, (it, w, rl, ql)
    assert wrong_rejected > 100 and narrow > 1000
