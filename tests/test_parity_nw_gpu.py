"""Global alignment of arbitrary sequence pairs on the GPU (dh_nw_batch / Context.nw_batch: k_nw, dh_nw.hip) against
oracle/nw.c: every op, score and status, both free_shift values; the reference's own vectors with their texts; a pair above
the widest band; refusals; the chunk knob."""
import json
import os

import numpy as np
import pytest

import dentist_amd
import nw_ref as nr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = [False, True]
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 700, 1023, 1024, 1025, 3000]  # strips of 64 x 4 and 64 x 16 cells
DIVS = [0.0, 0.02, 0.15, 0.35]


def _golden():
    with open(os.path.join(ROOT, "tests", "golden", "nw_cases.json")) as f:
        return [c for c in json.load(f)["cases"] if c["indel"] == 1]


def _as_bytes(s):
    return np.frombuffer(s.encode(), np.uint8)


@pytest.fixture(scope="module")
def batch():
    """about 300 seeded pairs with the oracle's answer for both modes, computed once"""
    rng = np.random.default_rng(20261018)
    refs, qrys = [], []
    for it in range(300):
        rl = int(rng.choice(LENGTHS))
        if rl >= 700:
            rl += int(rng.integers(-20, 21))
        kind = it % 4
        if kind == 0:  # unequal lengths: the query is another length of the list
            ql = int(rng.choice(LENGTHS))
        elif kind == 1:
            ql = max(0, rl + int(rng.integers(-90, 91)))
        else:
            ql = rl
        r, q = nr.pair_of(rng, rl, ql, float(rng.choice(DIVS)), ncodes=5 if it % 7 == 0 else 4)
        refs.append(r)
        qrys.append(q)
    exp = {fs: [nr.oracle(r, q, fs) for r, q in zip(refs, qrys)] for fs in MODES}
    return refs, qrys, exp


def classes_of(refs, qrys, exp, fs):
    """(cells per lane, strips) of the band that answers each pair"""
    out = set()
    for r, q, e in zip(refs, qrys, exp):
        if len(r) and len(q):
            st, _, w = nr.expected_attempts(len(r), len(q), fs, e[0])
            if st == 0:
                lo, hi, _ = nr.band(len(r), len(q), w, fs)
                W = hi - lo + 1
                out.add((4 if W <= 256 else (8 if W <= 512 else 16), 1 if W <= 1024 else (2 if W <= 2048 else 4)))
    return out


def check_against_oracle(ep, status, refs, qrys, exp, fs):
    assert len(ep) == len(refs) == len(status)
    assert np.all(ep.tile_off == 0) and len(ep.tile_score) == 0 and ep.general_tiles == 0
    exceeded = 0
    for i, (r, q) in enumerate(zip(refs, qrys)):
        score, ops = exp[i]
        est = nr.expected_attempts(len(r), len(q), fs, score)[0] if len(r) and len(q) else 0
        got = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        assert status[i] == est, (i, len(r), len(q), score)
        if est:
            exceeded += 1
            assert ep.score[i] == -1 and len(got) == 0
        else:
            assert ep.score[i] == score, (i, len(r), len(q))
            assert np.array_equal(got, ops), (i, len(r), len(q), score)
    return exceeded


@pytest.mark.parametrize("case", _golden(), ids=lambda c: f"string.d:{c['line']}")
def test_golden_vectors(gpu_ctx, case):
    fs = case["free_shift"]
    ep, status = gpu_ctx.nw_batch([case["ref"]], [case["qry"]], free_shift=fs)
    score, ops = nr.oracle(_as_bytes(case["ref"]), _as_bytes(case["qry"]), fs)
    assert status[0] == 0 and ep.score[0] == score == case.get("score", score)
    assert np.array_equal(ep.ops, ops)
    if "ops" in case:
        assert [{0: "sub", 3: "sub", 1: "del", 2: "ins"}[int(o)] for o in ep.ops] == case["ops"]
    assert dentist_amd.format_alignment(case["ref"], case["qry"], ep.ops, case["width"]) == case["text"]


def test_golden_vectors_as_one_batch(gpu_ctx):
    for fs in MODES:
        cases = [c for c in _golden() if c["free_shift"] == fs]
        ep, status = gpu_ctx.nw_batch([c["ref"] for c in cases], [c["qry"] for c in cases], free_shift=fs)
        assert not status.any()
        for i, c in enumerate(cases):
            assert dentist_amd.format_alignment(c["ref"], c["qry"], ep.ops[ep.op_off[i]:ep.op_off[i + 1]], c["width"]) == c["text"]


@pytest.mark.parametrize("fs", MODES, ids=["global", "free-shift"])
def test_seeded_batch_against_the_oracle(gpu_ctx, batch, fs):
    refs, qrys, exp = batch
    ep, status = gpu_ctx.nw_batch(refs, qrys, free_shift=fs)
    check_against_oracle(ep, status, refs, qrys, exp[fs], fs)
    assert sum(1 for r, q in zip(refs, qrys) if len(r) == 0 or len(q) == 0) > 5
    assert classes_of(refs, qrys, exp[fs], fs) == {(4, 1), (8, 1), (16, 1), (16, 2), (16, 4)}  # every kernel took part


@pytest.mark.parametrize("fs", MODES, ids=["global", "free-shift"])
def test_pair_above_the_widest_band(gpu_ctx, fs):
    """two unrelated 6 kb sequences need a half-width no kernel serves; a pair whose length difference alone is wider than
    the widest band never reaches the device.  Their neighbours in the batch are answered as ever."""
    rng = np.random.default_rng(3)
    near = [nr.pair_of(rng, 500, 510, 0.1) for _ in range(3)]
    far = (rng.integers(0, 4, 6000).astype(np.uint8), rng.integers(0, 4, 6000).astype(np.uint8))
    skew = (rng.integers(0, 4, 40).astype(np.uint8), rng.integers(0, 4, 5000).astype(np.uint8))
    pairs = [near[0], far, near[1], skew, near[2]]
    refs, qrys = [p[0] for p in pairs], [p[1] for p in pairs]
    ep, status = gpu_ctx.nw_batch(refs, qrys, free_shift=fs)
    assert status[1] == dentist_amd.NW_BAND_EXCEEDED and ep.score[1] == -1 and ep.op_off[2] == ep.op_off[1]
    if not fs:  # (with free shift the band is centred on the end diagonal and 40 x 5 000 is an ordinary pair)
        assert status[3] == dentist_amd.NW_BAND_EXCEEDED and ep.score[3] == -1 and ep.op_off[4] == ep.op_off[3]
    for i in (0, 2, 4) + ((3,) if fs else ()):
        score, ops = nr.oracle(refs[i], qrys[i], fs)
        assert status[i] == 0 and ep.score[i] == score and np.array_equal(ep.ops[ep.op_off[i]:ep.op_off[i + 1]], ops)


def test_refusals(gpu_ctx):
    r = np.zeros(100, np.uint8)
    ok = np.asarray([0, 50, 100], np.int64)
    for bad in ([0, 60, 50], [-1, 50, 100], [10, 5, 100]):
        with pytest.raises(dentist_amd.DhError) as e:
            gpu_ctx.nw_batch_raw(r, np.asarray(bad, np.int64), r, ok)
        assert e.value.code == -1
        with pytest.raises(dentist_amd.DhError):
            gpu_ctx.nw_batch_raw(r, ok, r, np.asarray(bad, np.int64))
    big = np.zeros(dentist_amd.NW_MAX_LEN + 1, np.uint8)
    with pytest.raises(dentist_amd.DhError) as e:
        gpu_ctx.nw_batch([r[:10], big], [r[:10], r[:10]])
    assert e.value.code == -1 and "pair 1" in str(e.value)
    with pytest.raises(ValueError):
        gpu_ctx.nw_batch([r], [r, r])
    ep, status = gpu_ctx.nw_batch([], [])  # an empty batch is not an error
    assert len(ep) == 0 and len(status) == 0
    ep, status = gpu_ctx.nw_batch([r[:7], r[:0], r[:0]], [r[:0], r[:5], r[:0]])  # empty sides: the host's answer
    assert ep.op_off.tolist() == [0, 7, 12, 12] and ep.ops.tolist() == [1] * 7 + [2] * 5 and ep.score.tolist() == [7, 5, 0]
    ep, status = gpu_ctx.nw_batch([r[:7], r[:0]], [r[:0], r[:5]], free_shift=True)
    assert ep.ops.tolist() == [1] * 7 + [2] * 5 and ep.score.tolist() == [0, 0]


def test_chunks_give_the_same_result(gpu_ctx, batch, monkeypatch):
    refs, qrys, exp = batch
    words = sum(nr.first_words(len(r), len(q), False) for r, q in zip(refs, qrys))
    kb = 4096
    assert words * 4 >= 3 * kb * 1024  # the knob splits the first attempts into three chunks at least
    ep, status = gpu_ctx.nw_batch(refs, qrys)
    monkeypatch.setenv("DH_NW_CHUNK_KB", str(kb))
    ep2, status2 = gpu_ctx.nw_batch(refs, qrys)
    for f in ("op_off", "tile_off", "score", "ops"):
        assert np.array_equal(getattr(ep, f), getattr(ep2, f)), f
    assert np.array_equal(status, status2)
    check_against_oracle(ep2, status2, refs, qrys, exp[False], False)
