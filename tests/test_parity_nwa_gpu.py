"""Global alignment with affine gap costs on the GPU (dh_nw_affine_batch / Context.nw_affine_batch: k_nwa, dh_nwa.hip)
against the full matrix of tests/nwa_ref.py: every op, score and status under two scorings; the unit-cost reduction against
Context.nw_batch; pairs above the widest band; refusals; the chunk knob."""
import numpy as np
import pytest

import dentist_amd
import nwa_ref as ar

pytestmark = pytest.mark.gpu
MAX_W = dentist_amd.NWA_MAX_BAND
LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 700, 1023, 1024, 1025, 1500]
DIVS = [0.0, 0.02, 0.15, 0.35]
SCORINGS = [None, (1, -1, 2, 1)]


def _sc(sc):
    return ar.DEFAULT if sc is None else sc


@pytest.fixture(scope="module")
def batch():
    """120 seeded pairs, at most 30 of them with a sequence of 1 000 bases or more, with the full matrix's answer for both
    scorings, computed once"""
    rng = np.random.default_rng(20261019)
    refs, qrys, long_ones = [], [], 0
    for it in range(120):
        while True:
            rl = int(rng.choice(LENGTHS))
            kind = it % 4
            if kind == 0:    # unequal lengths: the query is another length of the list
                ql = int(rng.choice(LENGTHS))
            elif kind == 1:  # +-90
                ql = max(0, rl + int(rng.integers(-90, 91)))
            else:
                ql = rl
            if max(rl, ql) < 1000 or long_ones < 30:
                break
        long_ones += max(rl, ql) >= 1000
        # (the widest classes answer only pairs that need them: a long pair of 35 % divergence every fourth time)
        div = 0.35 if (max(rl, ql) >= 1000 and it % 4 == 2) else float(rng.choice(DIVS))
        r, q = ar.pair_of(rng, rl, ql, div, ncodes=5 if it % 7 == 0 else 4)
        refs.append(r)
        qrys.append(q)
    exp = {sc: [ar.align(r, q, _sc(sc)) for r, q in zip(refs, qrys)] for sc in SCORINGS}
    return refs, qrys, exp


def classes_of(refs, qrys, exp, sc):
    """(cells per lane, strips) of the band that answers each pair, from the restated policy"""
    out = set()
    ce = ar.costs(_sc(sc))[1]
    for r, q, e in zip(refs, qrys, exp):
        if len(r) and len(q):
            st, _, w = ar.expected_attempts(len(r), len(q), e[1], ce, MAX_W)
            if st == 0:
                lo, hi, _ = ar.band(len(r), len(q), w)
                out.add(ar.band_class(hi - lo + 1))
    return out


def check_against_the_full_matrix(ep, status, refs, qrys, exp, sc):
    assert len(ep) == len(refs) == len(status)
    assert np.all(ep.tile_off == 0) and len(ep.tile_score) == 0 and ep.general_tiles == 0
    ce = ar.costs(_sc(sc))[1]
    exceeded = 0
    for i, (r, q) in enumerate(zip(refs, qrys)):
        score, cost, ops = exp[i]
        est = ar.expected_attempts(len(r), len(q), cost, ce, MAX_W)[0] if len(r) and len(q) else 0
        got = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        assert status[i] == est, (i, len(r), len(q), cost)
        if est:
            exceeded += 1
            assert ep.score[i] == -1 and len(got) == 0
        else:
            assert ep.score[i] == score, (i, len(r), len(q))
            assert np.array_equal(got, ops), (i, len(r), len(q), score)
    return exceeded


@pytest.mark.parametrize("sc", SCORINGS, ids=["default", "1,-1,2,1"])
def test_seeded_batch_against_the_full_matrix(gpu_ctx, batch, sc):
    refs, qrys, exp = batch
    assert len(refs) == 120 and sum(1 for r, q in zip(refs, qrys) if max(len(r), len(q)) >= 1000) <= 30
    ep, status = gpu_ctx.nw_affine_batch(refs, qrys, scoring=sc)
    check_against_the_full_matrix(ep, status, refs, qrys, exp[sc], sc)
    assert sum(1 for r, q in zip(refs, qrys) if len(r) == 0 or len(q) == 0) >= 3
    assert classes_of(refs, qrys, exp[sc], sc) == {(4, 1), (8, 1), (16, 1), (16, 2)}  # every instantiated kernel took part


def test_unit_costs_equal_nw_batch(gpu_ctx, batch):
    refs, qrys, _ = batch
    keep = [i for i in range(len(refs)) if max(len(refs[i]), len(qrys[i])) < 1000 or i % 3 == 0]
    refs, qrys = [refs[i] for i in keep], [qrys[i] for i in keep]
    ep, st = gpu_ctx.nw_affine_batch(refs, qrys, scoring=(0, -1, 0, 1))
    ep0, st0 = gpu_ctx.nw_batch(refs, qrys)
    answered = 0
    for i in range(len(refs)):
        if st[i] or st0[i]:  # (the two band limits differ)
            continue
        answered += 1
        assert ep.score[i] == -ep0.score[i], i
        assert np.array_equal(ep.ops[ep.op_off[i]:ep.op_off[i + 1]], ep0.ops[ep0.op_off[i]:ep0.op_off[i + 1]]), i
    assert answered >= len(refs) - 10


def test_pair_above_the_widest_band(gpu_ctx):
    """two unrelated 3 kb sequences need a half-width no kernel serves; a pair whose length difference alone is wider than
    the widest band never reaches the device.  Their neighbours in the batch are answered as ever."""
    rng = np.random.default_rng(3)
    near = [ar.pair_of(rng, 500, 510, 0.1) for _ in range(3)]
    far = (rng.integers(0, 4, 3000).astype(np.uint8), rng.integers(0, 4, 3000).astype(np.uint8))
    skew = (rng.integers(0, 4, 40).astype(np.uint8), rng.integers(0, 4, MAX_W + 500).astype(np.uint8))
    pairs = [near[0], far, near[1], skew, near[2]]
    refs, qrys = [p[0] for p in pairs], [p[1] for p in pairs]
    ep, status = gpu_ctx.nw_affine_batch(refs, qrys)
    for i in (1, 3):
        assert status[i] == dentist_amd.NW_BAND_EXCEEDED and ep.score[i] == -1 and ep.op_off[i + 1] == ep.op_off[i]
    for i in (0, 2, 4):
        score, cost, ops = ar.align(refs[i], qrys[i])
        assert status[i] == 0 and ep.score[i] == score and np.array_equal(ep.ops[ep.op_off[i]:ep.op_off[i + 1]], ops)


def test_refusals(gpu_ctx):
    r = np.zeros(100, np.uint8)
    ok = np.asarray([0, 50, 100], np.int64)
    for bad in ([0, 60, 50], [-1, 50, 100], [10, 5, 100]):
        with pytest.raises(dentist_amd.DhError) as e:
            gpu_ctx.nw_affine_batch_raw(r, np.asarray(bad, np.int64), r, ok)
        assert e.value.code == -1
        with pytest.raises(dentist_amd.DhError):
            gpu_ctx.nw_affine_batch_raw(r, ok, r, np.asarray(bad, np.int64))
    big = np.zeros(dentist_amd.NWA_MAX_LEN + 1, np.uint8)
    with pytest.raises(dentist_amd.DhError) as e:
        gpu_ctx.nw_affine_batch([r[:10], big], [r[:10], r[:10]])
    assert e.value.code == -1 and "pair 1" in str(e.value)
    for bad in ((0, -1, 0, 0), (-4, -5, 0, 2),    # ce <= 0
                (1, 2, 2, 1),                      # match < mismatch
                (1, -1, -1, 1),                    # gap_open < 0
                (5, -4, 16, 10 ** 6), (5, -4, 2 ** 30, 4), (10 ** 5, -4, 16, 4)):  # overflowable
        with pytest.raises(dentist_amd.DhError) as e:
            gpu_ctx.nw_affine_batch([r[:10]], [r[:10]], scoring=bad)
        assert e.value.code == -1, bad
    with pytest.raises(ValueError):
        gpu_ctx.nw_affine_batch([r], [r, r])
    ep, status = gpu_ctx.nw_affine_batch([], [])  # an empty batch is not an error
    assert len(ep) == 0 and len(status) == 0
    ep, status = gpu_ctx.nw_affine_batch([r[:7], r[:0], r[:0]], [r[:0], r[:5], r[:0]])  # empty sides: the host's answer
    assert ep.op_off.tolist() == [0, 7, 12, 12] and ep.ops.tolist() == [1] * 7 + [2] * 5
    assert ep.score.tolist() == [-(16 + 4 * 7), -(16 + 4 * 5), 0] and not status.any()


def test_chunks_give_the_same_result(gpu_ctx, batch, monkeypatch):
    refs, qrys, exp = batch
    words = sum(ar.first_words(len(r), len(q), MAX_W) for r, q in zip(refs, qrys))
    kb = 256
    assert words * 8 >= 3 * kb * 1024  # the knob splits the first attempts into three chunks at least
    ep, status = gpu_ctx.nw_affine_batch(refs, qrys)
    monkeypatch.setenv("DH_NW_CHUNK_KB", str(kb))
    ep2, status2 = gpu_ctx.nw_affine_batch(refs, qrys)
    for f in ("op_off", "tile_off", "score", "ops"):
        assert np.array_equal(getattr(ep, f), getattr(ep2, f)), f
    assert np.array_equal(status, status2)
    check_against_the_full_matrix(ep2, status2, refs, qrys, exp[None], None)
