"""One voting round of dh_consensus on the constructed pile-ups of consensus_cases.py against the oracle, bit for bit:
every named case and every seeded random pile on the default path, the band-class cases with the scalar fill forced, the
trace spacings up to 126 with the byte-wise vote passes forced, the scratch arena reused across piles of different sizes,
and the one malformed tile the fills refuse."""
import numpy as np
import pytest

import consensus_cases as cc
import dentist_amd

pytestmark = pytest.mark.gpu


def gpu_consensus(ctx, cid):
    _, db, las, trace, ts = cc.built(cid)
    return dentist_amd.consensus(ctx, ctx.db(db), las, trace, ts, 0, rounds=1)


def assert_cases_match(ctx, ids):
    bad = [cid for cid in ids if not np.array_equal(gpu_consensus(ctx, cid), cc.expected(cid)[0])]
    assert not bad, f"{len(bad)} of {len(ids)} cases differ from the oracle: {bad[:8]}"


@pytest.mark.parametrize("family", [f for f in cc.FAMILIES if f != "random"])
def test_named_cases_match_the_oracle(gpu_ctx, family):
    assert_cases_match(gpu_ctx, cc.ids_of(family))


@pytest.mark.parametrize("part", range(3))
def test_random_piles_match_the_oracle(gpu_ctx, part):
    ids = cc.ids_of("random")
    assert len(ids) == cc.NRANDOM
    assert_cases_match(gpu_ctx, ids[part::3])


def test_band_classes_with_the_scalar_fill_forced(gpu_ctx, monkeypatch):
    ids = cc.ids_of("band", "launch")
    fills = [0, 0, 0]
    for cid in ids:   # the classes as the host computes them from the trace that is passed in
        fills = [x + y for x, y in zip(fills, cc.band_classes(*cc.built(cid)[2:4]))]
    assert all(fills)
    default = {cid: gpu_consensus(gpu_ctx, cid) for cid in ids}
    monkeypatch.setenv("DH_CONS_SCALAR", "1")
    for cid in ids:
        got = gpu_consensus(gpu_ctx, cid)
        assert np.array_equal(got, default[cid]) and np.array_equal(got, cc.expected(cid)[0]), cid


def test_column_set_passes_against_the_bytewise_ones(gpu_ctx, monkeypatch):
    ids = [cid for cid in cc.ids_of("tspace", "ins", "homo", "codes", "random") if cc.built(cid)[4] <= 126]
    assert {cc.vote_kernel(cc.built(cid)[4]) for cid in ids} == {13, 16}
    ids = [cid for cid in ids if not cid.startswith("random") or int(cid.split("-")[1]) % 3 == 0]
    default = {cid: gpu_consensus(gpu_ctx, cid) for cid in ids}
    monkeypatch.setenv("DH_VOTE_BYTEWISE", "1")
    for cid in ids:
        got = gpu_consensus(gpu_ctx, cid)
        assert np.array_equal(got, default[cid]) and np.array_equal(got, cc.expected(cid)[0]), cid


def test_same_pile_again_after_a_larger_one(gpu_ctx):
    """The scratch arena only grows and is reused: a pile gives the same bytes before and after a larger one."""
    for small, large in (("tspace-100", "space-2046"), ("ties-sub-2of3", "band-dmax240"), ("space-255", "tspace-250")):
        first = gpu_consensus(gpu_ctx, small)
        assert np.array_equal(gpu_consensus(gpu_ctx, large), cc.expected(large)[0]), large
        again = gpu_consensus(gpu_ctx, small)
        assert first.tobytes() == again.tobytes() and np.array_equal(again, cc.expected(small)[0]), small


def test_tile_with_fewer_diffs_than_its_length_difference_is_refused(gpu_ctx):
    """A tile of 60 columns and 63 B bases that claims 0 diffs has no path inside its band: the fill flags it, the call
    fails with the capacity status, and the context goes on working."""
    tmpl, specs, ts = cc.refusal_case()
    db, las, trace = cc.pile(tmpl, specs, ts)
    with pytest.raises(dentist_amd.DhError, match="score-matrix capacity"):
        dentist_amd.consensus(gpu_ctx, gpu_ctx.db(db), las, trace, ts, 0, rounds=1)
    assert_cases_match(gpu_ctx, ["band-mixed", "tspace-126"])
