"""dh_nw_affine_batch has scratch-arena slots of its own (the SLOT_NWA_* group of DhSlot, dh_internal.h): a call between
Context.nw_batch, Context.edit_paths and an alignment call on one context changes none of them, and its own result equals
a fresh context's."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
import nwa_ref as ar

pytestmark = pytest.mark.gpu

TS = 100


def same_paths(got, exp):
    for f in ("op_off", "tile_off", "score", "ops", "tile_score"):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), f
    assert got.general_tiles == exp.general_tiles


def test_nw_affine_batch_between_other_calls():
    w = sim.Workload(150_000, 2, 250, 3000, seed=61, spacing=15000)
    g = dentist_amd.default_align_opts(algo=1, width=64, tspace=TS)
    rng = np.random.default_rng(7)
    pairs = [ar.pair_of(rng, int(n), int(n) + int(rng.integers(-30, 31)), 0.1) for n in rng.integers(200, 1500, 40)]
    refs, qrys = [p[0] for p in pairs], [p[1] for p in pairs]

    def fresh():
        ctx = dentist_amd.Context(0)
        return ctx, ctx.db(w.contigs), ctx.db(w.reads)

    ctx, A, B = fresh()
    try:
        las, trace = ctx.align_db(A, B, g)
        assert len(las) >= w.reads.n
        ep1 = ctx.edit_paths(A, B, las, trace, TS)
        nw1, _ = ctx.nw_batch(refs, qrys)
        aff, st = ctx.nw_affine_batch(refs, qrys)
        nw2, _ = ctx.nw_batch(refs, qrys)
        ep2 = ctx.edit_paths(A, B, las, trace, TS)
        aff2, st2 = ctx.nw_affine_batch(refs, qrys, scoring=(1, -1, 2, 1))
        las2, trace2 = ctx.align_db(A, B, g)
        aff3, _ = ctx.nw_affine_batch(refs, qrys)
        assert len(ep1.ops) > 0 and len(aff.ops) > 0 and not st.any() and not st2.any()
        same_paths(ep2, ep1)
        same_paths(nw2, nw1)
        same_paths(aff3, aff)
        assert las2.tobytes() == las.tobytes() and np.array_equal(trace2[:len(trace)], trace[:len(trace2)])
        c3, _, _ = fresh()
        try:
            same_paths(c3.nw_affine_batch(refs, qrys)[0], aff)
            same_paths(c3.nw_affine_batch(refs, qrys, scoring=(1, -1, 2, 1))[0], aff2)
            same_paths(c3.nw_batch(refs, qrys)[0], nw1)
        finally:
            c3.close()
        ctx.release_scratch()  # the NWA slots go back with the rest, and the next call allocates again
        same_paths(ctx.nw_affine_batch(refs, qrys)[0], aff)
    finally:
        ctx.close()
