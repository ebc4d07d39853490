"""dh_nw_batch has scratch-arena slots of its own (the SLOT_NW_* group of DhSlot, dh_internal.h): a call between two
Context.edit_paths calls on one context changes neither of them, and its own result equals a fresh context's."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
import nw_ref as nr

pytestmark = pytest.mark.gpu

TS = 100


def same_paths(got, exp):
    for f in ("op_off", "tile_off", "score", "ops", "tile_score"):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), f
    assert got.general_tiles == exp.general_tiles


def test_nw_batch_between_edit_paths_calls():
    w = sim.Workload(150_000, 2, 250, 3000, seed=61, spacing=15000)
    g = dentist_amd.default_align_opts(algo=1, width=64, tspace=TS)
    rng = np.random.default_rng(7)
    pairs = [nr.pair_of(rng, int(n), int(n) + int(rng.integers(-30, 31)), 0.1) for n in rng.integers(200, 1500, 40)]
    refs, qrys = [p[0] for p in pairs], [p[1] for p in pairs]

    def fresh():
        ctx = dentist_amd.Context(0)
        return ctx, ctx.db(w.contigs), ctx.db(w.reads)

    ctx, A, B = fresh()
    try:
        las, trace = ctx.align_db(A, B, g)
        assert len(las) >= w.reads.n
        ep1 = ctx.edit_paths(A, B, las, trace, TS)
        nwp, st = ctx.nw_batch(refs, qrys)
        ep2 = ctx.edit_paths(A, B, las, trace, TS)
        nwp2, st2 = ctx.nw_batch(refs, qrys, free_shift=True)
        assert len(ep1.ops) > 0 and len(nwp.ops) > 0 and not st.any() and not st2.any()
        same_paths(ep2, ep1)
        c2, A2, B2 = fresh()
        try:
            same_paths(c2.edit_paths(A2, B2, las, trace, TS), ep1)
        finally:
            c2.close()
        c3, _, _ = fresh()
        try:
            same_paths(c3.nw_batch(refs, qrys)[0], nwp)
            same_paths(c3.nw_batch(refs, qrys, free_shift=True)[0], nwp2)
        finally:
            c3.close()
        ctx.release_scratch()  # the NW slots go back with the rest, and the next call allocates again
        same_paths(ctx.nw_batch(refs, qrys)[0], nwp)
    finally:
        ctx.close()
