"""The entry points of one context share its scratch arena (DhSlot in dh_internal.h: every buffer has a slot of its own,
grouped by owner).  What the slot names protect: a call leaves nothing behind in the arena that changes a later call of
another entry point, and overwrites nothing a later call relies on.  One context runs a mapping, `process` on its pile-up,
edit paths, the transposition and the same mapping again; the second mapping equals the first bit for bit, and every
result in between equals the same call on a context that has run nothing else."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from helpers import FIELDS

pytestmark = pytest.mark.gpu

TS = 100


@pytest.fixture(scope="module")
def workload():
    """the mapping workload of test_parity_transpose_gpu.py: 3 contigs, 250 reads of 3 kb, one pile-up of 9 reads that closes"""
    return sim.Workload(150_000, 2, 250, 3000, seed=61, spacing=15000)


def assert_same_mapping(got, exp):
    (gl, gt), (el, et) = got, exp
    assert len(gl) == len(el) > 0
    for f in FIELDS + ("toff",):
        assert np.array_equal(gl[f], el[f]), f
    assert np.array_equal(gt, et)  # (same toff: every trace value in the same place)


def assert_same_process(got, exp):
    assert got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1])


def assert_same_edit_paths(got, exp):
    for f in ("op_off", "tile_off", "score", "ops", "tile_score"):
        assert np.array_equal(getattr(got, f), getattr(exp, f)), f
    assert got.general_tiles == exp.general_tiles


def assert_same_transposed(got, exp):
    assert got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])


@pytest.mark.parametrize("mjoin", [False, True], ids=["directory", "mapping-join"])
def test_calls_of_one_context_do_not_disturb_each_other(workload, monkeypatch, mjoin):
    w = workload
    if mjoin:  # the seeds of the mapping through the partitioned join (its own group of slots) instead of the directory
        monkeypatch.setenv("DH_MJOIN_MIN", "0")
    g = dentist_amd.default_align_opts(algo=1, width=64, tspace=TS)
    po = dentist_amd.default_process_opts(algo=1)

    def fresh():
        ctx = dentist_amd.Context(0)
        return ctx, ctx.db(w.contigs), ctx.db(w.reads)

    ctx, A, B = fresh()
    try:
        ctx.mjoin_counts(reset=True)
        las, trace = ctx.align_db(A, B, g)
        assert (ctx.mjoin_counts()[0] > 0) == mjoin
        assert len(las) >= w.reads.n and set((las["flags"] & 1).tolist()) == {0, 1}
        piles = dentist_amd.Pileups(las, w.contigs.off, po)
        assert len(piles) > 0
        proc = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po)
        assert np.any(proc[0]["status"] == 0) and len(proc[1]) > 0
        ep = ctx.edit_paths(A, B, las, trace, TS)
        assert len(ep.ops) > 0
        tr = ctx.transpose(A, B, las, trace, TS)
        assert len(tr[0]) == len(las)
        assert_same_mapping(ctx.align_db(A, B, g), (las, trace))
        # each result in between against the same call on a context of its own
        for exp, call, same in ((proc, lambda c, a, b: dentist_amd.process_pileups(c, a, b, las, trace, piles, po), assert_same_process),
                                (ep, lambda c, a, b: c.edit_paths(a, b, las, trace, TS), assert_same_edit_paths),
                                (tr, lambda c, a, b: c.transpose(a, b, las, trace, TS), assert_same_transposed)):
            c2, A2, B2 = fresh()
            try:
                same(call(c2, A2, B2), exp)
            finally:
                c2.close()
    finally:
        ctx.close()
