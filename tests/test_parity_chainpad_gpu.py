"""The chain padder on the device (dh_la_chain_paths: k_cp_plan, the edit-path and global-alignment kernels, k_cp_stitch)
against the restatement of its contract (tests/chainpad_ref.py) on the constructed chains of tests/chainpad_cases.py: ops,
op_off, score and status bit for bit, the replay of every chain's ops over its A range yielding its B range, the fillers
counted, the chain_off form against the flags form, the refusals, and one mapping taken through chaining end to end."""
import numpy as np
import pytest

import chainpad_cases as cc
import chainpad_ref as cr
import dentist_amd
from dentist_amd import _lib, sim

pytestmark = pytest.mark.gpu

NAMES = list(cc.cases().keys())


@pytest.fixture(scope="module")
def expected():
    """the restatement on every case, computed once and never modified"""
    return {n: cr.run(c) for n, c in cc.cases().items()}


def run_case(ctx, case, chain_off=None, las=None):
    A, B = ctx.db(case["A"]), ctx.db(case["B"])
    return ctx.chain_paths(A, B, case["las"] if las is None else las, case["trace"], case["ts"], chain_off=chain_off)


def same(got, exp):
    return (np.array_equal(got[0], exp[0]) and got[1].tobytes() == exp[1].tobytes() and np.array_equal(got[2], exp[2])
            and np.array_equal(got[3], exp[3]))


@pytest.mark.parametrize("name", NAMES)
def test_case_equals_the_restatement(gpu_ctx, expected, name):
    case, exp = cc.cases()[name], expected[name]
    got = run_case(gpu_ctx, case)
    assert np.array_equal(got[0], exp[0]), "op_off"
    assert np.array_equal(got[3], exp[3]), "status"
    assert got[1].tobytes() == exp[1].tobytes(), "ops"
    assert np.array_equal(got[2], exp[2]), "score"
    assert got[4] == exp[4], "fillers aligned on the device"
    assert (got[4] > 0) == case["fillers"]
    assert got[3].tolist() == case["expect"]
    # the replay invariant on the device result
    off = cr.chains_of(case["las"])
    for i in range(len(off) - 1):
        if got[3][i] == cr.NESTED:
            assert got[0][i + 1] == got[0][i] and got[2][i] == -1
            continue
        ch = case["las"][off[i]:off[i + 1]]
        a, b = case["A"].seq(int(ch[0]["aread"])), case["B"].seq(int(ch[0]["bread"]))
        b = sim.revcomp(b) if ch[0]["flags"] & 1 else b
        o = got[1][got[0][i]:got[0][i + 1]]
        assert cr.replay(o, a[ch[0]["abpos"]:ch[-1]["aepos"]], b[ch[0]["bbpos"]:ch[-1]["bepos"]])
        assert got[2][i] == np.count_nonzero(o)


def test_single_record_is_edit_paths(gpu_ctx):
    case = cc.cases()["single"]
    A, B = gpu_ctx.db(case["A"]), gpu_ctx.db(case["B"])
    ep = gpu_ctx.edit_paths(A, B, case["las"], case["trace"], case["ts"])
    got = gpu_ctx.chain_paths(A, B, case["las"], case["trace"], case["ts"])
    assert got[1].tobytes() == ep.ops.tobytes() and got[2][0] == ep.score[0] and got[4] == 0


def test_chain_off_form_equals_flags_form(gpu_ctx, expected):
    for name in ("five_alternating", "chains_300"):
        case = cc.cases()[name]
        off = np.asarray(cr.chains_of(case["las"]), np.int64)
        las = case["las"].copy()
        las["flags"] &= 1  # no chain flags: the offsets alone say where the chains are
        assert same(run_case(gpu_ctx, case, chain_off=off, las=las), expected[name])
    # a prefix of the chains: the records behind chain_off[nchains] are not looked at
    case = cc.cases()["chains_300"]
    off = np.asarray(cr.chains_of(case["las"]), np.int64)[:11]
    got = run_case(gpu_ctx, case, chain_off=off)
    exp = expected["chains_300"]
    assert np.array_equal(got[0], exp[0][:11]) and got[1].tobytes() == exp[1][:exp[0][10]].tobytes()


def test_launch_groups_do_not_change_the_result(gpu_ctx, expected, monkeypatch):
    monkeypatch.setenv("DH_EDIT_CHUNK", "64")
    monkeypatch.setenv("DH_NW_CHUNK_KB", "4")
    for name in ("chains_300", "short_records_200"):
        got = run_case(gpu_ctx, cc.cases()[name])
        assert same(got, expected[name]) and got[4] == expected[name][4]


def test_refusals_and_no_chains(gpu_ctx):
    case = cc.cases()["five_alternating"]
    A, B = gpu_ctx.db(case["A"]), gpu_ctx.db(case["B"])
    las, tr, ts = case["las"], case["trace"], case["ts"]
    call = lambda l, off=None, t=tr: gpu_ctx.chain_paths(A, B, l, t, ts, chain_off=off)
    for off in ([1, 5], [0, 3, 2, 5], [0, 6], [0, 2, 2, 5]):  # not from 0, decreasing, past n, an empty chain
        with pytest.raises(Exception, match="chain"):
            call(las, np.asarray(off, np.int64))
    bad = las.copy()
    bad["bread"][2] = 1
    with pytest.raises(Exception, match="LA 2"):
        call(bad)
    bad = las.copy()
    bad["flags"][3] ^= 1
    with pytest.raises(Exception, match="LA 3"):
        call(bad)
    bad = las[[0, 2, 1, 3, 4]].copy()
    bad["flags"] = las["flags"]
    with pytest.raises(Exception, match="LA 2.*decreases"):
        call(bad)
    bad = las.copy()
    bad["tlen"][1] += 1  # what dh_la_edit_paths refuses
    with pytest.raises(Exception, match="LA 1"):
        call(bad)
    for got in (call(las, np.zeros(1, np.int64)), call(las[:0], None, tr[:0])):
        assert len(got[2]) == 0 and got[0].tolist() == [0] and len(got[1]) == 0 and got[4] == 0


def test_mapping_through_chaining_end_to_end(gpu_ctx):
    w = sim.Workload(150_000, 2, 120, 3000, seed=61, spacing=15000)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    g = dentist_amd.default_align_opts(algo=1, width=64, tspace=100)
    las, trace = gpu_ctx.align_db(A, B, g, select_best=True)
    ch = gpu_ctx.chain(las, 100)
    rec, tr = ch.to_set(las, trace, 100)
    assert len(ch) > 0 and len(rec) >= len(ch)
    got = gpu_ctx.chain_paths(A, B, rec, tr, 100, chain_off=ch.off)
    assert same(gpu_ctx.chain_paths(A, B, rec, tr, 100), got), "the set's flags say what its offsets say"
    case = dict(A=w.contigs, B=w.reads, las=rec, trace=tr, ts=100, chain_off=ch.off)
    exp = cr.run(case)
    assert same(got, exp) and got[4] == exp[4]
    nested = int(np.count_nonzero(exp[3] == cr.NESTED))
    assert nested <= 0.05 * len(ch), "the restatement alone exceeds the cap on this workload"
    assert int(np.count_nonzero(got[3] == cr.NESTED)) == nested
    rc = {}
    for i in range(len(ch)):
        if got[3][i] == cr.NESTED:
            continue
        c = rec[ch.off[i]:ch.off[i + 1]]
        a, br = w.contigs.seq(int(c[0]["aread"])), int(c[0]["bread"])
        if c[0]["flags"] & 1:
            rc.setdefault(br, sim.revcomp(w.reads.seq(br)))
        b = rc[br] if c[0]["flags"] & 1 else w.reads.seq(br)
        assert cr.replay(got[1][got[0][i]:got[0][i + 1]], a[c[0]["abpos"]:c[-1]["aepos"]], b[c[0]["bbpos"]:c[-1]["bepos"]])


def test_set_form_reads_the_chains_from_the_flags(gpu_ctx):
    w = sim.Workload(100_000, 2, 40, 3000, seed=7, spacing=15000)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    g = dentist_amd.default_align_opts(algo=1, width=64, tspace=100)
    h = gpu_ctx.align_db_block(A, B, 0, w.reads.n, g, select_best=True, raw=True)
    got = gpu_ctx.chain_paths(A, B, h)
    las, trace, ts = _lib._take_la_set(h)  # (the views own the set from here on)
    assert len(got[2]) == len(cr.chains_of(las)) - 1 > 0
    exp = gpu_ctx.chain_paths(A, B, las, trace, ts)
    assert same(got, exp) and got[4] == exp[4]
    with pytest.raises(ValueError):
        gpu_ctx.chain_paths(A, B, h, chain_off=[0, 1])
