"""Context.collect_filter (dh_la_collect_filter: chains by a scan, stages 1-3 per chain, stages 4-6 per read in four tiers)
against the host function dentist_amd.collect_filter on every case of tests/cfilter_cases.py, in every input order, with the
default LDS cap and with the lowest; the set form on a real mapping; the refusals.  Every comparison is equality."""
import ctypes

import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib, sim

import cfilter_cases as cc

pytestmark = pytest.mark.gpu


def device(ctx, case):
    return ctx.collect_filter(case["las"], case["contig_off"], case["read_off"], cc.popts(case), repeat_mask=case["mask"])


@pytest.fixture(scope="module")
def ordered():
    """every shape in its own order, grouped by read, in LAsort order and permuted, with the host function's answer"""
    out = {}
    for name, case in cc.SHAPES.items():
        out[name] = []
        for kind in (None, "byread", "lasort", "random"):
            c = case if kind is None else cc.reorder(case, kind, seed=7)
            out[name].append((kind, c, cc.host(c)))
    return out


@pytest.mark.parametrize("name", list(cc.SHAPES))
def test_shapes_in_every_order(gpu_ctx, ordered, name):
    for kind, case, exp in ordered[name]:
        assert cc.same(device(gpu_ctx, case), exp), (name, kind)


@pytest.mark.parametrize("name", list(cc.SHAPES))
def test_shapes_with_the_lowest_lds_cap(gpu_ctx, ordered, monkeypatch, name):
    """DH_CFILT_LDS_UNITS = 64: every read of more than 64 units takes the slab of global memory"""
    monkeypatch.setenv("DH_CFILT_LDS_UNITS", str(cc.LOW_CAP))
    for kind, case, exp in ordered[name]:
        assert cc.same(device(gpu_ctx, case), exp), (name, kind)


def test_the_tiers_are_reached(gpu_ctx, monkeypatch, capfd):
    """the tier counts of the DH_TRACE line"""
    monkeypatch.setenv("DH_TRACE", "1")
    for cap, col in ((None, 1), (cc.LOW_CAP, 2)):
        if cap:
            monkeypatch.setenv("DH_CFILT_LDS_UNITS", str(cap))
        for name, tiers in cc.TIERS.items():
            capfd.readouterr()
            device(gpu_ctx, cc.SHAPES[name])
            line = [x for x in capfd.readouterr().err.splitlines() if x.startswith("[cfilt]")][-1]
            w, l, g = tiers[col - 1]
            assert f"tiers: {w} wave, {l} LDS" in line and f", {g} global" in line, line


def test_inplace_and_optional_arguments(gpu_ctx):
    case = cc.SHAPES["planted"]
    las = case["las"].copy()
    out, dropped, used = gpu_ctx.collect_filter(las, case["contig_off"], case["read_off"], cc.popts(case), repeat_mask=case["mask"], inplace=True)
    assert out is las and dropped.tolist() == [1, 1, 1, 1, 2, 1] and used.tolist() == [1, 1, 1, 1, 1, 0, 0]
    assert cc.same(device(gpu_ctx, cc.SHAPES["no_mask"]), cc.host(cc.SHAPES["no_mask"]))


def test_two_calls_in_a_row_give_the_same_result(gpu_ctx):
    """the scratch of the first call is the second's"""
    big, small = cc.SHAPES["units_700"], cc.SHAPES["contained"]
    a, s, b = device(gpu_ctx, big), device(gpu_ctx, small), device(gpu_ctx, big)
    assert cc.same(a, b) and cc.same(a, cc.host(big)) and cc.same(s, cc.host(small))


@pytest.mark.parametrize("name,case,words", cc.refusals(), ids=[r[0] for r in cc.refusals()])
def test_refusals(gpu_ctx, name, case, words):
    las = case["las"].copy()
    with pytest.raises(dentist_amd.DhError) as ei:
        gpu_ctx.collect_filter(las, case["contig_off"], case["read_off"], cc.popts(case), repeat_mask=case["mask"], inplace=True)
    assert ei.value.code == -1 and words in str(ei.value)
    assert las.tobytes() == case["las"].tobytes()   # untouched
    good = cc.SHAPES["planted"]
    assert device(gpu_ctx, good)[1].tolist() == [1, 1, 1, 1, 2, 1]   # the context is usable afterwards


def test_bad_arguments(gpu_ctx):
    L, case = _lib.lib(), cc.SHAPES["planted"]
    las = case["las"].copy()
    rc = L.dh_la_collect_filter(gpu_ctx._h, las.ctypes.data, len(las), case["contig_off"].ctypes.data, 2, case["read_off"].ctypes.data, 7,
                                None, None, None, None, None)
    assert rc == -1 and "bad argument" in L.dh_last_error().decode()
    rc = L.dh_la_collect_filter(gpu_ctx._h, None, 3, case["contig_off"].ctypes.data, 2, case["read_off"].ctypes.data, 7, None, None,
                                cc.popts(case), None, None)
    assert rc == -1 and "bad argument" in L.dh_last_error().decode()
    for n, ncontigs, nreads in ((-1, 2, 7), (len(las), -2, 7), (len(las), 2, -7)):   # a negative count
        rc = L.dh_la_collect_filter(gpu_ctx._h, las.ctypes.data, n, case["contig_off"].ctypes.data, ncontigs, case["read_off"].ctypes.data, nreads,
                                    None, None, cc.popts(case), None, None)
        assert rc == -1 and "bad argument" in L.dh_last_error().decode()
    assert las.tobytes() == case["las"].tobytes()


def test_raw_handle_of_a_real_mapping(gpu_ctx):
    """dh_la_set_collect_filter: the flags go into the set's records; the host function on a copy of the same records"""
    w = sim.Workload(120_000, 2, 600, 4000, seed=5, spacing=10000, gap_max=600)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    h = gpu_ctx.align_db_block(A, B, 0, w.reads.n, dentist_amd.default_align_opts(kmer_mod=4, k=20), select_best=True, raw=True)
    po = dentist_amd.default_process_opts()
    ptr = np.arange(w.contigs.n + 1, dtype=np.int64)
    iv = np.concatenate([[1000, 3000] for _ in range(w.contigs.n)]).astype(np.int32)
    L = _lib.lib()
    n = L.dh_la_set_count(h)
    before = np.frombuffer((ctypes.c_uint8 * (n * cc.LA.itemsize)).from_address(L.dh_la_set_records(h)), dtype=cc.LA).copy()
    got = gpu_ctx.collect_filter(h, w.contigs.off, w.reads.off, po, repeat_mask=(ptr, iv))
    las = _lib._take_la_set(h)[0]   # (owns the handle from here on): the set's records carry the flags
    assert las.tobytes() == got[0].tobytes() and n > 100
    exp = dentist_amd.collect_filter(before, w.contigs.off, w.reads.off, po, repeat_mask=(ptr, iv))
    assert cc.same(got, exp) and int(exp[1].sum()) > 0 and int((exp[0]["flags"] & cc.DISABLED == 0).sum()) > 0
