"""The lane code and the host plan of the collect filters (dentist_amd/csrc/dh_cfilt.h) compiled for the CPU and played as 64-lane
wavefronts and workgroups (tests/native/cfilt_host.cpp) against the contract on every case of tests/cfilter_cases.py: the oracle
restatement (oracle/collect_filters.py) on the small ones, the host function on the others; in every input order, with the
default LDS cap and with the lowest.  The harness claims the slots of a read's segment in descending order.  Every comparison
is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import cfilter_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libcfilt_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libcfilt_host.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.cfilt_host.argtypes = [vp, i64, vp, i32, vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp]
    L.cfilt_host.restype = i64
    return L


def run(L, case, lds_units=8192):
    """((las, dropped6, read_used) or None, info) of the harness"""
    las = np.ascontiguousarray(case["las"], dtype=cc.LA).copy()
    co, ro = np.ascontiguousarray(case["contig_off"], dtype=np.int64), np.ascontiguousarray(case["read_off"], dtype=np.int64)
    rp = ri = None
    if case["mask"] is not None:
        rp = np.ascontiguousarray(case["mask"][0], dtype=np.int64)
        ri = np.ascontiguousarray(case["mask"][1], dtype=np.int32)   # (exactly the intervals: nothing behind them)
    dropped, used, info = np.zeros(6, np.int64), np.zeros(len(ro) - 1, np.uint8), np.zeros(8, np.int64)
    o = case["opts"]
    rc = L.cfilt_host(las.ctypes.data if len(las) else None, len(las), co.ctypes.data, len(co) - 1, ro.ctypes.data, len(ro) - 1,
                      rp.ctypes.data if rp is not None else None, ri.ctypes.data if ri is not None and len(ri) else None,
                      o["max_align_err_ppm"], o["allowance"], o["min_anchor"], lds_units, dropped.ctypes.data, used.ctypes.data, info.ctypes.data)
    assert rc in (0, -1), rc
    if rc < 0:
        assert las.tobytes() == np.ascontiguousarray(case["las"], dtype=cc.LA).tobytes()   # a refusal leaves las untouched
        return None, info
    return (las, dropped, used), info


@pytest.mark.parametrize("name", list(cc.SHAPES))
def test_shapes_in_every_order(harness, name):
    for kind in (None, "byread", "lasort", "random"):
        case = cc.SHAPES[name] if kind is None else cc.reorder(cc.SHAPES[name], kind, seed=7)
        exp = cc.expected(case)
        for lds_units in (8192, cc.LOW_CAP):
            got, info = run(harness, case, lds_units)
            assert cc.same(got, exp), (name, kind, lds_units)
            assert info[0] == len(cc.cf.chain_ranges(case["las"])) if len(case["las"]) else info[0] == 0


@pytest.mark.parametrize("name", list(cc.TIERS))
def test_tiers_at_their_boundaries(harness, name):
    for lds_units, tiers in zip((8192, cc.LOW_CAP), cc.TIERS[name]):
        got, info = run(harness, cc.SHAPES[name], lds_units)
        assert tuple(info[1:4]) == tiers and cc.same(got, cc.expected(cc.SHAPES[name]))


def test_the_oracle_and_the_host_function_agree_on_the_small_shapes():
    """what lets expected() switch between them"""
    for name, case in cc.SHAPES.items():
        if 0 < len(case["las"]) <= cc.ORACLE_MAX:
            assert cc.same(cc.host(case), cc.oracle(case)), name


def test_boundary_pairs():
    """the hand-made pairs fall on the side their comment says (the oracle's word, checked here against intent)"""
    las, dropped, used = cc.oracle(cc.SHAPES["boundaries"])
    dis = (las["flags"] & cc.DISABLED != 0).tolist()
    assert dis == [False, True, False, True, False, False, True, False, True, False, False, False, False, False]
    assert dropped.tolist() == [1, 2, 1, 0, 0, 0] and used.all()
    las, dropped, used = cc.oracle(cc.SHAPES["contained"])
    # read 0: the nested unit is not Contained (the scan ended in front of it), so it makes the read ambiguous
    assert (las["flags"] & cc.DISABLED != 0).tolist() == [True, True, True, False, True, True, False, True, False, False, False, True, True,
                                                           False, False, False, False]
    assert dropped.tolist() == [0, 0, 0, 4, 3, 0] and used.tolist() == [0, 1, 1, 1, 1, 1, 1]
    las, dropped, used = cc.oracle(cc.SHAPES["chains"])
    assert not np.any(las["flags"][62:67] & cc.DISABLED) and np.all(las["flags"][258:328] & cc.DISABLED == 0)


def test_every_stage_drops_something_on_the_random_set():
    total, kept = np.zeros(6, dtype=np.int64), 0
    for name, case in cc.RANDOM.items():
        las, dropped, used = cc.host(case)
        total += dropped
        kept += int((las["flags"] & cc.DISABLED == 0).sum())
    assert all(d > 0 for d in total) and kept > 0, (total, kept)


@pytest.mark.parametrize("name,case,words", cc.refusals(), ids=[r[0] for r in cc.refusals()])
def test_refusals_name_the_lowest_index(harness, name, case, words):
    got, info = run(harness, case)
    assert got is None
    kind, idx = words.split(":")[0].split()
    assert (info[4], info[5]) == ((int(idx), -1) if kind == "record" else (-1, int(idx)))
