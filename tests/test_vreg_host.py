"""The lane code and the host plan of the region validation (dentist_amd/csrc/dh_vreg.h) compiled for the CPU and played as
workgroups of four 64-lane wavefronts (tests/native/vreg_host.cpp) against the restatement of the contract
(tests/validate_ref.py) on every case of tests/validate_cases.py: the candidate searches, the pair windows, the ranking of the
spanning records, the chunked scans with their carries, both tiers of the difference array and the launch groups.  The harness
claims the slots of a region's lists in descending record order.  Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import validate_cases as vc
import validate_ref as vr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGION_DTYPE = np.dtype([("contig", "<i4"), ("begin", "<i4"), ("end", "<i4")])


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libvreg_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libvreg_host.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.vreg_host.argtypes = [vp, i64, vp, i32, vp, i32, i32, i32, i32, i32, i64, i64, vp, vp, i64, vp, vp, i64, vp, vp, i64, vp]
    L.vreg_host.restype = i64
    return L


def run(L, case, lds_windows=8192, slab_mb=1024):
    """(a dict of the result arrays or None, info) of the harness"""
    las = np.ascontiguousarray(case["las"], dtype=vc.LA_DTYPE)
    co = np.ascontiguousarray(case["contig_off"], dtype=np.int64)
    rg = np.array(case["regions"], dtype=np.int32).reshape(-1, 3).view(REGION_DTYPE).reshape(-1).copy()
    nreg, ncontigs, cap = len(rg), len(co) - 1, 1 << 17
    rep = np.zeros(nreg, dtype=vr.REPORT_DTYPE)
    weak, ids, miv = np.zeros((cap, 3), np.int32), np.zeros(cap, np.int32), np.zeros((cap, 2), np.int32)
    off, mptr, info = np.zeros(nreg + 1, np.int64), np.zeros(ncontigs + 1, np.int64), np.zeros(8, np.int64)
    m = L.vreg_host(las.ctypes.data, len(las), co.ctypes.data, ncontigs, rg.ctypes.data, nreg, case["context"], case["window"], case["min_cov"],
                    case["min_span"], lds_windows, slab_mb << 20, rep.ctypes.data, weak.ctypes.data, cap, off.ctypes.data, ids.ctypes.data,
                    cap, mptr.ctypes.data, miv.ctypes.data, cap, info.ctypes.data)
    assert -1 <= m <= cap and off[nreg] <= cap and info[3] <= cap, (m, info)
    if m < 0:
        return None, info
    return dict(reports=rep, weak=weak[:m], span_off=off, span_ids=ids[:off[nreg]], mask=(mptr, miv[:info[3]])), info


@pytest.mark.parametrize("name", list(vc.HAND))
def test_hand_worked_cases(host, name):
    case, expected = vc.HAND[name]
    got, info = run(host, case)
    rep = got["reports"][0]
    assert got["span_ids"].tolist() == expected["span"] and [tuple(x) for x in got["weak"].tolist()] == expected["weak"]
    assert (rep["num_spanning_reads"], rep["weak_bp"], bool(rep["is_valid"])) == (len(expected["span"]), expected["weak_bp"], expected["valid"])


@pytest.mark.parametrize("name", list(vc.SHAPES))
def test_shapes(host, name):
    case = vc.SHAPES[name]
    exp = vr.validate(case)
    for lds_windows in (8192, 2):  # the LDS tier, and every region with a window in the global tier
        got, info = run(host, case, lds_windows=lds_windows)
        assert vr.same(got, exp) and info[0] == exp["pairs"]


@pytest.mark.parametrize("k", [-1, 0, 1])
def test_tier_boundary(host, k):
    case = vc.SHAPES[f"tier_cap{k:+d}"]
    got, info = run(host, case, lds_windows=vc.LOW_CAP)
    assert vr.same(got, vr.validate(case)) and info[1] == (1 if k > 0 else 0)


def test_launch_groups(host):
    case = vc.group_case()
    exp = vr.validate(case)
    got, info = run(host, case)
    assert vr.same(got, exp) and info[2] == 1 and info[1] == 4
    got, info = run(host, case, slab_mb=1)
    assert vr.same(got, exp) and info[2] == 4
    case = vc.SHAPES["regions_shuffled"]
    got, info = run(host, case, slab_mb=0)  # no budget at all: a group per region
    assert vr.same(got, vr.validate(case)) and info[2] == len(case["regions"])


def test_many_regions_on_one_contig(host):
    """expectation: the host function (see tests/test_validate_ref.py::test_many_regions_on_one_contig_by_the_host_function)"""
    case = vc.many_regions()
    exp = vr.from_host(case)
    got, info = run(host, case)
    assert vr.same(got, exp) and info[0] == exp["pairs"]


PLAN_REFUSALS = [r for r in vc.refusals() if r[2] != "bad argument"]  # (those are the driver's, not the plan's)


@pytest.mark.parametrize("name,case,words", PLAN_REFUSALS, ids=[r[0] for r in PLAN_REFUSALS])
def test_refusals_name_the_lowest_index(host, name, case, words):
    got, info = run(host, case)
    assert got is None
    kind, idx = words.split(":")[0].split()
    assert (info[4], info[5]) == ((int(idx), -1) if kind == "record" else (-1, int(idx)))
