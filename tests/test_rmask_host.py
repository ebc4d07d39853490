"""The lane code and the host plan of the repeat mask (dentist_amd/csrc/dh_rmask.h) compiled for the CPU and played as 64-lane
wavefronts and workgroups (tests/native/rmask_host.cpp) against the contract (tests/repeat_ref.py over oracle/maskcov.py) on every
case of tests/repeat_cases.py: at the default LDS cap and at the lowest, in one launch group and in many.  Every comparison is
equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import repeat_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/librmask_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "librmask_host.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.rmask_host.argtypes = [vp, i64, vp, i32, vp, i32, vp, i32, i64, vp, vp, i64, vp, vp, i32]
    L.rmask_host.restype = i64
    return L


def run(L, case, lds_events=rc.CAP, chunk_bytes=1 << 30):
    """(dict of triples per mask or None, info, message)"""
    las = np.ascontiguousarray(case["las"], dtype=rc.LA)
    co, ro = np.ascontiguousarray(case["contig_off"], dtype=np.int64), np.ascontiguousarray(case["read_off"], dtype=np.int64)
    nc = len(co) - 1
    imp = case["improper"]
    opts = np.asarray([case["lower"], case["upper"], imp[0] if imp else 0, imp[1] if imp else 0, case["allowance"], 1 if imp else 0], dtype=np.int32)
    cap = 2 * (len(las) + nc) + 4
    ptr3, iv3, info = np.zeros(3 * (nc + 1), np.int64), np.zeros(3 * 2 * cap, np.int32), np.zeros(8, np.int64)
    msg = ctypes.create_string_buffer(256)
    rcode = L.rmask_host(las.ctypes.data if len(las) else None, len(las), co.ctypes.data, nc, ro.ctypes.data, len(ro) - 1, opts.ctypes.data,
                         lds_events, chunk_bytes, ptr3.ctypes.data, iv3.ctypes.data, cap, info.ctypes.data, msg, 256)
    assert rcode in (0, -1), rcode
    if rcode < 0:
        return None, info, msg.value.decode()
    out = {}
    for k, which in enumerate(("mask", "all", "improper")):
        ptr = ptr3[k * (nc + 1):(k + 1) * (nc + 1)]
        out[which] = rc.triples((ptr, iv3[2 * k * cap:2 * k * cap + 2 * int(ptr[-1])]))
    return out, info, ""


@pytest.mark.parametrize("name", list(rc.ALL))
def test_every_case_at_both_caps_and_in_many_groups(harness, name):
    case, exp = rc.ALL[name], rc.expected_of(name)
    for lds_events, chunk in ((rc.CAP, 1 << 30), (rc.LOW_CAP, 1 << 30), (rc.CAP, 1)):
        got, info, _ = run(harness, case, lds_events, chunk)
        for which in ("mask", "all", "improper"):
            assert got[which] == exp[which], (name, which, lds_events, chunk)
        assert (info[0], info[1]) == (exp["units"], exp["improper_units"])
        assert info[2:6].sum() == len(case["contig_off"]) - 1
        assert info[6] == (len(case["contig_off"]) - 1 if chunk == 1 else 1)


def test_every_tier_runs(harness):
    _, info, _ = run(harness, rc.ALL["edges"], rc.LOW_CAP)
    assert list(info[2:6]) == [1, 3, 3, 1]            # 0 | 2, 62, 64 | 66, cap - 2, cap | cap + 2 events
    _, info, _ = run(harness, rc.ALL["edges"], rc.CAP)
    assert list(info[2:6]) == [1, 3, 4, 0]
    _, info, _ = run(harness, rc.ALL["above_default_cap"], rc.CAP)
    assert list(info[2:6]) == [1, 1, 0, 1]


def test_reference_vector_is_the_reference_result(harness):
    got, _, _ = run(harness, rc.reference_vector())
    assert got["all"] == got["mask"] == rc.REF_MASK_3_5 and got["improper"] == []


def test_no_records_give_three_empty_masks(harness):
    got, info, _ = run(harness, rc.case([10, 20], [], 1, 2))
    assert got == {"mask": [], "all": [], "improper": []} and info[6] == 0


@pytest.mark.parametrize("name,case,words", rc.refusals(), ids=[r[0] for r in rc.refusals()])
def test_refusals_name_the_lowest_index(harness, name, case, words):
    got, _, msg = run(harness, case)
    assert got is None and words in msg, msg
