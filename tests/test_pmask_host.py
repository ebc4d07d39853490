"""The lane code and the host plan of the mask propagation (dentist_amd/csrc/dh_pmask.h) compiled for the CPU and played as
64-lane wavefronts (tests/native/pmask_host.cpp) against the restatement of the contract (tests/propagate_ref.py) on every case
of tests/propagate_cases.py: the plan searches, the chunked trace walk with its carry and batch resume, the edge-word masks of
the painter, the run detection across word and sequence boundaries, with the destination cut into ranges and the records
into launch groups.  Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import propagate_cases as pc
import propagate_ref as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libpmask_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libpmask_host.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.pmask_host.argtypes = [vp, i64, vp, i64, i32, vp, vp, i32, vp, i32, i64, i64, vp, vp, i64, vp]
    L.pmask_host.restype = i64
    return L


def run(L, case, cap_bits=1 << 35, group_raw=1 << 31):
    """((ptr, iv) or None, info) of the harness"""
    las = np.ascontiguousarray(case["las"], dtype=pc.LA_DTYPE)
    tr = np.ascontiguousarray(case["trace"], dtype=np.uint16)
    mp = np.ascontiguousarray(case["mask"][0], dtype=np.int64)
    mi = np.ascontiguousarray(np.concatenate([np.asarray(case["mask"][1], dtype=np.int32).reshape(-1), [0, 0]]), dtype=np.int32)
    ro = np.ascontiguousarray(case["read_off"], dtype=np.int64)
    nreads = len(ro) - 1
    cap = 1 << 18
    ptr, iv, info = np.zeros(nreads + 1, np.int64), np.zeros((cap, 2), np.int32), np.zeros(8, np.int64)
    m = L.pmask_host(las.ctypes.data, len(las), tr.ctypes.data, len(tr), case["tspace"], mp.ctypes.data, mi.ctypes.data, case["ncontigs"],
                     ro.ctypes.data, nreads, cap_bits, group_raw, ptr.ctypes.data, iv.ctypes.data, cap, info.ctypes.data)
    assert m >= -1 and m <= cap, m
    return ((ptr, iv[:m]) if m >= 0 else None), info


def expect(case):
    exp, stats = pr.propagate(case["las"], case["trace"], case["tspace"], case["mask"][0], case["mask"][1], pc.read_len(case))
    return pr.arrays(exp, len(case["read_off"]) - 1), stats


def same(got, exp, info, stats):
    return (np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]) and got[1].dtype == exp[1].dtype
            and info[0] == stats["raw"] and info[1] == stats["hit"] and info[4] == stats["raw"] + stats["empty"])


@pytest.mark.parametrize("name", list(pc.HAND))
def test_hand_worked_cases(host, name):
    case, expected = pc.HAND[name]
    got, info = run(host, case)
    assert pr.as_dict(*got) == expected


@pytest.mark.parametrize("tspace", [100, 126])
def test_trace_shapes(host, tspace):
    case = pc.trace_shapes(tspace)
    exp, stats = expect(case)
    got, info = run(host, case)
    assert same(got, exp, info, stats) and info[2] == 1 and info[3] == 1
    got, info = run(host, case, cap_bits=4096, group_raw=300)  # several destination ranges, several launch groups
    assert same(got, exp, info, stats) and info[2] >= 3 and info[3] >= 3


def test_bitmap_edges(host):
    case, expected = pc.bitmap_edges()
    exp, stats = expect(case)
    for cap_bits in (1 << 35, 512, 1):  # one range, a few reads per range, a range per read
        got, info = run(host, case, cap_bits=cap_bits)
        assert same(got, exp, info, stats) and pr.as_dict(*got) == expected
    assert info[2] == len(case["read_off"]) - 1


def test_long_record_resumes_instead_of_rewalking(host):
    case = pc.long_record()
    exp, stats = expect(case)
    got, info = run(host, case)
    assert same(got, exp, info, stats)
    # 20 000 tiles are 313 chunks; 47 batches of intervals that each started at tile 0 would walk about 47 * 313 / 2
    assert 313 <= info[5] < 2 * 313 + 47


def test_many_into_one_and_wide_destination(host):
    case = pc.many_into_one()
    exp, stats = expect(case)
    got, info = run(host, case, group_raw=30_000)
    assert same(got, exp, info, stats) and info[3] > 3 and list(np.flatnonzero(np.diff(got[0]))) == [0]
    case = pc.wide_destination()
    exp, stats = expect(case)
    got, info = run(host, case, cap_bits=1 << 23)
    assert same(got, exp, info, stats) and info[2] == 6


def test_volume(host):
    case = pc.volume()
    exp, stats = expect(case)
    got, info = run(host, case)
    assert same(got, exp, info, stats) and 0 < info[1] < len(case["las"]) // 4


@pytest.mark.parametrize("name,case,names", pc.refusals(), ids=[r[0] for r in pc.refusals()])
def test_refusals_name_the_record_or_the_contig(host, name, case, names):
    got, info = run(host, case)
    assert got is None
    kind, idx = names.split()
    assert (info[6], info[7]) == ((int(idx), -1) if kind == "record" else (-1, int(idx)))


def test_empty_inputs(host):
    case = dict(pc.HAND["header_example"][0])
    for change in (dict(las=case["las"][:0]), dict(mask=(np.zeros(2, np.int64), np.zeros((0, 2), np.int32))),
                   dict(las=case["las"][:0], read_off=np.zeros(1, np.int64))):
        c = dict(case)
        c.update(change)
        got, info = run(host, c)
        assert not got[0].any() and len(got[1]) == 0
