"""The plan lane code of the chain padder (dentist_amd/csrc/dh_chainpad.h) compiled for the CPU (tests/native/chainpad_host.cpp)
against the restatement of the contract (tests/chainpad_ref.py): the segment list and the status of every chain of the
constructed cases (tests/chainpad_cases.py) and of 200 random cut sets from a seeded generator.  Every comparison is
equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chainpad_cases as cc
import chainpad_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REC = np.dtype([("aoff", "<i8"), ("boff", "<i8"), ("toff", "<i8"), ("abpos", "<i4"), ("aepos", "<i4"), ("bbpos", "<i4"),
                ("bepos", "<i4"), ("nt", "<i4"), ("comp", "<i4")])


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libchainpad_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libchainpad_host.so"))
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32
    L.chainpad_host_plan.argtypes = [vp, i64, vp, i32, vp, i64, vp]
    L.chainpad_host_plan.restype = i32
    L.chainpad_host_generated_op.argtypes = [vp, vp, i32, i32, i32]
    L.chainpad_host_generated_op.restype = i32
    return L


def plan(L, las, trace, ts):
    """(status, segments in the restatement's form) of one chain from the lane code"""
    recs = np.zeros(len(las), REC)
    for f in ("toff", "abpos", "aepos", "bbpos", "bepos"):
        recs[f] = las[f]
    recs["nt"] = las["tlen"] // 2
    recs["comp"] = las["flags"] & 1
    tr = np.ascontiguousarray(trace, np.uint16)
    n = ctypes.c_int64(0)
    st = L.chainpad_host_plan(recs.ctypes.data, len(recs), tr.ctypes.data, ts, None, 0, ctypes.byref(n))
    rows = np.zeros((max(n.value, 1), 6), np.int32)
    n2 = ctypes.c_int64(0)
    assert L.chainpad_host_plan(recs.ctypes.data, len(recs), tr.ctypes.data, ts, rows.ctypes.data, n.value, ctypes.byref(n2)) == st
    assert n2.value == n.value
    segs = [("t", int(r[1]), int(r[2]), int(r[3])) if r[0] == 0 else ("f", *[int(x) for x in r[1:]]) for r in rows[:n.value]]
    return st, segs


def test_record_layout_is_the_headers():
    hdr = open(os.path.join(ROOT, "dentist_amd", "csrc", "dh_chainpad.h")).read()
    body = hdr[hdr.index("struct CpRec {"):hdr.index("struct CpFill {")]
    names = [x.strip() for ln in body.splitlines()[1:] if ";" in ln and not ln.startswith("}") for x in ln.split(";")[0].split(None, 1)[1].split(",")]
    assert names == list(REC.names) and REC.itemsize == 48


@pytest.mark.parametrize("name", list(cc.cases().keys()))
def test_constructed_cases(host, name):
    case = cc.cases()[name]
    off = cr.chains_of(case["las"])
    for i in range(len(off) - 1):
        ch = case["las"][off[i]:off[i + 1]]
        assert plan(host, ch, case["trace"], case["ts"]) == cr.segments(ch, case["trace"], case["ts"])


def test_random_cut_sets(host):
    seen = set()
    for seed in range(200):
        case = cc.random_case(seed)
        got = plan(host, case["las"], case["trace"], case["ts"])
        assert got == cr.segments(case["las"], case["trace"], case["ts"]), f"seed {seed}"
        seen.add(got[0])
    assert seen == {cr.OK, cr.NESTED}, "the generator no longer reaches both outcomes"


def test_generated_filler(host):
    rng = np.random.default_rng(5)
    for la, lb in [(0, 7), (7, 0), (5, 5), (3, 11), (11, 3), (100, 31)]:
        a, b = rng.integers(0, 4, la).astype(np.uint8), rng.integers(0, 4, lb).astype(np.uint8)
        got = [host.chainpad_host_generated_op(a.ctypes.data, b.ctypes.data, la, lb, p) for p in range(max(la, lb))]
        exp = cr.faked(a, b) if la and lb else cr.filler_ops(a, b)[0]
        assert got == exp.tolist()
