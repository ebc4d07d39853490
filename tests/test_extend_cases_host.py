"""The DH-2 cases of tests/extend_cases.py through the lane state machine of dentist_amd/csrc/dh_tile.h compiled for the
CPU (tests/native/tile_host.cpp: the code k_tile runs, one lane after the other) against oz.extend_candidates: every record
in slot order (symmetric cases: as a sorted set, their slots are candidate-indexed), every trace value, both counters, and
the transposed file where the case asks for it.  No GPU.  What the device adds around this code -- the lock-step column loop,
the scan, work units, compaction, per-chunk copies -- is tests/test_parity_extendstage_gpu.py's.

Every DH-2 case is expressible here, none is skipped: the harness takes the candidates as they are, knows the symmetric and
the tandem mode, the transposed file and (dh_tile_host_align3) the pflags of a symmetric call, so the record-wanted branches
of the lane code run here on the two pflags cases -- which the GPU module has to leave out, as the binding cannot set pflags
on a device DB."""
import ctypes

import numpy as np
import pytest

import extend_cases as ec
from helpers import la_rows
from test_tile_host import DHCAND, host_lib  # noqa: F401

CASES = [c for c in ec.all_cases() if c["kw"]["algo"] == 1]


def run_host(L, c):
    A, B, o = c["A"], c["B"], ec.oracle_opts(c["kw"])
    dc = np.zeros(c["cand"].shape, dtype=DHCAND)
    for f in ("score", "aseq", "apos", "bpos"):
        dc[f] = c["cand"][f]
    dc = np.ascontiguousarray(dc)
    maxlen = int(max((A.off[1:] - A.off[:-1]).max(), (B.off[1:] - B.off[:-1]).max()))
    nbmax = maxlen // o.tspace + 3
    nslot = 2 * B.n * max(o.max_la, 2 * o.max_cand)
    cap = int(nslot * 2 * (2 * nbmax + 2))
    las, las2 = (np.zeros(nslot, dtype=ec.oz.LA_DTYPE) for _ in range(2))
    trace, trace2 = (np.zeros(cap, dtype=np.uint16) for _ in range(2))
    counters = np.zeros(2, dtype=np.uint64)
    n2 = ctypes.c_long(0)
    L.dh_tile_host_align3.restype = ctypes.c_long
    L.dh_tile_host_align3.argtypes = L.dh_tile_host_align.argtypes + [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_long),
                                                                      ctypes.c_void_p]
    pf = A.pflags.ctypes.data if c["pflags"] else None
    tr = c["transposed"]
    n = L.dh_tile_host_align3(A.bases.ctypes.data, A.off.ctypes.data, A.n, B.bases.ctypes.data, B.off.ctypes.data, B.n,
                              ctypes.byref(o), dc.ctypes.data, c["ncand"].ctypes.data, nbmax, las.ctypes.data, trace.ctypes.data,
                              cap, counters.ctypes.data, las2.ctypes.data if tr else None, trace2.ctypes.data if tr else None,
                              ctypes.byref(n2) if tr else None, pf)
    assert n >= 0, n
    return las[:n], trace, counters, las2[:n2.value], trace2


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_lane_code_equals_oracle_on_planted_candidates(host_lib, c):  # noqa: F811
    exp = ec.oracle(c)
    las, trace, counters, las2, trace2 = run_host(host_lib, c)
    got, want = la_rows(las, trace), la_rows(exp.las, exp.trace)
    if c["kw"].get("skip_self", 0) == 2:
        got, want = sorted(got), sorted(want)
    assert len(got) == len(want), f"{c['name']}: {len(got)} records, oracle {len(want)}"
    for i, (x, y) in enumerate(zip(got, want)):
        assert x == y, f"{c['name']}: record {i} differs\n got {x}\n exp {y}"
    assert (int(counters[1]), int(counters[0])) == (int(exp.stats[2]), int(exp.stats[3])), f"{c['name']}: attempts, cells"
    if c["transposed"]:
        assert la_rows(las2, trace2) == la_rows(exp.las2, exp.trace2), f"{c['name']}: the transposed file"
