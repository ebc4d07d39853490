"""The lane code of k_trace_transpose (dh_editpath.h: word loads in the order of the transposed path, slice counts, the walk
to the grid points) compiled for the CPU and played as a wavefront (tests/native/transpose_host.cpp), against the plain
restatement in tests/transpose_ref.py on the hand vectors and on random paths (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import transpose_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "tests", "native", "libdh_transpose_host.so")
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libdh_transpose_host.so"], check=True)
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.tr_host_record.argtypes = [vp, i32, i32, i32, i32, i32, vp, i32]
    L.tr_host_record.restype = i32
    return L


def host_tiles(L, ops, comp, a0, a1, ts, lead=0):
    buf = np.concatenate([np.full(lead, 0x77, np.uint8), np.asarray(ops, dtype=np.uint8)])  # (any alignment of the first op)
    pairs = np.zeros((a1 - a0) // ts + 2, np.uint32)
    n = L.tr_host_record(buf.ctypes.data + lead, len(ops), comp, a0, a1, ts, pairs.ctypes.data, len(pairs))
    assert n > 0, n
    return [(int(p) & 0xFFFF, int(p) >> 16) for p in pairs[:n]]


def test_hand_vectors(host):
    assert host_tiles(host, [0, 0, 3, 1, 0, 2, 0, 0, 2, 0, 0], 0, 3, 13, 4) == [(0, 1), (3, 4), (1, 3), (0, 1)]
    assert host_tiles(host, [0, 3, 0, 1, 0, 0, 0], 1, 5, 11, 4) == [(0, 3), (2, 4)]
    assert host_tiles(host, [0, 3, 0, 1, 0, 0, 0], 0, 5, 11, 4) == [(1, 3), (1, 4)]


@pytest.mark.parametrize("comp", [0, 1])
def test_random_paths_against_the_restatement(host, comp):
    rng = np.random.default_rng(17 + comp)
    for it in range(300):
        nops = int(rng.integers(4000, 13000)) if it % 10 == 0 else int(rng.integers(1, 70 if it % 7 == 0 else 1500))
        ts = int(rng.integers(1, 251)) if it % 3 == 0 else (100 if it % 3 == 1 else int(rng.integers(4, 12)))
        p = [[.85, .05, .05, .05], [.25, .25, .25, .25], [.3, .5, .15, .05]][it % 3]
        ops = rng.choice(4, nops, p=p).astype(np.uint8)
        # the restatement takes the SOURCE record: its B interval is the transposed record's A' interval
        if np.all(ops == 1):
            ops[0] = 0
        nb = int(np.count_nonzero(ops != 1))  # B bases of the source = A' bases
        na = int(np.count_nonzero(ops != 2))
        b0 = int(rng.integers(0, 1000))
        if it % 5 == 0:
            b0 -= b0 % ts
        alen, blen = 5000 + na, b0 + nb + int(rng.integers(0, 50))
        if comp:  # source B coordinates in the reverse-complement frame
            bbpos, bepos = blen - (b0 + nb), blen - b0
        else:
            bbpos, bepos = b0, b0 + nb
        ab, ae, _, _, _, tiles, _ = tr.transpose_record(7, 7 + na, bbpos, bepos, comp, ops, ts, alen, blen)
        assert (ab, ae) == (b0, b0 + nb)
        assert host_tiles(host, ops, comp, ab, ae, ts, lead=it % 9) == tiles, (it, nops, ts)
