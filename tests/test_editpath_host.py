"""The lane code of the edit-path kernel (dh_editpath.h: banded bit-parallel fill on 32-bit words, traceback over the three
decision planes, acceptance rule) compiled for the CPU, against oracle/nw.c on random tiles (no GPU needed)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as oz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def host():
    path = os.path.join(ROOT, "tests", "native", "libdh_editpath_host.so")
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libdh_editpath_host.so"], check=True)
    L = ctypes.CDLL(path)
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    L.ep_host_tile.argtypes = [vp, i32, vp, i32, i32, i32, i32, i32, vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    return L


def run_tile(L, ref, qry, diffs, nw, stride=1, lane=0):
    r = np.concatenate([ref, np.full(16, 4, np.uint8)]).astype(np.uint8)  # the DBs' padding
    q = np.concatenate([qry, np.full(16, 4, np.uint8)]).astype(np.uint8)
    ops = np.zeros(len(ref) + len(qry) + 8, np.uint8)
    nops, score = ctypes.c_int32(0), ctypes.c_int32(0)
    st = L.ep_host_tile(r.ctypes.data, len(ref), q.ctypes.data, len(qry), diffs, nw, stride, lane, ops.ctypes.data,
                        ctypes.byref(nops), ctypes.byref(score))
    return st, ops[:nops.value].copy(), score.value


def oracle_ops(ref, qry):
    """oracle/nw.c's path with the substitutions split into match (0) and mismatch (3)"""
    score, ops = oz.nw(ref, qry, 1, False)
    out, i, j = ops.copy(), 0, 0
    for k, op in enumerate(ops):
        if op == 0:
            out[k] = 0 if ref[i] == qry[j] else 3
            i, j = i + 1, j + 1
        elif op == 1:
            i += 1
        else:
            j += 1
    return score, out


def mutate(rng, ref, err):
    out = []
    for b in ref:
        x = rng.random()
        if x < err / 3:
            continue
        if x < 2 * err / 3:
            out.append((b + 1 + rng.integers(0, 3)) % 4)
            continue
        out.append(b)
        if x < err:
            out.append(rng.integers(0, 4))
    return np.asarray(out, dtype=np.uint8)


def tiles(seed, n):
    rng = np.random.default_rng(seed)
    for _ in range(n):
        rl = int(rng.choice([0, 1, 2, 7, 31, 32, 33, 63, 64, 65, 100, 126, 250, int(rng.integers(1, 251))]))
        ref = rng.integers(0, 4, rl).astype(np.uint8)
        if rng.random() < 0.15:  # low complexity: many equal scores, the tie-breaking rule decides
            ref = (ref & 1).astype(np.uint8)
        qry = mutate(rng, ref, float(rng.choice([0.0, 0.02, 0.1, 0.2, 0.3])))
        if rng.random() < 0.1 and len(qry):
            qry[rng.integers(0, len(qry))] = 4  # an N matches nothing but another N
        yield ref, qry


@pytest.mark.parametrize("nw", [1, 2])
def test_accepted_tiles_equal_the_oracle_and_honest_traces_are_accepted(host, nw):
    """With diffs >= the true score (an honest trace) every tile that fits the class is accepted with the oracle's ops and
    score; with diffs understated the tile is rejected or, if accepted, still exact (the acceptance rule is sound)."""
    accepted = understated = two_word = 0
    for k, (ref, qry) in enumerate(tiles(100 + nw, 700)):
        score, ops = oracle_ops(ref, qry)
        for diffs in (score, score + 3, 30 * nw, max(score - 1, 0), score // 2, 0):
            st, got, gs = run_tile(host, ref, qry, diffs, nw, stride=1 + k % 3, lane=k % (1 + k % 3))
            assert st != 3, "a store outside the lane's own words"
            if st == 2:
                band = diffs + 1
                assert band > 32 * nw - 1 or abs(len(ref) - len(qry)) >= band
                continue
            if diffs >= score:
                assert st == 0, (len(ref), len(qry), score, diffs)
            else:
                understated += 1
                assert st == 1, "a path of cost <= diffs < true score cannot exist"
            if st == 0:
                accepted += 1
                two_word += diffs + 1 > 31
                assert gs == score and np.array_equal(got, ops), (len(ref), len(qry), score, diffs)
    assert accepted > 500 and understated > 200
    assert (two_word > 0) == (nw == 2)
