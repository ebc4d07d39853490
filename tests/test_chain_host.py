"""The lane code and the host plan of the chaining (dentist_amd/csrc/dh_chain.h) compiled for the CPU and played as 64-lane
wavefronts (tests/native/chain_host.cpp) against the restatement of the contract (tests/chain_ref.py) on the shapes of
tests/chain_cases.py: every array of the contract, over all four tiers (the LDS limit forced to 128, so that 129-200 nodes
take the global tier).  Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chain_cases as cc
import chain_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Opts(ctypes.Structure):
    _fields_ = [("max_indel", ctypes.c_int32), ("max_chain_gap", ctypes.c_int32), ("min_score", ctypes.c_int32), ("pad_", ctypes.c_int32),
                ("max_relative_overlap", ctypes.c_double), ("min_relative_score", ctypes.c_double)]


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libchain_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libchain_host.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.chain_host.argtypes = [vp, i64, vp, i64, i64, vp, vp, i64, vp, vp, i64, vp]
    L.chain_host.restype = i64
    return L


def chain(L, las, lds_cap=1536, chunk_words=1 << 28, **opts):
    """((off, score, src_index, flags), info) of the harness"""
    o = dict(cr.DEFAULTS)
    o.update(opts)
    co = Opts(o["max_indel"], o["max_chain_gap"], o["min_score"], 0, o["max_relative_overlap"], o["min_relative_score"])
    arr = np.ascontiguousarray(las, dtype=cc.LA_DTYPE)
    cap = 1 << 16
    off, score = np.zeros(cap + 1, np.int64), np.zeros(cap, np.int32)
    src, flags = np.zeros(cap, np.int64), np.zeros(cap, np.uint32)
    info = np.zeros(8, np.int64)
    n = L.chain_host(arr.ctypes.data, len(arr), ctypes.addressof(co), lds_cap, chunk_words, off.ctypes.data, score.ctypes.data, cap,
                     src.ctypes.data, flags.ctypes.data, cap, info.ctypes.data)
    if n < 0:
        return None, info
    return (off[:n + 1], score[:n], src[:info[0]], flags[:info[0]]), info


def same(got, exp):
    return all(np.array_equal(g, e) and g.dtype == e.dtype for g, e in zip(got, exp))


def test_layouts_are_the_headers():
    assert ctypes.sizeof(Opts) == 32
    hdr = open(os.path.join(ROOT, "include", "dentist_hip.h")).read()
    body = hdr[hdr.index("typedef struct dh_chain_opts {"):hdr.index("} dh_chain_opts;")]
    assert [n for n, _ in Opts._fields_] == [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln]


@pytest.mark.parametrize("name", list(cc.HAND))
def test_hand_worked_cases(host, name):
    las, opts, expected = cc.HAND[name]
    got, info = chain(host, las, **opts)
    assert same(got, cr.arrays(expected))


@pytest.mark.parametrize("rel,min_score", cc.OPTION_SETS)
def test_random_shapes_equal_the_restatement_in_every_tier(host, rel, min_score):
    las = cc.random_case(seed=11)
    opts = cc.opts_of(rel, min_score)
    exp = cr.arrays(cr.chain(las, **opts))
    assert len(exp[1]) >= 10
    got, info = chain(host, las, **opts)
    assert same(got, exp)
    assert list(info[2:6]) == [2, 10, 4, 0]  # pairs of 1 | 2, 3, 9, 63, 64 | 65, 200 | none, two of each
    small, info = chain(host, las, lds_cap=128, chunk_words=2500, **opts)
    assert same(small, exp)
    assert list(info[2:6]) == [2, 10, 2, 2] and info[1] == 2 and info[7] == 2  # 200 nodes: the global tier, a launch each


def test_sizes_around_the_tier_limits(host):
    las = cc.random_case(seed=5, sizes=(63, 64, 65, 127, 128, 129), reps=1)
    exp = cr.arrays(cr.chain(las, min_relative_score=0.0))
    for cap in (1536, 128, 64):
        got, info = chain(host, las, lds_cap=cap, min_relative_score=0.0)
        assert same(got, exp), cap
        assert info[1] == {1536: 0, 128: 1, 64: 4}[cap]


def test_many_single_pairs_and_one_larger(host):
    rng = np.random.default_rng(7)
    parts = [cc.make_pair(rng, i // 50, i % 50, 1) for i in range(17000)] + [cc.make_pair(rng, 1000, 0, 65)]
    las = np.concatenate(parts)
    assert len(las) > (1 << 15)  # more than one chunk of the plan
    got, info = chain(host, las, min_score=1500)
    assert same(got, cr.arrays(cr.chain(las, min_score=1500)))
    assert info[2] == 17000 and info[4] == 1 and 0 < len(got[1]) < 17001  # some single records score below 1500


def test_unordered_input_names_the_record(host):
    las = cc.random_case(seed=3, sizes=(3, 9), reps=1)
    bad = las.copy()
    bad[-1]["aread"] = int(bad[0]["aread"]) - 1
    bad[-1]["flags"] &= ~np.uint32(cc.DISABLED)
    got, info = chain(host, bad)
    assert got is None and info[6] == len(bad) - 1
    off = bad.copy()
    off[-1]["flags"] |= np.uint32(cc.DISABLED)  # a disabled record is not looked at
    assert chain(host, off)[0] is not None


def test_empty_and_all_disabled(host):
    got, _ = chain(host, np.zeros(0, dtype=cc.LA_DTYPE))
    assert same(got, cr.arrays([]))
    las = cc.random_case(seed=3, sizes=(3,), reps=1)
    las["flags"] |= np.uint32(cc.DISABLED)
    got, _ = chain(host, las)
    assert same(got, cr.arrays([]))
