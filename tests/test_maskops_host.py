"""The lane code and the host plan of the mask algebra (dentist_amd/csrc/dh_maskops.h) compiled for the CPU and played as lanes,
64-lane wavefronts and whole workgroup tiles (tests/native/maskops_host.cpp) against the contract (tests/maskops_ref.py) on every
case of tests/maskops_cases.py: at the default tile and at the smallest, in one launch group and in many; the sort alone on odd
key counts; the key layout; the refusals.  Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import maskops_cases as mc
import maskops_ref as mr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = 2048


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libmaskops_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libmaskops_host.so"))
    vp, i32, i64, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
    L.maskops_host.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp, i32, i64, vp, vp, i64, vp, vp, i32]
    L.maskops_host.restype = i64
    L.maskops_tandem_host.argtypes = [vp, i64, vp, i32, i32, i32, i32, vp, vp, i64, vp, vp, i32]
    L.maskops_tandem_host.restype = i64
    L.maskops_rx_sort_host.argtypes = [vp, i64, i32, i32]
    L.maskops_rx_sort_host.restype = None
    L.maskops_key_host.argtypes = [u64, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.maskops_key_host.restype = None
    return L


def run(L, c, tile=TILE, chunk_bytes=1 << 30):
    """(triples or None, info, message)"""
    masks = [(np.ascontiguousarray(m[0], np.int64), np.ascontiguousarray(np.concatenate([m[1].reshape(-1), [0, 0]]), np.int32)) for m in c["masks"]]
    sub = c["subtract"]
    sub = None if sub is None else (np.ascontiguousarray(sub[0], np.int64), np.ascontiguousarray(np.concatenate([sub[1].reshape(-1), [0, 0]]), np.int32))
    co = np.ascontiguousarray(c["contig_off"], np.int64)
    nc = len(co) - 1
    ptrs = (ctypes.c_void_p * len(masks))(*[m[0].ctypes.data for m in masks])
    ivs = (ctypes.c_void_p * len(masks))(*[m[1].ctypes.data for m in masks])
    opts = np.asarray([c["min_count"], c["min_gap"], c["min_interval"], 0], np.int32)
    cap = sum(len(m[1]) // 2 for m in masks) + 1
    out_ptr, out_iv, info = np.zeros(nc + 1, np.int64), np.zeros(2 * cap, np.int32), np.zeros(3, np.int64)
    msg = ctypes.create_string_buffer(256)
    n = L.maskops_host(ptrs, ivs, len(masks), sub[0].ctypes.data if sub else None, sub[1].ctypes.data if sub else None, co.ctypes.data, nc,
                       opts.ctypes.data, tile, chunk_bytes, out_ptr.ctypes.data, out_iv.ctypes.data, cap, info.ctypes.data, msg, 256)
    assert n >= -1, n
    if n < 0:
        return None, info, msg.value.decode()
    return mc.triples(out_ptr, out_iv[:2 * n]), info, ""


@pytest.mark.parametrize("name", list(mc.ALL))
def test_every_case_at_both_tiles_and_in_many_groups(harness, name):
    c, exp = mc.ALL[name], mc.expected_of(name)
    for tile, chunk in ((TILE, 1 << 30), (mc.TILE_MIN, 1 << 30), (TILE, 1)):
        got, info, _ = run(harness, c, tile, chunk)
        assert got == exp, (name, tile, chunk)
        assert info[0] == 2 * mr.count_nonempty(c["masks"], c["subtract"])
        assert info[2] == (mc.groups_of(c) if chunk == 1 else min(1, mc.groups_of(c)))


def test_the_digits_in_use_decide_the_passes(harness):
    passes = {n: int(run(harness, mc.ALL[n])[1][1]) for n in ("nothing", "one_interval", "tile", "longest_contig", "many_contigs", "three_masks_min_2")}
    assert passes == {"nothing": 0, "one_interval": 1, "tile": 2, "longest_contig": 5, "many_contigs": 4, "three_masks_min_2": 2}


@pytest.mark.parametrize("tile", [256, 512, 2048])
@pytest.mark.parametrize("n", ["1", "tile - 1", "tile", "tile + 1", "3 * tile + 5"])
@pytest.mark.parametrize("bits,distinct", [(8, 3), (8, 256), (13, 2), (21, 1 << 21), (40, 1 << 40), (64, 1 << 62)])
def test_the_sort_is_stable_on_any_count(harness, tile, n, bits, distinct):
    n = eval(n, {"tile": tile})
    rng = np.random.default_rng(n + bits)
    low = rng.integers(0, distinct, n, dtype=np.uint64) * np.uint64(max(1, ((1 << bits) - 1) // max(distinct - 1, 1)) if distinct <= 256 else 1)
    low &= np.uint64((1 << bits) - 1)
    top = 8 * ((bits + 7) // 8)   # a pass sorts a whole digit: the input place goes above the last digit in use
    keys = low if top == 64 else low | (np.arange(n, dtype=np.uint64)[::-1] << np.uint64(top))
    exp = keys[np.argsort(low, kind="stable")]
    got = keys.copy()
    harness.maskops_rx_sort_host(got.ctypes.data, n, bits, tile)
    assert got.tobytes() == exp.tobytes()


def test_key_layout(harness):
    key, unit, dadd, dsub = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32()
    pos = ctypes.c_int32()
    for u, p, s, e, pb in ((0, 0, 0, 0, 1), (70000, 49, 1, 1, 6), (1, 2 ** 31 - 1, 0, 1, 31), (2 ** 31 - 1, 2 ** 31 - 1, 1, 0, 31), (5, 0, 1, 1, 3)):
        harness.maskops_key_host(u, p, s, e, pb, *[ctypes.byref(x) for x in (key, unit, pos, dadd, dsub)])
        assert key.value == (u << (pb + 2)) | (p << 2) | (s << 1) | e and (unit.value, pos.value) == (u, p)
        assert (dadd.value, dsub.value) == ((0, 0xFFFFFFFF if e else 1) if s else (0xFFFFFFFF if e else 1, 0))


def tandem(L, las, read_off, first, min_len, tile=TILE):
    las = np.ascontiguousarray(las)
    ro = np.ascontiguousarray(read_off, np.int64)
    nr = len(ro) - 1
    out_ptr, out_iv, info = np.zeros(nr + 1, np.int64), np.zeros(2 * (len(las) + 1), np.int32), np.zeros(3, np.int64)
    msg = ctypes.create_string_buffer(256)
    n = L.maskops_tandem_host(las.ctypes.data, len(las), ro.ctypes.data, nr, first, min_len, tile, out_ptr.ctypes.data, out_iv.ctypes.data,
                              len(las) + 1, info.ctypes.data, msg, 256)
    return (mc.triples(out_ptr, out_iv[:2 * n]) if n >= 0 else None), info, msg.value.decode()


@pytest.mark.parametrize("first", [0, 5])
def test_tandem_rule(harness, first):
    las, read_off, first, min_len = mc.tandem_case(first)
    got, info, _ = tandem(harness, las, read_off, first, min_len)
    assert got == mr.tandem(las, read_off, first, min_len) == [(0, 100, 1300), (2, 50, 1100), (3, 0, 2000)] and list(info) == [10, 2, 1]
    bad = las.copy()
    bad[3]["aepos"] = 1601
    assert tandem(harness, bad, read_off, first, min_len)[2] == "record 3: end behind the read's end"
    bad[3]["aread"] = bad[3]["bread"] = first + 4
    assert tandem(harness, bad, read_off, first, min_len)[2] == "record 3: aread outside the reads"


@pytest.mark.parametrize("name,case,words", mc.refusals(), ids=[r[0] for r in mc.refusals()])
def test_refusals_name_the_lowest_index(harness, name, case, words):
    got, _, msg = run(harness, case)
    assert got is None and words in msg, msg
