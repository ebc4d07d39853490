"""The lane code of the sparse packed read loader (dentist_amd/csrc/dh_bpsload.h) compiled for the CPU and played as 64-lane
wavefronts over chunks of reads (tests/native/bpsload_host.cpp) against a three-line numpy unpack.  The reads have the lengths
at which a 16-byte window can go wrong, stand in an order in which every destination residue mod 16 is the start of a read,
and carry set padding bits behind their last base.  Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 1000]


def ordered_lengths():
    """LENGTHS in an order whose read starts cover every residue mod 16 (the first one found by a seeded shuffle)"""
    rng = np.random.default_rng(16)
    for _ in range(10000):
        order = [int(x) for x in rng.permutation(LENGTHS)]
        starts = np.concatenate([[0], np.cumsum(order)[:-1]])
        if len(set(int(s) % 16 for s in starts)) == 16:
            return order
    raise AssertionError("no order of the lengths covers every residue")


def make_reads(order, seed=5):
    """(bps bytes with the padding bits set, boff, the expected bases)"""
    rng = np.random.default_rng(seed)
    bps, boff, bases = [], [], []
    at = 0
    for l in order:
        codes = rng.integers(0, 4, l).astype(np.uint8)
        padded = np.concatenate([codes, np.full(-l % 4, 3, np.uint8)])  # padding bits: ones
        q = padded.reshape(-1, 4)
        bps.append((q[:, 0] << 6 | q[:, 1] << 4 | q[:, 2] << 2 | q[:, 3]).astype(np.uint8))
        boff.append(at)
        at += len(bps[-1])
        bases.append(codes)
    return np.concatenate(bps), np.array(boff, np.int64), bases


def numpy_unpack(bps, boff, rlen):
    out = []
    for b, l in zip(boff, rlen):
        byte = bps[b + (np.arange(l) >> 2)]
        out.append((byte >> (6 - 2 * (np.arange(l) & 3))) & 3)
    return np.concatenate(out).astype(np.uint8)


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libbpsload_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libbpsload_host.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.bl_host_unpack.argtypes = [vp, vp, vp, i64, vp, i64, vp, i64]
    L.bl_host_unpack.restype = i64
    return L


def play(L, bps, boff, rlen, chunk_first):
    total = int(np.sum(rlen))
    # exact-size copies of the inputs; the output is a 16-byte aligned window of exactly `total` bytes inside a 0xAA buffer
    bps, boff = bps.copy(), boff.copy()
    rl, cf = np.array(rlen, np.int32), np.array(chunk_first, np.int64)
    back = np.full(total + 48, 0xAA, np.uint8)
    lead = (-back.ctypes.data) % 16 + 16
    out = back[lead:lead + total]
    stores = L.bl_host_unpack(bps.ctypes.data, boff.ctypes.data, rl.ctypes.data, len(rl), cf.ctypes.data, len(cf) - 1, out.ctypes.data, total)
    assert stores >= 0, stores
    assert (back[:lead] == 0xAA).all() and (back[lead + total:] == 0xAA).all()
    return out.copy(), stores


def test_the_order_starts_a_read_on_every_residue():
    order = ordered_lengths()
    assert sorted(order) == sorted(LENGTHS)
    starts = np.concatenate([[0], np.cumsum(order)[:-1]])
    assert set(int(s) % 16 for s in starts) == set(range(16))


def chunkings(order):
    n = len(order)
    yield "one chunk", [0, n]
    yield "one read per chunk", list(range(n + 1))
    ends = np.cumsum(order)
    on_window = [i + 1 for i in range(n - 1) if ends[i] % 16 == 0]
    assert on_window, "no read of the order ends on a 16-byte window"
    yield "a chunk that ends on a window", [0, on_window[0], n]
    yield "three chunks", [0, n // 3, 2 * n // 3, n]


def test_lanes_equal_numpy_at_every_chunking(harness):
    order = ordered_lengths()
    # make sure a boundary on a 16-byte window exists: 16 in front of the rest keeps every start's residue
    if not any(e % 16 == 0 for e in np.cumsum(order)[:-1]):
        order.remove(16)
        order.insert(0, 16)
        starts = np.concatenate([[0], np.cumsum(order)[:-1]])
        assert set(int(s) % 16 for s in starts) == set(range(16))
    bps, boff, bases = make_reads(order)
    want = numpy_unpack(bps, boff, order)
    assert np.array_equal(want, np.concatenate(bases))  # the padding bits did not reach the reference either
    for name, cf in chunkings(order):
        got, stores = play(harness, bps, boff, order, cf)
        assert np.array_equal(got, want), name
        assert stores > 0, name


def test_a_selection_with_holes_in_the_file(harness):
    """every other read: the runs do not touch in the file, the packed offsets inside a chunk are not the file's"""
    order = ordered_lengths()
    bps, boff, bases = make_reads(order, seed=9)
    sel = list(range(0, len(order), 2))
    rlen = [order[i] for i in sel]
    want = numpy_unpack(bps, boff[sel], rlen)
    for cf in ([0, len(sel)], list(range(len(sel) + 1)), [0, 3, len(sel)]):
        got, _ = play(harness, bps, boff[sel], rlen, cf)
        assert np.array_equal(got, want), cf


def test_reads_without_a_base_and_single_reads(harness):
    for rlen in ([0, 5, 0, 0, 33, 0], [1], [16], [15], [17], [4000]):
        bps, boff, bases = make_reads(rlen, seed=3)
        if len(bps) == 0:
            continue
        want = np.concatenate(bases)
        for cf in ([0, len(rlen)], list(range(len(rlen) + 1))):
            got, _ = play(harness, bps, boff, rlen, cf)
            assert np.array_equal(got, want), (rlen, cf)


def test_bad_chunks_are_refused(harness):
    bps, boff, _ = make_reads([5, 6])
    out = np.zeros(11, np.uint8)
    rl = np.array([5, 6], np.int32)
    for cf in ([1, 2], [0, 1]):
        c = np.array(cf, np.int64)
        assert harness.bl_host_unpack(bps.ctypes.data, boff.ctypes.data, rl.ctypes.data, 2, c.ctypes.data, 1, out.ctypes.data, 11) == -1
    c = np.array([0, 2], np.int64)
    assert harness.bl_host_unpack(bps.ctypes.data, boff.ctypes.data, rl.ctypes.data, 2, c.ctypes.data, 1, out.ctypes.data, 12) == -2
