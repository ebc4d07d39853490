"""The lane code of dh_output_db's FASTA formatter (dentist_amd/csrc/dh_outfmt.h) compiled for the CPU and played as 64-lane
wavefronts over chunks of the file (tests/native/outfmt_host.cpp) against the restatement (tests/outfmt_ref.py) on every case of
tests/outfmt_cases.py and every chunking: the default, 64 bytes, 112 bytes and one that ends exactly on a record boundary.
Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import outfmt_cases as oc
import outfmt_ref as orf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFAULT_CHUNK = 256 << 20


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/liboutfmt_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "liboutfmt_host.so"))
    vp, i64 = ctypes.c_void_p, ctypes.c_int64
    L.of_host_format.argtypes = [vp] * 9 + [i64, i64, ctypes.c_int32, i64, vp]
    L.of_host_format.restype = i64
    return L


def play(L, p, contig, cons, chunk):
    total = int(p["rec_off"][-1])
    # exact-size copies: the harness must not need a byte more than the plan states
    arrs = [np.ascontiguousarray(p[n]).copy() for n in ("rec_off", "hdr_off", "seg_first", "seg_base", "seg_src", "seg_flags", "hdr")]
    cb, cs = np.ascontiguousarray(contig).copy(), np.ascontiguousarray(cons).copy()
    out = np.full(total, 0xAA, np.uint8)
    n = L.of_host_format(*[a.ctypes.data for a in arrs], cb.ctypes.data, cs.ctypes.data if len(cs) else None, len(arrs[1]) - 1, len(arrs[4]),
                         p["width"], chunk, out.ctypes.data)
    assert n == total, n
    return out.tobytes()


@pytest.mark.parametrize("name", list(oc.ALL))
def test_every_case_at_every_chunking(harness, name):
    c = oc.ALL[name]
    p = oc.plan_of(c)
    contig = np.concatenate(c["contigs"])
    want = orf.plan_bytes(p, contig, c["bases"])
    chunks = [DEFAULT_CHUNK, 64, 112]
    if oc.chunk_at_record_boundary(p):
        chunks.append(oc.chunk_at_record_boundary(p))
    for chunk in chunks:
        assert play(harness, p, contig, c["bases"], chunk) == want, chunk


def test_a_bad_chunk_size_is_refused(harness):
    c = oc.ALL["cyclic"]
    p = oc.plan_of(c)
    out = np.zeros(int(p["rec_off"][-1]), np.uint8)
    arrs = [np.ascontiguousarray(p[n]) for n in ("rec_off", "hdr_off", "seg_first", "seg_base", "seg_src", "seg_flags", "hdr")]
    cb = np.concatenate(c["contigs"])
    for chunk in (48, 100):
        assert harness.of_host_format(*[a.ctypes.data for a in arrs], cb.ctypes.data, c["bases"].ctypes.data, len(arrs[1]) - 1, len(arrs[4]),
                                      p["width"], chunk, out.ctypes.data) == -1
