"""The lane code and the host planning of the exact-match locator (dentist_amd/csrc/dh_locate.h) compiled for the CPU and
played as 64-lane wavefronts (tests/native/locate_host.cpp) against the brute-force oracle (tests/locate_ref.py) on the
shapes of tests/locate_cases.py: every hit, in the order of the contract.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import locate_cases as lc
import locate_ref as lr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT = np.dtype([("query", "<i4"), ("ref", "<i4"), ("begin", "<i8"), ("end", "<i8"), ("complement", "<i4"), ("pad", "<i4")])
CAP, SEG = 1 << 20, 1 << 20  # the defaults of the driver


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/liblocate_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "liblocate_host.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.locate_host.argtypes = [vp, vp, i64, vp, vp, i64, i32, i64, i64, i32, vp, i64, vp]
    L.locate_host.restype = i64
    return L


def concat(seqs):
    off = np.zeros(len(seqs) + 1, dtype=np.int64)
    if len(seqs):
        off[1:] = np.cumsum([len(s) for s in seqs])
    return (np.concatenate(seqs).astype(np.uint8) if len(seqs) else np.zeros(0, np.uint8)), off


def locate(L, refs, queries, both=True, cap=CAP, seg=SEG, bitmap=False, raw=None):
    """(hit tuples, info) of the harness; raw = (ref, ref_off, qry, qry_off) instead of lists"""
    r, roff, q, qoff = raw if raw is not None else (*concat(refs), *concat(queries))
    info = np.zeros(3, dtype=np.int64)
    hits = np.zeros(1 << 17, dtype=HIT)
    n = L.locate_host(r.ctypes.data, roff.ctypes.data, len(roff) - 1, q.ctypes.data, qoff.ctypes.data, len(qoff) - 1, int(both), cap, seg,
                      int(bitmap), hits.ctypes.data, len(hits), info.ctypes.data)
    if n < 0:
        return None, info
    assert n <= len(hits)
    return lc.as_tuples(hits[:n]), info


def test_hit_layout_is_the_headers():
    assert HIT.itemsize == 32
    hdr = open(os.path.join(ROOT, "include", "dentist_hip.h")).read()
    assert "int32_t query, ref; int64_t begin, end; int32_t complement, pad_; } dh_exact_hit;" in hdr


@pytest.mark.parametrize("both", [True, False], ids=["both-strands", "forward"])
@pytest.mark.parametrize("bitmap", [False, True], ids=["table", "bitmap"])
def test_main_case_equals_the_oracle(host, both, bitmap):
    refs, queries, notes = lc.main_case()
    exp = lc.main_expected(both)
    got, info = locate(host, refs, queries, both, bitmap=bitmap)
    assert got == exp
    # the case keeps its points: 61 hits of a x 40 in a x 100, nothing across a boundary or for the oversized queries
    by_query = {}
    for h in exp:
        by_query.setdefault(h[0], []).append(h)
    pa = notes["poly-a"][0]
    assert [h for h in by_query[pa] if h[1] == 11 and h[4] == 0] == [(pa, 11, b, b + 40, 0) for b in range(61)]
    for name in ("longer than a record", "longer than the reference", "empty"):
        assert notes[name][0] not in by_query
    assert notes["across"][0] not in by_query
    if both:
        p = notes["palindrome"][0]
        fwd = [h[1:4] for h in by_query[p] if h[4] == 0]
        assert fwd and fwd == [h[1:4] for h in by_query[p] if h[4] == 1]
    tw, tr = notes["twins"][0], notes["triple"]
    assert [h[1] for h in by_query[tw] if h[4] == 0] == [3, 4]
    assert [[h[1] for h in by_query[q] if h[4] == 0] for q in tr] == [[6], [6, 7], [6, 7, 8], [7], [8]]
    for q, n in zip(notes["lengths"], lc.LENGTHS):
        assert any(h[1] == 0 and h[3] - h[2] == n for h in by_query[q])
    assert all(any(h[1] == 12 and h[4] == 0 for h in by_query[q]) for q in notes["residues"])
    hitting = [q for q in notes["anchor group"] if q in by_query]
    assert hitting == notes["anchor group"][0::2]


def test_small_candidate_buffer_and_short_segments_change_nothing(host):
    refs, queries, _ = lc.main_case()
    exp = lc.main_expected(True)
    assert len(exp) >= 500  # every hit was a candidate
    got, info = locate(host, refs, queries, True, cap=64, seg=64)
    assert got == exp
    assert info[2] > 100 and info[1] > 0  # ranges were halved; units were cut


def test_three_segments(host):
    refs, queries = lc.segment_case()
    for seg in (4096, SEG):
        got, info = locate(host, refs, queries, True, seg=seg)
        assert got == lr.locate(refs, queries) == [(0, 1, 1003, 11003, 0)]
        assert (info[0], info[1]) == (3, 9 if seg == 4096 else 3)  # three candidates passed the scan's own compare


def test_degenerate_and_refused_inputs(host):
    refs, queries, _ = lc.main_case()
    assert locate(host, [], queries[:5])[0] == [] and locate(host, refs, [])[0] == []
    assert locate(host, [np.zeros(0, np.uint8)], queries[:5])[0] == []
    r, roff = concat(refs[:4])
    q, qoff = concat(queries[:4])
    bad = q.copy()
    bad[3] = 4
    assert locate(host, None, None, raw=(r, roff, bad, qoff))[0] is None
    badr = r.copy()
    badr[-1] = 4
    assert locate(host, None, None, raw=(badr, roff, q, qoff))[0] is None
    dec = roff.copy()
    dec[2] = dec[1] - 1
    assert locate(host, None, None, raw=(r, dec, q, qoff))[0] is None
    neg = qoff.copy()
    neg[0] = -1
    assert locate(host, None, None, raw=(r, roff, q, neg))[0] is None


def test_text_ends_inside_and_at_a_word(host):
    """records whose end is the end of the text, at every length mod 32 around a word boundary: the two-word loads at the end of
    the packed text"""
    rng = np.random.default_rng(3)
    for n in list(range(1, 70)) + [95, 96, 97, 127, 128, 129]:
        rec = rng.integers(0, 4, n).astype(np.uint8)
        qs = [rec, rec[-min(n, 33):], rec[-min(n, 5):], rec[:min(n, 32)], lc.rc(rec)]
        assert locate(host, [rec], qs)[0] == lr.locate([rec], qs), n
