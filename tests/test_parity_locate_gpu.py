"""The exact-match locator on the GPU (dh_exact_locate / Context.exact_locate: k_locate_scan, k_locate_verify,
k_locate_short of dh_locate.hip) against the brute-force oracle of tests/locate_ref.py on the shapes of
tests/locate_cases.py: every hit, in the order of the contract.  Every comparison is equality."""
import numpy as np
import pytest

import dentist_amd
import locate_cases as lc
import locate_ref as lr

pytestmark = pytest.mark.gpu


def test_hit_dtype_is_the_headers():
    assert dentist_amd.EXACT_HIT_DTYPE.itemsize == 32
    assert dentist_amd.EXACT_HIT_DTYPE.names == ("query", "ref", "begin", "end", "complement", "pad")


@pytest.mark.parametrize("both", [True, False], ids=["both-strands", "forward"])
def test_main_case_equals_the_oracle(gpu_ctx, both):
    refs, queries, notes = lc.main_case()
    assert len(refs) == 40 and len(refs[1]) == 0 and len(refs[2]) == 1
    exp = lc.main_expected(both)
    got = lc.as_tuples(gpu_ctx.exact_locate(refs, queries, both_strands=both))
    assert got == exp
    pa = notes["poly-a"][0]
    assert [h for h in got if h[0] == pa and h[1] == 11 and h[4] == 0] == [(pa, 11, b, b + 40, 0) for b in range(61)]
    assert not any(h[0] in (notes["across"][0], notes["longer than a record"][0], notes["longer than the reference"][0]) for h in got)
    if both:
        p = notes["palindrome"][0]
        fwd = [h[1:4] for h in got if h[0] == p and h[4] == 0]
        assert fwd and fwd == [h[1:4] for h in got if h[0] == p and h[4] == 1]
    # bit-identical from run to run
    again = gpu_ctx.exact_locate(refs, queries, both_strands=both)
    assert again.tobytes() == gpu_ctx.exact_locate(refs, queries, both_strands=both).tobytes()


def test_pre_filter_bitmap_changes_nothing(gpu_ctx, monkeypatch):
    refs, queries, _ = lc.main_case()
    monkeypatch.setenv("DH_LOCATE_BITMAP", "1")
    assert lc.as_tuples(gpu_ctx.exact_locate(refs, queries)) == lc.main_expected(True)


def test_three_segments(gpu_ctx, monkeypatch):
    """DH_LOCATE_SEG=4096 cuts the 10 000-base query into three verify units: matching fully, a mismatch only in the last
    segment, a mismatch only in the first"""
    refs, queries = lc.segment_case()
    exp = lr.locate(refs, queries)
    assert exp == [(0, 1, 1003, 11003, 0)]
    monkeypatch.setenv("DH_LOCATE_SEG", "4096")
    assert lc.as_tuples(gpu_ctx.exact_locate(refs, queries)) == exp
    monkeypatch.delenv("DH_LOCATE_SEG")
    assert lc.as_tuples(gpu_ctx.exact_locate(refs, queries)) == exp


def test_small_candidate_buffer_changes_nothing(gpu_ctx, monkeypatch):
    """DH_LOCATE_CAND_CAP=64: ranges whose candidates exceed the buffer are scanned again in halves, nothing is dropped"""
    refs, queries, _ = lc.main_case()
    exp = lc.main_expected(True)
    assert len(exp) >= 500  # every hit of the oracle was a candidate of the scan: the case overflows 64 entries many times
    default = gpu_ctx.exact_locate(refs, queries)
    monkeypatch.setenv("DH_LOCATE_CAND_CAP", "64")
    small = gpu_ctx.exact_locate(refs, queries)
    assert small.tobytes() == default.tobytes() and lc.as_tuples(small) == exp


def test_nothing_to_search(gpu_ctx):
    refs, queries, _ = lc.main_case()
    for r, q in (([], queries[:5]), (refs, []), ([], []), ([np.zeros(0, np.uint8)], queries[:5])):
        out = gpu_ctx.exact_locate(r, q)
        assert out.dtype == dentist_amd.EXACT_HIT_DTYPE and len(out) == 0


def test_refused_inputs(gpu_ctx):
    refs, queries, _ = lc.main_case()
    bad = queries[20].copy()
    bad[7] = 4
    with pytest.raises(dentist_amd.DhError) as ei:
        gpu_ctx.exact_locate(refs, queries[:3] + [bad])
    assert ei.value.code == -1 and "query 3" in str(ei.value)
    badr = refs[3].copy()
    badr[-1] = 4
    with pytest.raises(dentist_amd.DhError) as ei:
        gpu_ctx.exact_locate(refs[:3] + [badr], queries[:3])
    assert ei.value.code == -1 and "record 3" in str(ei.value)
    r = np.concatenate(refs[:4])
    roff = np.concatenate([[0], np.cumsum([len(x) for x in refs[:4]])]).astype(np.int64)
    q = np.concatenate(queries[:4])
    qoff = np.concatenate([[0], np.cumsum([len(x) for x in queries[:4]])]).astype(np.int64)
    dec = roff.copy()
    dec[2] = dec[1] - 1
    neg = qoff.copy()
    neg[0] = -1
    for a, b in ((dec, qoff), (roff, neg)):
        with pytest.raises(dentist_amd.DhError) as ei:
            gpu_ctx.exact_locate_raw(r, a, q, b)
        assert ei.value.code == -1
    assert lc.as_tuples(gpu_ctx.exact_locate_raw(r, roff, q, qoff)) == lr.locate(refs[:4], queries[:4])
