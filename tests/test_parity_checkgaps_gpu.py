"""Context.check_gaps (dh_check_gaps: k_cg_bind, the scans, k_cg_gather, the Gotoh kernel on device-resident pairs, k_cg_stats)
against the contract (tests/checkgaps_ref.py) on every scene of tests/checkgaps_cases.py: every field of every summary, the
identity, every op and the score; the counters; the launch-group knob; run-to-run identity; the refusals.  Every comparison is
equality."""
import types

import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib

import checkgaps_cases as cc
import checkgaps_ref as cr
import nwa_ref

pytestmark = pytest.mark.gpu

LEGAL = [n for n in cc.ALL if n not in cc.GAP_0]


def dbs_of(ctx, s):
    def db(seqs):
        off = np.zeros(len(seqs) + 1, np.int64)
        off[1:] = np.cumsum([len(x) for x in seqs])
        return dentist_amd.Db(ctx, types.SimpleNamespace(bases=np.concatenate(seqs).astype(np.uint8), off=off))
    return db(s["true_seqs"]), db(s["result_seqs"])


def call(ctx, s, dbs=None):
    t, r = dbs or dbs_of(ctx, s)
    ptr, iv = cc.dust_arrays(s["dust"], len(s["true_seqs"]))
    return ctx.check_gaps(t, r, s["mapped"], cc.maps_array(s["maps"]), s["result_gap"], dust=None if ptr is None else (ptr, iv[:-2]), crop=s["crop"],
                          scoring=s["scoring"], first_contig=s["first_contig"], count=s["count"])


def check(got, name):
    exp, ident, ops = cc.expected_of(name)
    assert got.summaries.dtype == cc.SUMMARY_DTYPE == _lib.GAP_SUMMARY_DTYPE and _lib.CONTIG_MAPPING_DTYPE == cc.MAP_DTYPE
    for f in cr.FIELDS:
        assert got.summaries[f].tolist() == exp[f].tolist(), (name, f)
    assert np.array_equal(got.identity, ident, equal_nan=True), name
    for g in range(len(exp)):
        if ops[g] is None:
            assert len(got.ops_of(g)) == 0 and got.score[g] == 0, (name, g)
        else:
            assert got.ops_of(g).tobytes() == ops[g].tobytes(), (name, g)
    assert got.aligned == int(np.isin(exp["align_status"], (cr.OK, cr.BAND_EXCEEDED)).sum())


@pytest.mark.parametrize("name", LEGAL)
def test_every_scene_equals_the_contract(gpu_ctx, monkeypatch, name):
    monkeypatch.delenv("DH_NW_CHUNK_KB", raising=False)
    got = call(gpu_ctx, cc.scene(name))
    check(got, name)
    assert got.groups >= (1 if got.aligned else 0)


def test_scores_are_the_aligners(gpu_ctx, monkeypatch):
    monkeypatch.delenv("DH_NW_CHUNK_KB", raising=False)
    for name in ("states_crop_20", "other_scoring"):
        s = cc.scene(name)
        got = call(gpu_ctx, s)
        an = cr.Analyzer(s["true_seqs"], s["result_seqs"], s["mapped"], s["maps"], s["result_gap"], s["dust"], s["crop"])
        for g in np.flatnonzero(got.summaries["align_status"] == cr.OK):
            x = got.summaries[g]
            ref = s["true_seqs"][x["true_contig"] - 1][x["true_begin"]:x["true_end"]]
            qry = an.result_subseq((x["result_begin_contig"], x["result_begin"]), (x["result_end_contig"], x["result_end"]))
            qry = cr.revcomp(qry) if x["complement"] else qry
            assert got.score[g] == nwa_ref.score_of_ops(ref, qry, got.ops_of(g), s["scoring"] or nwa_ref.DEFAULT)


@pytest.mark.parametrize("name", ["many_gaps_crop_7", "columns_crop_10", "band_and_length", "states_crop_20"])
def test_the_launch_group_knob_changes_nothing_but_the_groups(gpu_ctx, monkeypatch, name):
    s = cc.scene(name)
    dbs = dbs_of(gpu_ctx, s)
    monkeypatch.delenv("DH_NW_CHUNK_KB", raising=False)
    a = call(gpu_ctx, s, dbs)
    monkeypatch.setenv("DH_NW_CHUNK_KB", "1")
    b = call(gpu_ctx, s, dbs)
    c = call(gpu_ctx, s, dbs)
    check(b, name)
    for x in (a, c):
        assert x.summaries.tobytes() == b.summaries.tobytes() and x.ops.tobytes() == b.ops.tobytes() and x.score.tobytes() == b.score.tobytes()
    assert b.groups == c.groups > a.groups >= 1


def test_more_than_64_gaps_in_one_call(gpu_ctx, monkeypatch):
    monkeypatch.delenv("DH_NW_CHUNK_KB", raising=False)
    got = call(gpu_ctx, cc.scene("many_gaps"))
    assert len(got) == 71 and got.aligned == 70 and got.groups == 1


def test_no_gaps_is_an_empty_report(gpu_ctx):
    s = dict(cc.scene("no_dust_mask"), count=0)
    got = call(gpu_ctx, s)
    assert len(got) == 0 and len(got.ops) == 0 and got.aligned == 0 and got.groups == 0
    got = call(gpu_ctx, dict(s, first_contig=3))     # (behind the last contig there is nothing to refuse either)
    assert len(got) == 0


@pytest.mark.parametrize("name,s,words", cc.refusals(), ids=[r[0] for r in cc.refusals()])
def test_refusals_name_the_offender(gpu_ctx, name, s, words):
    with pytest.raises(dentist_amd.DhError) as e:
        call(gpu_ctx, s)
    assert "dh_check_gaps: " in str(e.value) and words in str(e.value)


def test_null_pointers_are_refused(gpu_ctx):
    s = cc.scene("no_dust_mask")
    t, r = dbs_of(gpu_ctx, s)
    L = _lib.lib()
    import ctypes
    h = ctypes.c_void_p()
    mp = np.ascontiguousarray(s["mapped"], np.int32)
    ma = cc.maps_array(s["maps"])
    rg = np.asarray(s["result_gap"], np.int32)
    good = [gpu_ctx._h, t._h, r._h, mp.ctypes.data, 2, ma.ctypes.data, 2, rg.ctypes.data, None, None, 0, None, 1, 2, ctypes.byref(h)]
    for k in (0, 1, 2, 3, 5, 7, 14):
        args = list(good)
        args[k] = None
        assert L.dh_check_gaps(*args) == -1 and b"dh_check_gaps: bad argument" in L.dh_last_error()
    dp = np.zeros(2, np.int64)
    assert L.dh_check_gaps(*(good[:8] + [dp.ctypes.data, None] + good[10:])) == -1    # a dust mask needs both arrays
    assert L.dh_check_gaps(*good) == 0
    L.dh_gap_report_destroy(h)
