"""The lane code of the gap analysis (dentist_amd/csrc/dh_checkgaps.h) compiled for the CPU and played as 64-lane wavefronts
(tests/native/checkgaps_host.cpp) against the restatement (tests/checkgaps_ref.py) on every scene of tests/checkgaps_cases.py, the
scenes with a gap of 0 bases included (the checks are left out for those): every field of every summary and the gathered pairs.  The
ops come from the restatement's aligner; the refusals are the driver's own checks.  Every comparison is equality.  No GPU needed."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import checkgaps_cases as cc
import checkgaps_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libcheckgaps_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libcheckgaps_host.so"))
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    L.checkgaps_host.argtypes = [vp, vp, i32, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i32]
    L.checkgaps_host.restype = i32
    return L


def cat(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(x) for x in seqs])
    return np.ascontiguousarray(np.concatenate(list(seqs) + [np.zeros(1, np.uint8)]), np.uint8), off


def run(L, s, ops=None, given_up=None, check=True):
    """(summaries, lengths, ref bytes, qry bytes) or the refusal's text"""
    tb, toff = cat(s["true_seqs"])
    rb, roff = cat(s["result_seqs"])
    mp = np.ascontiguousarray(s["mapped"], np.int32).reshape(-1, 3)
    ma = cc.maps_array(s["maps"])
    rg = np.ascontiguousarray(list(s["result_gap"]) + [0], np.int32)
    dp, di = cc.dust_arrays(s["dust"], len(s["true_seqs"]))
    count = max(s["count"], 0)
    ops = ops or [None] * count
    op_off = np.zeros(count + 1, np.int64)
    op_off[1:] = np.cumsum([0 if o is None else len(o) for o in ops])
    flat = np.ascontiguousarray(np.concatenate([o for o in ops if o is not None] + [np.zeros(1, np.uint8)]), np.uint8)
    gu = np.ascontiguousarray(given_up if given_up is not None else np.zeros(count + 1), np.uint8)
    out, lens = np.zeros(count, cc.SUMMARY_DTYPE), np.zeros(2 * count + 1, np.int32)
    cap = 1 << 20
    oref, oqry = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    msg = ctypes.create_string_buffer(256)
    rc = L.checkgaps_host(tb.ctypes.data, toff.ctypes.data, len(toff) - 1, rb.ctypes.data, roff.ctypes.data, len(roff) - 1, mp.ctypes.data, len(mp),
                          ma.ctypes.data, len(ma), rg.ctypes.data, dp.ctypes.data if dp is not None else None, di.ctypes.data if di is not None else None,
                          s["crop"], s["first_contig"], s["count"], int(check), gu.ctypes.data, op_off.ctypes.data, flat.ctypes.data, out.ctypes.data,
                          lens.ctypes.data, oref.ctypes.data, oqry.ctypes.data, cap, msg, 256)
    assert rc in (0, -1), rc
    if rc:
        return msg.value.decode()
    return out, lens[:2 * count].reshape(-1, 2), oref, oqry


@pytest.mark.parametrize("name", list(cc.ALL))
def test_every_scene_equals_the_contract(harness, name):
    s = cc.scene(name)
    exp, _, ops = cc.expected_of(name)
    got, lens, oref, oqry = run(harness, s, list(ops), exp["align_status"] == cr.BAND_EXCEEDED, check=s["legal"])
    for f in cr.FIELDS:
        assert got[f].tolist() == exp[f].tolist(), (name, f)
    # the gathered pairs are the restatement's sequences
    an = cr.Analyzer(s["true_seqs"], s["result_seqs"], s["mapped"], s["maps"], s["result_gap"], s["dust"], s["crop"])
    rat = qat = 0
    for g, x in enumerate(exp):
        rl, ql = lens[g]
        if x["align_status"] not in (cr.OK, cr.BAND_EXCEEDED) and not (x["align_status"] == cr.EMPTY and rl):
            assert (rl, ql) == (0, 0)
            continue
        ref = s["true_seqs"][x["true_contig"] - 1][x["true_begin"]:x["true_end"]]
        qry = an.result_subseq((x["result_begin_contig"], x["result_begin"]), (x["result_end_contig"], x["result_end"]))
        qry = cr.revcomp(qry) if x["complement"] else qry
        assert oref[rat:rat + rl].tobytes() == ref.tobytes() and oqry[qat:qat + ql].tobytes() == np.asarray(qry, np.uint8).tobytes(), (name, g)
        rat, qat = rat + rl, qat + ql


@pytest.mark.parametrize("name,s,words", [r for r in cc.refusals() if "bad argument" not in r[2] and r[0] != "scoring"],
                         ids=[r[0] for r in cc.refusals() if "bad argument" not in r[2] and r[0] != "scoring"])
def test_the_checks_name_the_offender(harness, name, s, words):
    got = run(harness, s)
    assert isinstance(got, str) and words in got, got
