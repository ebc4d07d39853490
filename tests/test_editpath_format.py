"""dh_format_alignment / dh_format_cigar (host only, no GPU needed) against the reference's own alignment texts
(util/string.d:523-751, tests/golden/nw_cases.json)."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import dentist_amd

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPS = {"sub": 0, "del": 1, "ins": 2}


def _cases():
    with open(os.path.join(GOLD, "nw_cases.json")) as f:
        return [c for c in json.load(f)["cases"] if not c["free_shift"]]


def _ops_of(case):
    """the case's edit path as op bytes 0/1/2/3: the golden ops where the case lists them, else oracle/nw.c's (pinned on
    these very cases by test_oracle_golden.py); substitutions split by base equality"""
    ref, qry = case["ref"], case["qry"]
    if "ops" in case:
        raw = [OPS[o] for o in case["ops"]]
    else:
        from oracle import pyoracle as oz
        raw = oz.nw(np.frombuffer(ref.encode(), np.uint8), np.frombuffer(qry.encode(), np.uint8), case["indel"], False)[1].tolist()
    out, i, j = [], 0, 0
    for op in raw:
        if op == 0:
            out.append(0 if ref[i] == qry[j] else 3)
            i, j = i + 1, j + 1
        elif op == 1:
            out.append(1)
            i += 1
        else:
            out.append(2)
            j += 1
    assert (i, j) == (len(ref), len(qry))
    return np.asarray(out, dtype=np.uint8)


def test_there_are_cases():
    assert len(_cases()) >= 3


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"string.d:{c['line']}")
def test_format_alignment_gives_the_reference_text(case):
    ops = _ops_of(case)
    assert dentist_amd.format_alignment(case["ref"], case["qry"], ops, case["width"]) == case["text"]


@pytest.mark.parametrize("case", _cases(), ids=lambda c: f"string.d:{c['line']}")
def test_format_cigar_consumes_both_sequences(case):
    ops = _ops_of(case)
    ext = dentist_amd.format_cigar(ops, extended=True)
    runs = re.findall(r"(\d+)([=XID])", ext)
    assert "".join(n + c for n, c in runs) == ext and ext
    assert all(a[1] != b[1] for a, b in zip(runs, runs[1:])), "adjacent runs of one symbol"
    assert sum(int(n) for n, c in runs if c in "=XD") == len(case["ref"])
    assert sum(int(n) for n, c in runs if c in "=XI") == len(case["qry"])
    assert sum(int(n) for n, c in runs if c == "=") == int(np.count_nonzero(ops == 0))
    assert sum(int(n) for n, c in runs if c == "X") == int(np.count_nonzero(ops == 3))
    # M / I / D: = and X merge
    mid = dentist_amd.format_cigar(ops, extended=False)
    mruns = re.findall(r"(\d+)([MID])", mid)
    assert "".join(n + c for n, c in mruns) == mid
    assert all(a[1] != b[1] for a, b in zip(mruns, mruns[1:]))
    assert sum(int(n) for n, c in mruns if c == "M") == int(np.count_nonzero((ops == 0) | (ops == 3)))
    assert re.sub(r"[=X]", "M", "".join(c * int(n) for n, c in runs)) == "".join(c * int(n) for n, c in mruns)


def test_known_strings_and_base_codes():
    ops = np.asarray([0, 0, 3, 1, 1, 0, 2, 3, 3, 0], dtype=np.uint8)
    assert dentist_amd.format_cigar(ops) == "2=1X2D1=1I2X1="
    assert dentist_amd.format_cigar(ops, extended=False) == "3M2D1M1I3M"
    assert dentist_amd.format_cigar(np.zeros(0, np.uint8)) == ""
    a = np.asarray([0, 1, 2, 3, 4, 0, 1, 2, 3], dtype=np.uint8)  # base codes print as acgtn
    b = np.asarray([0, 1, 3, 0, 2, 0, 0, 3], dtype=np.uint8)
    assert dentist_amd.format_alignment(a, b, ops) == "acgtna-cgt\n||*  | **|\nact--agaat"
    assert dentist_amd.format_alignment(a, b, ops, 4) == "acgt\n||* \nact-\n\nna-c\n | *\n-aga\n\ngt\n*|\nat"


def test_cap_too_small_returns_the_needed_length():
    L = dentist_amd.lib()
    ops = np.asarray([0] * 12 + [1] + [3] * 2, dtype=np.uint8)
    want = "12=1D2X"
    assert L.dh_format_cigar(ops.ctypes.data, len(ops), 1, None, 0) == len(want)
    buf = ctypes.create_string_buffer(b"#" * 16, 16)
    for cap in (0, 1, len(want)):  # no room for the text and its terminating 0: nothing is written
        assert L.dh_format_cigar(ops.ctypes.data, len(ops), 1, buf, cap) == len(want)
        assert buf.raw == b"#" * 16
    assert L.dh_format_cigar(ops.ctypes.data, len(ops), 1, buf, len(want) + 1) == len(want)
    assert buf.value.decode() == want
    a = np.frombuffer(b"ACGTACGTACGTAAA", dtype=np.uint8)
    n = L.dh_format_alignment(a.ctypes.data, a.ctypes.data, ops.ctypes.data, len(ops), 0, None, 0)
    assert n == 3 * len(ops) + 2
    big = ctypes.create_string_buffer(b"#" * 64, 64)
    assert L.dh_format_alignment(a.ctypes.data, a.ctypes.data, ops.ctypes.data, len(ops), 0, big, n) == n
    assert big.raw == b"#" * 64
    assert L.dh_format_alignment(a.ctypes.data, a.ctypes.data, ops.ctypes.data, len(ops), 0, big, n + 1) == n
    assert len(big.value) == n


def test_bad_op_codes_are_refused():
    bad = np.asarray([0, 4], dtype=np.uint8)
    assert dentist_amd.lib().dh_format_cigar(bad.ctypes.data, 2, 1, None, 0) == -1
    with pytest.raises(dentist_amd.DhError):
        dentist_amd.format_cigar(bad)
