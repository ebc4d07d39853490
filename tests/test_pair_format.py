"""dh_format_pair / dentist_amd.format_pair: the EMBOSS `pair` text of an alignment as `dentist check-results` reads it
from stretcher (commands/checkResults.d:2113-2162), against hand-written expectations (no GPU needed)."""
import json
import os
import re

import numpy as np
import pytest

import dentist_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "pair_format_cases.json")) as f:
    CASES = json.load(f)["cases"]


def read_like_check_results(text):
    """checkResults.d:2113-2133 (stretcherReadPercentIdentity: the first line that starts with "# Identity:", then
    formattedRead of "# Identity: %d/%d", where a blank of the format matches any run of blanks) and :2135-2162
    (stretcherReadAlignmentString: the lines that are neither empty nor comments must be exactly three; the sequences are
    captured by the regular expression below, the edit ops are the middle line behind the length of the first line's
    prefix, blanks turned into '-').  Returns (identical, length, reference line, edit ops, query line)."""
    lines = text.split("\n")
    ident = next(l for l in lines if l.startswith("# Identity:"))
    m = re.match(r"# Identity:\s*(\d+)/(\d+)", ident)
    body = [l for l in lines if len(l) > 0 and l[0] != "#"]
    assert len(body) == 3, body
    rx = re.compile(r"^\s*(?P<prefix>(?:true|inserted)-[0-9@-]+\s+\d+\s+)(?P<seq>[ACTGN-]+).*$")
    m0, m2 = rx.match(body[0]), rx.match(body[2])
    assert m0 and m2, body
    edit = body[1][len(m0.group("prefix")):].replace(" ", "-")
    return int(m.group(1)), int(m.group(2)), m0.group("seq").lower(), edit, m2.group("seq").lower()


def fmt(c, **kw):
    b = c["b"] if isinstance(c["b"], str) else np.asarray(c["b"], np.uint8)
    args = dict(scoring=c["scoring"], width=c["width"])
    args.update(kw)
    return dentist_amd.format_pair(c["name_a"], c["a"], c["name_b"], b, c["ops"], c["score"], **args)


def body_of(text):
    return [l for l in text.split("\n") if l and l[0] != "#"]


def test_exact_text_of_a_tiny_pair():
    c = CASES[0]
    assert fmt(c) == "".join(l + "\n" for l in c["text"])
    assert fmt(c, width=50) == fmt(c) == fmt(c, width=4)  # one block whenever the width covers the alignment


@pytest.mark.parametrize("c", CASES[1:], ids=lambda c: c["id"])
def test_alignment_lines(c):
    text = fmt(c)
    assert body_of(text) == c["alignment"]
    assert f"# Identity:   {c['identity'][0]:7d}/{c['identity'][1]} ({100 * c['identity'][0] / c['identity'][1]:4.1f}%)" in text.split("\n")
    for h in c.get("header", []):
        assert h in text.split("\n"), h
    assert text.endswith("\n") and "\n\n\n\n" not in text


def test_trailing_gap_keeps_the_markup_as_long_as_the_sequences():
    c = CASES[1]
    a, m, b = body_of(fmt(c))
    assert len(m) == 21 + len(c["ops"]) and m.endswith("  ")
    assert a[21:21 + len(c["ops"])] == "ACGTTACG--" and b[21:21 + len(c["ops"])] == "ACG--ACGGN"


def test_names_are_cut_to_thirteen_characters():
    c = CASES[2]
    for l in body_of(fmt(c))[0::3]:
        assert l.startswith("a-very-long-s ") and l[13] == " " and l[20] == " "
    assert "# 1: a-very-long-sequence-name" in fmt(c)  # the header keeps the whole name


@pytest.mark.parametrize("c", CASES[:2], ids=lambda c: c["id"])
def test_the_reference_reader_recovers_identity_and_three_lines(c):
    n, m, ref_line, edit, qry_line = read_like_check_results(fmt(c, width=2 ** 32 - 1))
    ops = np.asarray(c["ops"])
    assert (n, m) == tuple(c["identity"]) == (int(np.count_nonzero(ops == 0)), len(ops))
    assert len(ref_line) == len(edit) == len(qry_line) == len(ops)
    assert edit == "".join({0: "|", 3: ".", 1: "-", 2: "-"}[int(o)] for o in ops)
    assert [ch == "-" for ch in ref_line] == [o == 2 for o in ops] and [ch == "-" for ch in qry_line] == [o == 1 for o in ops]


def test_sizing_convention_and_refusals():
    L = dentist_amd.lib()
    a = np.frombuffer(b"ACGT", np.uint8)
    ops = np.asarray([0, 0, 0, 0], np.uint8)
    n = L.dh_format_pair(b"x", a.ctypes.data, 4, b"y", a.ctypes.data, 4, ops.ctypes.data, 4, 20, None, 0, None, 0)
    assert n == len(dentist_amd.format_pair("x", "ACGT", "y", "ACGT", ops, 20))
    import ctypes
    buf = ctypes.create_string_buffer(int(n))  # one byte short: nothing is written
    assert L.dh_format_pair(b"x", a.ctypes.data, 4, b"y", a.ctypes.data, 4, ops.ctypes.data, 4, 20, None, 0, buf, int(n)) == n
    assert buf.raw == b"\0" * n
    with pytest.raises(dentist_amd.DhError):
        dentist_amd.format_pair("x", "ACG", "y", "ACGT", ops, 0)  # the ops consume more bases than a has
    with pytest.raises(dentist_amd.DhError):
        dentist_amd.format_pair("x", "ACGT", "y", "ACGT", [0, 0, 0, 7], 0)
    empty = dentist_amd.format_pair("x", "", "y", "", [], 0)
    assert "# Length: 0" in empty and body_of(empty) == []
