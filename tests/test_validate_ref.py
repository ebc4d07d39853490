"""The restatement of the region-validation contract (tests/validate_ref.py, around the oracle's literal window loop), the host
function dentist_amd.validate_regions and the hand-worked literals of tests/validate_cases.py agree on every shape.  Every
comparison is equality.  No GPU needed."""
import numpy as np
import pytest

import validate_cases as vc
import validate_ref as vr


@pytest.mark.parametrize("name", list(vc.HAND))
def test_hand_worked_cases(name):
    case, expected = vc.HAND[name]
    for got in (vr.validate(case), vr.from_host(case)):
        rep = got["reports"][0]
        assert (rep["ctx_begin"], rep["ctx_end"]) == (30, 60)
        assert got["span_ids"].tolist() == expected["span"] and rep["num_spanning_reads"] == len(expected["span"])
        assert [tuple(x) for x in got["weak"].tolist()] == expected["weak"]
        assert rep["weak_bp"] == expected["weak_bp"] and bool(rep["is_valid"]) == expected["valid"]
        assert [tuple(x) for x in got["mask"][1].tolist()] == [(b, e) for _, b, e in expected["weak"]]


@pytest.mark.parametrize("name", list(vc.SHAPES))
def test_the_host_function_equals_the_restatement(name):
    case = vc.SHAPES[name]
    exp, host = vr.validate(case), vr.from_host(case)
    assert vr.same(host, exp) and host["pairs"] == exp["pairs"]


def test_the_shapes_are_what_their_names_say():
    s = {k: vr.validate(c) for k, c in vc.SHAPES.items()}
    for k in (0, 1, 63, 64, 65):
        assert s[f"pairs_{k}"]["pairs"] == k
    for k in (1, 64, 65):
        off = s[f"spanning_{k}"]["span_off"]
        ids = s[f"spanning_{k}"]["span_ids"]
        assert off.tolist() == [0, k] and (k == 1 or sorted(ids.tolist()) != ids.tolist())  # not in the order of the ids
    assert len(s["runs_exactly_wlen_apart"]["weak"]) == 1 and len(s["runs_wlen_plus_one_apart"]["weak"]) == 2
    r = s["contig_without_records"]["reports"][0]
    assert (r["weak_bp"], r["is_valid"], len(s["contig_without_records"]["weak"])) == (0, 0, 0)
    assert len(s["empty_extended_region"]["weak"]) == 0 and len(s["region_behind_the_contig"]["weak"]) == 0
    assert len(s["region_shorter_than_the_window"]["weak"]) == 0
    assert s["region_shorter_than_the_window_weak"]["weak"].tolist() == [[0, 95, 125]]
    assert s["context_clipped_at_the_start"]["reports"][0]["ctx_begin"] == 0
    assert s["context_clipped_at_the_end"]["reports"][0]["ctx_end"] == 300
    c = s["weak_run_across_chunks"]
    assert any(b < 100 + 2 * vc.CHUNK < e for _, b, e in c["weak"].tolist())
    c = s["regions_shuffled"]
    assert len(c["mask"][1]) < len(c["weak"])  # the union merges what nested and repeated regions report more than once
    for k in (-1, 0, 1):
        case = vc.SHAPES[f"tier_cap{k:+d}"]
        rep = s[f"tier_cap{k:+d}"]["reports"][0]
        assert rep["ctx_end"] - rep["ctx_begin"] - case["window"] + 2 == vc.LOW_CAP + k and 0 < rep["weak_bp"]


def test_group_case_fills_a_megabyte_per_region():
    case = vc.group_case()
    exp, host = vr.validate(case), vr.from_host(case)
    assert vr.same(host, exp)
    assert all(4 * (r["ctx_end"] - r["ctx_begin"] - case["window"] + 2) > (1 << 20) for r in exp["reports"])
    assert len(exp["weak"]) >= 4 and exp["reports"]["num_spanning_reads"].tolist() == [1, 1, 1, 1]


def test_many_regions_on_one_contig_by_the_host_function():
    """The literal loop is too slow for 1 000 regions over 100 000 records: the expectation of this shape is the host
    function's, which tests/test_maskcov.py::test_validate_regions_matches_the_literal_restatement pins to the literal loop."""
    case = vc.many_regions()
    host = vr.from_host(case)
    assert len(host["reports"]) == 1000 and host["pairs"] > 10_000 and 0 < len(host["weak"])
    assert 0 < host["reports"]["is_valid"].sum() < 1000 and host["span_off"][-1] > 0
    assert np.array_equal(np.diff(host["span_off"]), host["reports"]["num_spanning_reads"])
