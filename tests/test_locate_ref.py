"""tests/locate_ref.py (the brute-force oracle of dh_exact_locate and tools/fm-index) against hand-derived cases
(tests/golden/fm_index_cases.json): each is small enough to check by eye and names the lines of the reference's
external/fm-index.cpp it follows from.  No GPU needed."""
import json
import os

import pytest

import locate_ref as lr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fm_index_cases.json")
CASES = json.load(open(GOLD))["cases"]
REQUIRED = ["overlapping poly-a", "a palindrome is reported on both strands", "an empty query line does not advance the id",
            "an empty reference record is counted", "a query that would match only across a record boundary"]


def test_the_required_cases_are_there_and_tagged():
    names = [c["name"] for c in CASES]
    assert all(r in names for r in REQUIRED)
    assert all("fm-index.cpp:" in c["tag"] for c in CASES)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_text_equals_the_hand_derived_lines(case):
    text = lr.tool_output(case["reference"], [tuple(s) for s in case["sources"]], case["reverse"])
    assert text == "".join(line + "\n" for line in case["expected"])


def test_hit_tuples_and_order():
    refs = ["acgtacgt", "", "ttacg"]
    assert lr.locate(refs, ["acg", "", "cgt"]) == [
        (0, 0, 0, 3, 0), (0, 0, 4, 7, 0), (0, 2, 2, 5, 0), (0, 0, 1, 4, 1), (0, 0, 5, 8, 1),  # cgt is acg's reverse complement
        (2, 0, 1, 4, 0), (2, 0, 5, 8, 0), (2, 0, 0, 3, 1), (2, 0, 4, 7, 1), (2, 2, 2, 5, 1)]
    assert lr.locate(refs, ["acg"], both_strands=False) == [(0, 0, 0, 3, 0), (0, 0, 4, 7, 0), (0, 2, 2, 5, 0)]
    assert lr.locate([[0, 1, 2, 3]], [[1, 2]]) == [(0, 0, 1, 3, 0), (0, 0, 1, 3, 1)]  # base codes; cg is a palindrome
    assert lr.records_of("acg\n\nttt") == ["acg", "", "ttt"] and lr.records_of("acg\n\n") == ["acg", ""]
