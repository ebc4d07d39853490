"""The restatement of the mask-algebra contract (tests/maskops_ref.py) against the reference's own unit vectors
(tests/golden/region_cases.json, from util/region.d) in both forms, and the interval form against the per-base form on every
small case of tests/maskops_cases.py.  CPU only."""
import json
import os

import numpy as np
import pytest

import maskops_cases as mc
import maskops_ref as mr

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "region_cases.json")))


@pytest.mark.parametrize("k", range(len(GOLDEN["cases"])), ids=[c["source"] + " " + c["op"] for c in GOLDEN["cases"]])
def test_reference_vectors_on_both_forms(k):
    g = GOLDEN["cases"][k]
    n = GOLDEN["ncontigs"]
    masks = [mc.mask(n, m) for m in g["masks"]]
    sub = mc.mask(n, g["subtract"]) if g["subtract"] is not None else None
    off = np.arange(n + 1, dtype=np.int64) * GOLDEN["contig_length"]
    min_count = len(masks) if g["op"] == "and" else 1
    exp = sorted(tuple(t) for t in g["expect"])
    assert mr.combine_bases(masks, off, min_count, sub) == exp
    assert mr.combine_intervals(masks, off, min_count, sub) == exp


@pytest.mark.parametrize("name", [n for n, c in mc.ALL.items() if c["small"]])
def test_interval_form_equals_per_base_form(name):
    c = mc.ALL[name]
    assert mc.expected_of(name) == mr.combine_bases(c["masks"], c["contig_off"], **mc.args_of(c))


def test_the_cases_say_what_their_names_say():
    e = mc.expected_of
    assert e("nothing") == [] and e("only_empty_intervals") == [] and e("one_interval") == [(0, 2, 7)]
    assert e("three_masks_min_2") == [(0, 0, 10)] and e("touching_across_masks_min_2") == []
    assert e("raw_intervals_do_not_count") == [(0, 12, 15)]
    assert e("within_one_mask") == [(1, 0, 3), (1, 10, 35), (1, 40, 70), (1, 90, 100)]
    assert e("subtract") == [(0, 10, 15), (0, 25, 30), (0, 70, 80), (1, 0, 20)]
    assert e("gap_equal_joined_one_more_not") == [(0, 0, 20), (0, 26, 30), (1, 0, 5)] and e("both_gaps_joined") == [(0, 0, 30), (1, 0, 5)]
    assert e("cascade") == [(0, 0, 44), (0, 60, 62)] and e("no_join_across_contigs") == [(0, 90, 100), (1, 0, 10)]
    assert e("size_equal_kept") == [(0, 0, 7), (1, 3, 10)] and e("size_one_less_dropped") == []
    assert e("crumbs_survive_by_gaps") == [(0, 0, 8)] and e("everything_filtered") == []
    assert e("closed_gap_covers_subtracted") == [(0, 0, 30)]
    top = 2 ** 31 - 1
    assert e("longest_contig") == [(0, 0, 100), (1, 0, top)] and e("longest_contig_min_2") == [(1, 2, 3), (1, top - 5, top - 4)]
    assert e("all_keys_equal") == [(1, 7, 19)] == e("all_keys_equal_min_2")


def test_tandem_restated():
    las, read_off, first, min_len = mc.tandem_case(5)
    assert mr.tandem(las, read_off, first, min_len) == [(0, 100, 1300), (2, 50, 1100), (3, 0, 2000)]
