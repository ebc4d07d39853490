"""The restatement of the gap analysis (tests/checkgaps_ref.py) against the reference's own unit vector of cropReference
(tests/golden/checkgaps_cases.json), against alignments worked by hand, and on the scenes of tests/checkgaps_cases.py: that every
scene shows what it was built to show.  No GPU needed."""
import json
import math
import os

import numpy as np
import pytest

import checkgaps_cases as cc
import checkgaps_ref as cr

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "checkgaps_cases.json")))


@pytest.mark.parametrize("v", GOLDEN["crop_reference"])
def test_crop_reference_is_the_references_unit_vector(v):
    al, exp = v["alignment"], v["cropped"]
    got = cr.crop_reference(al, v["crop"])
    for k in ("referenceLength", "queryLength", "complement", "referenceLine", "editOps", "queryLine"):
        assert got[k] == exp[k], k
    assert got["percentIdentity"] == exp["identity"][0] / exp["identity"][1]
    assert (got["gapBegin"], got["gapEnd"]) == (10, 40)
    assert al["editOps"].count("|") == al["identity"][0] and len(al["editOps"]) == al["identity"][1]


def test_crop_reference_by_hand():
    al = {"referenceLine": "-ac--gt-", "editOps": "-||--|.-", "queryLine": "tacgggac"}
    # base #1 is column 1, so the kept columns start at 2; base #(4 - 1 + 1) = #4 is column 6
    got = cr.crop_reference(al, 1)
    assert (got["gapBegin"], got["gapEnd"], got["referenceLine"], got["editOps"]) == (2, 6, "c--g", "|--|")
    assert (got["referenceLength"], got["queryLength"], got["percentIdentity"]) == (2, 4, 0.5)
    # two bases on each side of four: nothing is left, the identity is 0 / 0
    got = cr.crop_reference(al, 2)
    assert (got["gapBegin"], got["gapEnd"]) == (3, 5) and got["referenceLine"] == "--" and got["referenceLength"] == 0 and got["percentIdentity"] == 0.0
    # crop is never reached: countUntil gives -1, the bounds are 0 and the length
    got = cr.crop_reference(al, 5)
    assert (got["gapBegin"], got["gapEnd"]) == (0, 8)
    # no lines at all
    got = cr.crop_reference({"referenceLine": "", "editOps": "", "queryLine": ""}, 3)
    assert (got["gapBegin"], got["gapEnd"], got["referenceLength"], got["queryLength"]) == (0, 0, 0, 0) and math.isnan(got["percentIdentity"])
    # n is no base
    got = cr.crop_reference({"referenceLine": "nacgt", "editOps": ".||||", "queryLine": "tacgt"}, 1)
    assert (got["gapBegin"], got["gapEnd"]) == (2, 4)


def test_early_return_lengths():
    a = cr.stretcher(np.zeros(0, np.uint8), np.asarray([0, 1, 2], np.uint8), False, cr.nwa_ref.DEFAULT)
    assert (a["status"], a["referenceLength"], a["queryLength"], a["editOps"]) == (cr.EMPTY, 0, 3, "") and math.isnan(a["percentIdentity"])
    a = cr.stretcher(np.asarray([0, 1], np.uint8), np.asarray([4, 4, 4], np.uint8), True, cr.nwa_ref.DEFAULT)
    assert (a["status"], a["referenceLength"], a["queryLength"]) == (cr.EMPTY, 2, 3)
    c = cr.crop_reference(a, 1)
    assert (c["referenceLength"], c["queryLength"]) == (0, 0) and math.isnan(c["percentIdentity"])


def test_lines_and_complement():
    ref, qry = np.asarray([0, 1, 2, 3, 0], np.uint8), np.asarray([3, 4, 1, 0], np.uint8)    # acgta against rc(tnca) = tgna
    a = cr.stretcher(ref, qry, True, (1, -1, 1, 1))
    assert cr.lines_of(ref, cr.revcomp(qry), a["ops"]) == (a["referenceLine"], a["editOps"], a["queryLine"])
    assert a["queryLine"].replace("-", "") == "tgna" and a["referenceLine"].replace("-", "") == "acgta"


def states_of(name):
    return [cr.STATE_NAMES[s] for s in cc.expected_of(name)[0]["state"]]


@pytest.mark.parametrize("crop", [0, 20])
def test_one_gap_of_every_state(crop):
    exp, ident, ops = cc.expected_of("states_crop_%d" % crop)
    assert states_of("states_crop_%d" % crop) == ["closed", "unclosed", "partiallyClosed", "closed", "broken", "broken", "unkown", "unkown", "unkown", "unkown",
                                                  "unkown", "ignored", "closed", "partiallyClosed", "ignored"]
    assert list(exp["align_status"][[0, 1, 2, 4, 11, 13]]) == [cr.OK, cr.NONE, cr.OK, cr.NONE, cr.NONE, cr.OK]
    assert exp["gap_length"][0] == 100 and exp["gap_length"][11] == 0 and exp["lhs_map"][6] == -1
    q = cr.Analyzer(**{k: cc.scene("states_crop_%d" % crop)[k] for k in ("true_seqs", "result_seqs", "mapped", "maps", "result_gap", "dust", "crop")})
    assert 4 in q.result_subseq((exp["result_begin_contig"][2], exp["result_begin"][2]), (exp["result_end_contig"][2], exp["result_end"][2]))
    assert ident[0] < 1.0 and ident[3] == 1.0 and math.isnan(ident[1])


def test_scenes_show_what_they_were_built_for():
    e = lambda n: cc.expected_of(n)
    assert states_of("complemented_contig") == ["closed", "closed", "ignored"] and list(e("complemented_contig")[0]["complement"]) == [1, 1, 0]
    assert states_of("complemented_partial")[0] == "partiallyClosed" and e("complemented_partial")[0]["complement"][0] == 1
    assert states_of("strands_differ")[0] == "broken"
    for n, lens in (("query_all_n", (60, 45)), ("query_empty", (60, 0)), ("reference_empty_gap_0", (0, 5))):
        s = e(n)[0][0]
        assert (s["state"], s["align_status"], s["reference_length"], s["query_length"]) == (cr.CLOSED, cr.EMPTY) + lens, n
        assert math.isnan(e(n)[1][0])
    s = e("query_all_n_crop")[0][0]   # with the crop flanks around them the n are aligned, and are no bases
    assert s["align_status"] == cr.OK and s["col_end"] - s["col_begin"] >= 60 and s["reference_length"] == 60 and s["query_length"] < 45
    s = e("query_with_n_inside")[0][0]
    assert s["align_status"] == cr.OK and s["query_length"] == s["reference_length"] - 7
    s, _, ops = e("gap_0_crop_insertions")
    assert s[0]["gap_length"] == 0 and s[0]["col_end"] - s[0]["col_begin"] == 5 and s[0]["reference_length"] == 0 and s[0]["query_length"] == 5
    assert list(ops[0][s[0]["col_begin"]:s[0]["col_end"]]) == [2] * 5
    s, _, ops = e("crop_bounds_move")
    assert list(ops[0][:3]) == [2, 2, 2] and list(ops[0][-3:]) == [2, 2, 2] and s[0]["col_begin"] == 13 and s[0]["col_end"] == len(ops[0]) - 13
    s = e("crop_is_the_whole_contig")[0]
    assert list(s["state"][:2]) == [cr.CLOSED, cr.CLOSED] and cc.scene("crop_is_the_whole_contig")["maps"][1]["ref_begin"] == cc.scene("crop_is_the_whole_contig")["maps"][1]["ref_end"]
    for crop in (0, 10):
        s, _, ops = e("columns_crop_%d" % crop)
        assert [len(o) - 2 * crop for o in ops[:7]] == [max(n - 2 * crop, 1) for n in (63, 64, 65, 260, 127, 128, 129)]
        assert [int(x) for x in (s["col_end"] - s["col_begin"])[:7]] == [max(n - 2 * crop, 1) for n in (63, 64, 65, 260, 127, 128, 129)]
    assert cc.scene("many_gaps")["count"] == 71 and (e("many_gaps")[0]["state"][:70] == cr.CLOSED).all()
    s = e("band_and_length")[0]
    assert list(s["align_status"]) == [cr.OK, cr.BAND_EXCEEDED, cr.OK, cr.TOO_LONG, cr.OK, cr.NONE] and (s["state"][:5] == cr.CLOSED).all()
    s = e("batch_in_the_middle")[0]
    assert len(s) == 4 and list(s["lhs_map"]) == [2, 3, 4, 5]
    assert states_of("last_contig_alone") == ["ignored"]


def test_dust_by_hand():
    s, _, ops = cc.expected_of("dust_at_insertions")
    # gap 1 is [500, 700): the 4 inserted bases stand in front of reference base 560; the dust interval [540, 560) ends there, so the
    # insertion columns (refPos 560, its left neighbour in the dust) count as dust: 20 + 4 ops, 20 matches at least
    assert s[0]["dust_ops"] == 24 and s[0]["dust_matches"] >= 20 and s[0]["dust_ops"] + s[0]["none_dust_ops"] == s[0]["col_end"] - s[0]["col_begin"]
    # gap 2 is [1100, 1300): the insertion stands in front of base 1160, where [1160, 1180) begins: 20 + 4 again
    assert s[1]["dust_ops"] == 24
    s = cc.expected_of("dust_edges")[0]
    # [450, 510) clipped to [500, 510), [560, 580) with the insertion in front of 560 (+ 4), [690, 700): 10 + 24 + 10
    assert s[0]["dust_ops"] == 44
    # [1100, 1101) and [1299, 1300): the first and the last gap base
    assert s[1]["dust_ops"] >= 2 and s[1]["dust_matches"] <= s[1]["dust_ops"]
    # [1650, 1720) touches the gap [1700, 1900) with 20 bases; [2400, 2500) lies outside
    assert 20 <= s[2]["dust_ops"] <= 24
    assert cc.expected_of("dust_but_partial")[0][0]["dust_ops"] == 0 and cc.expected_of("dust_but_partial")[0][0]["none_dust_ops"] == 0
    s = cc.expected_of("no_dust_mask")[0][0]
    assert (s["dust_ops"], s["none_dust_ops"]) == (0, 0) and s["matches"] > 0
    s = cc.expected_of("dust_crop_0")[0]
    assert s[0]["dust_ops"] + s[0]["none_dust_ops"] == s[0]["col_end"] and s[1]["none_dust_ops"] == 0 and s[1]["dust_ops"] == s[1]["col_end"]
