"""The restatement of dh_la_repeat_mask's contract (tests/repeat_ref.py) against the reference's own vectors
(maskRepetitiveRegions.d:299-333, 402-410), against the per-base statement of the contract written out naively, and -- on units of
one record -- against the restatement the tests of dh_db_mask_coverage use (tests/mask_ref.py).  No GPU needed."""
import numpy as np
import pytest

import mask_ref
import repeat_cases as rc
import repeat_ref as rr


def test_reference_vector():
    exp = rc.expected(rc.reference_vector())
    assert exp["all"] == exp["mask"] == rc.REF_MASK_3_5 and exp["improper"] == [] and exp["units"] == 33
    none = rc.expected(rc.case(rc.REF_LENS, [], 3, 5))
    assert none["all"] == none["mask"] == []


def per_base(case):
    """the contract's per-base statement, one counter per base"""
    las, co, ro = case["las"], case["contig_off"], case["read_off"]
    lens = np.diff(co)
    cov = {"all": [np.zeros(n, np.int64) for n in lens], "improper": [np.zeros(n, np.int64) for n in lens]}
    counted = {"all": 0, "improper": 0}
    for i, e in rr.units_of(las):
        f, l = las[i], las[e]
        c = int(f["aread"])
        cov["all"][c][int(f["abpos"]):int(l["aepos"])] += 1
        counted["all"] += 1
        if case["improper"] is not None and not rr.is_proper(f, l, int(lens[c]), int(ro[f["bread"] + 1] - ro[f["bread"]]), case["allowance"]):
            cov["improper"][c][int(f["abpos"]):int(l["aepos"])] += 1
            counted["improper"] += 1
    out = {}
    for which, bounds in (("all", (case["lower"], case["upper"])), ("improper", case["improper"])):
        runs = []
        if bounds is not None and counted[which]:
            for c, v in enumerate(cov[which]):
                bad = np.concatenate([[0], ((v < bounds[0]) | (v > bounds[1])).astype(np.int8), [0]])
                edges = np.flatnonzero(np.diff(bad))
                runs += [(c, int(b), int(e)) for b, e in zip(edges[::2], edges[1::2])]
        out[which] = runs
    out["mask"] = rr.union(out["all"], out["improper"])
    return out


@pytest.mark.parametrize("name", list(rc.ALL))
def test_event_machine_equals_the_per_base_statement(name):
    exp, naive = rc.expected_of(name), per_base(rc.ALL[name])
    for which in ("all", "improper", "mask"):
        assert exp[which] == naive[which], (name, which)


@pytest.mark.parametrize("name", ["reference_vector", "edges", "one_base_ok_between_bad", "cov_equals_bounds", "gaps_lower_1"])
def test_single_record_units_equal_the_coverage_mask_restatement(name):
    """what the tests of dh_db_mask_coverage compare with (mask_ref.coverage_mask over the records' own intervals)"""
    case = rc.ALL[name]
    assert len(rr.units_of(case["las"])) == len(case["las"])
    lens = np.diff(case["contig_off"]).tolist()
    ivs = [(int(l["aread"]), int(l["abpos"]), int(l["aepos"])) for l in case["las"]]
    ptr, iv = mask_ref.coverage_mask(lens, ivs, case["lower"], case["upper"])
    assert rc.triples((ptr, iv)) == rc.expected_of(name)["all"]


def test_chain_cases_say_what_the_contract_says():
    c = rc.ALL
    assert rc.expected_of("gaps_covered")["all"] == [(0, 100, 700)]                      # the gaps are covered
    assert rc.expected_of("middle_sticks_out")["all"] == [(0, 100, 500)]                 # not beyond last.aepos
    assert rc.expected_of("next_after_change")["units"] == 4                             # bread, strand, START end a chain
    e = rc.expected_of("proper_whole_improper_members")
    assert e["units"] == 1 and e["improper_units"] == 0 and e["improper"] == []
    assert not any(rr.is_proper(l, l, 2000, rc.RLEN, 0) for l in c["proper_whole_improper_members"]["las"])
    e = rc.expected_of("improper_whole_proper_member")
    assert e["improper_units"] == 1 and e["improper"] == [(1, 500, 1200)]
    assert rr.is_proper(*[c["improper_whole_proper_member"]["las"][1]] * 2, 2000, rc.RLEN, 0)
    e = rc.expected_of("no_improper_unit")
    assert e["improper"] == [] and e["mask"] == e["all"] == [(0, 0, 500)]
    assert rc.expected_of("one_improper_unit")["improper"] == [(0, 0, 100), (0, 300, 500), (1, 0, 500)]
    e = rc.expected_of("touch_nest_interleave")
    assert e["mask"] == [(0, 100, 300), (0, 400, 500), (0, 600, 800)]
