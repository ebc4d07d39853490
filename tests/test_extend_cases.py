"""What tests/extend_cases.py claims about its inputs, shown on the CPU oracle (oz.extend_candidates and its attempts log):
the states every case expects of its candidate slots, its further claims (boxes, counts), and for every pair of cases on
the two sides of a rule that the two differ in records or counters -- a kernel with that rule off by one fails one half.
tests/test_parity_extendstage_gpu.py runs the same cases through dh_extend_candidates, tests/test_extend_cases_host.py the
DH-2 ones through the lane code on the host."""
import numpy as np
import pytest

import extend_cases as ec
from helpers import check_trace_invariants, la_rows
from oracle import pyoracle as oz

CASES = ec.all_cases()
BY_NAME = ec.by_name()
STATE = {0: "not reached", 1: "covered", 2: "rejected", 3: "accepted"}


def test_every_rule_has_cases_on_both_sides():
    rules = {}
    for c in CASES:
        rules.setdefault(c["rule"], []).append(c)
    assert len(rules) >= 20
    with_pairs = {r for r, cs in rules.items() if any(c["pair"] for c in cs)}
    for needle in ("covered rule: box", "covered rule: excursion", "covered rule: the k-th", "acceptance: min_len", "acceptance: error",
                   "x-drop", "DH-1: dmax", "DH-1: width", "DH-1: N against", "DH-2: one indel"):
        assert any(r.startswith(needle) for r in with_pairs), needle
    for needle in ("attempt cap and max_la", "symmetric: pflags"):
        assert any(r.startswith(needle) for r in with_pairs), needle
    # every width of the list with a pair for either direction (the builder drops a direction whose search finds no flip)
    sides = {(c["kw"]["width"], c["name"].split("-")[1][:3]) for c in CASES if c["rule"].startswith("DH-1: width") and c["pair"]}
    assert sides == {(w, s) for w in (1, 2, 5, 14, 15, 30, 31, 62) for s in ("ins", "del")}


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_claims_hold_on_the_oracle(c):
    r = ec.oracle(c)
    nitems = 2 * c["B"].n
    assert c["cand"].shape == (nitems, c["kw"]["max_cand"]) and r.stats[0] == 0 and r.stats[1] == c["ncand"].sum()
    for (item, slot), states in c["expect"].items():
        got = r.a(item, slot, "state")
        assert got in states, f"{c['name']}: item {item} slot {slot} is {STATE[got]}, the case expects {sorted(STATE[s] for s in states)}"
    state = r.att[:, :, 0]
    live = np.arange(state.shape[1])[None, :] < c["ncand"][:, None]
    assert not state[~live].any(), "no state behind the last candidate"
    assert r.stats[2] == int((state >= 2).sum()) and r.stats[3] == int(r.att[:, :, 8].sum())
    real = r.las[r.las["aepos"] > r.las["abpos"]]   # (a zero-length record has no trace pair)
    check_trace_invariants(real, r.trace, c["kw"]["tspace"])
    assert (r.las["tlen"][r.las["aepos"] == r.las["abpos"]] == 0).all()
    if c["check"]:
        c["check"](r)
    if c["pair"]:
        p = BY_NAME[c["pair"]]
        assert p["pair"] == c["name"]
        q = ec.oracle(p)
        mine = (la_rows(r.las, r.trace), int(r.stats[2]), int(r.stats[3]))
        theirs = (la_rows(q.las, q.trace), int(q.stats[2]), int(q.stats[3]))
        assert mine != theirs, f"{c['name']} and {p['name']} stand on the two sides of a rule and give the same result"


@pytest.mark.parametrize("algo,width,strands", [(1, 64, 3), (0, 62, 3), (0, 30, 1)])
def test_extend_of_seed_candidates_is_align_db(algo, width, strands):
    """the lifted loop is the loop: oz.extend_candidates on the oracle's own seeds gives oz.align_db's records and counters"""
    from dentist_amd import sim
    w = sim.Workload(60_000, 2, 40, 3000, seed=17, spacing=10000, gap_max=500)
    o = oz.default_opts(algo=algo, width=width, strands=strands)
    exp_las, exp_trace, exp_stats = oz.align_db(w.contigs, w.reads, o, nthreads=2, sort=False)
    cand, ncand = oz.seed_candidates_all(w.contigs, w.reads, o)
    las, trace, stats, att = oz.extend_candidates(w.contigs, w.reads, o, cand, ncand)
    assert len(exp_las) > 15 and la_rows(las, trace) == la_rows(exp_las, exp_trace)
    assert tuple(stats[1:]) == tuple(exp_stats[1:]) and stats[0] == 0
    assert int((att[:, :, 0] >= 2).sum()) == exp_stats[2]
