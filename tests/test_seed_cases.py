"""The constructed inputs of tests/seed_cases.py on the CPU oracle alone: every case does what its builder claims -- the
candidates worked out by hand are the oracle's, the ties exist, the cut drops candidates of the score it keeps, kept and
dropped flip at hmin = L and L + 1.  tests/test_parity_seedstage_gpu.py runs the same cases through dh_seed_candidates."""
import numpy as np
import pytest

import seed_cases as sc
from oracle import pyoracle as oz

FIELDS = ("score", "aseq", "apos", "bpos")
CASES = sc.all_cases()


def oracle_seeds(c, **kw):
    o = oz.default_opts(**dict(c["kw"], **kw))
    return oz.seed_candidates_all(c["A"], c["B"], o, with_nhits=True)


def rows(cand, ncand, it):
    return [tuple(int(cand[it][r][f]) for f in FIELDS) for r in range(ncand[it])]


def items_of(c, key, pred, ncand):
    """the items a case names under `key`; "some": the items the predicate holds for, at least one"""
    if c[key] == "some":
        found = [it for it in range(len(ncand)) if pred(it)]
        assert found, (c["name"], key)
        return found
    return list(c[key])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_case_does_what_it_claims(c):
    cand, ncand, nhits = oracle_seeds(c)
    assert len(ncand) == 2 * c["B"].n and (ncand <= c["kw"].get("max_cand", 32)).all()
    if c["none"]:
        assert not ncand.any()
    else:
        assert ncand.any()
    assert ((nhits == 0) <= (ncand == 0)).all()
    for it, exp in c["expect"].items():
        assert rows(cand, ncand, it) == exp, (c["name"], it)
    strands = c["kw"].get("strands", 3)
    for s in range(2):
        if not strands & (1 << s):
            assert not ncand[s::2].any() and not nhits[s::2].any()

    def has_tie(it):
        sc_ = sorted(int(cand[it][r]["score"]) for r in range(ncand[it]))
        return any(a == b for a, b in zip(sc_, sc_[1:]))
    for it in items_of(c, "ties", has_tie, ncand):
        assert has_tie(it), (c["name"], it)
    if c["cut"]:
        mc = c["kw"]["max_cand"]
        full, nfull, _ = oracle_seeds(c, max_cand=64)
        assert nfull.max() < 64

        def cut_in_a_tie(it):
            sc_ = sorted((int(full[it][r]["score"]) for r in range(nfull[it])), reverse=True)
            return nfull[it] > mc and sc_[mc - 1] == sc_[mc]
        for it in items_of(c, "cut", cut_in_a_tie, ncand):
            assert cut_in_a_tie(it) and ncand[it] == mc, (c["name"], it)
            # what is kept are the first max_cand by (score, band): a subset of the uncut list
            assert set(rows(cand, ncand, it)) < set(rows(full, nfull, it))
    if c["kw"].get("skip_self", 0) == 2:
        for it in range(len(ncand)):
            aseq = [int(cand[it][r]["aseq"]) for r in range(ncand[it])]
            assert aseq == sorted(aseq), (c["name"], it)


def test_hmin_flips_between_L_and_L_plus_1():
    for w in (6, 4, 8):
        kept = oracle_seeds(sc.by_name(f"lone_block_L40_h40_w{w}"))
        dropped = oracle_seeds(sc.by_name(f"lone_block_L40_h41_w{w}"))
        assert kept[1].tolist() == [1, 0, 0, 1] and not dropped[1].any()
        assert np.array_equal(kept[2], dropped[2]) and kept[2].sum() == 2 * (40 - sc.K + 1)
        assert all(int(kept[0][it][0]["score"]) == 40 for it in (0, 3))


def test_regrouping_by_partner_changes_the_order():
    """symmetric_units: an item's kept candidates by partner are not its kept candidates by score"""
    c = sc.by_name("symmetric_units_cut5_algo1")
    cand, ncand, _ = oracle_seeds(c)
    moved = 0
    for it in range(len(ncand)):
        s = [int(cand[it][r]["score"]) for r in range(ncand[it])]
        moved += s != sorted(s, reverse=True)
    assert moved >= 4


def test_sampled_steps_of_k_and_k_plus_1():
    c = sc.by_name("sampled_links_mod4")
    assert sc.K in c["steps"] and sc.K + 1 in c["steps"]
    cand, ncand, nhits = oracle_seeds(c)
    assert ncand.tolist() == [1, 0, 0, 1] and nhits[0] == nhits[3] > 100


def test_the_symmetric_rule_splits_the_pairs():
    """skip_self 2 sees each pair once, skip_self 1 both ways: half the hits"""
    one = oracle_seeds(sc.by_name("overlapping_reads_self1_strands3_algo1"))
    two = oracle_seeds(sc.by_name("overlapping_reads_self2_strands3_algo1"))
    assert 2 * two[2].sum() == one[2].sum()
    tandem = oracle_seeds(sc.by_name("overlapping_reads_self3_strands1_algo1"))
    assert tandem[1].tolist() == [1, 0] * 8
    for r in range(8):  # the second copy of the unit against the first: 200 below the main diagonal
        row = tandem[0][2 * r][0]
        assert row["aseq"] == r and row["apos"] - row["bpos"] == 200 and row["score"] >= 90
