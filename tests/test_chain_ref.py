"""The restatement of the chaining contract (tests/chain_ref.py): the hand-worked cases of tests/chain_cases.py, whose
expected chains are written out there, and the random shapes against oracle.process.chain_pile_las as the multiset of
(record fields, chain flags) -- the oracle leaves the records in place, so only the multiset compares.  No GPU needed."""
from collections import Counter

import numpy as np
import pytest

import chain_cases as cc
import chain_ref as cr

FIELDS = ("aread", "bread", "abpos", "aepos", "bbpos", "bepos")


@pytest.mark.parametrize("name", list(cc.HAND))
def test_hand_worked_cases(name):
    las, opts, expected = cc.HAND[name]
    assert cr.chain(las, **opts) == expected


def test_hand_cases_in_one_input_keep_pair_order():
    names = list(cc.HAND)
    parts, expected, base = [], [], 0
    for k, name in enumerate(names):
        las, opts, exp = cc.HAND[name]
        if opts:
            continue
        las = las.copy()
        las["bread"] = 10 + k
        parts.append(las)
        expected += [([base + i for i in idx], fl, sc) for idx, fl, sc in exp]
        base += len(las)
    assert cr.chain(np.concatenate(parts)) == expected


def test_unordered_input_names_the_record():
    las = cc.random_case(seed=3, sizes=(3, 9), reps=1)
    bad = las.copy()
    bad[-1]["aread"] = -1 + int(bad[0]["aread"])
    bad[-1]["flags"] &= ~np.uint32(cc.DISABLED)
    with pytest.raises(cr.Unordered) as e:
        cr.chain(bad)
    assert e.value.index == len(bad) - 1


def multiset(las, rows, flags):
    return Counter(tuple(int(las[i][f]) for f in FIELDS) + (int(fl),) for i, fl in zip(rows, flags))


@pytest.mark.parametrize("rel,min_score", cc.OPTION_SETS)
def test_random_shapes_equal_the_oracle_as_multisets(rel, min_score):
    from oracle import process as pr
    las = cc.random_case(seed=11)
    chains = cr.chain(las, **cc.opts_of(rel, min_score))
    _, _, src, flags = cr.arrays(chains)
    exp = pr.chain_pile_las(las, min_rel_score=rel, min_score=min_score)
    keep = [i for i in range(len(exp)) if not exp[i]["flags"] & cc.DISABLED]
    assert multiset(las, src, flags) == multiset(exp, keep, [exp[i]["flags"] for i in keep])
    # the case reaches the hard paths: alternate chains, records shared between chains, rejected chains
    n_alt = sum(1 for c in chains if not c[1][0] & cc.BEST)
    if rel < 1.0:
        assert n_alt > 0 and len(src) > len(set(src.tolist()))
    enabled = int((~las["flags"] & cc.DISABLED).astype(bool).sum())
    assert 0 < len(set(src.tolist())) <= enabled
    if rel == 1.0:
        assert len(set(src.tolist())) < enabled


def test_every_chain_is_a_path_of_chainable_records():
    las = cc.random_case(seed=11)
    for idx, flags, score in cr.chain(las, min_relative_score=0.0):
        assert flags[0] & cc.START and all(f & cc.NEXT and not f & cc.START for f in flags[1:])
        for i, j in zip(idx, idx[1:]):
            assert las[i]["abpos"] < las[j]["abpos"] and las[i]["bbpos"] < las[j]["bbpos"]
            assert (las[i]["flags"] & cc.COMP) == (las[j]["flags"] & cc.COMP)
