"""The constructed pile-ups of consensus_cases.py on the CPU: the plain-Python restatement (consensus_ref.py) against the
oracle in bases and votes, known answers that need neither, what the oracle must not depend on, and a check that the named
cases tell six deliberately wrong implementations from a right one."""
import numpy as np
import pytest

import consensus_cases as cc
import consensus_ref as cr
from helpers import check_trace_invariants
from oracle import pyoracle as oz

NAMED = [cid for cid, fam, _ in cc.CASES if fam != "random"]


def tiles_of(cid):
    """(columns, B bases, diffs) of every tile of the voting overlaps of a case."""
    _, _, las, trace, ts = cc.built(cid)
    out = []
    for i in cc.voting(las, trace):
        la = las[i]
        a0 = int(la["abpos"])
        for d, b in trace[la["toff"]:la["toff"] + la["tlen"]].reshape(-1, 2):
            a1 = min((a0 // ts + 1) * ts, int(la["aepos"]))
            out.append((a1 - a0, int(b), int(d)))
            a0 = a1
    return out


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_python_reference_equals_the_oracle(family):
    for cid in cc.ids_of(family):
        tmpl, db, las, trace, ts = cc.built(cid)
        exp, exp_votes = cc.expected(cid)
        got, votes = cr.consensus(tmpl, db, las, trace, 0, ts)
        assert np.array_equal(votes, exp_votes), f"{cid}: vote table differs"
        assert np.array_equal(got, exp), f"{cid}: consensus differs"


def test_generated_records_are_self_consistent():
    for cid, _, _ in cc.CASES:
        tmpl, db, las, trace, ts = cc.built(cid)
        check_trace_invariants(las, trace, ts)
        assert db.n == len(las) + 1 and np.array_equal(db.seq(0), tmpl)
        assert len(trace) == int(las["tlen"].sum())
        for la in las:
            assert 0 <= la["abpos"] < la["aepos"] <= len(tmpl)
            assert 0 <= la["bbpos"] <= la["bepos"] <= db.length(int(la["bread"]))
            a0 = int(la["abpos"])
            for d, b in trace[la["toff"]:la["toff"] + la["tlen"]].reshape(-1, 2):
                a1 = min((a0 // ts + 1) * ts, int(la["aepos"]))
                assert int(d) >= abs(a1 - a0 - int(b))
                a0 = a1


def test_cases_reach_what_they_are_named_for():
    # band classes: the largest tile diffs sit where the name says, and every fill occurs
    cls = {cid: cc.band_classes(*cc.built(cid)[2:4]) for cid in cc.ids_of("band")}
    for target, c in ((29, 0), (30, 0), (31, 1), (61, 1), (62, 1), (63, 2), (240, 2)):
        _, _, las, trace, _ = cc.built(f"band-dmax{target}")
        assert int(trace[las[0]["toff"]:las[0]["toff"] + las[0]["tlen"]][0::2].max()) == target
        assert cls[f"band-dmax{target}"][c] > 0
    assert all(n > 0 for n in cls["band-mixed"])
    for n, c in ((30, 0), (31, 1), (62, 1), (63, 2), (90, 2)):   # a path n (n - 1) cells off the diagonal in a tile of n diffs
        for sub in (0, 1):
            for kind, nb in (("del", 100 - (n - sub)), ("ins", 100 + n - sub)):
                cid = f"band-edge-{kind}{n}" + "-sub" * sub
                assert tiles_of(cid).count((100, nb, n)) == 3 and cls[cid][c] == 9
    # launch edges: all tiles in the one class, as many as the name says
    for n in (1, 63, 64, 65):
        for c in range(3):
            exp = [0, 0, 0]
            exp[c] = n
            assert cc.band_classes(*cc.built(f"launch-{n}tiles-class{c}")[2:4]) == exp
    # tile sides
    for w in ("begin", "end", "first", "last"):
        assert any(t[0] == 1 for t in tiles_of(f"sides-one-column-{w}"))
    assert sum(t[:2] == (100, 0) for t in tiles_of("sides-empty-b")) == 3
    assert sum(t[1] == 250 for t in tiles_of("sides-b250")) == 3
    _, _, las, trace, _ = cc.built("sides-b251")
    assert int(trace[1::2].max()) == 251 and len(cc.voting(las, trace)) == 1
    # the three vote kernels, both sides of their borders
    assert [cc.vote_kernel(ts) for ts in cc.TSPACES] == [13, 13, 13, 16, 16, 0, 0, 0]
    assert {cc.built(cid)[4] for cid in cc.ids_of("tspace")} == set(cc.TSPACES)
    # insertions land on the tile boundary, on the side the spec asks for
    for side, tile in (("next", 1), ("prev", 0)):
        _, _, las, trace, _ = cc.built(f"ins-4-foreign-slot0-{side}")
        for la in las:
            assert int(trace[la["toff"] + 2 * tile + 1]) == 104
    # random piles: every trace spacing, every fill, both strands, empty piles
    seen, fills, flags, depth = set(), [0, 0, 0], 0, set()
    for cid in cc.ids_of("random"):
        _, _, las, trace, ts = cc.built(cid)
        seen.add(ts)
        fills = [x + y for x, y in zip(fills, cc.band_classes(las, trace))]
        flags |= int(np.bitwise_or.reduce(las["flags"])) if len(las) else 0
        depth.add(len(las))
    assert seen == set(cc.TSPACES) and all(fills) and flags & cc.COMP and flags & cc.DISABLED and {0, 12} <= depth


def apply(tmpl, edits):
    return cc.edited(tmpl, 0, len(tmpl), edits)


def keeps_the_template(cid):
    """The named cases whose consensus is the template by design."""
    p = cid.split("-")
    if p[0] == "ties":            # no overlap; carriers below the majority (see the ladder test)
        if p[1] not in ("sub", "del", "ins"):
            return cid == "ties-no-overlap"
        k, d = (int(x) for x in p[2].split("of"))
        return not (2 * k >= d + 1 if p[1] == "del" else 2 * k > d + 1)
    if p[0] == "ins" and "template-end" in cid:   # the slot behind the template's last column is never emitted; only a
        return p[2] == "foreign" or int(p[1]) > cc.MAXINS    # run of up to MAXINS copies of the last base joins its run
    # more than SEG_MAX B bases: the exact read alone; a run longer by more than MAXINS is no vote; N in reads is no vote
    return cid in ("sides-b251", "homo-single+6") or cid.startswith("codes-n-reads")


def test_named_cases_show_their_edits():
    """Every enabled record of the template votes (but for the three reads of sides-b251), and the consensus differs from
    the template unless the case is about keeping it: a wrong alignment, placement or vote has bases to show in."""
    for cid in NAMED:
        tmpl, _, las, trace, _ = cc.built(cid)
        enabled = int(((las["aread"] == 0) & ((las["flags"] & cc.DISABLED) == 0)).sum())
        assert len(cc.voting(las, trace)) == (1 if cid == "sides-b251" else enabled), cid
        assert np.array_equal(cc.expected(cid)[0], tmpl) == keeps_the_template(cid), cid
    # the launch edges: every tile carries an edit, all of them win
    for n in (1, 63, 64, 65):
        tmpl, edits, _ = cc.launch_parts(n)
        for c in range(3):
            assert np.array_equal(cc.expected(f"launch-{n}tiles-class{c}")[0], apply(tmpl, edits)), (n, c)


def test_most_random_piles_show_edits():
    """The piles are seeded, so these are counts, not chances: 22 of the 150 have no voting record (no overlap drawn, or all
    disabled or beyond SEG_MAX) and 12 more keep the template.  A change of the generator that empties more of them, or
    turns more of them into the template, is a loss of coverage."""
    ids = cc.ids_of("random")
    empty = sum(len(cc.voting(*cc.built(cid)[2:4])) == 0 for cid in ids)
    same = sum(np.array_equal(cc.expected(cid)[0], cc.built(cid)[0]) for cid in ids)
    assert empty <= 22 and same <= 34, (empty, same)


@pytest.mark.parametrize("kind,dmin", [("sub", 2), ("del", 1), ("ins", 2)])
def test_known_answer_every_read_carries_one_edit(kind, dmin):
    for d in range(dmin, 6):
        tmpl, db, las, trace, ts = cc.built(f"ties-{kind}-{d}of{d}")
        _, e = cc.tie_parts(kind, d, d)
        assert np.array_equal(cc.expected(f"ties-{kind}-{d}of{d}")[0], apply(tmpl, [e])), (kind, d)


@pytest.mark.parametrize("delta", [-2, 2])
def test_known_answer_run_over_a_tile_boundary(delta):
    tmpl, e = cc.homo_parts("boundary", delta)
    for d in (3, 4, 7):
        for side in ("next", "prev"):
            db, las, trace = cc.pile(tmpl, cc.carriers(tmpl, e, d, d, ins_side=side), 100)
            assert np.array_equal(oz.consensus(tmpl, db, las, trace, 0, 100), apply(tmpl, e)), (d, side)


def test_known_answer_ladder_goes_to_the_template_on_ties():
    """k carriers among d reads, the template has no runs.  A substitution needs more votes than the template base, which
    has the template's own vote: k > d - k + 1.  A foreign insertion needs 2 k > d + 1.  A deletion shortens the run of one
    column by round(k / (d + 1)), halves rounded up: 2 k >= d + 1."""
    for kind in ("sub", "del", "ins"):
        for d in range(1, 6):
            for k in range(d + 1):
                tmpl, e = cc.tie_parts(kind, d, k)
                wins = 2 * k >= d + 1 if kind == "del" else 2 * k > d + 1
                assert np.array_equal(cc.expected(f"ties-{kind}-{k}of{d}")[0], apply(tmpl, [e]) if wins else tmpl), (kind, d, k)


@pytest.mark.parametrize("cid", ["band-mixed", "tspace-16", "tspace-126", "tspace-250", "ignore-order1", "space-257", "random-3",
                                 "random-12", "random-77", "random-140"])
def test_oracle_ignores_slack_and_record_order(cid):
    tmpl, specs, ts = next(fn for i, _, fn in cc.CASES if i == cid)()
    exp, exp_votes = cc.expected(cid)
    rng = np.random.default_rng(5)
    for slack in (1, 17, 64, 300):
        other = [dict(s, slack=s["slack"] + slack) for s in specs]
        other = [other[i] for i in rng.permutation(len(other))]
        db, las, trace = cc.pile(tmpl, other, ts)
        got, votes = oz.consensus(tmpl, db, las, trace, 0, ts, want_votes=True)
        assert np.array_equal(got, exp) and np.array_equal(votes, exp_votes), slack


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_named_cases_catch_a_wrong_implementation(mutant):
    """Each deliberate error of the Python reference changes the consensus bases of at least one named case."""
    for cid in NAMED:
        tmpl, db, las, trace, ts = cc.built(cid)
        if not np.array_equal(cr.consensus(tmpl, db, las, trace, 0, ts, mutate=mutant)[0], cc.expected(cid)[0]):
            return
    pytest.fail(f"no named case tells the mutant {mutant} from the oracle")
