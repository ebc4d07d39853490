"""The three pile-up readers of the scaffold graph (dh_scaffold_spanning, dh_scaffold_gap_pileups,
dh_scaffold_all_pileups) against a restatement in Python that derives every view from the builder's own result
(dentist_amd.scaffold_pileups: joins, entries) and the LA records: which joins qualify, the index bounds, the flank and
complement rule, the (read, LA, LA) layout with -1, the stable order by read, the node order of the all-joins view and
the skipped count.  CPU only.  Inputs: the seeded random mappings of test_scaffold.py and one constructed mapping with
the kinds of join those lack (anti-parallel, contig-skipping with a complement clash, a lone extension); the sharded
`only_joins` plan is checked against the single-rank all-joins view on the constructed mapping."""
import collections
import functools

import numpy as np
import pytest

import dentist_amd
from dentist_amd._lib import ShardPlan, shard_read_joins
from oracle import scaffold as sc
from test_scaffold import _oracle_piles, _product_piles, _random_mapping, _to_arrays

FRONT, BACK = sc.FRONT, sc.BACK
PRE, BEGIN, END, POST = sc.PRE, sc.BEGIN, sc.END, sc.POST
COMP = 1
RANDOM_OPTS = [dict(), dict(min_spanning_reads=1, best_pile_up_margin=1.0, existing_gap_bonus=1.0),
               dict(merge_extensions=False, min_spanning_reads=2)]
CONSTRUCTED_OPTS = dict(min_spanning_reads=1, best_pile_up_margin=1.0, existing_gap_bonus=1.0)
ADJACENT = [("spanning", dict(with_extensions=False)), ("gap", dict(with_extensions=True))]
ONLY = {"spanning": 1, "extending": 2, "both": 3}


def _constructed():
    """4 contigs of 5 000: reads 1-3 join (1, end) and (3, end) anti-parallel; reads 4-6 join (2, end) and (4, begin) over
    contig 3, read 6 with complement flags that differ; read 7 extends contig 4 at its back."""
    rows = []
    for r in (1, 2, 3):
        rows += [(1, 5000, r, 4000, False, 4000, 5000, 0, 1000), (3, 5000, r, 4000, True, 4000, 5000, 500, 1500)]
    for r in (4, 5):
        rows += [(2, 5000, r, 4000, False, 4000, 5000, 0, 1000), (4, 5000, r, 4000, False, 0, 1000, 2500, 3500)]
    rows += [(2, 5000, 6, 4000, False, 4000, 5000, 0, 1000), (4, 5000, 6, 4000, True, 0, 1000, 500, 1500),
             (4, 5000, 7, 3000, False, 4200, 5000, 100, 900)]
    return [sc.chain(i, *row) for i, row in enumerate(rows)], [], 4


@functools.lru_cache(maxsize=None)
def _case(seed, oi):
    """(chains, 1-based input gaps, contigs, options, las, contig_off, read_off, 0-based gaps, joins, entries); seed 0 = the
    constructed mapping.  Built once per case and shared: nothing below writes to it."""
    chains, input_gaps, nc = _random_mapping(seed) if seed else _constructed()
    opts = RANDOM_OPTS[oi] if seed else CONSTRUCTED_OPTS
    las, co, ro = _to_arrays(chains)
    if nc > len(co) - 1:
        co = np.concatenate([co, co[-1] + np.arange(1, nc - (len(co) - 1) + 1)])
    gaps = np.array(input_gaps, dtype=np.int32).reshape(-1, 2) - 1
    joins, ent = dentist_amd.scaffold_pileups(las, co, ro, gaps, **opts)
    return chains, input_gaps, nc, opts, las, co, ro, gaps, joins, ent


CASES = [(0, 0)] + [(seed, oi) for oi in range(len(RANDOM_OPTS)) for seed in (1, 2, 3, 4, 5, 6)]


# ------------------------------------------------------------------ the model
def _model(joins, ent, las, adjacent, only, one_la, seen=None):
    """(nodes4, counts, triples, skipped) of one view.  adjacent: gap joins (c, end) -- (c + 1, begin) of type gap only;
    else the gap joins of any two contig ends (only & 1) and the extension joins (only & 2).  one_la: keep entries of one
    LA.  seen (a Counter): what the input contained."""
    seen = collections.Counter() if seen is None else seen
    n, piles, skipped = len(las), [], 0
    for j in joins:
        c0, p0, c1, p1 = (int(j[k]) for k in ("contig0", "part0", "contig1", "part1"))
        gap = p0 in (BEGIN, END) and p1 in (BEGIN, END) and c0 != c1
        ext = c0 == c1 and (p0, p1) in ((PRE, BEGIN), (END, POST))
        if adjacent:
            ok = j["type"] == 1 and (p0, p1) == (END, BEGIN) and c1 == c0 + 1
        else:
            ok = bool((gap and only & 1) or (ext and only & 2))
        s0 = (FRONT if p0 == BEGIN else BACK) if gap else (FRONT if p0 == PRE else BACK)
        s1 = (FRONT if p1 == BEGIN else BACK) if gap else FRONT
        seen["non_adjacent_gap"] += gap and c1 != c0 + 1
        seen["adjacent_other_ends"] += gap and c1 == c0 + 1 and (p0, p1) != (END, BEGIN)   # e.g. (c, begin) -- (c + 1, end)
        seen["anti_parallel"] += gap and s0 == s1
        seen["extension_join"] += ext

        def flank(la, seed):
            if las[la]["aread"] == c0 and seed == s0:
                return 0
            return 1 if gap and las[la]["aread"] == c1 and seed == s1 else -1
        t = []
        for e in ent[j["first"]:j["first"] + j["count"]] if ok else ():
            rd, a, b = int(e["read"]), int(e["la0"]), int(e["la1"])
            if not 0 <= a < n or (e["n"] == 2 and not 0 <= b < n):
                continue
            f0 = flank(a, e["seed0"])
            if e["n"] == 2:
                f1 = flank(b, e["seed1"])
                if f0 < 0 or f1 < 0 or f0 == f1:
                    continue
                if ((las[a]["flags"] & COMP) == (las[b]["flags"] & COMP)) != (s0 != s1):   # parallel: equal flags
                    seen["complement_dropped"] += 1
                    continue
                t.append((rd, a, b) if f0 == 0 else (rd, b, a))
            elif one_la and f0 >= 0:
                seen["adjacent_one_la"] += adjacent
                t.append((rd, a, -1) if f0 == 0 else (rd, -1, a))
        t.sort(key=lambda x: x[0])   # stable: entries of one read keep the builder's order
        if t:
            piles.append(((c0, s0, c1 if gap else -1, s1), t))
        else:
            skipped += 1
    if not adjacent:   # node order, "no second contig" last
        piles.sort(key=lambda p: (p[0][0], p[0][1], p[0][2] if p[0][2] >= 0 else 2 ** 31 - 1, p[0][3]))
    tri = np.array([x for _, t in piles for x in t], dtype=np.int32).reshape(-1, 3)
    return [p[0] for p in piles], [len(p[1]) for p in piles], tri, skipped


def _assert_equal(p, skipped, model):
    nodes, cnt, tri, mskipped = model
    cl, pcnt, ptri = p.flat()
    assert skipped == mskipped
    assert cl.tolist() == [nd[0] for nd in nodes] and pcnt.tolist() == cnt
    assert np.array_equal(ptri.reshape(-1, 3), tri)
    assert [p.get_join(i) for i in range(len(p))] == nodes


# ------------------------------------------------------------------ library == model
@pytest.mark.parametrize("name,kw", ADJACENT)
@pytest.mark.parametrize("seed,oi", CASES)
def test_adjacent_gap_views_equal_the_model(seed, oi, name, kw):
    _, _, _, opts, las, co, ro, gaps, joins, ent = _case(seed, oi)
    p, skipped = dentist_amd.scaffold_spanning_pileups(las, co, ro, gaps, **kw, **opts)
    _assert_equal(p, skipped, _model(joins, ent, las, True, 0, kw["with_extensions"]))


@pytest.mark.parametrize("only", list(ONLY))
@pytest.mark.parametrize("seed,oi", CASES)
def test_all_joins_view_equals_the_model(seed, oi, only):
    _, _, _, opts, las, co, ro, gaps, joins, ent = _case(seed, oi)
    p, skipped = dentist_amd.scaffold_all_pileups(las, co, ro, gaps, only=only, **opts)
    _assert_equal(p, skipped, _model(joins, ent, las, False, ONLY[only], True))


# ------------------------------------------------------------------ the inputs are what they claim to be
def test_constructed_mapping_yields_the_joins_it_was_built_for():
    chains, input_gaps, nc, opts, las, co, ro, gaps, joins, ent = _case(0, 0)
    assert _product_piles(chains, input_gaps, nc=nc, **opts) == _oracle_piles(chains, input_gaps, nc, **opts)
    nodes, cnt, _, skipped = _model(joins, ent, las, False, 3, True)
    assert nodes == [(0, 1, 2, 1), (1, 1, 3, 0), (3, 1, -1, 0)] and cnt == [3, 2, 1] and skipped == 0
    assert _model(joins, ent, las, False, 1, True)[3] == 1 and _model(joins, ent, las, False, 2, True)[3] == 2
    for one_la in (False, True):
        assert _model(joins, ent, las, True, 0, one_la)[:2] == ([], []) and _model(joins, ent, las, True, 0, one_la)[3] == 3
    assert [int(j["count"]) for j in joins] == [3, 3, 1]   # the contig-skipping join holds three entries, the views keep two


def test_inputs_hold_every_kind_of_join_and_entry():
    seen = collections.Counter()
    for seed, oi in CASES:
        _, _, _, _, las, _, _, _, joins, ent = _case(seed, oi)
        per = collections.Counter()
        _model(joins, ent, las, True, 0, True, per)
        _model(joins, ent, las, False, 3, True, per)
        if seed == 0:   # only the constructed mapping has these two
            assert per["anti_parallel"] > 0 and per["complement_dropped"] > 0
        seen += per
    for kind in ("adjacent_one_la", "non_adjacent_gap", "adjacent_other_ends", "anti_parallel", "complement_dropped", "extension_join"):
        assert seen[kind] > 0, kind


# ------------------------------------------------------------------ the sharded only_joins plan
def test_sharded_only_joins_plan_equals_the_all_joins_view():
    """dh_shard_read_joins of two ranks (reads split 4 / 3) -> dh_shard_graph_plan_create with only_joins = 3: the same
    pile-ups as dh_scaffold_all_pileups of the whole mapping.  The plan's records are its own array, so an entry is
    compared by the records it names."""
    _, _, nc, opts, las, co, ro, gaps, _, _ = _case(0, 0)
    single, skipped = dentist_amd.scaffold_all_pileups(las, co, ro, gaps, only="both", **opts)
    nreads = len(ro) - 1
    blobs = []
    for lo, hi in ((0, 4), (4, nreads)):
        mine = np.ascontiguousarray(las[(las["bread"] >= lo) & (las["bread"] < hi)])
        blobs.append(shard_read_joins(mine, co, ro[lo:hi + 1] - ro[lo], lo))
    po = dentist_amd.default_process_opts(min_reads=1, max_reads=0)   # the cut keeps every pile-up
    plan = ShardPlan(blobs, po, graph=(nc, None, dict(opts, only_joins=3)))

    def content(p, recs):
        fields = ("bread", "aread", "abpos", "aepos", "bbpos", "bepos", "flags")
        rec = lambda i: None if i < 0 else tuple(int(recs[i][f]) for f in fields)   # noqa: E731
        _, cnt, tri = p.flat()
        return ([p.get_join(i) for i in range(len(p))], cnt.tolist(),
                [(int(rd), rec(a), rec(b)) for rd, a, b in tri.reshape(-1, 3)])
    got, exp = content(plan.piles, plan.las), content(single, las)
    plan.close()
    assert skipped == 0 and exp[1] == [3, 2, 1]
    assert got == exp
