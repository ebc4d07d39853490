"""dh_pileups_from_db, the inverse of dh_pileups_write_db: pile-ups.db back into pile-ups ordered by node, the records of
their chains and the trace values.  Round trips of every kind of join, a file whose pile-ups are not in node order (file_index
and a first / count selection in file order), an entry stored right flank first, a chain of three local alignments against
what las_read yields for the same chain, the reference's own chain fixture, and every refusal by its message.  CPU only
(host code)."""
import json
import os

import numpy as np
import pytest

import dentist_amd
from dentist_amd import DhError, Pileups, pileupdb_read, pileupdb_write, pileups_from_db

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TS = 100
FRONT, BACK = 0, 1
COMP, START, NEXT, BEST = 0x1, 0x4, 0x8, 0x10
CONTIG_LEN = [5000, 6000, 7000, 4000]
READ_LEN = [3000 + 10 * i for i in range(12)]
CONTIG_OFF = np.concatenate([[0], np.cumsum(CONTIG_LEN)]).astype(np.int64)
READ_OFF = np.concatenate([[0], np.cumsum(READ_LEN)]).astype(np.int64)
FIELDS = ("tlen", "diffs", "abpos", "bbpos", "aepos", "bepos", "flags", "aread", "bread")


class World:
    """records with consistent traces, built one by one"""

    def __init__(self):
        self.las, self.trace = [], []

    def la(self, aread, bread, abpos, aepos, bbpos, comp=False, flags=0):
        cuts = [abpos] + [x for x in range((abpos // TS + 1) * TS, aepos, TS)] + [aepos]
        seg = np.diff(cuts)
        b = seg.copy()
        b[0] += 1  # one insertion in the first tile
        tr = np.stack([np.ones(len(seg), np.int64), b], axis=1).reshape(-1)
        rec = np.zeros(1, dentist_amd.LA_DTYPE)[0]
        rec["tlen"], rec["diffs"] = len(tr), len(seg)
        rec["abpos"], rec["aepos"], rec["bbpos"], rec["bepos"] = abpos, aepos, bbpos, bbpos + int(b.sum())
        rec["flags"] = (COMP if comp else 0) | flags
        rec["aread"], rec["bread"] = aread, bread
        rec["toff"] = len(self.trace)
        self.trace += [int(x) for x in tr]
        self.las.append(rec)
        return len(self.las) - 1

    def arrays(self):
        return np.array(self.las, dtype=dentist_amd.LA_DTYPE), np.array(self.trace, np.uint16)


def back_of(w, c, rd, comp=False):
    """an alignment that reaches the end of contig c"""
    return w.la(c, rd, CONTIG_LEN[c] - 1234, CONTIG_LEN[c], 17, comp)


def front_of(w, c, rd, comp=False):
    return w.la(c, rd, 0, 1111, 1500, comp)


def build_world():
    """five pile-ups in node order: a join that skips contigs, a plain gap, an anti-parallel join, an extension pile-up and a
    gap pile-up with extension entries on either side"""
    w = World()
    nodes, triples = [], []
    nodes.append((0, FRONT, 3, FRONT))
    triples.append([(r, front_of(w, 0, r, True), front_of(w, 3, r)) for r in (0, 1)])
    nodes.append((0, BACK, 1, FRONT))
    triples.append([(r, back_of(w, 0, r), front_of(w, 1, r)) for r in (2, 3, 4)])
    nodes.append((1, BACK, 2, BACK))
    triples.append([(r, back_of(w, 1, r), back_of(w, 2, r, True)) for r in (5, 6)])
    nodes.append((2, FRONT, -1, 0))
    triples.append([(r, front_of(w, 2, r), -1) for r in (7, 8)])
    nodes.append((2, BACK, 3, FRONT))
    triples.append([(9, back_of(w, 2, 9), front_of(w, 3, 9)), (10, back_of(w, 2, 10), -1), (11, -1, front_of(w, 3, 11))])
    las, trace = w.arrays()
    return nodes, triples, las, trace


def write_world(path, nodes, triples, las, trace):
    p = Pileups.from_joins(nodes, triples)
    p.write_db(path, las, trace, CONTIG_OFF, READ_OFF, TS)


def split_piles(path):
    """the container as nested lists: piles -> read alignments -> (seeded record, [(la record, trace values)])"""
    d = pileupdb_read(path)
    piles, ra, si, li, ti = [], 0, 0, 0, 0
    for npc in d["pile_counts"]:
        pile = []
        for _ in range(npc):
            entry = []
            for _ in range(d["ra_counts"][ra]):
                s = d["seeded"][si].copy()
                si += 1
                chain = []
                for _ in range(s["nla"]):
                    l = d["las"][li].copy()
                    li += 1
                    chain.append((l, d["trace"][ti:ti + 2 * l["ntp"]].copy()))
                    ti += 2 * l["ntp"]
                entry.append((s, chain))
            ra += 1
            pile.append(entry)
        piles.append(pile)
    return piles


def write_piles(path, piles):
    pc, rc, sa, la, tp = [], [], [], [], []
    for pile in piles:
        pc.append(len(pile))
        for entry in pile:
            rc.append(len(entry))
            for s, chain in entry:
                s = s.copy()
                s["nla"] = len(chain)
                sa.append(s)
                for l, t in chain:
                    l = l.copy()
                    l["ntp"] = len(t) // 2
                    la.append(l)
                    tp += [int(x) for x in t]
    pileupdb_write(path, np.array(pc, np.int32), np.array(rc, np.int32), np.array(sa, dtype=dentist_amd.SEEDED_DTYPE),
                   np.array(la, dtype=dentist_amd.CHAIN_LA_DTYPE), np.array(tp, np.uint16))


def same_record(a, b):
    return all(a[f] == b[f] for f in FIELDS)


def check_against(nodes, triples, las, trace, got, order=None):
    """got = pileups_from_db(...): the joins, read ids, record fields and trace values of the original pile-ups `order`"""
    piles, las2, trace2, ts, file_index = got
    order = list(range(len(nodes))) if order is None else order
    assert ts == TS and len(piles) == len(order)
    for i, src in enumerate(order):
        assert piles.get_join(i) == tuple(nodes[src]), (i, src)
        _, tri = piles.get(i)
        assert len(tri) == len(triples[src])
        for t2, t1 in zip(tri, triples[src]):
            assert t2[0] == t1[0]
            for side in (1, 2):
                assert (t2[side] < 0) == (t1[side] < 0)
                if t1[side] >= 0:
                    a, b = las[t1[side]], las2[t2[side]]
                    assert same_record(a, b), (a, b)
                    assert np.array_equal(trace[a["toff"]:a["toff"] + a["tlen"]], trace2[b["toff"]:b["toff"] + b["tlen"]])


def test_round_trip_of_every_kind_of_join(tmp_path):
    nodes, triples, las, trace = build_world()
    path = str(tmp_path / "pile-ups.db")
    write_world(path, nodes, triples, las, trace)
    got = pileups_from_db(path, 0, -1, CONTIG_OFF)
    check_against(nodes, triples, las, trace, got)
    assert list(got[4]) == [0, 1, 2, 3, 4]
    # every chain is one record: no chain flag, records in file order, every record named once
    assert not (got[1]["flags"] & (START | NEXT | BEST)).any()
    assert len(got[1]) == len(las) and np.array_equal(np.sort(got[1]["toff"]), got[1]["toff"])


def test_file_order_differs_from_node_order(tmp_path):
    nodes, triples, las, trace = build_world()
    path, shuffled = str(tmp_path / "sorted.db"), str(tmp_path / "shuffled.db")
    write_world(path, nodes, triples, las, trace)
    piles = split_piles(path)
    perm = [3, 0, 4, 2, 1]  # file position -> pile-up of the world
    write_piles(shuffled, [piles[k] for k in perm])
    got = pileups_from_db(shuffled, 0, -1, CONTIG_OFF)
    check_against(nodes, triples, las, trace, got)
    assert [perm[f] for f in got[4]] == [0, 1, 2, 3, 4]
    # the selection is made in file order, before the ordering by node: file entries 1..3 are pile-ups 0, 4, 2
    got = pileups_from_db(shuffled, 1, 3, CONTIG_OFF)
    check_against(nodes, triples, las, trace, got, order=[0, 2, 4])
    assert list(got[4]) == [1, 3, 2]
    got = pileups_from_db(shuffled, 4, -1, CONTIG_OFF)
    check_against(nodes, triples, las, trace, got, order=[1])
    assert list(got[4]) == [4]
    empty = pileups_from_db(shuffled, 5, -1, CONTIG_OFF)
    assert len(empty[0]) == 0 and len(empty[1]) == 0 and len(empty[4]) == 0
    assert len(pileups_from_db(shuffled, 2, 0, CONTIG_OFF)[0]) == 0


def test_an_entry_stored_right_flank_first(tmp_path):
    nodes, triples, las, trace = build_world()
    path, swapped = str(tmp_path / "a.db"), str(tmp_path / "b.db")
    write_world(path, nodes, triples, las, trace)
    piles = split_piles(path)
    piles[1][1] = piles[1][1][::-1]   # second entry of the plain gap
    piles[2][0] = piles[2][0][::-1]   # first entry of the anti-parallel join: the nodes come from this one first
    write_piles(swapped, piles)
    check_against(nodes, triples, las, trace, pileups_from_db(swapped, 0, -1, CONTIG_OFF))


def test_a_chain_of_three_is_what_las_read_yields(tmp_path):
    w = World()
    chain = [w.la(0, 2, 3000, 3400, 100, True, START | BEST), w.la(0, 2, 3450, 4100, 560, True, NEXT), w.la(0, 2, 4200, 5000, 1300, True, NEXT)]
    right = w.la(1, 2, 0, 800, 2150, True)
    other = [w.la(0, 3, 3766, 5000, 17), w.la(1, 3, 0, 1111, 1500)]
    las, trace = w.arrays()
    path = str(tmp_path / "chain.db")
    write_world(path, [(0, BACK, 1, FRONT)], [[(2, chain[0], right), (3, other[0], other[1])]], las, trace)
    piles = split_piles(path)
    # write_db stores the first record of the chain only: put the three into its seeded alignment
    s, _ = piles[0][0][0]
    piles[0][0][0] = (s, [(np.array((l["abpos"], l["aepos"], l["bbpos"], l["bepos"], l["diffs"], l["tlen"] // 2), dtype=dentist_amd.CHAIN_LA_DTYPE),
                           trace[l["toff"]:l["toff"] + l["tlen"]]) for l in las[chain]])
    write_piles(path, piles)
    p, las2, trace2, ts, _ = pileups_from_db(path, 0, -1, CONTIG_OFF)
    las_path = str(tmp_path / "chain.las")
    dentist_amd.las_write(las_path, las[chain], trace, TS)
    want, want_trace, _ = dentist_amd.las_read(las_path)
    _, tri = p.get(0)
    first = tri[0][1]
    assert tri[0][0] == 2 and tri[0][2] == first + 3 and tri[1][1] == first + 4
    for k in range(3):
        assert same_record(want[k], las2[first + k]), k
        a, b = want[k], las2[first + k]
        assert np.array_equal(want_trace[a["toff"]:a["toff"] + a["tlen"]], trace2[b["toff"]:b["toff"] + b["tlen"]])
    assert [int(f) for f in las2["flags"][first:first + 3]] == [COMP | START | BEST, COMP | NEXT, COMP | NEXT]
    assert int(las2["flags"][first + 3]) == COMP and int(las2["flags"][first + 4]) == 0


def test_the_reference_fixture_of_realistic_chains(tmp_path):
    """tests/golden/pileupdb_chains.json (binio/_testdata/pileupdb.d): its chains fit the contract once the spacing the
    fixture keeps beside them is written into the seeded alignments (the fixture's own value there is 0)."""
    g = json.load(open(os.path.join(GOLD, "pileupdb_chains.json")))
    ts = g["trace_point_distance"]
    pc, rc, sa, la, tp = [], [], [], [], []
    contig_len = {}
    for pile in g["pile_ups"]:
        pc.append(len(pile))
        for ra in pile:
            rc.append(len(ra))
            for s in ra:
                contig_len[s["contigA"][0]] = s["contigA"][1]
                sa.append((s["id"], s["contigA"][0], s["contigA"][1], s["contigB"][0], s["contigB"][1], 1 if s["complement"] else 0,
                           {"front": 0, "back": 1}[s["seed"]], ts, len(s["las"])))
                for l in s["las"]:
                    la.append((l["a"][0], l["a"][1], l["b"][0], l["b"][1], l["diffs"], len(l["tp"])))
                    for d, b in l["tp"]:
                        tp += [d, b]
    path = str(tmp_path / "fixture.db")
    sa = np.asarray(sa, dtype=dentist_amd.SEEDED_DTYPE)
    la = np.asarray(la, dtype=dentist_amd.CHAIN_LA_DTYPE)
    pileupdb_write(path, np.asarray(pc, np.int32), np.asarray(rc, np.int32), sa, la, np.asarray(tp, np.uint16))
    ncontigs = max(contig_len)
    off = np.concatenate([[0], np.cumsum([contig_len.get(c, 1) for c in range(1, ncontigs + 1)])]).astype(np.int64)
    piles, las2, trace2, ts2, file_index = pileups_from_db(path, 0, -1, off)
    assert ts2 == ts and len(piles) == len(pc) and sorted(file_index) == list(range(len(pc)))
    # every local alignment became one record, in file order, with its trace values
    assert len(las2) == len(la) and np.array_equal(trace2, np.asarray(tp, np.uint16))
    assert np.array_equal(las2["abpos"], la["a_begin"].astype(np.int32)) and np.array_equal(las2["bepos"], la["b_end"].astype(np.int32))
    assert np.array_equal(las2["tlen"], 2 * la["ntp"])
    # chain members follow their first record: NEXT exactly on the records behind the first of a seeded alignment
    is_next = np.concatenate([[False] + [True] * (n - 1) for n in sa["nla"]])
    assert np.array_equal((las2["flags"] & NEXT) != 0, is_next)
    for i in range(len(piles)):
        c0, s0, c1, s1 = piles.get_join(i)
        assert c1 == -1 or c0 < c1


def refusal(tmp_path, change, first=0, count=-1):
    nodes, triples, las, trace = build_world()
    path = str(tmp_path / "good.db")
    write_world(path, nodes, triples, las, trace)
    piles = split_piles(path)
    change(piles)
    bad = str(tmp_path / "bad.db")
    write_piles(bad, piles)
    with pytest.raises(DhError) as e:
        pileups_from_db(bad, first, count, CONTIG_OFF)
    return str(e.value)


def test_refusals_name_the_pile_up(tmp_path):
    def disagree(p):
        p[1][2][0][0]["seed"] = FRONT  # third entry of pile-up 1 says (0, front) where the others say (0, back)
    msg = refusal(tmp_path, disagree)
    assert "dh_pileups_from_db" in msg and "pile-up 1:" in msg and "disagree about its nodes" in msg

    def extension_disagrees(p):
        p[3][1][0][0]["seed"] = BACK
    msg = refusal(tmp_path, extension_disagrees)
    assert "pile-up 3:" in msg and "disagree about its nodes" in msg

    def unmatched_extension_entry(p):
        p[4][1][0][0]["seed"] = FRONT  # the one-alignment entry on (2, back) now names (2, front): no flank of the gap
    msg = refusal(tmp_path, unmatched_extension_entry)
    assert "pile-up 4:" in msg and "disagree about its nodes" in msg

    def self_join(p):
        s = p[2][0][1][0]
        s["contig_a_id"], s["contig_a_len"] = 2, CONTIG_LEN[1]
        for l, _ in p[2][0][1][1]:
            l["a_begin"], l["a_end"] = 0, 1234
    msg = refusal(tmp_path, self_join)
    assert "pile-up 2:" in msg and "joined with itself" in msg

    def contig_outside(p):
        p[0][1][1][0]["contig_a_id"] = 5
    msg = refusal(tmp_path, contig_outside)
    assert "pile-up 0:" in msg and "contig id 5 outside [1, 4]" in msg

    def contig_zero(p):
        p[0][1][1][0]["contig_a_id"] = 0
    assert "contig id 0 outside [1, 4]" in refusal(tmp_path, contig_zero)

    def wrong_length(p):
        p[4][0][0][0]["contig_a_len"] = CONTIG_LEN[2] + 1
    msg = refusal(tmp_path, wrong_length)
    assert "pile-up 4:" in msg and "contig 3 has 7000 bases, the file says 7001" in msg

    def b_sum(p):
        p[1][0][1][1][0][1][3] += 1  # one B base more in the second trace point
    msg = refusal(tmp_path, b_sum)
    assert "pile-up 1:" in msg and "does not sum to its extents" in msg

    def a_points(p):
        l, t = p[1][0][1][1][0]
        merged = t.copy()[2:]
        merged[1] += t[1]           # B still sums, but a trace point is missing on A
        p[1][0][1][1][0] = (l, merged)
    msg = refusal(tmp_path, a_points)
    assert "pile-up 1:" in msg and "does not sum to its extents" in msg


def test_first_and_count_outside_the_file(tmp_path):
    for first, count in ((6, -1), (-1, 2), (0, 6), (3, 3), (0, -2)):
        msg = refusal(tmp_path, lambda p: None, first, count)
        assert "dh_pileups_from_db" in msg and "outside the file's 5 pile-ups" in msg, (first, count)


def test_a_missing_file_is_an_io_error(tmp_path):
    with pytest.raises(DhError):
        pileups_from_db(str(tmp_path / "none.db"), 0, -1, CONTIG_OFF)
