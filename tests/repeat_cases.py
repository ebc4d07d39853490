"""Inputs of the repeat-mask tests (dh_la_repeat_mask): every shape the smallest at which its code can go wrong.  A case is a dict
with las, contig_off, read_off, lower, upper, improper (None or a pair of bounds) and allowance; repeat_ref.repeat_mask gives the
contract's answer.  Not a test module."""
import numpy as np

import dentist_amd
import repeat_ref as rr

LA = dentist_amd.LA_DTYPE
LOW_CAP = 1024   # DH_RMASK_LDS_EVENTS at its lowest
CAP = 8192       # and at its default
RLEN = 400       # every read of the constructed cases


def case(lens, rows, lower=0, upper=4, improper=None, allowance=0, nreads=None):
    """rows: (aread, abpos, aepos[, bread, bbpos, bepos, flags]) in input order; a row without a read gets one of its own, and
    read coordinates that make it improper (the middle of the read)"""
    las = np.zeros(len(rows), dtype=LA)
    top = 0
    for i, r in enumerate(rows):
        r = tuple(r) + (i, 100, 300, 0)[len(r) - 3:] if len(r) < 7 else tuple(r)
        las[i]["aread"], las[i]["abpos"], las[i]["aepos"], las[i]["bread"], las[i]["bbpos"], las[i]["bepos"], las[i]["flags"] = r
        top = max(top, r[3] + 1)
    nreads = top if nreads is None else nreads
    return {"las": las, "contig_off": np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
            "read_off": np.arange(nreads + 1, dtype=np.int64) * RLEN, "lower": lower, "upper": upper, "improper": improper,
            "allowance": allowance}


def expected(c):
    return rr.repeat_mask(c["las"], c["contig_off"], c["read_off"], c["lower"], c["upper"], c["improper"], c["allowance"])


def triples(mask):
    """(ptr, iv) of a result -> sorted (contig, begin, end) triples; checks the layout on the way"""
    ptr, iv = np.asarray(mask[0]), np.asarray(mask[1]).reshape(-1, 2)
    assert ptr[0] == 0 and ptr[-1] == len(iv) and np.all(np.diff(ptr) >= 0)
    return [(c, int(iv[j][0]), int(iv[j][1])) for c in range(len(ptr) - 1) for j in range(ptr[c], ptr[c + 1])]


# ---- the reference's own vector: maskRepetitiveRegions.d:299-333 with bounds (3, 5), result :402-410 (contigs 0-based here)
REF_ALIGNMENTS = [(1, 5, 18), (1, 5, 18), (1, 5, 20), (1, 10, 20), (1, 10, 30), (1, 10, 30), (1, 13, 30), (1, 20, 30),
                  (1, 20, 30), (1, 20, 30), (1, 24, 30), (2, 0, 3), (2, 0, 3), (2, 0, 5), (2, 0, 5), (2, 0, 15), (2, 0, 15),
                  (2, 0, 15), (2, 5, 15), (2, 5, 15), (2, 5, 15), (2, 9, 15), (3, 1, 4), (3, 2, 5), (3, 3, 6), (3, 4, 7),
                  (3, 5, 8), (3, 6, 9), (3, 7, 10), (3, 8, 11), (3, 9, 12), (3, 10, 13), (3, 11, 14)]
REF_LENS = [30, 15, 15]
REF_MASK_3_5 = [(0, 0, 5), (0, 10, 18), (0, 20, 30), (1, 0, 3), (1, 5, 15), (2, 0, 3), (2, 12, 15)]


def reference_vector():
    return case(REF_LENS, [(c - 1, b, e) for c, b, e in REF_ALIGNMENTS], 3, 5)


def staircase(c, units, clen, step=3):
    """`units` single-record units on contig c with distinct begins and ends (2 * units events)"""
    return [(c, (k * step) % (clen // 2), clen // 2 + (k * 7) % (clen // 2) + 1) for k in range(units)]


def tier_edges():
    """name -> case: contigs of 0, 2, 62, 64, 66 events; of cap - 2, cap, cap + 2 events at the low cap; one far above the low cap
    (about five times) and one above the default cap"""
    out = {}
    counts = [0, 1, 31, 32, 33, LOW_CAP // 2 - 1, LOW_CAP // 2, LOW_CAP // 2 + 1]
    rows = []
    for c, u in enumerate(counts):
        rows += staircase(c, u, 4000)
    out["edges"] = case([4000] * len(counts), rows, 2, 20)
    out["far_above_low_cap"] = case([9000], staircase(0, 2600, 9000), 100, 900)
    out["above_default_cap"] = case([500, 20000, 300], staircase(1, CAP // 2 + 5, 20000) + staircase(2, 3, 300), 300, 2000)
    return out


def equal_positions():
    n = LOW_CAP // 2 + 40
    return {"all_equal": case([777], [(0, 0, 777)] * n, 0, n - 1),
            "all_equal_ok": case([777], [(0, 0, 777)] * n, 0, n),
            "one_base_apart": case([777], [(0, k & 1, 777 - ((k >> 1) & 1)) for k in range(n)], n // 2 + 3, n - 1),
            "overhang_at_zero": case([5000], [(0, 0, 100 + 4 * k) for k in range(n)] + [(0, 4000, 5000)] * 3, 2, 300)}


def zone_edges():
    return {
        "one_base_ok_between_bad": case([40], [(0, 0, 10), (0, 0, 10), (0, 11, 30), (0, 11, 30), (0, 0, 40)], 0, 2),
        "touching_no_boundary": case([40], [(0, 5, 20), (0, 20, 35)], 1, 1),
        "high_to_low_one_run": case([40], [(0, 0, 20), (0, 0, 20), (0, 0, 20)], 1, 2),
        "bad_to_last_base": case([40], [(0, 0, 25)], 1, 1),
        "bad_from_first_base_to_last": case([40], [(0, 10, 25)], 2, 3),
        "cov_equals_bounds": case([60], [(0, 0, 60), (0, 10, 50), (0, 20, 40), (0, 25, 35)], 2, 3),
        "empty_interval": case([30], [(0, 7, 7), (0, 0, 30), (0, 30, 30), (0, 0, 0)], 2, 5),
        "empty_contig": case([0, 10], [(0, 0, 0), (1, 2, 5)], 1, 1),
    }


def gaps_between_contigs(lower):
    """contigs without units between contigs with units, first and last contig included"""
    lens = [50, 60, 70, 80, 90, 100, 110]
    return case(lens, [(1, 0, 30), (1, 10, 60), (4, 5, 85), (4, 5, 85), (5, 0, 100)], lower, 1)


def chains():
    S, N = rr.START, rr.NEXT
    out = {}
    # three members with gaps between them: the gaps are covered
    out["gaps_covered"] = case([1000], [(0, 100, 200, 0, 0, 100, S), (0, 300, 400, 0, 150, 250, N), (0, 600, 700, 0, 300, 400, N)], 0, 0,
                               improper=(0, 0), allowance=0)
    # a middle member sticks out behind the last: not covered beyond last.aepos
    out["middle_sticks_out"] = case([1000], [(0, 100, 200, 0, 0, 100, S), (0, 250, 900, 0, 120, 300, N), (0, 300, 500, 0, 300, 400, N)], 0, 0)
    # NEXT after a change of bread or strand: no continuation
    out["next_after_change"] = case([1000], [(0, 100, 200, 0, 0, 100, S), (0, 300, 400, 1, 150, 250, N), (0, 500, 600, 1, 260, 300, N | rr.COMP),
                                             (0, 700, 800, 1, 310, 400, N | rr.COMP), (0, 820, 900, 1, 0, 50, S | N | rr.COMP)], 0, 0)
    # proper as a whole, every member improper (allowance 0: begins at the read's begin, ends at the read's end)
    out["proper_whole_improper_members"] = case([2000], [(0, 500, 700, 0, 0, 150, S), (0, 800, 1000, 0, 200, RLEN, N)], 0, 5,
                                                improper=(1, 5), allowance=0)
    # and the reverse: improper as a whole (the first member begins, the last ends, inside both sequences) with a member that is
    # proper alone (no chain can be improper with every member proper: its begin is its first member's, its end its last's)
    out["improper_whole_proper_member"] = case([300, 2000], [(1, 500, 700, 0, 100, 250, S), (1, 700, 900, 0, 0, RLEN, N),
                                                             (1, 1000, 1200, 0, 100, 300, N)], 0, 5, improper=(0, 0), allowance=0)
    return out


def unions():
    P = (0, 0, RLEN)  # proper read coordinates: the whole read
    rows = [
        # all: cov > 1 on [100, 200); improper (cov > 0): [200, 300) touches it
        (0, 100, 200) + (0,) + P[1:] + (0,), (0, 100, 200) + (1,) + P[1:] + (0,), (0, 200, 300, 2, 100, 300, 0),
        # nested: improper [420, 440) inside all [400, 500)
        (0, 400, 500) + (3,) + P[1:] + (0,), (0, 400, 500) + (4,) + P[1:] + (0,), (0, 420, 440, 5, 100, 300, 0),
        # interleaved: all [600, 700), improper [650, 750) and [740, 800)
        (0, 600, 700) + (6,) + P[1:] + (0,), (0, 600, 700) + (7,) + P[1:] + (0,), (0, 650, 750, 8, 100, 300, 0), (0, 740, 800, 9, 100, 300, 0),
    ]
    out = {"touch_nest_interleave": case([1000], rows, 0, 1, improper=(0, 0), allowance=0)}
    # improper with no unit at all: empty even with improper_lower > 0
    out["no_improper_unit"] = case([500, 500], [(0, 0, 500) + (0,) + P[1:] + (0,), (0, 0, 500) + (1,) + P[1:] + (0,)], 0, 1,
                                   improper=(1, 5), allowance=0)
    # one improper unit: the other contig is one full run of improper
    out["one_improper_unit"] = case([500, 500], [(0, 0, 500) + (0,) + P[1:] + (0,), (0, 100, 300, 1, 100, 300, 0)], 0, 1,
                                    improper=(1, 5), allowance=0)
    return out


# (seed, (lower, upper), improper bounds or None): listed, not drawn at test time
RANDOM = [(11, (0, 8), None), (12, (2, 6), (0, 3)), (13, (0, 3), (1, 40)), (14, (5, 40), (0, 0))]


def random_case(seed, bounds, improper, units=4000, ncontigs=40):
    rng = np.random.default_rng(seed)
    lens = rng.integers(50, 6001, ncontigs).tolist()
    per = [[] for _ in lens]
    nreads = 0
    for _ in range(units):
        c = int(rng.integers(0, ncontigs))
        if c % 9 == 4:
            continue  # (contigs without units)
        members = int(rng.integers(1, 5)) if rng.integers(0, 3) == 0 else 1
        at = int(rng.integers(0, lens[c])) if rng.integers(0, 4) else 0
        bb = int(rng.choice([0, 0, 50, 120]))
        comp = int(rng.integers(0, 2))
        for m in range(members):
            e = int(min(lens[c], at + rng.integers(0, 1500 // members + 1)))
            if rng.integers(0, 5) == 0:
                e = lens[c]
            be = int(min(RLEN, bb + rng.integers(1, 200)))
            if m == members - 1 and rng.integers(0, 2):
                be = RLEN
            per[c].append((c, at, e, nreads, bb, be, comp | (rr.START if m == 0 else rr.NEXT)))
            at, bb = int(min(lens[c], e + rng.integers(0, 60))), be
        nreads += 1
    rows = [r for rows_c in per for r in rows_c]
    return case(lens, rows, bounds[0], bounds[1], improper=improper, allowance=int(rng.choice([0, 20, 100])), nreads=nreads)


def all_cases():
    """name -> case"""
    out = {"reference_vector": reference_vector()}
    for group in (tier_edges(), equal_positions(), zone_edges(), chains(), unions()):
        out.update(group)
    out["gaps_lower_0"], out["gaps_lower_1"] = gaps_between_contigs(0), gaps_between_contigs(1)
    for seed, bounds, improper in RANDOM:
        out["random_%d" % seed] = random_case(seed, bounds, improper)
    return out


_EXPECTED = {}


def expected_of(name):
    """the contract's answer of all_cases()[name], computed once"""
    if name not in _EXPECTED:
        _EXPECTED[name] = expected(ALL[name])
    return _EXPECTED[name]


ALL = all_cases()


def refusals():
    """(name, case, the words dh_last_error must hold)"""
    ok = reference_vector()

    def las_with(i, **kw):
        c = dict(ok, las=ok["las"].copy())
        for k, v in kw.items():
            c["las"][i][k] = v
        return c
    S, N = rr.START, rr.NEXT
    out = [("lower_above_upper", dict(ok, lower=6, upper=5), "lower > upper"),
           ("negative_bound", dict(ok, lower=-1), "negative"),
           ("negative_allowance", dict(ok, allowance=-1), "negative"),
           ("improper_lower_above_upper", dict(ok, improper=(3, 2)), "improper_lower > improper_upper"),
           ("aread_out_of_range", las_with(32, aread=3), "record 32: aread out of range"),
           ("aread_negative", las_with(0, aread=-1), "record 0: aread out of range"),
           ("bread_out_of_range", dict(las_with(7, bread=99), improper=(0, 1)), "record 7: bread out of range"),
           ("aread_decreases", las_with(20, aread=0), "record 20: aread below"),
           ("abpos_negative", las_with(5, abpos=-1), "record 5: abpos < 0"),
           ("abpos_above_aepos", las_with(6, abpos=31), "record 6: abpos > aepos"),
           ("aepos_behind_end", las_with(11, aepos=16), "record 11: aepos behind"),
           ("lowest_of_two", dict(ok, las=_two_faults(ok["las"])), "record 9: abpos < 0"),
           ("chain_ends_before_it_begins", case([1000], [(0, 5, 9), (0, 500, 600, 1, 0, 100, S), (0, 100, 200, 1, 100, 200, N)]),
            "record 1: the chain"),
           ("long_contig", dict(ok, contig_off=np.asarray([0, 30, 30 + 2 ** 31, 45 + 2 ** 31], dtype=np.int64)), "contig 1: longer")]
    return out


def _two_faults(las):
    las = las.copy()
    las[9]["abpos"], las[20]["aepos"] = -1, 99
    return las
