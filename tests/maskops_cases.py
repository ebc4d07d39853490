"""Inputs of the mask-algebra tests (dh_mask_combine, dh_la_tandem_mask): every shape the smallest at which its code can go wrong.
A case is a dict with masks, contig_off, min_count, subtract, min_gap, min_interval and small (the per-base restatement can
run on it); maskops_ref gives the contract's answer.  An interval always gives two events, so the event counts around a tile
of the sort are tile - 2, tile, tile + 2 and 3 * tile + 6 here; the odd counts the sort can see are played on the CPU
(tests/native/maskops_host.cpp).  Not a test module."""
import numpy as np

import maskops_ref as mr

TILE_MIN = 256   # DH_MASKOPS_TILE_KEYS at its lowest


def mask(ncontigs, triples):
    """(contig, begin, end) in any order -> (ptr, iv); the order within a contig stays as given"""
    per = [[] for _ in range(ncontigs)]
    for c, b, e in triples:
        per[c].append((b, e))
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in per])]).astype(np.int64)
    iv = np.array([x for p in per for x in p], dtype=np.int32).reshape(-1, 2)
    return ptr, iv


def case(lens, masks, min_count=1, subtract=None, min_gap=0, min_interval=0, small=True):
    n = len(lens)
    return {"masks": [mask(n, m) for m in masks], "contig_off": np.concatenate([[0], np.cumsum(lens, dtype=np.int64)]).astype(np.int64),
            "min_count": min_count, "subtract": mask(n, subtract) if subtract is not None else None, "min_gap": min_gap,
            "min_interval": min_interval, "small": small}


def args_of(c):
    return dict(min_count=c["min_count"], subtract=c["subtract"], min_gap=c["min_gap"], min_interval=c["min_interval"])


def triples(ptr, iv):
    """(ptr, iv) of a result -> (contig, begin, end) triples; checks the layout on the way"""
    ptr, iv = np.asarray(ptr), np.asarray(iv).reshape(-1, 2)
    assert ptr[0] == 0 and ptr[-1] == len(iv) and np.all(np.diff(ptr) >= 0)
    return [(c, int(iv[j][0]), int(iv[j][1])) for c in range(len(ptr) - 1) for j in range(ptr[c], ptr[c + 1])]


def constructed():
    within = [(1, 40, 60), (1, 10, 30), (1, 20, 25), (1, 10, 30), (1, 60, 70), (1, 5, 5), (1, 0, 3), (1, 90, 100), (1, 100, 100), (1, 28, 35)]
    same = [(0, 10, 20), (2, 0, 50)]
    three = [[(0, 0, 5)], [(0, 0, 10)], [(0, 5, 10)]]
    base = [(0, 10, 30), (0, 40, 60), (0, 70, 80), (1, 0, 20)]
    sub = [(0, 15, 20), (0, 18, 25), (0, 40, 60), (0, 80, 90), (0, 65, 70), (1, 5, 5)]
    gaps = [(0, 0, 10), (0, 15, 20), (0, 26, 30), (1, 0, 5)]                                   # gaps of 5 and 6
    cascade = [(0, 10 * k, 10 * k + 4) for k in range(5)] + [(0, 60, 62)]                      # five runs 6 apart, one 14 behind
    border = [(0, 90, 100), (1, 0, 10)]
    sizes = [(0, 0, 7), (0, 20, 26), (1, 3, 10)]
    crumbs = [(0, 0, 2), (0, 3, 5), (0, 6, 8), (0, 30, 32)]
    out = {
        "nothing": case([10, 20], [[], []]),
        "only_empty_intervals": case([10, 20], [[(0, 3, 3), (1, 20, 20)]]),
        "one_interval": case([10], [[(0, 2, 7)]]),
        "empty_contigs_between": case([5, 0, 30, 7, 0, 0, 12], [[(2, 1, 4), (6, 0, 12)], [(0, 0, 5), (6, 3, 9)]]),
        "within_one_mask": case([50, 100], [within]),
        "same_interval_min_1": case([30, 5, 50], [same, same, same], 1),
        "same_interval_min_2": case([30, 5, 50], [same, same, same + [(0, 25, 30)]], 2),
        "same_interval_min_all": case([30, 5, 50], [same, same, same + [(0, 25, 30)]], 3),
        "raw_intervals_do_not_count": case([30], [[(0, 0, 10), (0, 5, 15), (0, 5, 15)], [(0, 12, 20)]], 2),
        "three_masks_min_2": case([10], three, 2),
        "touching_across_masks_min_2": case([10], [[(0, 0, 5)], [(0, 5, 10)]], 2),
        "subtract": case([100, 20], [base], 1, sub),
        "subtract_alone_in_a_contig": case([100, 20], [[(0, 1, 2)]], 1, [(1, 0, 20), (0, 0, 1)]),
        "subtract_min_2": case([100, 20], [base, [(0, 0, 100), (1, 10, 20)]], 2, sub),
        "gap_equal_joined_one_more_not": case([40, 10], [gaps], min_gap=5),
        "both_gaps_joined": case([40, 10], [gaps], min_gap=6),
        "cascade": case([100], [cascade], min_gap=6),
        "no_join_across_contigs": case([100, 100], [border], min_gap=50),
        "size_equal_kept": case([30, 10], [sizes], min_interval=7),
        "size_one_less_dropped": case([30, 10], [sizes], min_interval=8),
        "min_interval_1": case([30, 10], [sizes], min_interval=1),
        "crumbs_survive_by_gaps": case([40], [crumbs], min_gap=1, min_interval=8),
        "closed_gap_covers_subtracted": case([40], [[(0, 0, 30)]], 1, [(0, 10, 12)], min_gap=2),
        "everything_filtered": case([40], [crumbs], min_interval=3),
    }
    return out


def sort_shapes():
    out = {}
    for name, n in (("tile_minus", TILE_MIN // 2 - 1), ("tile", TILE_MIN // 2), ("tile_plus", TILE_MIN // 2 + 1), ("three_tiles", 3 * TILE_MIN // 2 + 3)):
        rng = np.random.default_rng(n)
        b = rng.integers(0, 4000, n)
        out[name] = case([5000], [[(0, int(x), int(x) + 1 + int(k) % 7) for k, x in enumerate(b)]])
    out["all_keys_equal"] = case([50, 50], [[(1, 7, 19)] * 3000])
    out["all_keys_equal_min_2"] = case([50, 50], [[(1, 7, 19)] * 1500, [(1, 7, 19)] * 1500], 2)
    out["two_keys_alternating"] = case([50], [[(0, 7, 19), (0, 7, 19)] * 1000])
    top = 2 ** 31 - 1
    out["longest_contig"] = case([100, top], [[(1, top - 5, top), (1, 0, 3), (0, 0, 100)], [(1, 2, top - 3)]], small=False)
    out["longest_contig_min_2"] = case([100, top], [[(1, top - 5, top), (1, 0, 3), (0, 0, 100)], [(1, 2, top - 3)]], 2, [(1, top - 4, top - 3)], small=False)
    rng = np.random.default_rng(70001)
    some = sorted(set([0, 70000] + rng.integers(0, 70001, 2000).tolist()))
    out["many_contigs"] = case([50] * 70001, [[(c, c % 30, c % 30 + 1 + c % 20) for c in some], [(c, 5, 45) for c in some[::3]]], small=False)
    return out


def random_case(seed=40, nmasks=4, ncontigs=40, n=40000, **kw):
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 6000, ncontigs)
    lens[rng.integers(0, ncontigs, 4)] = 0
    masks = []
    for _ in range(nmasks + 1):
        c = rng.choice(np.flatnonzero(lens > 0), n // nmasks if len(masks) < nmasks else 300)
        b = (rng.random(len(c)) * lens[c]).astype(np.int64)
        e = np.minimum(lens[c], b + rng.integers(0, 12, len(c)))
        masks.append(list(zip(c.tolist(), b.tolist(), e.tolist())))
    return case(lens.tolist(), masks[:nmasks], subtract=masks[nmasks], **kw)


def randoms():
    return {"random_or": random_case(), "random_min_2_filtered": random_case(41, min_count=2, min_gap=3, min_interval=4),
            "random_and": random_case(42, nmasks=2, ncontigs=7, n=30000, min_count=2)}


ALL = {}
ALL.update(constructed())
ALL.update(sort_shapes())
ALL.update(randoms())
_EXPECTED = {}


def expected_of(name):
    """the contract's answer (interval form), computed once"""
    if name not in _EXPECTED:
        c = ALL[name]
        _EXPECTED[name] = mr.combine_intervals(c["masks"], c["contig_off"], **args_of(c))
    return _EXPECTED[name]


def groups_of(c):
    """the launch groups with one contig each: a contig launches iff an input mask has a non-empty interval in it"""
    n = 0
    for k in range(len(c["contig_off"]) - 1):
        n += any(b < e for m in c["masks"] for b, e in mr.intervals_of(m, k))
    return n


def refusals():
    """(name, case, words of the message)"""
    good = [(0, 1, 5), (1, 0, 20)]
    out = []

    def add(name, words, lens=(10, 20), masks=None, **kw):
        out.append((name, case(list(lens), masks if masks is not None else [good, good], **kw), words))
    add("min_count_0", "min_count < 1", min_count=0)
    add("min_count_above", "min_count > nmasks", min_count=3)
    add("min_gap_negative", "a negative min_gap", min_gap=-1)
    add("min_interval_negative", "a negative min_interval", min_interval=-1)
    add("begin_negative", "mask 1: contig 0: interval 0: begin < 0", masks=[good, [(0, -1, 5), (1, 30, 40)]])
    add("begin_above_end", "mask 0: contig 1: interval 2: begin > end", masks=[[(0, 1, 5), (0, 2, 3), (1, 7, 6), (1, 9, 8)], good])
    add("end_behind", "mask 1: contig 0: interval 0: end behind the contig's end", masks=[good, [(0, 1, 11)]])
    add("subtract_end_behind", "subtract mask: contig 1: interval 1: end behind the contig's end", subtract=[(0, 0, 1), (1, 0, 21)])
    add("lowest_mask_wins", "mask 0: contig 1: interval 1: begin > end", masks=[[(0, 1, 5), (1, 7, 6)], [(0, -1, 5)]])
    c = case([10, 20], [good, good])
    c["masks"][1] = (np.array([1, 1, 2], dtype=np.int64), c["masks"][1][1])
    out.append(("ptr_not_at_0", c, "mask 1: ptr does not start at 0"))
    c = case([10, 20], [good, good])
    c["masks"][0] = (np.array([0, 2, 1], dtype=np.int64), c["masks"][0][1])
    out.append(("ptr_decreases", c, "mask 0: contig 1: ptr decreases"))
    c = case([10, 20], [good])
    c["contig_off"] = np.array([0, 10, 10 + 2 ** 31], dtype=np.int64)
    out.append(("contig_too_long", c, "contig 1: longer than 2^31 - 1"))
    c = case([10, 20], [good])
    c["contig_off"] = np.array([0, 10, 5], dtype=np.int64)
    out.append(("contig_off_decreases", c, "contig 1: contig_off decreases"))
    return out


# ---- tandem: (aread, bread, abpos, aepos, bbpos, bepos, flags) rows
def tandem_case(first_read=0):
    import dentist_amd
    f = first_read
    rows = [(f + 0, f + 0, 100, 600, 150, 700, 0),    # [100, 700)
            (f + 0, f + 1, 0, 900, 0, 900, 0),        # aread != bread
            (f + 0, f + 0, 0, 900, 0, 900, 1),        # complement
            (f + 2, f + 2, 50, 500, 100, 550, 0),     # exactly min_len: [50, 550)
            (f + 2, f + 2, 1000, 1400, 1001, 1499, 0),   # min_len - 1: dropped
            (f + 2, f + 2, 550, 1000, 600, 1100, 0),  # touches [50, 550): merged to [50, 1100)
            (f + 0, f + 0, 650, 1300, 600, 1200, 0),  # overlaps [100, 700): [100, 1300)
            (f + 3, f + 3, 0, 2000, 5, 1990, 0)]      # to the read's end
    las = np.zeros(len(rows), dtype=dentist_amd.LA_DTYPE)
    for i, r in enumerate(rows):
        las[i]["aread"], las[i]["bread"], las[i]["abpos"], las[i]["aepos"], las[i]["bbpos"], las[i]["bepos"], las[i]["flags"] = r
    read_off = np.concatenate([[0], np.cumsum([1500, 100, 1600, 2000])]).astype(np.int64)
    return las, read_off, first_read, 500
