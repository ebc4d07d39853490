"""Inputs of the collect-filter tests (dh_la_collect_filter): every shape the smallest at which its code can go wrong.  A case is
a dict: las, contig_off, read_off, mask ((ptr, iv) or None), opts (max_align_err_ppm, allowance, min_anchor).  expected() gives
the contract's answer: the oracle restatement (oracle/collect_filters.py) on the small cases, the host function
dentist_amd.collect_filter -- which tests/test_collect_filters.py pins to the oracle -- on those too large for its Python loops."""
import numpy as np

import dentist_amd
from oracle import collect_filters as cf

LA = dentist_amd.LA_DTYPE
COMP, START, NEXT, DISABLED = 0x1, 0x4, 0x8, 0x20
LOW_CAP = 64          # DH_CFILT_LDS_UNITS of the tier-boundary cases: 63 / 64 a wavefront, 65 the slab
ORACLE_MAX = 400      # records up to which the oracle's loops are quick
DEFAULT = dict(max_align_err_ppm=300000, allowance=100, min_anchor=500)
LOOSE = dict(max_align_err_ppm=300000, allowance=1 << 30, min_anchor=0)   # stages 2 and 3 drop nothing


def la(aread, bread, abpos, aepos, bbpos, bepos, diffs=0, flags=0):
    r = np.zeros(1, dtype=LA)[0]
    r["aread"], r["bread"], r["abpos"], r["aepos"], r["bbpos"], r["bepos"], r["diffs"], r["flags"] = \
        aread, bread, abpos, aepos, bbpos, bepos, diffs, flags
    return r


def chained(rows):
    """rows of one chain, in order: START on the first, NEXT on the others (dazzler.d:1728-1758)"""
    out = np.stack(rows)
    out["flags"] |= NEXT
    out["flags"][0] = (int(out["flags"][0]) & ~NEXT & 0xFFFFFFFF) | START
    return out


def case(rows, clens, rlens, mask=None, opts=DEFAULT):
    las = np.concatenate([np.atleast_1d(r) for r in rows]).astype(LA) if len(rows) else np.zeros(0, dtype=LA)
    coff = np.concatenate([[0], np.cumsum(clens)]).astype(np.int64)
    roff = np.concatenate([[0], np.cumsum(rlens)]).astype(np.int64)
    if mask is not None:
        mask = (np.asarray(mask[0], dtype=np.int64), np.asarray(mask[1], dtype=np.int32).reshape(-1))
    return dict(las=las, contig_off=coff, read_off=roff, mask=mask, opts=dict(opts))


def popts(c):
    return dentist_amd.default_process_opts(**c["opts"])


def host(c):
    """the host function dh_collect_filter"""
    return dentist_amd.collect_filter(c["las"], c["contig_off"], c["read_off"], popts(c), repeat_mask=c["mask"])


def oracle(c):
    o = c["opts"]
    return cf.collect_filter(c["las"], c["contig_off"], c["read_off"], max_align_err=o["max_align_err_ppm"] / 1e6, allowance=o["allowance"],
                             min_anchor=o["min_anchor"], repeat_mask=c["mask"])


def expected(c):
    if len(c["las"]) == 0:
        return c["las"].copy(), np.zeros(6, dtype=np.int64), np.ones(len(c["read_off"]) - 1, dtype=np.uint8)
    return oracle(c) if len(c["las"]) <= ORACLE_MAX else host(c)


def same(got, exp):
    return np.array_equal(got[0]["flags"], exp[0]["flags"]) and got[0].tobytes() == exp[0].tobytes() and \
        np.array_equal(np.asarray(got[1]), np.asarray(exp[1])) and np.array_equal(np.asarray(got[2]), np.asarray(exp[2]))


def reorder(c, kind, seed=0):
    """the same chains in another order: 'byread' (bread never decreases), 'lasort' (by contig, then read), 'random'"""
    las = c["las"]
    rng = cf.chain_ranges(las) if len(las) else []
    if kind == "byread":
        order = sorted(range(len(rng)), key=lambda k: (int(las[rng[k][0]]["bread"]), k))
    elif kind == "lasort":
        order = sorted(range(len(rng)), key=lambda k: (int(las[rng[k][0]]["aread"]), int(las[rng[k][0]]["bread"]),
                                                       int(las[rng[k][0]]["flags"]) & COMP, int(las[rng[k][0]]["abpos"]), k))
    else:
        order = np.random.default_rng(seed).permutation(len(rng)).tolist()
    out = dict(c)
    out["las"] = np.concatenate([las[rng[k][0]:rng[k][1]] for k in order]) if len(rng) else las.copy()
    return out


# ------------------------------------------------------------------------------------------------ units per read
def units_of_a_read(k, seed, big=10_000_000, rlen=4_000_000):
    """read 1 has k units on two contigs: nests of up to three (Contained), a unit that ends a scan in front of a nested one,
    low-quality units; the read intervals of different nests do not intersect, so some units survive.  Reads 0 and 3 have one
    unit, read 2 and read 4 none."""
    rng = np.random.default_rng(seed)
    rows, slot = [], 0
    while len(rows) < k:
        c, comp = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        ab, bb, ln = 1000 + 3000 * slot, 1000 + 3000 * slot, int(rng.integers(1200, 2400))
        bad = 0.35 if rng.random() < 0.15 else 0.1
        nest = [la(c, 1, ab, ab + ln, bb, bb + ln, int(ln * bad), comp)]
        depth = int(rng.integers(0, 3))
        for d in range(1, depth + 1):
            flip = comp ^ 1 if rng.random() < 0.2 else comp
            nest.append(la(c, 1, ab + 100 * d, ab + ln - 100 * d, bb + 100 * d, bb + ln - 100 * d, 10, flip))
        if rng.random() < 0.3:   # sticks out on A: ends the scan of the outer unit; the nested units behind it stay
            nest.insert(1, la(c, 1, ab + 50, ab + ln + 50, bb + 50, bb + ln - 60, 10, comp))
        rows += nest
        slot += 1
    rows = rows[:k]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    one = [la(0, 0, 0, 3000, 997_000, 1_000_000, 100), la(1, 3, 5000, 9000, 0, 4000, 100)]
    return case([one[0]] + rows + [one[1]], [big, big], [1_000_000, rlen, 500, 4000, 500], opts=LOOSE)


def ambiguous_read(k):
    """k units of one read, pairwise disjoint on the read but for the last two"""
    rows = [la(i % 3, 0, 5000 * i, 5000 * i + 2000, 3000 * i, 3000 * i + 2000, 50, i & 1) for i in range(k)]
    rows[-1]["bbpos"], rows[-1]["bepos"] = rows[-2]["bbpos"] + 1999, rows[-2]["bbpos"] + 3000
    if rows[-1]["flags"] & COMP != rows[-2]["flags"] & COMP:   # (forward coordinates: give both the same strand)
        rows[-1]["flags"] = rows[-2]["flags"]
    return case(rows, [10_000_000] * 3, [10_000_000], opts=LOOSE)


# ------------------------------------------------------------------------------------------------ chains
def chain_of(m, aread, bread, a0, b0, comp=0, step=1000, ln=900, diffs=30):
    return chained([la(aread, bread, a0 + step * i, a0 + step * i + ln, b0 + step * i, b0 + step * i + ln, diffs, comp) for i in range(m)])


def chains_case():
    """chains of 1, 2 and 70 members; chains across records 64 and 256; a member disabled on entry; NEXT behind another strand
    or read starts a chain; overlapping members (the running `done` position)"""
    rows, r = [], 0
    for i in range(62):   # fillers: one record each
        rows.append(la(0, r, 0, 2000, 8000, 10000, 100))
        r += 1
    rows.append(chain_of(5, 0, r, 0, 5000))            # records 62..66
    r += 1
    while sum(len(np.atleast_1d(x)) for x in rows) < 254:
        rows.append(la(1, r, 0, 2000, 8000, 10000, 100))
        r += 1
    rows.append(chain_of(4, 1, r, 0, 6000, comp=1))     # records 254..257
    r += 1
    rows.append(chain_of(70, 0, r, 30010, 0, step=1000, ln=990))   # ends at the contig's end; its read has 70 000 bases
    long_read = r
    r += 1
    dis = chain_of(3, 1, r, 0, 7000)
    dis["flags"][1] |= DISABLED                         # the whole chain is disabled on entry, and counted nowhere
    rows.append(dis)
    r += 1
    brk = chain_of(2, 0, r, 0, 8000)
    brk["flags"][1] |= COMP                             # NEXT on the other strand: a chain of its own
    rows.append(brk)
    r += 1
    rows.append(chain_of(2, 0, r, 0, 8000))
    nxt = la(0, r + 1, 0, 2000, 8000, 10000, 100, NEXT)  # NEXT behind another read
    rows.append(nxt)
    r += 2
    over = chained([la(1, r, 0, 600, 9000, 9600, 10), la(1, r, 500, 1000, 9500, 10000, 10), la(1, r, 800, 1001, 9800, 10000, 5)])
    rows.append(over)                                   # union 0..1001, covered 1301
    r += 1
    rlens = [10000] * r
    rlens[long_read] = 70000
    return case(rows, [100_000, 100_000], rlens, mask=([0, 1, 2], [600, 700, 0, 500]))


# ------------------------------------------------------------------------------------------------ masks and boundaries
def boundaries_case():
    """pairs of units one step apart on either side of every comparison; reads of 30 000 (no read fits inside a contig)"""
    E = 30000
    rows = [
        la(0, 0, 0, 1000, E - 1000, E, 300), la(0, 1, 0, 1000, E - 1000, E, 301),                  # LQ: 300 * 10^6 == ppm * 1000 | above
        la(0, 2, 100, 3000, 5000, E, 10), la(0, 3, 101, 3000, 101, E, 10),                          # begins: == allowance | both one above
        la(0, 4, 101, 9900, 100, 9899, 10),                                                         # ... by bbpos alone
        la(0, 5, 0, 9900, 0, 5000, 10), la(0, 6, 0, 9899, 0, 9899, 10), la(0, 7, 0, 9899, 1, E - 100, 10),   # ends: == | both below | by bepos
        la(1, 8, 0, 1500, E - 1500, E, 10), la(1, 9, 0, 1501, E - 1501, E, 10),                     # unmasked == 500 | 501 (mask 200..1200)
        la(2, 10, 1000, 1501, 100, 601, 10),            # intervals end at abpos and begin at aepos: 501 unmasked
        la(2, 11, 999, 1502, 100, 603, 10),             # ... one base of each: 501 again
        la(3, 12, 0, 701, 1, 702, 10),                  # touching intervals 100..200, 200..300 and an empty one: 501
        la(4, 13, 0, 1000, E - 1000, E, 10),            # a contig without intervals
    ]
    mask = ([0, 0, 1, 3, 6, 6], [200, 1200, 0, 1000, 1501, 1600, 100, 200, 200, 300, 400, 400])
    return case(rows, [10000, 10000, 1600, 800, 10000], [E] * 14, mask=mask)


def many_intervals_case():
    """300 intervals of 10 bases every 30 on contig 0; units that begin and end inside, between and on the edges of intervals"""
    iv = np.stack([np.arange(300) * 30, np.arange(300) * 30 + 10], axis=1).reshape(-1)
    rows = [la(0, i, b, e, 0, 10000, 5) for i, (b, e) in enumerate([(0, 9000), (5, 755), (10, 760), (9, 761), (30, 780), (8990, 10000), (29, 31),
                                                                      (0, 750), (15, 765), (8999, 9750)])]
    rows.append(chained([la(0, 10, 0, 400, 0, 400, 5), la(0, 10, 395, 800, 400, 10000, 5)]))
    return case(rows, [10000], [10000] * 11, mask=([0, 300], iv), opts=dict(DEFAULT, allowance=10000))


# ------------------------------------------------------------------------------------------------ Contained
def contained_case():
    rows = [
        # read 0: x = 0..5000; a unit that sticks out on A ends its scan in front of a nested unit, which stays
        la(0, 0, 0, 5000, 0, 5000, 10), la(0, 0, 100, 5100, 6000, 9000, 10), la(0, 0, 200, 4000, 200, 4000, 10),
        # read 1: a unit disabled on entry inside the scan does not end it and is not counted
        la(0, 1, 0, 5000, 0, 5000, 10), la(0, 1, 100, 4900, 100, 4900, 10, DISABLED), la(0, 1, 200, 4000, 200, 4000, 10),
        # read 2 / 3: two identical records, equal strand (the second in the input goes) / opposite strand (both stay)
        la(0, 2, 0, 5000, 0, 5000, 10), la(0, 2, 0, 5000, 0, 5000, 10),
        la(0, 3, 0, 5000, 0, 5000, 10), la(0, 3, 0, 5000, 0, 5000, 10, COMP),
        # read 4: a nest of three
        la(0, 4, 0, 5000, 0, 5000, 10), la(0, 4, 100, 4900, 100, 4900, 10), la(0, 4, 200, 4800, 200, 4800, 10),
        # read 5: nested on A, not on the read; read 6: on another contig
        la(0, 5, 0, 5000, 0, 5000, 10), la(0, 5, 100, 4900, 5000, 9800, 10),
        la(0, 6, 0, 5000, 0, 5000, 10), la(1, 6, 100, 4900, 5100, 9900, 10),
    ]
    return case(rows, [100_000, 100_000], [200_000] * 7, opts=LOOSE)   # (reads longer than the contigs: none is redundant)


# ------------------------------------------------------------------------------------------------ random sets and the planted scenario
def random_las(rng, nreads, ncontigs, clen, rlen):
    """the generator of tests/test_collect_filters.py"""
    rows = []
    for r in range(nreads):
        for _ in range(int(rng.integers(1, 4))):
            c, comp = int(rng.integers(0, ncontigs)), int(rng.integers(0, 2))
            ln = int(rng.integers(600, 5000))
            kind = rng.random()
            if kind < 0.35:
                ab, bb = 0, rlen - ln
            elif kind < 0.7:
                ab, bb = clen - ln, 0
            elif kind < 0.85:
                ab, bb, ln = int(rng.integers(1000, clen - 7000)), 0, rlen
            else:
                ab, bb = int(rng.integers(100, clen - 6000)), int(rng.integers(100, rlen - ln))
            d = int(ln * rng.choice([0.05, 0.13, 0.2, 0.35]))
            rows.append(la(c, r, ab, ab + ln, bb, bb + ln, d, comp))
            if rng.random() < 0.15:
                rows.append(la(c, r, ab + 50, ab + ln - 50, bb + 50, bb + ln - 50, d // 2, comp))
    out = np.stack(rows)
    return out[rng.permutation(len(out))]


def random_case(seed, chains):
    rng = np.random.default_rng(seed)
    nc, nr, clen, rlen = 5, 60, 20000, 9000 if chains else 6000
    base = random_las(rng, nr, nc, clen, rlen)
    rows = []
    if chains:   # a third of the records split into a chain of two around a gap of 0 .. 2 kb
        for r in base[np.argsort(base["bread"], kind="stable")]:
            ln = int(r["aepos"] - r["abpos"])
            if rng.random() < 0.33 and ln > 1500:
                cut, gap = int(rng.integers(500, ln - 500)), int(rng.integers(0, 2000))
                p, q = r.copy(), r.copy()
                p["aepos"], p["bepos"], p["diffs"] = r["abpos"] + cut, r["bbpos"] + cut, r["diffs"] // 2
                q["abpos"], q["bbpos"], q["diffs"] = r["abpos"] + cut + 20, min(int(r["bepos"]) - 10, int(r["bbpos"]) + cut + 20 + gap), \
                    r["diffs"] - r["diffs"] // 2
                if q["abpos"] < q["aepos"] and q["bbpos"] < q["bepos"]:
                    rows.append(chained([p, q]))
                    continue
            r = r.copy()
            r["flags"] |= START
            rows.append(r)
    else:
        rows = [base]
    mask = (np.arange(nc + 1) * 2, np.tile(np.asarray([0, 4000, 15000, 19990]), nc))
    return case(rows, [clen] * nc, [rlen] * nr, mask=mask)


def planted_case():
    """tests/test_collect_filters.py::test_planted_scenario: dropped [1, 1, 1, 1, 2, 1]"""
    rows = [
        la(0, 0, 7000, 10000, 0, 3000, 300), la(1, 0, 0, 2900, 3100, 6000, 300), la(0, 1, 7000, 10000, 0, 3000, 1200),
        la(0, 2, 3000, 5000, 2000, 4000, 100), la(0, 3, 9400, 10000, 0, 600, 50), la(0, 4, 6000, 10000, 0, 4000, 300),
        la(0, 4, 6050, 10000, 50, 4000, 290), la(0, 5, 7000, 10000, 0, 3000, 300), la(1, 5, 0, 4000, 2000, 6000, 300),
        la(0, 6, 1000, 7000, 0, 6000, 500),
    ]
    return case(rows, [10000, 10000], [6000] * 7, mask=([0, 1, 1], [9300, 10000]))


def empty_reads_case():
    """reads without records at the front, in the middle and at the end"""
    rows = [la(0, 2, 0, 3000, 3000, 6000, 100), la(0, 2, 100, 2900, 3100, 5900, 100), la(0, 5, 1000, 7000, 0, 6000, 100)]
    return case(rows, [10000], [6000] * 9)


def scan_blocks_case(nreads=4200, block=2048):
    """both device scans across their blocks of 2048 values: three blocks of per-record flags and of the nreads + 1 per-read
    counts.  Most reads have one chain of one record (every 97th of low quality); reads at the front, around the first block
    boundary and at the end have none; read block + 4 has a chain of two, whose records are block - 1 and block, and a unit
    inside it on the same strand (Contained): its unit ids and its read offset need the carry of the block in front"""
    empty = {0, 1, block - 1, block, block + 1, nreads - 2, nreads - 1}
    rows = []
    for r in range(nreads):
        if r in empty:
            continue
        if r == block + 4:
            assert sum(len(np.atleast_1d(x)) for x in rows) == block - 1
            rows.append(chain_of(2, 0, r, 500, 1000))             # (the read sticks out of the contig: not redundant)
            rows.append(la(0, r, 600, 1300, 1100, 1800, 10))
            continue
        rows.append(la(r & 1, r, 0, 3000, 1000, 4000, 1200 if r % 97 == 0 else 100, (r >> 1) & 1))
    return case(rows, [100_000, 100_000], [4000] * nreads, opts=LOOSE)


def all_disabled_case():
    c = planted_case()
    c["las"]["flags"] |= DISABLED
    return c


RANDOM = {f"random_{s}": random_case(s, False) for s in (1, 2, 3)}
RANDOM.update({f"random_chains_{s}": random_case(100 + s, True) for s in (1, 2, 3)})

SHAPES = {
    "units_1": units_of_a_read(1, 11), "units_2": units_of_a_read(2, 12), "units_63": units_of_a_read(63, 13),
    "units_64": units_of_a_read(64, 14), "units_65": units_of_a_read(65, 15), "units_700": units_of_a_read(700, 16),
    "ambiguous_2": ambiguous_read(2), "ambiguous_64": ambiguous_read(64), "ambiguous_65": ambiguous_read(65),
    "chains": chains_case(), "boundaries": boundaries_case(), "many_intervals": many_intervals_case(), "contained": contained_case(),
    "planted": planted_case(), "empty_reads": empty_reads_case(), "all_disabled": all_disabled_case(),
    "no_mask": dict(planted_case(), mask=None), "no_records": case([], [1000], [100, 100]), "scan_blocks": scan_blocks_case(),
}
SHAPES.update(RANDOM)
# the tiers at their boundaries: name -> (reads of the wave tier, of the LDS tier, of the global tier) with the default cap and
# with DH_CFILT_LDS_UNITS = LOW_CAP
TIERS = {"units_63": ((1, 0, 0), (1, 0, 0)), "units_64": ((1, 0, 0), (1, 0, 0)), "units_65": ((0, 1, 0), (0, 0, 1)),
         "units_700": ((0, 1, 0), (0, 0, 1)), "ambiguous_65": ((0, 1, 0), (0, 0, 1))}


def refusals():
    """(name, case, the words dh_last_error has to hold)"""
    good = planted_case()
    out = []
    for field, idx in (("aread", (3, 7)), ("bread", (4, 9))):
        for bad in (-1, 99):
            c = dict(good, las=good["las"].copy())
            for i in idx:
                c["las"][field][i] = bad
            out.append((f"{field}_{bad}", c, f"record {idx[0]}: {field} out of range"))
    three = case(list(good["las"]), [10000, 10000, 10000], [6000] * 7)
    out.append(("mask_unsorted", dict(three, mask=(np.asarray([0, 1, 3, 5]), np.asarray([0, 10, 50, 60, 20, 30, 5, 9, 0, 4]))),
                "contig 1: the mask intervals are not sorted and disjoint"))
    out.append(("mask_overlap", dict(three, mask=(np.asarray([0, 0, 0, 2]), np.asarray([0, 10, 9, 30]))),
                "contig 2: the mask intervals are not sorted and disjoint"))
    out.append(("mask_outside", dict(three, mask=(np.asarray([0, 1, 2, 2]), np.asarray([0, 10, 9000, 10001]))),
                "contig 1: a mask interval lies outside the contig"))
    return out
