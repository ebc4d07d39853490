"""The contract of dh_la_repeat_mask restated in plain Python: records -> units (the collect filter's chain rule), unit intervals
and proper bits, then oracle.maskcov.bad_coverage_mask per assessor -- the reference's literal event machine stays the yardstick
-- and the touching-merging ReferenceRegion union.  Not a test module."""
from oracle import maskcov as mc

COMP, START, NEXT = 0x1, 0x4, 0x8


def continues(prev, cur):
    """dh_continues_chain / cf::continues"""
    f = int(cur["flags"])
    return bool(f & NEXT) and not (f & START) and int(cur["aread"]) == int(prev["aread"]) and int(cur["bread"]) == int(prev["bread"]) \
        and (f & COMP) == (int(prev["flags"]) & COMP)


def units_of(las):
    """[(first record, last record)] of every chain"""
    out, i = [], 0
    while i < len(las):
        e = i
        while e + 1 < len(las) and continues(las[e], las[e + 1]):
            e += 1
        out.append((i, e))
        i = e + 1
    return out


def is_proper(first, last, alen, blen, allowance):
    """base.d:537-557 on a chain: the first record's begins, the last record's ends"""
    begins = int(first["abpos"]) <= allowance or int(first["bbpos"]) <= allowance
    ends = int(last["aepos"]) + allowance >= alen or int(last["bepos"]) + allowance >= blen
    return begins and ends


def union(a, b):
    """util/region.d:776-816: sorted, intersecting or touching intervals merged; (contig, begin, end) triples"""
    out = []
    for c, s, e in sorted(a + b):
        if out and out[-1][0] == c and s <= out[-1][2]:
            out[-1] = (c, out[-1][1], max(out[-1][2], e))
        else:
            out.append((c, s, e))
    return out


def as_ptr_iv(triples, ncontigs):
    ptr, iv = [0] * (ncontigs + 1), []
    for c, s, e in triples:
        ptr[c + 1] += 1
        iv.append((s, e))
    for c in range(ncontigs):
        ptr[c + 1] += ptr[c]
    return ptr, iv


def repeat_mask(las, contig_off, read_off=None, lower=0, upper=4, improper=None, allowance=100):
    """{"mask", "all", "improper"}: sorted (contig, begin, end) triples; "units", "improper_units": the chains counted"""
    ncontigs = len(contig_off) - 1
    contigs = [(c, 0, int(contig_off[c + 1] - contig_off[c])) for c in range(ncontigs)]
    every, bad = [], []
    for i, e in units_of(las):
        f, l = las[i], las[e]
        c = int(f["aread"])
        iv = (c, int(f["abpos"]), int(l["aepos"]))
        every.append(iv)
        if improper is not None:
            r = int(f["bread"])
            if not is_proper(f, l, contigs[c][2], int(read_off[r + 1] - read_off[r]), allowance):
                bad.append(iv)
    res = {"all": sorted(mc.bad_coverage_mask(every, contigs, lower, upper)), "improper": [], "units": len(every), "improper_units": len(bad)}
    if improper is not None:
        res["improper"] = sorted(mc.bad_coverage_mask(bad, contigs, improper[0], improper[1]))
    res["mask"] = union(res["all"], res["improper"])
    return res
