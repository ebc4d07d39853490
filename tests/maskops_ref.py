"""The contract of dh_mask_combine and dh_la_tandem_mask (include/dentist_hip.h) restated twice: per base on numpy boolean arrays
with the literal loops of commands/filterMask.d:124-159, and on intervals for coordinates too large for arrays.  A mask is
(ptr[ncontigs + 1], iv pairs); a result is a list of (contig, begin, end).  Not a test module."""
import numpy as np


def intervals_of(mask, c):
    ptr, iv = np.asarray(mask[0]), np.asarray(mask[1]).reshape(-1, 2)
    return [(int(b), int(e)) for b, e in iv[ptr[c]:ptr[c + 1]]]


def count_nonempty(masks, subtract=None):
    return sum(int(np.sum(np.asarray(m[1]).reshape(-1, 2)[:, 0] < np.asarray(m[1]).reshape(-1, 2)[:, 1]))
               for m in list(masks) + ([subtract] if subtract is not None else []))


def filter_runs(runs, min_gap, min_interval):
    """removeSmallGaps, then removeSmallContigs: runs = ascending (contig, begin, end)"""
    acc = []
    for c, b, e in runs:
        if acc and acc[-1][0] == c and acc[-1][2] + min_gap >= b:
            acc[-1][2] = e
        else:
            acc.append([c, b, e])
    return [(c, b, e) for c, b, e in acc if e - b >= min_interval]


def combine_bases(masks, contig_off, min_count=1, subtract=None, min_gap=0, min_interval=0):
    """per base: membership per mask, the threshold, the subtraction, the maximal runs, the two filters"""
    runs = []
    for c in range(len(contig_off) - 1):
        n = int(contig_off[c + 1] - contig_off[c])
        cov = np.zeros(n, dtype=np.int64)
        for m in masks:
            member = np.zeros(n, dtype=bool)
            for b, e in intervals_of(m, c):
                member[b:e] = True
            cov += member
        kept = cov >= min_count
        if subtract is not None:
            for b, e in intervals_of(subtract, c):
                kept[b:e] = False
        edge = np.flatnonzero(np.diff(np.concatenate([[0], kept.astype(np.int8), [0]])))
        runs += [(c, int(edge[k]), int(edge[k + 1])) for k in range(0, len(edge), 2)]
    return filter_runs(runs, min_gap, min_interval)


def normalize(ivs):
    """one contig's intervals -> ascending, disjoint, never touching; empty ones have no effect"""
    out = []
    for b, e in sorted(iv for iv in ivs if iv[0] < iv[1]):
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return out


def combine_intervals(masks, contig_off, min_count=1, subtract=None, min_gap=0, min_interval=0):
    """on intervals: every mask normalised, a walk over the distinct positions with the count of masks and of the subtract mask"""
    runs = []
    for c in range(len(contig_off) - 1):
        delta = {}
        for m in masks:
            for b, e in normalize(intervals_of(m, c)):
                delta.setdefault(b, [0, 0])[0] += 1
                delta.setdefault(e, [0, 0])[0] -= 1
        for b, e in normalize(intervals_of(subtract, c)) if subtract is not None else []:
            delta.setdefault(b, [0, 0])[1] += 1
            delta.setdefault(e, [0, 0])[1] -= 1
        cov = sub = 0
        start = None
        for pos in sorted(delta):
            cov, sub = cov + delta[pos][0], sub + delta[pos][1]
            kept = cov >= min_count and sub == 0
            if kept and start is None:
                start = pos
            elif not kept and start is not None:
                runs.append((c, start, pos))
                start = None
        assert start is None and cov == 0 and sub == 0
    return filter_runs(runs, min_gap, min_interval)


def tandem(las, read_off, first_read=0, min_len=500):
    """tools/TANmask's rule: the union per read of the self alignments on the same strand that are long enough"""
    per = {}
    for l in las:
        if l["aread"] != l["bread"] or (int(l["flags"]) & 1):
            continue
        b, e = int(min(l["abpos"], l["bbpos"])), int(max(l["aepos"], l["bepos"]))
        if e > b and e - b >= min_len:
            per.setdefault(int(l["aread"]) - first_read, []).append((b, e))
    return [(r, b, e) for r in sorted(per) for b, e in normalize(per[r])]
