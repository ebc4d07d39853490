"""The mask layer of a DB restated from its definitions, in plain numpy: the low-complexity mask (dh_db_dust), the
alignment-coverage mask (dh_db_mask_coverage) and the rule that says which alignments are improper.  Nothing here slides a
window or scans a shared difference array: a window's triplet counts come from per-code prefix counts, a sequence's
coverage from a difference array of its own.  A mask is (ptr int64[n + 1], iv int32 (begin, end) pairs, flat), what
Db.get_mask() and oracle.pyoracle.dust() return; the functions ending in _flags give it as one bool per base of the DB."""
import numpy as np

DUST_WINDOWS = (16, 32, 64)


def dust_threshold(L):
    """a window of L bases is low-complexity when its score is above this"""
    return 2 * (L - 3)


def intervals_of(flags, off):
    """runs of set flags as intervals per sequence; a run never continues into the next sequence"""
    flags = np.asarray(flags, dtype=bool)
    off = np.asarray(off, dtype=np.int64)
    total = int(off[-1])
    assert len(flags) == total
    nonempty = off[1:] > off[:-1]
    first = np.zeros(total, dtype=bool)
    last = np.zeros(total, dtype=bool)
    first[off[:-1][nonempty]] = True
    last[off[1:][nonempty] - 1] = True
    prev = np.concatenate([[False], flags[:-1]])
    nxt = np.concatenate([flags[1:], [False]])
    b = np.flatnonzero(flags & (~prev | first))
    e = np.flatnonzero(flags & (~nxt | last)) + 1
    seq = np.searchsorted(off, b, side="right") - 1
    iv = np.stack([b - off[seq], e - off[seq]], axis=1).astype(np.int32).reshape(-1)
    return np.searchsorted(b, off, side="left").astype(np.int64), iv


def flags_of(ptr, iv, off):
    """the bitmap of a mask given as intervals"""
    off = np.asarray(off, dtype=np.int64)
    iv = np.asarray(iv, dtype=np.int64).reshape(-1, 2)
    flags = np.zeros(int(off[-1]), dtype=bool)
    for s in range(len(off) - 1):
        for b, e in iv[ptr[s]:ptr[s + 1]]:
            flags[off[s] + b:off[s] + e] = True
    return flags


def triplet_codes(bases):
    """code of the triplet that starts at every base but the last two, -1 where it holds a code above 3"""
    b = np.asarray(bases, dtype=np.int32)
    if len(b) < 3:
        return np.zeros(0, dtype=np.int32)
    code = b[:-2] << 4 | b[1:-1] << 2 | b[2:]
    return np.where((b[:-2] > 3) | (b[1:-1] > 3) | (b[2:] > 3), -1, code)


def window_scores(bases):
    """{L: (S, clean)} for every window start of a run of bases: S = sum over triplet codes of c (c - 1) / 2 over the L - 2
    triplets inside the window, clean = the window holds no code above 3.  Windows are taken over the whole array: the
    caller keeps those that lie inside one sequence."""
    b = np.asarray(bases, dtype=np.uint8)
    total = len(b)
    code = triplet_codes(b)
    nonbase = np.concatenate([[0], np.cumsum(b > 3)])
    out = {L: np.zeros(max(total - L + 1, 0), dtype=np.int32) for L in DUST_WINDOWS}
    for t in range(64):
        pc = np.zeros(len(code) + 1, dtype=np.int32)  # triplets t that start before base i
        np.cumsum(code == t, dtype=np.int32, out=pc[1:])
        for L in DUST_WINDOWS:
            nw = total - L + 1
            if nw > 0:
                c = pc[L - 2:] - pc[:nw]
                out[L] += c * (c - 1) // 2
    return {L: (out[L], (nonbase[L:] - nonbase[:len(out[L])]) == 0) for L in DUST_WINDOWS}


def dust_flags(bases, off):
    b = np.asarray(bases, dtype=np.uint8)
    off = np.asarray(off, dtype=np.int64)
    total = len(b)
    assert total == int(off[-1])
    flags = np.zeros(total, dtype=bool)
    seq = np.repeat(np.arange(len(off) - 1), np.diff(off))
    for L, (S, clean) in window_scores(b).items():
        nw = len(S)
        if nw == 0:
            continue
        inside = seq[:nw] == seq[L - 1:]
        low = np.flatnonzero(inside & clean & (S > dust_threshold(L)))
        d = np.zeros(total + 1, dtype=np.int64)
        d[low] += 1
        np.add.at(d, low + L, -1)
        flags |= np.cumsum(d)[:total] > 0
    return flags


def dust_mask(bases, off):
    """DESIGN / dh_kernels.hip: a window of L in {16, 32, 64} bases is low-complexity when S > 2 (L - 3); windows holding a
    code above 3 are skipped; the mask is the union of the low windows of a sequence."""
    return intervals_of(dust_flags(bases, off), off)


def coverage_flags(lens, intervals, lower, upper):
    lens = np.asarray(lens, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])
    flags = np.zeros(int(off[-1]), dtype=bool)
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 3)
    if len(iv) == 0:  # no alignment at all: no mask
        return flags
    iv = iv[iv[:, 2] > iv[:, 1]]  # an empty interval covers nothing
    assert np.all((iv[:, 1] >= 0) & (iv[:, 2] <= lens[iv[:, 0]]))
    if 0 < lower or 0 > upper:
        flags[:] = True  # sequences without an interval have coverage 0 throughout
    iv = iv[np.argsort(iv[:, 0], kind="stable")]
    seqs, first = np.unique(iv[:, 0], return_index=True)
    for s, i0, i1 in zip(seqs.tolist(), first.tolist(), first.tolist()[1:] + [len(iv)]):
        d = np.zeros(int(lens[s]) + 1, dtype=np.int64)
        np.add.at(d, iv[i0:i1, 1], 1)
        np.add.at(d, iv[i0:i1, 2], -1)
        cov = np.cumsum(d, dtype=np.int64)[:lens[s]]
        flags[off[s]:off[s + 1]] = (cov < lower) | (cov > upper)
    return flags


def coverage_mask(lens, intervals, lower, upper):
    """intervals: (sequence, begin, end) rows.  The bases whose coverage is below lower or above upper, as runs."""
    lens = np.asarray(lens, dtype=np.int64)
    return intervals_of(coverage_flags(lens, intervals, lower, upper), np.concatenate([[0], np.cumsum(lens)]))


def improper(la, alen, blen, allowance):
    """base.d:537-557 as k_cov_events states it: proper = begins within the allowance of the begin of A or of B and ends
    within the allowance of the end of A or of B"""
    begins = int(la["abpos"]) <= allowance or int(la["bbpos"]) <= allowance
    ends = int(la["aepos"]) + allowance >= alen or int(la["bepos"]) + allowance >= blen
    return not (begins and ends)
