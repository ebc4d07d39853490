"""The contract of dh_la_propagate_mask (include/dentist_hip.h; `dentist propagate-mask`, commands/propagateMask.d:136-305)
restated in plain Python: no ctypes, none of the library's code.  For every record and every mask interval of its A sequence
that intersects [abpos, aepos): cut to [abpos, aepos), begin translated to its trace point rounding down, end rounding up
(base.d:185-244), mirrored on complement records, empty results dropped; per destination sequence the union, by sorting and
merging intersecting or touching intervals."""
import bisect

import numpy as np

COMP = 0x1


def trace_point_floor(abpos, aepos, ntp, ts, apos):
    """index of the trace point at or before apos"""
    second = abpos // ts * ts + ts
    if apos < second:
        return 0
    if apos < aepos:
        return 1 + (apos - second) // ts
    return ntp


def trace_point_ceil(abpos, aepos, ntp, ts, apos):
    """index of the trace point at or behind apos"""
    second = abpos // ts * ts + ts
    second_from_last = (aepos - 1) // ts * ts
    if apos == abpos:
        return 0
    if apos <= second:
        return 1
    if apos <= second_from_last:
        return 1 + (apos - second + ts - 1) // ts
    return ntp


def raw_intervals(las, trace, tspace, mask_ptr, mask_iv, read_len):
    """([(read, begin, end)] before the union, empty ones included, in input order; records with an intersecting interval)"""
    mask_ptr = [int(x) for x in mask_ptr]
    flat = np.asarray(mask_iv, dtype=np.int64).reshape(-1).tolist()
    begins, ends = flat[0::2], flat[1::2]
    read_len = [int(x) for x in read_len]
    cols = {f: las[f].tolist() for f in ("aread", "bread", "abpos", "aepos", "bbpos", "flags", "tlen", "toff")}
    per_contig = {}
    raw, hit = [], 0
    for i in range(len(las)):
        c = cols["aread"][i]
        if c not in per_contig:
            per_contig[c] = (begins[mask_ptr[c]:mask_ptr[c + 1]], ends[mask_ptr[c]:mask_ptr[c + 1]])
        cb, ce = per_contig[c]
        ab, ae = cols["abpos"][i], cols["aepos"][i]
        lo = bisect.bisect_right(ce, ab)   # the first interval that ends after abpos
        hi = bisect.bisect_left(cb, ae)    # the first interval that begins at or after aepos
        if hi <= lo:
            continue
        hit += 1
        ntp, toff = cols["tlen"][i] // 2, cols["toff"][i]
        before = [0] + np.cumsum(np.asarray(trace[toff + 1:toff + 2 * ntp:2], dtype=np.int64)).tolist()  # b-bases before trace point k
        bb, rd = cols["bbpos"][i], cols["bread"][i]
        for j in range(lo, hi):
            b0 = bb + before[trace_point_floor(ab, ae, ntp, tspace, max(cb[j], ab))]
            b1 = bb + before[trace_point_ceil(ab, ae, ntp, tspace, min(ce[j], ae))]
            if cols["flags"][i] & COMP:
                b0, b1 = read_len[rd] - b1, read_len[rd] - b0
            raw.append((rd, b0, b1))
    return raw, hit


def union(raw):
    """{read: [(begin, end)]}: sorted, intersecting or touching intervals merged, empty ones dropped"""
    out = {}
    for rd, b, e in sorted(x for x in raw if x[2] > x[1]):
        ivs = out.setdefault(rd, [])
        if ivs and b <= ivs[-1][1]:
            ivs[-1] = (ivs[-1][0], max(ivs[-1][1], e))
        else:
            ivs.append((b, e))
    return out


def propagate(las, trace, tspace, mask_ptr, mask_iv, read_len):
    """({read: [(begin, end)]}, dict(raw=non-empty raw intervals, empty=empty ones, hit=records with an intersecting interval))"""
    raw, hit = raw_intervals(las, trace, tspace, mask_ptr, mask_iv, read_len)
    full = sum(1 for x in raw if x[2] > x[1])
    return union(raw), dict(raw=full, empty=len(raw) - full, hit=hit)


def arrays(result, nreads):
    """(ptr int64[nreads + 1], iv int32[m, 2]) of a {read: [(begin, end)]}"""
    ptr = np.zeros(nreads + 1, dtype=np.int64)
    rows = []
    for r in range(nreads):
        rows += result.get(r, [])
        ptr[r + 1] = len(rows)
    return ptr, np.asarray(rows, dtype=np.int32).reshape(-1, 2)


def as_dict(ptr, iv):
    """{read: [(begin, end)]} of (ptr, iv)"""
    iv = np.asarray(iv).reshape(-1, 2).tolist()
    return {r: [tuple(x) for x in iv[ptr[r]:ptr[r + 1]]] for r in range(len(ptr) - 1) if ptr[r + 1] > ptr[r]}
