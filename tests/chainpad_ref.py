"""The chain padder's contract (dh_la_chain_paths; AlignmentPadder, dazzler.d:2249-2607) in plain Python: the two
translations, the junction rule, the segment list and the status of a chain, and its ops from the oracle's NW (no free shift
for tiles, free shift for fillers, the faked filler).  Not a test module."""
import numpy as np

import nw_ref
from dentist_amd import sim
from oracle import pyoracle as oz

OK, FAKED, NESTED = 0, 1, 2


def ntiles(la, ts):
    return int(la["tlen"]) // 2


def points(la, trace, ts):
    """the trace points of a record as (A, B) pairs: its begin, its tile ends, its end"""
    nt = ntiles(la, ts)
    tb = trace[int(la["toff"]) + 1:int(la["toff"]) + 2 * nt:2].astype(np.int64)
    ab, ae = int(la["abpos"]), int(la["aepos"])
    pa = [ab] + [ae if (i >= nt or (ab // ts + i) * ts > ae) else (ab // ts + i) * ts for i in range(1, nt + 1)]
    pb = [int(la["bbpos"])] + (int(la["bbpos"]) + np.cumsum(tb)).tolist()
    return list(zip(pa, pb))


def translate(pts, pos, onb, mode):
    """index of the last point at or before pos (mode 0, floor) / the first at or behind it (mode 1, ceil)"""
    c = [p[1] if onb else p[0] for p in pts]
    if mode == 0:
        idx = [i for i, x in enumerate(c) if x <= pos]
        return idx[-1] if idx else 0
    idx = [i for i, x in enumerate(c) if x >= pos]
    return idx[0] if idx else len(pts) - 1


def junction(p, q, pp, qp, s):
    """(status, end of p's tile run, start of q's, filler a0, a1, b0, b1)"""
    if p["aepos"] <= q["abpos"] and p["bepos"] <= q["bbpos"]:
        return OK, len(pp) - 1, 0, int(p["aepos"]), int(q["abpos"]), int(p["bepos"]), int(q["bbpos"])
    begins, ends = [], []
    if p["aepos"] > q["abpos"]:
        begins.append(translate(pp, int(q["abpos"]), False, 0))
        ends.append(translate(qp, int(p["aepos"]), False, 1))
    if p["bepos"] > q["bbpos"]:
        begins.append(translate(pp, int(q["bbpos"]), True, 0))
        ends.append(translate(qp, int(p["bepos"]), True, 1))
    b = min(begins, key=lambda i: pp[i][0])  # (the first one on a tie: the A resolution)
    e = max(ends, key=lambda i: qp[i][0])
    (a0, b0), (a1, b1) = pp[b], qp[e]
    status = NESTED if (b < s or a1 < a0 or b1 < b0) else OK
    return status, b, e, a0, a1, b0, b1


def segments(las, trace, ts):
    """(status, segments) of one chain: ("t", record, first tile, end tile) and ("f", record p, a0, a1, b0, b1)"""
    pts = [points(la, trace, ts) for la in las]
    segs, s = [], 0
    for k in range(len(las)):
        nt = len(pts[k]) - 1
        if k + 1 == len(las):
            if nt > s:
                segs.append(("t", k, s, nt))
            break
        st, pe, qs, a0, a1, b0, b1 = junction(las[k], las[k + 1], pts[k], pts[k + 1], s)
        if st != OK:
            return st, []
        if pe > s:
            segs.append(("t", k, s, pe))
        if a1 > a0 or b1 > b0:
            segs.append(("f", k, a0, a1, b0, b1))
        s = qs
    return OK, segs


def faked(a, b):
    la, lb = len(a), len(b)
    n = abs(la - lb)
    x, y = (a[n:], b) if la > lb else (a, b[n:])
    return np.concatenate([np.full(n, 2 if la < lb else 1, np.uint8), np.where(x == y, 0, 3).astype(np.uint8)])


def filler_ops(a, b):
    """(ops, faked, aligned on the device) of one filler"""
    if len(a) == 0 or len(b) == 0:
        return np.full(len(a) + len(b), 1 if len(a) else 2, np.uint8), False, False
    if len(a) > nw_ref.MAX_LEN or len(b) > nw_ref.MAX_LEN:
        return faked(a, b), True, False
    score, ops = nw_ref.oracle(a, b, True)
    status, _, _ = nw_ref.expected_attempts(len(a), len(b), 1, score)  # (the band policy of dh_nw.h on the true score)
    if status != 0:
        return faked(a, b), True, False
    return ops, False, True


def tile_ops(a, b):
    return nw_ref.oracle(a, b, False)[1]


def chain_ops(las, trace, ts, aseq, bseq):
    """(status, ops, score, fillers aligned) of one chain; bseq is the B read in the chain's frame"""
    st, segs = segments(las, trace, ts)
    if st == NESTED:
        return NESTED, np.zeros(0, np.uint8), -1, 0
    pts = [points(la, trace, ts) for la in las]
    out, nf = [], 0
    for sg in segs:
        if sg[0] == "t":
            _, k, t0, t1 = sg
            for t in range(t0, t1):
                (a0, b0), (a1, b1) = pts[k][t], pts[k][t + 1]
                out.append(tile_ops(aseq[a0:a1], bseq[b0:b1]))
        else:
            _, k, a0, a1, b0, b1 = sg
            ops, fk, dev = filler_ops(aseq[a0:a1], bseq[b0:b1])
            out.append(ops)
            nf += dev
            if fk:
                st = FAKED
    ops = np.concatenate(out).astype(np.uint8) if out else np.zeros(0, np.uint8)
    return st, ops, int(np.count_nonzero(ops)), nf


def chains_of(las, chain_off=None):
    if chain_off is not None:
        return [int(x) for x in chain_off]
    off = [i for i in range(len(las)) if i == 0 or not (las[i]["flags"] & 8)]
    return off + [len(las)]


def run(case):
    """the whole call on a case of chainpad_cases: (op_off, ops, score, status, fillers)"""
    las, trace, ts = case["las"], case["trace"], case["ts"]
    off = chains_of(las, case.get("chain_off"))
    rc = {}
    op_off, ops, score, status, fillers = [0], [], [], [], 0
    for c in range(len(off) - 1):
        ch = las[off[c]:off[c + 1]]
        a = case["A"].seq(int(ch[0]["aread"]))
        br = int(ch[0]["bread"])
        if ch[0]["flags"] & 1:
            if br not in rc:
                rc[br] = sim.revcomp(case["B"].seq(br))
            b = rc[br]
        else:
            b = case["B"].seq(br)
        st, o, sc, nf = chain_ops(ch, trace, ts, a, b)
        ops.append(o)
        op_off.append(op_off[-1] + len(o))
        score.append(sc)
        status.append(st)
        fillers += nf
    return (np.asarray(op_off, np.int64), np.concatenate(ops) if ops else np.zeros(0, np.uint8), np.asarray(score, np.int32),
            np.asarray(status, np.int32), fillers)


def replay(ops, a, b):
    """True when the ops consume exactly a and b and their codes 0 / 3 tell equal from unequal bases"""
    i = j = 0
    for op in ops:
        if op == 0 or op == 3:
            if i >= len(a) or j >= len(b) or (a[i] == b[j]) != (op == 0):
                return False
            i, j = i + 1, j + 1
        elif op == 1:
            i += 1
        else:
            j += 1
    return i == len(a) and j == len(b)
