"""Shared by the affine-gap global-alignment tests (dh_nw_affine_batch): a plain full-matrix Gotoh with the traceback rule
the kernel has to follow op for op, and a restatement of the host's band policy (dh_nwa.h: costs, band, accepted, next_w,
band_class) from which the expected status, the number of attempts and the kernel class of a pair follow.  Not a test module.

Scoring (match, mismatch, gap_open, gap_extend): equal bytes score match, other pairs mismatch, a gap of k bases
-(gap_open + k * gap_extend), end gaps included.  The matrices hold costs: cm = 2 (match - mismatch) per unequal pair,
ce = 2 gap_extend + match per gap base, co = 2 gap_open per gap, and 2 score = match (rl + ql) - cost.

Traceback rule, from (rl, ql) in state H:
  H: among the sources that attain H[i][j] -- H[i-1][j-1] + sub, E[i][j], F[i][j] -- the diagonal, then E, then F; but where
     the diagonal ties with E or F it is taken only if sub >= ce (the smaller predecessor: H - sub against H - ce).  That
     clause is what makes (0, -1, 0, 1) findAlignment's rule, which moves to the neighbour of the smallest score;
  E at (i, j): an insertion, move to (i, j-1); back to H there if H[i][j-1] + co + ce == E[i][j] (opening wins a tie), else E;
  F at (i, j): a deletion, move to (i-1, j); back to H there if H[i-1][j] + co + ce == F[i][j], else F;
  at a border: deletions, then insertions.
Ops: 0 match, 3 mismatch, 2 insertion (query base only), 1 deletion (reference base only)."""
import numpy as np

from nw_ref import mutate, pair_of  # noqa: F401  (the seeded pairs of the unit-cost tests)

DEFAULT = (5, -4, 16, 4)
W0 = 64
INF = 1 << 40


def costs(sc):
    """(cm, ce, co) or None when the host refuses the scoring (cm < 0, ce <= 0, co < 0; the overflow bound is the
    library's own and is not restated)"""
    match, mismatch, gap_open, gap_extend = (int(x) for x in sc)
    cm, ce, co = 2 * (match - mismatch), 2 * gap_extend + match, 2 * gap_open
    if cm < 0 or ce <= 0 or co < 0:
        return None
    return cm, ce, co


def score_of(sc, rl, ql, cost):
    v = int(sc[0]) * (rl + ql) - cost
    assert v % 2 == 0
    return v // 2


def matrices(ref, qry, sc):
    """H, E, F of the full matrix as int64 arrays of (rl + 1, ql + 1)"""
    cm, ce, co = costs(sc)
    r, q = np.asarray(ref, dtype=np.uint8), np.asarray(qry, dtype=np.uint8)
    rl, ql = len(r), len(q)
    H = np.full((rl + 1, ql + 1), INF, np.int64)
    E = np.full((rl + 1, ql + 1), INF, np.int64)
    F = np.full((rl + 1, ql + 1), INF, np.int64)
    jj = np.arange(ql + 1, dtype=np.int64)
    H[0] = co + ce * jj
    E[0] = H[0]
    H[0, 0] = 0
    E[0, 0] = INF
    for i in range(1, rl + 1):
        F[i] = np.minimum(H[i - 1] + co + ce, F[i - 1] + ce)
        F[i, 0] = co + ce * i
        G = np.full(ql + 1, INF, np.int64)
        G[1:] = np.minimum(H[i - 1, :-1] + np.where(q != r[i - 1], cm, 0), F[i, 1:])
        G[0] = F[i, 0]
        # E[j] = min over j' < j of H[j'] + co + ce (j - j'); a term with H[j'] = E[j'] < G[j'] is never below the term that
        # extends that gap, so G stands in for H (gotoh_plain below does not use this)
        pm = np.minimum.accumulate(G - ce * jj)
        E[i, 1:] = pm[:-1] + ce * jj[1:] + co
        H[i] = np.minimum(G, E[i])
    return H, E, F


def gotoh_plain(ref, qry, sc):
    """the same three matrices cell by cell, straight from the definition (for short sequences)"""
    cm, ce, co = costs(sc)
    rl, ql = len(ref), len(qry)
    H = [[INF] * (ql + 1) for _ in range(rl + 1)]
    E = [[INF] * (ql + 1) for _ in range(rl + 1)]
    F = [[INF] * (ql + 1) for _ in range(rl + 1)]
    H[0][0] = 0
    for j in range(1, ql + 1):
        H[0][j] = E[0][j] = co + ce * j
    for i in range(1, rl + 1):
        H[i][0] = F[i][0] = co + ce * i
        for j in range(1, ql + 1):
            E[i][j] = min(H[i][j - 1] + co + ce, E[i][j - 1] + ce)
            F[i][j] = min(H[i - 1][j] + co + ce, F[i - 1][j] + ce)
            H[i][j] = min(H[i - 1][j - 1] + (cm if ref[i - 1] != qry[j - 1] else 0), E[i][j], F[i][j])
    return np.asarray(H, np.int64), np.asarray(E, np.int64), np.asarray(F, np.int64)


def walk(ref, qry, sc, H, E, F):
    """ops of the traceback rule, in path order"""
    cm, ce, co = costs(sc)
    i, j = len(ref), len(qry)
    ops = []
    state = "H"
    while i > 0 and j > 0:
        if state == "H":
            mm = ref[i - 1] != qry[j - 1]
            sub = cm if mm else 0
            gap = E[i, j] == H[i, j] or F[i, j] == H[i, j]
            if H[i - 1, j - 1] + sub == H[i, j] and (sub >= ce or not gap):
                ops.append(3 if mm else 0)
                i, j = i - 1, j - 1
                continue
            state = "E" if E[i, j] == H[i, j] else "F"
        if state == "E":
            ops.append(2)
            state = "H" if H[i, j - 1] + co + ce == E[i, j] else "E"
            j -= 1
        else:
            ops.append(1)
            state = "H" if H[i - 1, j] + co + ce == F[i, j] else "F"
            i -= 1
    ops += [1] * i + [2] * j
    return np.asarray(ops[::-1], dtype=np.uint8)


def align(ref, qry, sc=DEFAULT):
    """(score, cost, ops) of the full matrix"""
    r, q = np.ascontiguousarray(ref, dtype=np.uint8), np.ascontiguousarray(qry, dtype=np.uint8)
    cm, ce, co = costs(sc)
    if len(r) == 0 or len(q) == 0:
        k = len(r) + len(q)
        cost = co + ce * k if k else 0
        return score_of(sc, len(r), len(q), cost), cost, np.full(k, 1 if len(r) else 2, np.uint8)
    H, E, F = matrices(r, q, sc)
    cost = int(H[-1, -1])
    return score_of(sc, len(r), len(q), cost), cost, walk(r, q, sc, H, E, F)


def score_of_ops(ref, qry, ops, sc):
    """the score of an alignment straight from the scoring's definition"""
    match, mismatch, gap_open, gap_extend = (int(x) for x in sc)
    i = j = s = 0
    prev = None
    for op in ops:
        op = int(op)
        if op in (0, 3):
            assert (ref[i] == qry[j]) == (op == 0)
            s += match if op == 0 else mismatch
            i, j = i + 1, j + 1
        else:
            s -= gap_extend + (gap_open if op != prev else 0)
            i, j = i + (op == 1), j + (op == 2)
        prev = op
    assert (i, j) == (len(ref), len(qry))
    return s


# ---- the host's policy


def band(rl, ql, w):
    d = ql - rl
    lo, hi = max(min(d, 0) - w, -rl), min(max(d, 0) + w, ql)
    return lo, hi, (lo == -rl and hi == ql)


def accepted(cost, w, ce, full):
    return full or cost <= ce * w


def band_class(W):
    return (4 if W <= 256 else (8 if W <= 512 else 16)), (1 if W <= 1024 else 2)


def next_w(rl, ql, w_prev, w0, max_w):
    fits = lambda x: band(rl, ql, x)[1] - band(rl, ql, x)[0] + 1 <= max_w
    w = 2 * w_prev if w_prev else w0
    if fits(w):
        return w
    a, b = w_prev, w
    while b - a > 1:
        m = (a + b) // 2
        a, b = (m, b) if fits(m) else (a, m)
    return -1 if a == w_prev else a


def expected_attempts(rl, ql, cost, ce, max_w, w0=W0):
    """(status, attempts, last half-width) of a pair whose full-matrix cost is `cost`: a band is accepted exactly when the
    predicate holds for the TRUE cost (then the banded corner is exact; and an accepted band is exact)"""
    w, k = 0, 0
    while True:
        w = next_w(rl, ql, w, w0, max_w)
        if w < 0:
            return 1, k, 0
        k += 1
        if accepted(cost, w, ce, band(rl, ql, w)[2]):
            return 0, k, w


def first_words(rl, ql, max_w, w0=W0):
    """decision words (64 bits, sixteen cells) of a pair's first attempt"""
    if rl == 0 or ql == 0:
        return 0
    w = next_w(rl, ql, 0, w0, max_w)
    if w < 0:
        return 0
    lo, hi, _ = band(rl, ql, w)
    return rl * ((hi - lo + 1 + 15) // 16)
