"""Shared by the global-alignment tests (dh_nw_batch): the oracle's answer in the library's op codes, seeded sequence pairs,
and a plain restatement of the host's band policy (dh_nw.h: band, accepted, next_w) from which the expected status and
the number of attempts of a pair follow.  Not a test module."""
import numpy as np

from oracle import pyoracle as oz

MAX_W = 4096   # widest band the kernel serves
MAX_LEN = 65536
W0 = 64        # first half-width


def oracle(ref, qry, free_shift):
    """(score, ops) of oracle/nw.c with its substitutions split into 0 match / 3 mismatch"""
    r, q = np.ascontiguousarray(ref, dtype=np.uint8), np.ascontiguousarray(qry, dtype=np.uint8)
    score, raw = oz.nw(r, q, 1, bool(free_shift))
    ops = raw.astype(np.uint8).copy()
    adv_r, adv_q = np.cumsum(raw != 2) - 1, np.cumsum(raw != 1) - 1
    sub = raw == 0
    ops[sub] = np.where(r[adv_r[sub]] == q[adv_q[sub]], 0, 3)
    return score, ops


def band(rl, ql, w, fs):
    d = ql - rl
    lo, hi = ((d, d) if fs else (min(d, 0), max(d, 0)))
    lo, hi = max(lo - w, -rl), min(hi + w, ql)
    return lo, hi, (lo == -rl and hi == ql)


def accepted(c, w, fs, full):
    return full or ((2 * (c + 1) <= w) if fs else (c + 1 <= w))


def next_w(rl, ql, fs, w_prev, w0=W0):
    fits = lambda x: band(rl, ql, x, fs)[1] - band(rl, ql, x, fs)[0] + 1 <= MAX_W
    w = 2 * w_prev if w_prev else w0
    if fits(w):
        return w
    a, b = w_prev, w
    while b - a > 1:
        m = (a + b) // 2
        a, b = (m, b) if fits(m) else (a, m)
    return -1 if a == w_prev else a


def expected_attempts(rl, ql, fs, score, w0=W0):
    """(status, attempts, last half-width) of a pair whose full-matrix score is `score`: a band is accepted exactly when
    the predicate holds for the TRUE score (then the banded corner is exact; and an accepted band is exact)"""
    w, k = 0, 0
    while True:
        w = next_w(rl, ql, fs, w, w0)
        if w < 0:
            return 1, k, 0
        k += 1
        if accepted(score, w, fs, band(rl, ql, w, fs)[2]):
            return 0, k, w


def first_words(rl, ql, fs, w0=W0):
    """decision words (32 bits) of a pair's first attempt"""
    if rl == 0 or ql == 0:
        return 0
    w = next_w(rl, ql, fs, 0, w0)
    if w < 0:
        return 0
    lo, hi, _ = band(rl, ql, w, fs)
    W = hi - lo + 1
    cpl = 4 if W <= 256 else (8 if W <= 512 else 16)
    return rl * ((W + cpl - 1) // cpl)


def mutate(rng, seq, div, ncodes=4):
    """a copy of seq with substitutions, insertions and deletions at rate div / 3 each"""
    x = rng.random(len(seq))
    keep = x >= div / 3
    out = seq.copy()
    sub = (x >= div / 3) & (x < 2 * div / 3)
    out[sub] = rng.integers(0, ncodes, int(sub.sum()))
    ins = (x >= 2 * div / 3) & (x < div)
    pieces = []
    last = 0
    for p in np.flatnonzero(ins | ~keep):
        pieces.append(out[last:p])
        if ins[p]:
            pieces.append(np.asarray([rng.integers(0, ncodes), out[p]], dtype=np.uint8))
        last = p + 1
    pieces.append(out[last:])
    return np.concatenate(pieces).astype(np.uint8) if pieces else out


def pair_of(rng, rl, ql, div, ncodes=4):
    """a reference of rl bases and a query of ql: the mutated reference cut or extended with random bases to ql"""
    r = rng.integers(0, ncodes, rl).astype(np.uint8)
    q = mutate(rng, r, div, ncodes)[:ql]
    if len(q) < ql:
        q = np.concatenate([q, rng.integers(0, ncodes, ql - len(q)).astype(np.uint8)])
    return r, q
