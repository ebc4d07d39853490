"""Brute-force restatement of the contract of dh_la_chain (include/dentist_hip.h, "chaining of local alignments"), written
from that text alone: no code is shared with chain_pair of dh_tracepoint.cpp, with dh_chain.h or with the oracle.  Plain Python
integers and floats (a Python float is the C double).

chain(las, **opts) returns the chains in output order, each as (record indices, flags, score); arrays() flattens them into
the four arrays of the C ABI."""
import numpy as np

COMP, START, NEXT, BEST, DISABLED = 0x1, 0x4, 0x8, 0x10, 0x20
CHAIN_FLAGS = START | NEXT | BEST

DEFAULTS = dict(max_indel=1000, max_chain_gap=10000, min_score=100, max_relative_overlap=0.3, min_relative_score=1.0)


class Unordered(ValueError):
    def __init__(self, index):
        super().__init__(f"record {index} precedes the enabled record before it")
        self.index = index


def _c_div(a, b):
    """C integer division (truncation towards zero)"""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def _threshold(min_score, rel, best):
    return int(max(float(min_score), rel * best))  # int(): truncation, as the C cast


def _chain_pair(las, idxs, o):
    """the chains of one pair: [(record indices, flags, score)] in output order"""
    order = sorted(idxs, key=lambda i: (int(las[i]["abpos"]), int(las[i]["bbpos"]), i))
    n = len(order)
    ab = [int(las[i]["abpos"]) for i in order]
    ae = [int(las[i]["aepos"]) for i in order]
    bb = [int(las[i]["bbpos"]) for i in order]
    be = [int(las[i]["bepos"]) for i in order]
    comp = [int(las[i]["flags"]) & COMP for i in order]
    score = [_c_div((ae[v] - ab[v]) + (be[v] - bb[v]), 2) for v in range(n)]

    def chainable(u, v):
        if comp[u] != comp[v] or not (ab[u] < ab[v] and bb[u] < bb[v]):
            return False
        ga, gb = ab[v] - ae[u], bb[v] - be[u]
        if abs(ga - gb) > o["max_indel"] or max(abs(ga), abs(gb)) > o["max_chain_gap"]:
            return False
        mla, mlb = min(ae[u] - ab[u], ae[v] - ab[v]), min(be[u] - bb[u], be[v] - bb[v])
        return max(0, -ga) <= o["max_relative_overlap"] * mla and max(0, -gb) <= o["max_relative_overlap"] * mlb

    dist = [-s for s in score]
    pred = [-1] * n
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for u in range(n):
        for v in range(u + 1, n):
            if ab[v] - ae[u] > o["max_chain_gap"]:
                break  # abpos ascends: nothing further is chainable
            if not chainable(u, v):
                continue
            ga, gb = ab[v] - ae[u], bb[v] - be[u]
            d = dist[u] + abs(ga - gb) + _c_div(max(abs(ga), abs(gb)), 10) - score[v]
            if dist[v] > d:
                dist[v], pred[v] = d, u
            ru, rv = find(u), find(v)
            if ru != rv:
                parent[max(ru, rv)] = min(ru, rv)
    label = [find(v) for v in range(n)]
    sel = sorted(range(n), key=lambda v: (label[v], dist[v], v))
    taken = [False] * n
    chains = []  # (end, alternate)
    cur, cthr = None, 0
    for e in sel:
        if label[e] != cur:
            cur, cthr = label[e], _threshold(o["min_score"], o["min_relative_score"], -dist[e])
        if taken[e] or -dist[e] < cthr:
            continue
        alt, v = False, e
        while v >= 0:
            if taken[v]:
                alt = True
                break  # every ancestor of a taken node is taken
            taken[v] = True
            v = pred[v]
        chains.append((e, alt))
    if not chains:
        return []
    thr = _threshold(o["min_score"], o["min_relative_score"], max(-dist[e] for e, _ in chains))
    out = []
    for e, alt in chains:
        if -dist[e] < thr:
            continue
        path, v = [], e
        while v >= 0:
            path.append(v)
            v = pred[v]
        path.reverse()
        out.append(((ab[path[0]], bb[path[0]], ae[e], be[e], e), path, alt, -dist[e]))
    out.sort(key=lambda c: c[0])
    res = []
    for _, path, alt, sc in out:
        recs = [order[v] for v in path]
        flags = [(int(las[i]["flags"]) & ~CHAIN_FLAGS) | (NEXT if k else (START | (0 if alt else BEST))) for k, i in enumerate(recs)]
        res.append((recs, flags, sc))
    return res


def chain(las, **opts):
    o = dict(DEFAULTS)
    o.update(opts)
    pairs, prev = [], None
    for i in range(len(las)):
        if int(las[i]["flags"]) & DISABLED:
            continue
        key = (int(las[i]["aread"]), int(las[i]["bread"]))
        if prev is not None and key < prev:
            raise Unordered(i)
        if key != prev:
            pairs.append([])
        pairs[-1].append(i)
        prev = key
    out = []
    for idxs in pairs:
        out.extend(_chain_pair(las, idxs, o))
    return out


def arrays(chains):
    """(off, score, src_index, flags) of the C ABI"""
    off = np.zeros(len(chains) + 1, dtype=np.int64)
    if chains:
        off[1:] = np.cumsum([len(c[0]) for c in chains])
    score = np.asarray([c[2] for c in chains], dtype=np.int32)
    src = np.asarray([i for c in chains for i in c[0]], dtype=np.int64)
    flags = np.asarray([f for c in chains for f in c[1]], dtype=np.uint32)
    return off, score, src, flags
