"""Plain restatement of the exact transposition of a local alignment (dh_la_transpose, include/dentist_hip.h): the expected
value of the transposition tests.  tests/test_transpose_restatement.py pins it to two hand-worked vectors."""
import numpy as np

CHAIN_BITS = 0x4 | 0x8 | 0x10 | 0x20  # START, NEXT, BEST, DISABLED
KEYS = ("aread", "bread", "comp", "abpos", "aepos", "bbpos", "bepos", "diffs")  # LAsort order, base.d:1787-1809


def transposed_ops(ops, comp):
    """the ops with codes 1 and 2 exchanged, for a COMP record in reverse order"""
    ops = np.asarray(ops, dtype=np.uint8)
    out = ops.copy()
    out[ops == 1] = 2
    out[ops == 2] = 1
    return out[::-1].copy() if comp else out


def transpose_record(abpos, aepos, bbpos, bepos, comp, ops, ts, alen=None, blen=None):
    """(abpos', aepos', bbpos', bepos', ops', [(diffs, bbases), ...], code-2 ops that directly follow a grid crossing)"""
    if comp:
        ab, ae, bb, be = blen - bepos, blen - bbpos, alen - aepos, alen - abpos
    else:
        ab, ae, bb, be = bbpos, bepos, abpos, aepos
    t = transposed_ops(ops, comp)
    tiles, d, b, pos, after_crossing, follows = [], 0, 0, ab, False, 0
    for op in t.tolist():
        if after_crossing and op == 2:
            follows += 1
        after_crossing = False
        d += op != 0
        b += op != 1
        if op != 2:
            pos += 1
            if pos % ts == 0 and pos < ae:  # a grid point strictly inside (abpos', aepos'): the tile ends after this op
                tiles.append((d, b))
                d = b = 0
                after_crossing = True
    tiles.append((d, b))  # the last tile takes everything up to the end of the path
    assert pos == ae and sum(x for _, x in tiles) == be - bb
    return ab, ae, bb, be, t, tiles, follows


def transpose_set(las, ep, ts, alens, blens, la_dtype):
    """The transposed set of `las` from their edit paths `ep` (Context.edit_paths): (las', trace', src_index, stats) with
    the records in LAsort order (equal keys: by source index), toff in source order.  stats counts the records with
    abpos' / aepos' on the grid, with a single tile, and the code-2 ops right behind a grid crossing."""
    n = len(las)
    out = np.zeros(n, dtype=la_dtype)
    trace = []
    stats = dict(abpos_on_grid=0, aepos_on_grid=0, single_tile=0, code2_after_crossing=0)
    for i, la in enumerate(las):
        comp = int(la["flags"]) & 1
        ops = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        ab, ae, bb, be, _, tiles, follows = transpose_record(int(la["abpos"]), int(la["aepos"]), int(la["bbpos"]), int(la["bepos"]),
                                                             comp, ops, ts, int(alens[la["aread"]]), int(blens[la["bread"]]))
        o = out[i]
        o["aread"], o["bread"] = la["bread"], la["aread"]
        o["abpos"], o["aepos"], o["bbpos"], o["bepos"] = ab, ae, bb, be
        o["flags"] = int(la["flags"]) & ~CHAIN_BITS
        o["tlen"], o["toff"] = 2 * len(tiles), len(trace)
        o["diffs"] = sum(d for d, _ in tiles)
        assert o["diffs"] == int(np.count_nonzero(ops))
        for d, b in tiles:
            trace += [d, b]
        stats["abpos_on_grid"] += ab % ts == 0
        stats["aepos_on_grid"] += ae % ts == 0
        stats["single_tile"] += len(tiles) == 1
        stats["code2_after_crossing"] += follows
    order = sorted(range(n), key=lambda i: tuple(int(out[i][k]) if k != "comp" else int(out[i]["flags"]) & 1 for k in KEYS) + (i,))
    src = np.asarray(order, dtype=np.int64)
    return out[src], np.asarray(trace, dtype=np.uint16), src, stats
