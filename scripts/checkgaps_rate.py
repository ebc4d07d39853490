"""Timed calls of the gap analysis on constructed gaps (not a test): --gaps closed gaps (default 1 000) of 2..10 kb on one true
contig, each closed by the true sequence mutated at --div (default 0.02), crop 20, a dust interval in every gap.

  check_gaps   Context.check_gaps (dh_check_gaps): host checks, upload, bind, gather, the alignments, stats and download.
  nw_affine    Context.nw_affine_batch_raw alone on the same pairs from host memory (the upload of the pairs included).

Per variant: --reps calls after one warm-up call (wall time: median, min, max); one JSON line each on stdout, and a third with
what bind, gather and stats add (the difference of the medians).  The two sets of ops are compared before anything is timed.
--traced calls with DH_TRACE=1 print the library's line per call to stderr."""
import argparse
import json
import os
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dentist_amd  # noqa: E402


def mutate(rng, seq, div):
    x = rng.random(len(seq))
    out = seq.copy()
    sub = x < div / 3
    out[sub] = (out[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
    keep = ~((x >= div / 3) & (x < 2 * div / 3))
    dup = (x >= 2 * div / 3) & (x < div)
    return np.repeat(out[keep], 1 + dup[keep].astype(np.int64)).astype(np.uint8)


def workload(ngaps, div, crop, seed=5):
    rng = np.random.default_rng(seed)
    holes = rng.integers(2000, 10001, ngaps)
    clen = 400
    total = int(holes.sum()) + clen * (ngaps + 1) + 200
    true = rng.integers(0, 4, total).astype(np.uint8)
    mapped, maps, pieces, dust, at, pos = [], np.zeros(ngaps + 1, dentist_amd.CONTIG_MAPPING_DTYPE), [], [], 100, 0
    for k in range(ngaps + 1):
        mapped.append((1, at, at + clen))
        maps[k] = (1, pos + crop, pos + clen - crop, 0, k + 1, 0, 0, 0.0)
        pieces.append(true[at:at + clen])
        pos += clen
        if k < ngaps:
            ins = mutate(rng, true[at + clen:at + clen + holes[k]], div)
            pieces.append(ins)
            pos += len(ins)
            dust.append((at + clen + 100, at + clen + 600))
            at += clen + int(holes[k])
    result = np.concatenate(pieces)
    maps["ref_contig_length"] = len(result)
    return true, result, np.asarray(mapped, np.int32), maps, (np.asarray([0, len(dust)], np.int64), np.asarray(dust, np.int32))


def timed(name, call, reps, extra):
    wall = []
    for k in range(1 + reps):
        t0 = time.perf_counter()
        call()
        if k >= 1:
            wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    row = dict(variant=name, wall_ms_median=wall[len(wall) // 2], wall_ms_min=wall[0], wall_ms_max=wall[-1], reps=reps, **extra)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gaps", type=int, default=1000)
    ap.add_argument("--div", type=float, default=0.02)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--traced", action="store_true")
    a = ap.parse_args()
    if a.traced:
        os.environ["DH_TRACE"] = "1"
    crop = 20
    true, result, mapped, maps, dust = workload(a.gaps, a.div, crop)
    ctx = dentist_amd.Context(0)
    db = lambda s: dentist_amd.Db(ctx, types.SimpleNamespace(bases=s, off=np.asarray([0, len(s)], np.int64)))
    T, R = db(true), db(result)
    call = lambda: ctx.check_gaps(T, R, mapped, maps, [0], dust=dust, crop=crop, count=a.gaps)
    rep = call()
    g = rep.summaries
    assert (g["align_status"] == 1).all() and (g["state"] == 4).all(), "the workload is all closed, aligned gaps"
    roff = np.concatenate([[0], np.cumsum(g["true_end"] - g["true_begin"])]).astype(np.int64)
    qoff = np.concatenate([[0], np.cumsum(g["result_end"] - g["result_begin"])]).astype(np.int64)
    refs = np.concatenate([true[b:e] for b, e in zip(g["true_begin"], g["true_end"])])
    qrys = np.concatenate([result[b:e] for b, e in zip(g["result_begin"], g["result_end"])])
    alone = lambda: ctx.nw_affine_batch_raw(refs, roff, qrys, qoff)
    paths, status = alone()
    assert not status.any() and paths.ops.tobytes() == rep.ops.tobytes(), "both routes give the same ops"
    extra = dict(gaps=a.gaps, ref_bases=int(roff[-1]), qry_bases=int(qoff[-1]), ops=int(len(rep.ops)), groups=rep.groups,
                 mean_identity=float(np.mean(rep.identity)))
    x = timed("check_gaps", call, a.reps, extra)
    y = timed("nw_affine", alone, a.reps, extra)
    print(json.dumps(dict(variant="bind+gather+stats", wall_ms_median_difference=x["wall_ms_median"] - y["wall_ms_median"])), flush=True)


if __name__ == "__main__":
    main()
