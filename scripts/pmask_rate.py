"""Timed calls of the mask propagation on a read mapping (not a test): Context.propagate_mask with the trace values in host
arrays and with the trace values left on the device by map_reads, and the host function dh_propagate_mask as the baseline.

  --scale 1   the mapping of tests/test_maskcov.py::test_propagate_mask_matches_the_oracle_on_a_mapping (400 kbp, 3 000 reads)
  --scale 10  ten times the assembly, the gaps and the reads

Per variant: two warm-up calls, --reps calls without DH_TRACE (wall time: median, min, max), then --traced calls with
DH_TRACE=1, whose stage lines the library prints to stderr.  One JSON line per variant on stdout.  The three results are
compared before anything is timed."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dentist_amd  # noqa: E402
from dentist_amd import sim  # noqa: E402


def mask_of(w, seed=9):
    rng = np.random.default_rng(seed)
    ptr, iv = [0], []
    for c in range(w.contigs.n):
        n = int(w.contigs.off[c + 1] - w.contigs.off[c])
        cuts = np.sort(rng.choice(np.arange(1, n), size=24, replace=False))
        for b, e in cuts.reshape(-1, 2):
            iv.append((int(b), int(min(e, b + 900))))
        ptr.append(len(iv))
    return np.array(ptr, dtype=np.int64), np.array(iv, dtype=np.int32)


def timed(name, call, reps, traced, extra):
    os.environ.pop("DH_TRACE", None)
    for _ in range(2):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    os.environ["DH_TRACE"] = "1"
    for _ in range(traced):
        print(f"[pmask_rate] traced call of {name}", file=sys.stderr, flush=True)
        call()
    os.environ.pop("DH_TRACE", None)
    wall.sort()
    print(json.dumps(dict(variant=name, wall_ms_median=wall[len(wall) // 2], wall_ms_min=wall[0], wall_ms_max=wall[-1], reps=reps, **extra)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--traced", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    s = args.scale
    w = sim.Workload(400_000 * s, 4 * s, 3000 * s, 6000, seed=5)
    ctx = dentist_amd.Context(0)
    A, B = ctx.db(w.contigs), ctx.db(w.reads)
    mo = dentist_amd.default_align_opts(kmer_mod=4, k=20)
    las, trace = ctx.align_db(A, B, mo, select_best=True)
    mask = mask_of(w)
    nc, ro = w.contigs.n, w.reads.off
    host = dentist_amd.propagate_mask(las, trace, mo.tspace, mask, nc, ro)
    dev = ctx.propagate_mask(las, trace, mo.tspace, mask, nc, ro)
    assert np.array_equal(dev.ptr, host[0]) and np.array_equal(dev.iv, host[1]), "device and host results differ"
    extra = dict(scale=s, records=int(len(las)), trace_values=int(len(trace)), mask_intervals=int(len(mask[1])), hit=dev.hit, raw=dev.raw,
                 intervals=int(len(dev)))
    timed("device, trace in host arrays", lambda: ctx.propagate_mask(las, trace, mo.tspace, mask, nc, ro), args.reps, args.traced, extra)
    timed("host dh_propagate_mask", lambda: dentist_amd.propagate_mask(las, trace, mo.tspace, mask, nc, ro), args.reps, 0, extra)
    # the same reads mapped with the trace values left on the device: map_reads keeps them there for the tiled extension
    # (algo 1) only, and its collect filters apply, so the records are not the ones above
    mo = dentist_amd.default_align_opts(kmer_mod=4, k=20, width=64, xdrop=60, algo=1)
    mlas, dtrace, _ = ctx.map_reads(A, B, mo, dentist_amd.default_process_opts(algo=1), trace_on_device=True)[:3]
    assert dtrace.on_device()
    on_dev = ctx.propagate_mask(mlas, dtrace, mo.tspace, mask, nc, ro)
    extra2 = dict(scale=s, records=int(len(mlas)), trace_values=int(len(dtrace)), mask_intervals=int(len(mask[1])), hit=on_dev.hit, raw=on_dev.raw,
                  intervals=int(len(on_dev)))
    timed("device, trace on the device", lambda: ctx.propagate_mask(mlas, dtrace, mo.tspace, mask, nc, ro), args.reps, args.traced, extra2)
    assert dtrace.on_device()
    mtrace = dtrace.numpy()
    mhost = dentist_amd.propagate_mask(mlas, mtrace, mo.tspace, mask, nc, ro)
    assert np.array_equal(on_dev.ptr, mhost[0]) and np.array_equal(on_dev.iv, mhost[1]), "set path and host results differ"
    timed("host dh_propagate_mask, records of map_reads", lambda: dentist_amd.propagate_mask(mlas, mtrace, mo.tspace, mask, nc, ro), args.reps, 0,
          extra2)


if __name__ == "__main__":
    main()
