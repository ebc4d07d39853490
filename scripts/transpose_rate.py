"""Warm-call time of dh_la_transpose (the edit-path kernels + k_trace_transpose / k_trace_pairs) next to dh_la_edit_paths on
the same records.

Workload: that of scripts/editpath_rate.py -- sim.Workload(1_000_000, 8, 3000, 10_000, seed=23) mapped once with bench.py's
mapping options.  Two warm-up calls each, then --reps timed calls between HIP events on the context's stream (both calls end
in a stream synchronise).  Prints one JSON line.  The times are those of the whole calls: host validation and tiling,
uploads, kernels and downloads -- of the ops for edit_paths, of the trace pairs for transpose, which also sorts the records.
With --once the script runs one warm-up and one call of transpose and prints nothing but the record count: the run to put
under `rocprofv3 --kernel-trace --stats` for the time of k_trace_transpose itself."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dentist_amd  # noqa: E402
from dentist_amd import sim  # noqa: E402


def timed(stream, fn, warmup, reps):
    times, out = [], None
    for it in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        if it >= warmup:
            times.append(e0.elapsed_time(e1))
    return out, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    w = sim.Workload(1_000_000, 8, 3000, 10_000, seed=23)
    stream = torch.cuda.Stream()
    ctx = dentist_amd.Context(0, stream=stream.cuda_stream)
    A, B = ctx.db(w.contigs), ctx.db(w.reads)
    g = dentist_amd.default_align_opts(k=20, kmer_mod=8, xdrop=60, algo=1, width=64)
    las, trace = ctx.align_db(A, B, g)
    if args.once:
        (tl, _, _), _ = timed(stream, lambda: ctx.transpose(A, B, las, trace, g.tspace), 1, 1)
        print(json.dumps({"records": len(tl)}))
        return
    ep, t_ep = timed(stream, lambda: ctx.edit_paths(A, B, las, trace, g.tspace), args.warmup, args.reps)
    (tl, tt, _), t_tr = timed(stream, lambda: ctx.transpose(A, B, las, trace, g.tspace), args.warmup, args.reps)
    assert np.array_equal(np.sort(tl["diffs"]), np.sort(ep.score))
    print(json.dumps({"records": len(las), "tiles": int(ep.tile_off[-1]), "ops": int(ep.op_off[-1]), "transposed_tiles": len(tt) // 2,
                      "reps": args.reps, "edit_paths_ms_median": float(np.median(t_ep)), "edit_paths_ms_min": float(min(t_ep)),
                      "edit_paths_ms_max": float(max(t_ep)), "transpose_ms_median": float(np.median(t_tr)),
                      "transpose_ms_min": float(min(t_tr)), "transpose_ms_max": float(max(t_tr))}))


if __name__ == "__main__":
    main()
