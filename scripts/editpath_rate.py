"""Rate of dh_la_edit_paths (k_edit_fast / k_edit_general / k_edit_compact) on a mapping result.

Workload: sim.Workload(1_000_000, 8, 3000, 10_000, seed=23) mapped once with bench.py's mapping options, then the edit paths
of all records: two warm-up calls, then --reps timed calls between HIP events on the context's stream (the call ends in a
stream synchronise).  Prints one JSON line: warm tiles/s and ops/s (median and spread over the repeats) and general_tiles.
The time is that of the whole call -- host validation and tiling, uploads, the kernels, the download of the ops."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dentist_amd  # noqa: E402
from dentist_amd import sim  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--copies", type=int, default=1, help="the records repeated this many times in one call")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a rate is only measured on the device")
    w = sim.Workload(1_000_000, 8, 3000, 10_000, seed=23)
    stream = torch.cuda.Stream()
    ctx = dentist_amd.Context(0, stream=stream.cuda_stream)
    A, B = ctx.db(w.contigs), ctx.db(w.reads)
    g = dentist_amd.default_align_opts(k=20, kmer_mod=8, xdrop=60, algo=1, width=64)
    las, trace = ctx.align_db(A, B, g)
    las = np.concatenate([las] * args.copies)
    times = []
    for it in range(args.warmup + args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        ep = ctx.edit_paths(A, B, las, trace, g.tspace)
        e1.record(stream)
        e1.synchronize()
        if it >= args.warmup:
            times.append(e0.elapsed_time(e1))
    ntiles, nops = int(ep.tile_off[-1]), int(ep.op_off[-1])
    med = float(np.median(times))
    print(json.dumps({"records": len(las), "tiles": ntiles, "ops": nops, "general_tiles": ep.general_tiles,
                      "ms_median": med, "ms_min": float(min(times)), "ms_max": float(max(times)), "reps": len(times),
                      "tiles_per_s": ntiles / med * 1e3, "ops_per_s": nops / med * 1e3,
                      "two_word_tiles": int(np.count_nonzero(trace[0::2] >= 31))}))


if __name__ == "__main__":
    main()
