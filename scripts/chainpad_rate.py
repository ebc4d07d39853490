"""Rate of dh_la_chain_paths (k_cp_plan, the edit-path and global-alignment kernels, k_cp_stitch) on the chains of a mapping.

Workload: sim.Workload(1_000_000, 8, 3000, 10_000, seed=23) mapped once with bench.py's mapping options and select_best,
chained (dh_la_chain) and gathered (dh_la_chains_to_set).  Timed between HIP events on the context's stream, warm: the chain
call on those records and, as the baseline of the same run, dh_la_edit_paths on the same records (the same tile work without
plan, fillers or stitch) -- --reps repetitions, the two calls alternating.  Prints one JSON line: chains/s and ops/s of the
chain call (median and spread), the baseline's median, and their ratio.  The time is that of the whole call."""
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a rate is only measured on the device")
    w = sim.Workload(1_000_000, 8, 3000, 10_000, seed=23)
    stream = torch.cuda.Stream()
    ctx = dentist_amd.Context(0, stream=stream.cuda_stream)
    A, B = ctx.db(w.contigs), ctx.db(w.reads)
    g = dentist_amd.default_align_opts(k=20, kmer_mod=8, xdrop=60, algo=1, width=64)
    las, trace = ctx.align_db(A, B, g, select_best=True)
    ch = ctx.chain(las, g.tspace)
    rec, tr = ch.to_set(las, trace, g.tspace)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        out = fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), out

    chain_call = lambda: ctx.chain_paths(A, B, rec, tr, g.tspace, chain_off=ch.off)
    record_call = lambda: ctx.edit_paths(A, B, rec, tr, g.tspace)
    tc, tr_ = [], []
    for it in range(args.warmup + args.reps):  # alternating
        t0, cp = timed(chain_call)
        t1, ep = timed(record_call)
        if it >= args.warmup:
            tc.append(t0)
            tr_.append(t1)
    op_off, ops, score, status, fillers = cp
    med, base = float(np.median(tc)), float(np.median(tr_))
    print(json.dumps({"records": len(rec), "chains": len(ch), "multi_record_chains": int(np.count_nonzero(np.diff(ch.off) > 1)),
                      "ops": int(op_off[-1]), "fillers": fillers, "faked": int(np.count_nonzero(status == dentist_amd.CP_FAKED)),
                      "nested": int(np.count_nonzero(status == dentist_amd.CP_NESTED)), "ms_median": med, "ms_min": float(min(tc)),
                      "ms_max": float(max(tc)), "reps": len(tc), "chains_per_s": len(ch) / med * 1e3, "ops_per_s": int(op_off[-1]) / med * 1e3,
                      "edit_paths_ms_median": base, "edit_paths_ms_min": float(min(tr_)), "edit_paths_ms_max": float(max(tr_)),
                      "edit_paths_ops": int(ep.op_off[-1]), "ratio": med / base}))


if __name__ == "__main__":
    main()
