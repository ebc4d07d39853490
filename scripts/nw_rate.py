"""Warm-call time of dh_nw_batch (k_nw / k_edit_compact) next to oracle/nw.c on the same pairs.

Workload: --pairs (1 000) seeded pairs, the reference 2-6 kb of random bases, the query the reference with 2 % divergence
(substitutions, insertions and deletions in equal parts) -- the shape of closed gaps with their flanks.  Two warm-up calls,
then --reps timed calls (wall clock around the call, which ends in a stream synchronise): host validation, uploads, the
band attempts with their kernels, the download of the ops.  Then oz.nw on the first --oracle-pairs pairs (all by default)
on one CPU thread, and every op and score of those compared.  Prints one JSON line.  --free-shift times that mode."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dentist_amd  # noqa: E402
import nw_ref as nr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--oracle-pairs", type=int, default=-1)
    ap.add_argument("--free-shift", action="store_true")
    ap.add_argument("--seed", type=int, default=20261018)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a rate is only measured on the device")
    rng = np.random.default_rng(args.seed)
    refs, qrys = [], []
    for _ in range(args.pairs):
        r = rng.integers(0, 4, int(rng.integers(2000, 6001))).astype(np.uint8)
        refs.append(r)
        qrys.append(nr.mutate(rng, r, 0.02))
    ctx = dentist_amd.Context(0)
    times = []
    for it in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        ep, status = ctx.nw_batch(refs, qrys, free_shift=args.free_shift)
        dt = (time.perf_counter() - t0) * 1e3
        if it >= args.warmup:
            times.append(dt)
    n_or = args.pairs if args.oracle_pairs < 0 else min(args.oracle_pairs, args.pairs)
    t0 = time.perf_counter()
    exp = [nr.oz.nw(refs[i], qrys[i], 1, args.free_shift) for i in range(n_or)]
    oracle_ms = (time.perf_counter() - t0) * 1e3
    equal = True
    for i in range(n_or):
        score, ops = nr.oracle(refs[i], qrys[i], args.free_shift) if i < 20 else (exp[i][0], None)
        equal &= int(ep.score[i]) == score and status[i] == 0
        if ops is not None:
            equal &= np.array_equal(ep.ops[ep.op_off[i]:ep.op_off[i + 1]], ops)
    cells = int(sum(len(r) * len(q) for r, q in zip(refs, qrys)))
    print(json.dumps({"pairs": args.pairs, "free_shift": bool(args.free_shift), "bases": int(sum(len(r) + len(q) for r, q in zip(refs, qrys))),
                      "matrix_cells": cells, "ops": int(ep.op_off[-1]), "band_exceeded": int(np.count_nonzero(status)),
                      "ms_median": float(np.median(times)), "ms_min": float(min(times)), "ms_max": float(max(times)),
                      "reps": len(times), "oracle_pairs": n_or, "oracle_ms": oracle_ms, "equal_to_oracle": bool(equal)}))


if __name__ == "__main__":
    main()
