"""Warm-call times of dh_nw_affine_batch (k_nwa / k_edit_compact) and dh_nw_batch (k_nw) on the same pairs.

Workload: --pairs (1 000) seeded pairs, the reference 2-6 kb of random bases, the query the reference with 2 % divergence
(substitutions, insertions and deletions in equal parts) -- the shape of closed gaps with their flanks.  Per entry point two
warm-up calls, then --reps timed calls (wall clock around the call, which ends in a stream synchronise): host validation,
uploads, the band attempts with their kernels, the download of the ops.  The attempts per pair follow from the restated
policy (tests/nwa_ref.py, tests/nw_ref.py) and the costs the calls return.  Prints one JSON line."""
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
import nwa_ref as ar  # noqa: E402


def timed(fn, warmup, reps):
    times, out = [], None
    for it in range(warmup + reps):
        t0 = time.perf_counter()
        out = fn()
        dt = (time.perf_counter() - t0) * 1e3
        if it >= warmup:
            times.append(dt)
    return out, {"ms_median": float(np.median(times)), "ms_min": float(min(times)), "ms_max": float(max(times)), "reps": len(times)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
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
    (ep, st), t_aff = timed(lambda: ctx.nw_affine_batch(refs, qrys), args.warmup, args.reps)
    (ep0, st0), t_unit = timed(lambda: ctx.nw_batch(refs, qrys), args.warmup, args.reps)
    cm, ce, co = ar.costs(ar.DEFAULT)
    att_aff, att_unit = [], []
    for i, (r, q) in enumerate(zip(refs, qrys)):
        if not st[i]:
            cost = ar.DEFAULT[0] * (len(r) + len(q)) - 2 * int(ep.score[i])
            att_aff.append(ar.expected_attempts(len(r), len(q), cost, ce, dentist_amd.NWA_MAX_BAND)[1])
        if not st0[i]:
            att_unit.append(nr.expected_attempts(len(r), len(q), 0, int(ep0.score[i]))[1])
    print(json.dumps({"pairs": args.pairs, "bases": int(sum(len(r) + len(q) for r, q in zip(refs, qrys))),
                      "affine": dict(t_aff, band_exceeded=int(np.count_nonzero(st)), attempts_per_pair=float(np.mean(att_aff))),
                      "unit": dict(t_unit, band_exceeded=int(np.count_nonzero(st0)), attempts_per_pair=float(np.mean(att_unit)))}))


if __name__ == "__main__":
    main()
