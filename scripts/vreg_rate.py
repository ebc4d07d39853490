"""Timed calls of the region validation on the shape of a gap-closed scaffold (not a test): one contig of 100 Mb, 10^6 random
records of 15 kb sorted by aread, 1 000 regions of 50-5 000 bases.  Context.validate_regions (upload included) after one
warm-up call, and the host function dh_validate_regions on the host threads of the machine as the baseline.

Per variant: --reps calls (wall time: median, min, max); one JSON line per variant on stdout.  The two results are compared
before anything is timed.  --traced calls with DH_TRACE=1 print the library's line to stderr."""
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


def workload(contig_len, nrec, nreg, seed=11):
    rng = np.random.default_rng(seed)
    las = np.zeros(nrec, dtype=dentist_amd.LA_DTYPE)
    b = rng.integers(0, contig_len - 15_000, nrec)
    las["abpos"], las["aepos"], las["bread"] = b, b + 15_000, np.arange(nrec)
    rb = np.sort(rng.integers(1000, contig_len - 7000, nreg))
    regions = np.stack([np.zeros(nreg, np.int64), rb, rb + rng.integers(50, 5001, nreg)], axis=1).astype(np.int32)
    return las, np.array([0, contig_len], dtype=np.int64), regions


def timed(name, call, warmup, reps, extra):
    for _ in range(warmup):
        call()
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    print(json.dumps(dict(variant=name, wall_ms_median=wall[len(wall) // 2], wall_ms_min=wall[0], wall_ms_max=wall[-1], reps=reps, **extra)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig-mb", type=int, default=100)
    ap.add_argument("--records", type=int, default=1_000_000)
    ap.add_argument("--regions", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=1)
    ap.add_argument("--traced", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    las, co, regions = workload(args.contig_mb * 1_000_000, args.records, args.regions)
    ctx = dentist_amd.Context(0)
    # coverage is records * 15 kb / contig: half of it as the bound, as the command derives it for ploidy 1
    min_cov = max(1, int(0.5 * args.records * 15_000 / (args.contig_mb * 1_000_000)))
    t0 = time.perf_counter()
    rep, weak = dentist_amd.validate_regions(las, co, regions, min_cov)
    first_host_ms = (time.perf_counter() - t0) * 1e3
    dev = ctx.validate_regions(las, co, regions, min_cov)
    assert np.array_equal(dev.reports, rep) and np.array_equal(dev.weak, weak), "device and host results differ"
    extra = dict(records=int(len(las)), regions=int(len(regions)), min_coverage_reads=min_cov, pairs=dev.pairs, big_regions=dev.big_regions,
                 groups=dev.groups, weak_intervals=int(len(dev.weak)), spanning_ids=int(len(dev.span_ids)),
                 host_threads=os.environ.get("DH_HOST_THREADS", "default"))
    timed("device dh_la_validate_regions, upload included", lambda: ctx.validate_regions(las, co, regions, min_cov), 1, args.reps, extra)
    os.environ["DH_TRACE"] = "1"
    for _ in range(args.traced):
        ctx.validate_regions(las, co, regions, min_cov)
    os.environ.pop("DH_TRACE", None)
    extra["first_host_call_ms"] = first_host_ms
    timed("host dh_validate_regions", lambda: dentist_amd.validate_regions(las, co, regions, min_cov), 0, args.host_reps, extra)


if __name__ == "__main__":
    main()
