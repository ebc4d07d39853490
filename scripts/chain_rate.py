"""Timed calls of dh_la_chain under DH_TRACE=1 on the two shapes its callers give it (not a test).

  mapping   2 M pairs of 1-5 collinear records (a read mapping: the flat kernel and the register tier)
  assembly  200 pairs of 4 000 records (an assembly against an assembly: the global-memory tier; --lds-nodes N lowers the
            LDS tier's limit, --records N sizes the pairs, so that the same pairs can be sent through the LDS tier)

The library's own trace line (tier counts; plan = the host-side grouping, upload, kernel ms per tier, scan + emission +
download, total) goes to stderr; this script prints one JSON line per set with the wall time of the last call and the
records per second it amounts to.  The first call pays the allocations."""
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


def collinear(rng, npairs, counts, step, length):
    """pairs of counts[p] records that follow each other on both sequences, every fourth pair on the complement strand"""
    n = int(counts.sum())
    las = np.zeros(n, dtype=dentist_amd.LA_DTYPE)
    pair = np.repeat(np.arange(npairs), counts)
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    j = np.arange(n) - np.repeat(first, counts)
    las["abpos"] = j * step + rng.integers(0, step - length, n)
    las["aepos"] = las["abpos"] + length + rng.integers(-20, 21, n)
    las["bbpos"] = las["abpos"] + 5000 + rng.integers(-40, 41, n)
    las["bepos"] = las["bbpos"] + length + rng.integers(-20, 21, n)
    las["flags"] = (pair % 4 == 3).astype(np.uint32)
    las["aread"], las["bread"] = pair // 1000, pair % 1000
    return las


def timed(ctx, las, calls, name):
    for _ in range(calls):
        t0 = time.perf_counter()
        ch = ctx.chain(las, 100)
        wall = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"set": name, "records": int(len(las)), "chains": int(len(ch)), "output_records": int(len(ch.src_index)),
                      "big_pairs": ch.big_pairs, "wall_ms_last_call": wall, "records_per_s": len(las) / wall * 1e3}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=2_000_000)
    ap.add_argument("--big-pairs", type=int, default=200)
    ap.add_argument("--records", type=int, default=4000)
    ap.add_argument("--lds-nodes", type=int, default=None)
    ap.add_argument("--calls", type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    if args.lds_nodes is not None:
        os.environ["DH_CHAIN_LDS_NODES"] = str(args.lds_nodes)
    os.environ["DH_TRACE"] = "1"
    rng = np.random.default_rng(1)
    ctx = dentist_amd.Context(0)
    if args.pairs:
        timed(ctx, collinear(rng, args.pairs, rng.integers(1, 6, args.pairs), 2000, 1500), args.calls, "mapping")
    if args.big_pairs:
        timed(ctx, collinear(rng, args.big_pairs, np.full(args.big_pairs, args.records), 1300, 1000), args.calls, "assembly")


if __name__ == "__main__":
    main()
