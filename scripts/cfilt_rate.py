"""Timed calls of the collect filters on the shape of a read mapping (not a test): 1 001 contigs of 100 kb, 10^6 reads of 10 kb
with one record each, a tenth of them with a second one (a contained copy, or the read's other half on the next contig), a mask of
four intervals per contig.  Every chain is one record.  Context.collect_filter (upload and download included) after one warm-up
call, and the host function dh_collect_filter on the host threads (DH_HOST_THREADS) as the baseline -- once with the records
grouped by read, once in LAsort order by contig.

Per variant: --reps calls, each on a fresh copy of the records made outside the timed region (wall time: median, min, max); one
JSON line per variant on stdout.  The two results are compared before anything is timed.  --traced calls with DH_TRACE=1 print
the library's line to stderr."""
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


def workload(nreads, ncontigs, clen=100_000, rlen=10_000, seed=11):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, ncontigs - 1, nreads)
    ln = rng.integers(600, 9000, nreads)
    kind = rng.random(nreads)
    ab = np.where(kind < 0.45, 0, np.where(kind < 0.9, clen - ln, rng.integers(1000, clen - 20_000, nreads)))
    bb = np.where(kind < 0.45, rlen - ln, np.where(kind < 0.9, 0, np.where(kind < 0.95, 0, rng.integers(100, 900, nreads))))
    ln = np.where((kind >= 0.9) & (kind < 0.95), rlen, ln)   # the whole read inside a contig: redundant
    first = np.zeros(nreads, dtype=dentist_amd.LA_DTYPE)
    first["aread"], first["bread"], first["abpos"], first["aepos"], first["bbpos"], first["bepos"] = c, np.arange(nreads), ab, ab + ln, bb, bb + ln
    first["diffs"] = (ln * rng.choice([0.05, 0.13, 0.2, 0.35], nreads, p=[0.4, 0.3, 0.2, 0.1])).astype(np.int32)
    first["flags"] = rng.integers(0, 2, nreads)
    pick = rng.random(nreads)
    inner = first[(pick < 0.05) & (ln > 2000)].copy()         # a contained copy
    for f, d in (("abpos", 50), ("aepos", -50), ("bbpos", 50), ("bepos", -50)):
        inner[f] += d
    other = first[(pick >= 0.05) & (pick < 0.1) & (kind >= 0.45) & (kind < 0.9)].copy()   # the rest of a read that hangs over a contig's end
    rest = rlen - (other["bepos"] - other["bbpos"]) + np.where(rng.random(len(other)) < 0.3, 400, 0)   # a third of them overlap on the read: ambiguous
    other["aread"] += 1
    other["abpos"], other["aepos"], other["bbpos"], other["bepos"] = 0, rest, rlen - rest, rlen
    other["flags"] = first["flags"][other["bread"]]
    las = np.concatenate([first, inner, other])
    coff, roff = np.arange(ncontigs + 1, dtype=np.int64) * clen, np.arange(nreads + 1, dtype=np.int64) * rlen
    mask = (np.arange(ncontigs + 1, dtype=np.int64) * 4, np.tile(np.asarray([0, 300, 20_000, 24_000, 60_000, 60_500, clen - 400, clen], np.int32), ncontigs))
    return las, coff, roff, mask


def timed(name, call, fresh, warmup, reps, extra):
    wall = []
    for k in range(warmup + reps):
        arr = fresh()
        t0 = time.perf_counter()
        call(arr)
        if k >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    print(json.dumps(dict(variant=name, wall_ms_median=wall[len(wall) // 2], wall_ms_min=wall[0], wall_ms_max=wall[-1], reps=reps, **extra)),
          flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--contigs", type=int, default=1001)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--host-reps", type=int, default=5)
    ap.add_argument("--traced", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    base, coff, roff, mask = workload(args.reads, args.contigs)
    ctx = dentist_amd.Context(0)
    po = dentist_amd.default_process_opts()
    orders = {"grouped by read": np.argsort(base["bread"], kind="stable"),
              "LAsort order": np.lexsort((base["abpos"], base["bread"], base["aread"]))}
    for order, perm in orders.items():
        las = base[perm]
        host = dentist_amd.collect_filter(las, coff, roff, po, repeat_mask=mask)
        dev = ctx.collect_filter(las, coff, roff, po, repeat_mask=mask)
        assert np.array_equal(dev[0]["flags"], host[0]["flags"]) and np.array_equal(dev[1], host[1]) and np.array_equal(dev[2], host[2]), \
            "device and host results differ"
        extra = dict(order=order, records=int(len(las)), reads=args.reads, contigs=args.contigs, mask_intervals=int(len(mask[1]) // 2),
                     dropped=host[1].tolist(), left=int((host[0]["flags"] & 0x20 == 0).sum()), reads_used=int(host[2].sum()),
                     host_threads=os.environ.get("DH_HOST_THREADS", "default"))
        timed("device dh_la_collect_filter, upload and download included",
              lambda arr: ctx.collect_filter(arr, coff, roff, po, repeat_mask=mask, inplace=True), las.copy, 1, args.reps, extra)
        os.environ["DH_TRACE"] = "1"
        for _ in range(args.traced):
            ctx.collect_filter(las.copy(), coff, roff, po, repeat_mask=mask, inplace=True)
        os.environ.pop("DH_TRACE", None)
        timed("host dh_collect_filter", lambda arr: dentist_amd.collect_filter(arr, coff, roff, po, repeat_mask=mask, inplace=True), las.copy, 1,
              args.host_reps, extra)


if __name__ == "__main__":
    main()
