"""Timed loads of reads from a DAZZ_DB on disk to the device (not a test): dh_dazz_load_reads against today's route.

One simulated reads DB (--reads x --length bases, written with dazz_create_db into --dir) is loaded three ways, each warmed
up once and then repeated --reps times; the median is reported:

  sparse   every hundredth read through dh_dazz_load_reads (what a batch of `process` touches)
  all      every read through dh_dazz_load_reads
  open     dh_dazz_open + dh_db_create of the whole DB: the only way to those reads before the loader

For the loader the library's own split of the call is printed -- file reads (host clock around the preads), uploads and
kernels (device events on the context's stream) -- and the kernel's traffic, packed bytes in plus unpacked bytes out, over
the kernel time, next to the 6.29 TB/s a float4 copy reaches on this chip.  The files are in the page cache after the warm-up:
the file time is a memory copy, not a disk.  One JSON line per set."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dentist_amd  # noqa: E402

HBM_COPY_TBS = 6.29


def write_db(path, nreads, length, seed):
    """reads of about `length` bases (uniform in [length / 2, 3 length / 2)) as a .db; returns the number of bases"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(length // 2, length + length // 2, nreads)
    letters = np.frombuffer(b"acgt", dtype=np.uint8)
    parts = []
    for i, l in enumerate(lens):
        parts.append((">sim/%d/0_%d RQ=0.850\n" % (i + 1, l)).encode())
        parts.append(letters[rng.integers(0, 4, l)].tobytes())
        parts.append(b"\n")
    dentist_amd.dazz_create_db(path, b"".join(parts))
    return int(lens.sum())


def load(ctx, path, ids, reps):
    rows = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        db = dentist_amd.load_reads(ctx, path, ids)
        wall = (time.perf_counter() - t0) * 1e3
        st = dentist_amd.load_stats(ctx)
        db.close()
        if rep:   # (the first call is the warm-up: allocations, code objects, the page cache)
            rows.append(dict(st, wall_ms=wall))
    med = {k: statistics.median(r[k] for r in rows) for k in ("ms_file", "ms_copy", "ms_kernel", "ms_total", "wall_ms")}
    med.update({k: rows[0][k] for k in ("packed_bytes", "bases", "runs", "chunks")})
    traffic = med["packed_bytes"] + med["bases"]
    med["kernel_GBs"] = traffic / med["ms_kernel"] / 1e6 if med["ms_kernel"] > 0 else None
    med["kernel_share_of_copy_rate"] = med["kernel_GBs"] / (HBM_COPY_TBS * 1e3) if med["kernel_GBs"] else None
    med["upload_GBs"] = med["packed_bytes"] / med["ms_copy"] / 1e6 if med["ms_copy"] > 0 else None
    return med


def open_and_create(ctx, path, reps):
    t_open, t_create = [], []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        dz = dentist_amd.DazzDb(path)     # (the binding also copies the arrays once: counted, it is part of what a caller pays)
        t1 = time.perf_counter()
        db = ctx.db(dz)
        ctx.sync()
        t2 = time.perf_counter()
        db.close()
        dz.close()
        if rep:
            t_open.append((t1 - t0) * 1e3)
            t_create.append((t2 - t1) * 1e3)
    return {"ms_open": statistics.median(t_open), "ms_create": statistics.median(t_create),
            "ms_total": statistics.median(a + b for a, b in zip(t_open, t_create))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000)
    ap.add_argument("--length", type=int, default=15_000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dir", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    d = args.dir or tempfile.mkdtemp(prefix="load_rate")
    path = os.path.join(d, "reads.db")
    bases = write_db(path, args.reads, args.length, 20261020)
    print(json.dumps({"set": "db", "reads": args.reads, "bases": bases, "bps_bytes": os.path.getsize(os.path.join(d, ".reads.bps")),
                      "chunk_mb": os.environ.get("DH_LOAD_CHUNK_MB", "64 (default)")}), flush=True)
    ctx = dentist_amd.Context(0)
    print(json.dumps(dict(load(ctx, path, np.arange(0, args.reads, 100, dtype=np.int32), args.reps), set="sparse")), flush=True)
    print(json.dumps(dict(load(ctx, path, np.arange(args.reads, dtype=np.int32), args.reps), set="all")), flush=True)
    print(json.dumps(dict(open_and_create(ctx, path, args.reps), set="open")), flush=True)


if __name__ == "__main__":
    main()
