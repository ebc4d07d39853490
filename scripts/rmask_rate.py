"""Timed calls of the repeat mask on the shape of a read mapping (not a test): 1 001 contigs of 100 kb (100 Mb), 10^6 reads of
10 kb with one record each in LAsort order, so that every chain is one record and both routes answer the same question.

  new     Context.repeat_mask (dh_la_repeat_mask): both assessors and the union in one call, host checks, upload and download
          included.
  parent  the route to the same intervals before that call existed: two dh_db_mask_coverage calls on a fresh DB (all records, then
          the improper ones) and dh_db_get_mask.  The upload of the DB's bases, which the command never reads, is timed on its own.

Per variant: --reps calls after one warm-up call (wall time: median, min, max); one JSON line per variant on stdout.  The two
results are compared before anything is timed.  Device memory: for the new call the growth of the context's scratch arena over
the first call (free memory before and after, nothing is freed in between); for the parent the DB as uploaded (measured the same
way) and the buffers every dh_db_mask_coverage call allocates and frees again, computed from their sizes in dh_db.cpp.
--traced calls with DH_TRACE=1 print the library's line to stderr."""
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


def workload(nreads, ncontigs, clen=100_000, rlen=10_000, seed=11):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, ncontigs, nreads)
    ln = rng.integers(600, 9000, nreads)
    kind = rng.random(nreads)
    # reads that hang over a contig's begin (abpos 0) or end, reads inside a contig (a fifth of those improper), a repeat per contig
    ab = np.where(kind < 0.1, 0, np.where(kind < 0.2, clen - ln, rng.integers(0, clen - 9000, nreads)))
    ab = np.where(kind > 0.97, 40_000 + rng.integers(0, 50, nreads), ab)
    bb = np.where(kind < 0.1, rlen - ln, np.where((kind < 0.2) | (rng.random(nreads) < 0.8), 0, rng.integers(200, 900, nreads)))
    ln = np.where(kind >= 0.2, np.minimum(ln, rlen - bb), ln)
    full = (kind >= 0.2) & (rng.random(nreads) < 0.8)
    be = np.where(full, rlen, bb + ln)
    las = np.zeros(nreads, dtype=dentist_amd.LA_DTYPE)
    las["aread"], las["bread"], las["abpos"], las["aepos"], las["bbpos"], las["bepos"] = c, np.arange(nreads), ab, ab + ln, bb, be
    las["flags"] = rng.integers(0, 2, nreads)
    las = las[np.lexsort((las["abpos"], las["bread"], las["aread"]))]
    return las, np.arange(ncontigs + 1, dtype=np.int64) * clen, np.arange(nreads + 1, dtype=np.int64) * rlen


def timed(name, call, warmup, reps, extra):
    wall = []
    for k in range(warmup + reps):
        t0 = time.perf_counter()
        call()
        if k >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    wall.sort()
    print(json.dumps(dict(variant=name, wall_ms_median=wall[len(wall) // 2], wall_ms_min=wall[0], wall_ms_max=wall[-1], reps=reps, **extra)),
          flush=True)


def free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--contigs", type=int, default=1001)
    ap.add_argument("--contig-len", type=int, default=100_000)
    ap.add_argument("--upper", type=int, default=20, help="the upper bound of the assessor over all chains")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--traced", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    las, coff, roff = workload(args.reads, args.contigs, clen=args.contig_len)
    upper, iupper, allowance = args.upper, 4, 100
    torch.zeros(1, device="cuda")   # (the runtime's own allocations are not the routes')
    ctx = dentist_amd.Context(0)
    seqs = sim.SeqDb.from_list([np.zeros(int(n), dtype=np.uint8) for n in np.diff(coff)])

    def new_route():
        return ctx.repeat_mask(las, coff, roff, 0, upper, improper=(0, iupper), allowance=allowance)

    def parent_route(db):
        db.mask_coverage(las, 0, upper)
        db.mask_coverage(las, 0, iupper, read_off=roff, improper_only=True, allowance=allowance)
        return db.get_mask()

    f0 = free_bytes()
    new = new_route()
    new_bytes = f0 - free_bytes()
    f0 = free_bytes()
    db = ctx.db(seqs)
    db_bytes = f0 - free_bytes()
    ptr, iv = parent_route(db)
    assert np.array_equal(np.asarray(ptr), new.mask[0]) and np.array_equal(np.asarray(iv).reshape(-1, 2), new.mask[1]), "the two routes differ"
    bases = int(coff[-1])
    per_call = 4 * (bases + args.contigs + 2) + 4 * ((bases + args.contigs + 2) // 2048 + 4) + dentist_amd.LA_DTYPE.itemsize * len(las) \
        + 8 * (args.reads + 1)
    extra = dict(records=int(len(las)), units=new.units, improper_units=new.improper_units, contigs=args.contigs, bases=bases,
                 mask_intervals=int(len(new.mask[1])), tier_contigs=new.tier_contigs, groups=new.groups)
    timed("new: dh_la_repeat_mask, both assessors and the union, upload and download included", new_route, 1, args.reps,
          dict(extra, device_bytes_measured=int(new_bytes)))
    os.environ["DH_TRACE"] = "1"
    for _ in range(args.traced):
        new_route()
    os.environ.pop("DH_TRACE", None)
    fresh = []

    def upload():
        fresh.append(ctx.db(seqs))
    timed("parent: upload of the DB (dh_db_create)", upload, 1, args.reps, dict(extra, device_bytes_measured=int(db_bytes)))
    it = iter(fresh)
    timed("parent: 2 x dh_db_mask_coverage + dh_db_get_mask on a fresh DB, upload excluded", lambda: parent_route(next(it)), 1, args.reps,
          dict(extra, device_bytes_db_measured=int(db_bytes), device_bytes_per_call_computed=int(per_call)))


if __name__ == "__main__":
    main()
