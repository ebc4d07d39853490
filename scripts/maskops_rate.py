"""Timed calls of the mask union on the shapes of an assembly's masks (not a test): 4 masks of 10^6 intervals each, once spread
over 1 001 contigs of 250 kb and once all on one contig of 250 Mb.

  new   Context.combine_masks (dh_mask_combine, min_count 1): host checks, upload, sort, sweep and download included.
  host  the route this replaces: the sort and merge per contig of read_united_masks (tools/dazz_main.cpp), one core, through
        tests/native/libmaskops_host.so -- built for this comparison only.

Per shape and variant: --reps calls after one warm-up call (wall time: median, min, max); one JSON line each on stdout.  The two
results are compared before anything is timed.  Device memory: the growth of the context's scratch arena over the first call
(free memory before and after, nothing is freed in between; the arena is released between the shapes).  --traced calls with
DH_TRACE=1 print the library's stage times to stderr.  --min-count 2 times the two-sweep route instead (no host counterpart)."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dentist_amd  # noqa: E402


def workload(nmasks, n, ncontigs, clen, seed=13):
    rng = np.random.default_rng(seed)
    masks = []
    for _ in range(nmasks):
        c = np.sort(rng.integers(0, ncontigs, n))
        b = rng.integers(0, clen - 400, n)
        iv = np.stack([b, b + rng.integers(0, 400, n)], axis=1).astype(np.int32)     # unsorted within a contig, some empty
        ptr = np.searchsorted(c, np.arange(ncontigs + 1)).astype(np.int64)
        masks.append((ptr, iv))
    return masks, np.arange(ncontigs + 1, dtype=np.int64) * clen


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
    ap.add_argument("--masks", type=int, default=4)
    ap.add_argument("--intervals", type=int, default=1_000_000, help="per mask")
    ap.add_argument("--min-count", type=int, default=1)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--traced", type=int, default=1)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libmaskops_host.so"], check=True)
    H = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libmaskops_host.so"))
    vp = ctypes.c_void_p
    H.maskops_host_route.argtypes = [vp, vp, ctypes.c_int32, ctypes.c_int32, vp, vp]
    H.maskops_host_route.restype = ctypes.c_int64
    torch.zeros(1, device="cuda")   # (the runtime's own allocations are not the call's)
    ctx = dentist_amd.Context(0)
    for shape, ncontigs, clen in (("spread over 1 001 contigs of 250 kb", 1001, 250_000), ("all on one contig of 250 Mb", 1, 250_000_000)):
        masks, coff = workload(args.masks, args.intervals, ncontigs, clen)
        ptrs = (vp * args.masks)(*[m[0].ctypes.data for m in masks])
        ivs = (vp * args.masks)(*[m[1].ctypes.data for m in masks])
        out_ptr, out_iv = np.zeros(ncontigs + 1, np.int64), np.zeros((args.masks * args.intervals + 1, 2), np.int32)

        def new_route():
            return ctx.combine_masks(masks, coff, min_count=args.min_count)

        def host_route():
            return H.maskops_host_route(ptrs, ivs, args.masks, ncontigs, out_ptr.ctypes.data, out_iv.ctypes.data)

        ctx.release_scratch()
        f0 = free_bytes()
        new = new_route()
        new_bytes = f0 - free_bytes()
        extra = dict(shape=shape, masks=args.masks, intervals=args.masks * args.intervals, contigs=ncontigs, min_count=args.min_count,
                     events=new.events, sort_passes=new.sort_passes, groups=new.groups, runs=int(len(new.iv)))
        if args.min_count == 1:
            m = host_route()
            assert m == len(new.iv) and np.array_equal(out_ptr, new.ptr) and np.array_equal(out_iv[:m], new.iv), "the two routes differ"
        timed("new: dh_mask_combine, checks, upload and download included", new_route, 1, args.reps, dict(extra, device_bytes_measured=int(new_bytes)))
        os.environ["DH_TRACE"] = "1"
        for _ in range(args.traced):
            new_route()
        os.environ.pop("DH_TRACE", None)
        if args.min_count == 1:
            timed("host: sort and merge per contig (read_united_masks), one core", host_route, 1, args.reps, extra)


if __name__ == "__main__":
    main()
