"""One timed call of dh_exact_locate under DH_TRACE=1 on the shape `dentist check-results` gives it.

Workload: the 100 Mb assembly of bench.py (seed 20260929) split at its 1 000 gaps into 1 001 records; the queries are the
1 001 records cropped by 100 bases per side, both strands.  The library's own trace line (upload/pack, scan, verify, total,
in milliseconds) goes to stderr; this script checks the result (one forward hit per contig at [100, len - 100)), prices the
scan against the HBM peak of profiles/constants.json (bytes = the packed text once) and prints one JSON line.  --bitmap 0|1
sets DH_LOCATE_BITMAP (the pre-filter in LDS); --queries-64 N replaces the queries by N random 64-mers of the reference
(a table that outgrows the L2) for the same comparison."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--gaps", type=int, default=1000)
    ap.add_argument("--crop", type=int, default=100)
    ap.add_argument("--bitmap", type=int, default=None)
    ap.add_argument("--queries-64", type=int, default=0)
    ap.add_argument("--calls", type=int, default=2, help="the first call pays the allocations; the last is reported")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: a time is only measured on the device")
    seed = 20260929
    truth = sim.genome(seed, args.genome)
    gb, ge = sim.gaps(seed + 1, args.genome, args.gaps)
    contigs, _ = sim.contigs_from_gaps(truth, gb, ge)
    off = np.asarray(contigs.off, dtype=np.int64)
    bases = np.asarray(contigs.bases, dtype=np.uint8)
    n = len(off) - 1
    if args.queries_64:
        rng = np.random.default_rng(1)
        at = rng.integers(0, len(bases) - 64, args.queries_64)
        q = np.concatenate([bases[a:a + 64] for a in at])
        qoff = np.arange(args.queries_64 + 1, dtype=np.int64) * 64
    else:
        parts = [bases[off[i] + args.crop:off[i + 1] - args.crop] for i in range(n)]
        q = np.concatenate(parts)
        qoff = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    if args.bitmap is not None:
        os.environ["DH_LOCATE_BITMAP"] = str(args.bitmap)
    os.environ["DH_TRACE"] = "1"
    ctx = dentist_amd.Context(0)
    for _ in range(args.calls):
        t0 = time.perf_counter()
        hits = ctx.exact_locate_raw(bases, off, q, qoff, True)
        wall = (time.perf_counter() - t0) * 1e3
    if not args.queries_64:
        fwd = hits[hits["complement"] == 0]
        ok = (len(hits) == n and np.array_equal(fwd["query"], np.arange(n)) and np.array_equal(fwd["ref"], np.arange(n))
              and np.all(fwd["begin"] == args.crop) and np.array_equal(fwd["end"], np.diff(off) - args.crop))
        if not ok:
            raise SystemExit(f"wrong result: {len(hits)} hits for {n} contigs")
    peak = json.load(open(os.path.join(ROOT, "profiles", "constants.json")))["hbm_peak_GBs"]["value"]
    print(json.dumps({"records": n, "reference_bases": int(off[-1]), "queries": int(len(qoff) - 1), "query_bases": int(qoff[-1]),
                      "hits": int(len(hits)), "wall_ms_last_call": wall, "packed_text_bytes": int((off[-1] + 31) // 32 * 8),
                      "hbm_peak_GBs": peak, "note": "scan fraction of the HBM peak = packed_text_bytes / scan ms of the trace line / peak"}))


if __name__ == "__main__":
    main()
