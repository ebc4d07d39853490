"""Timed calls of the two writers of `dentist output` on the assembly of bench.py's configs[2] (not a test): 100 Mb, 1 000 gaps,
seeded, every gap closed by a synthetic insertion of its size.  No alignment is needed.

  host    dentist_amd.output_assembly (dh_output_assembly): the walk and one fputc per base on the host.
  device  Context.output_db (dh_output_db): insertions.db read, the walk, the FASTA text formatted by k_outfmt in chunks of
          DH_OUT_CHUNK_MB, copied back and written; AGP and BED on the host.  Its kernel / copy / fwrite times are the
          library's own (Context.output_stats: events around the kernels and copies, a host clock around fwrite).

Both routes write into the same temporary directory and alternate in one process after a warm-up call of each; every call ends
with its files closed (the device route synchronises before it returns).  Per route one JSON line: wall ms of every repetition,
median, min, max.  The files of the two routes are compared byte by byte in this run before anything is reported."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dentist_amd  # noqa: E402
from dentist_amd import sim  # noqa: E402
import outfmt_cases as oc  # noqa: E402  (write_db: a case as an insertions.db)


def workload(genome_len, ngaps, seed):
    truth = sim.genome(seed, genome_len)
    gb, ge = sim.gaps(seed + 1, genome_len, ngaps, 50, 5000, 20000)
    contigs, _ = sim.contigs_from_gaps(truth, gb, ge)
    n = len(gb)
    rec = np.zeros(n, dtype=dentist_amd.INSERTION_DTYPE)
    cons, at = [], 0
    for i in range(n):
        glen = int(ge[i] - gb[i])
        rec[i]["contig_left"], rec[i]["contig_right"] = i, i + 1
        rec[i]["left_aepos"], rec[i]["right_abpos"] = int(contigs.off[i + 1] - contigs.off[i]), 0
        rec[i]["ins_begin"], rec[i]["ins_end"], rec[i]["cons_off"], rec[i]["cons_len"], rec[i]["ref_read_id"] = 0, glen, at, glen, i
        cons.append(truth[gb[i]:ge[i]])
        at += glen
    ids = (np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int64))
    case = dict(contigs=[contigs.seq(i) for i in range(contigs.n)], scaffold_of=[0] * contigs.n, headers=["scaffold_1 bench assembly"],
                gap_len=[int(e - b) for b, e in zip(gb, ge)] + [0], rec=rec, bases=np.concatenate(cons), ids=ids,
                opts=dict(line_width=50, highlight=True, join_policy="scaffoldGaps", only="spanning", min_extension_length=100))
    return contigs, case


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=100_000_000)
    ap.add_argument("--gaps", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=20260929)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    contigs, c = workload(args.genome, args.gaps, args.seed)
    ctx = dentist_amd.Context(0)   # (raises without a device: a time is only measured there)
    A = ctx.db(contigs)
    with tempfile.TemporaryDirectory() as d:
        db = os.path.join(d, "insertions.db")
        oc.write_db(c, db)
        files = {r: [os.path.join(d, f"{r}.{e}") for e in ("fasta", "bed", "agp")] for r in ("host", "device")}

        def host():
            f = files["host"]
            dentist_amd.output_assembly(f[0], contigs, c["scaffold_of"], c["headers"], c["gap_len"], c["rec"], c["bases"], read_ids=c["ids"],
                                        bed_path=f[1], agp_path=f[2], agp_dazzler=True, **c["opts"])

        def device():
            f = files["device"]
            ctx.output_db(f[0], A, c["scaffold_of"], c["headers"], c["gap_len"], db, bed_path=f[1], agp_path=f[2], agp_dazzler=True, **c["opts"])

        host()      # warm-up of each, and the comparison
        device()
        for a, b in zip(files["host"], files["device"]):
            assert open(a, "rb").read() == open(b, "rb").read(), f"{a} and {b} differ"
        size = os.path.getsize(files["host"][0])
        wall = {"host": [], "device": []}
        parts = []
        for _ in range(args.reps):
            for name, call in (("host", host), ("device", device)):
                t0 = time.perf_counter()
                call()
                wall[name].append((time.perf_counter() - t0) * 1e3)
                if name == "device":
                    parts.append(ctx.output_stats())
        for a, b in zip(files["host"], files["device"]):
            assert open(a, "rb").read() == open(b, "rb").read(), f"{a} and {b} differ"
        for name in ("host", "device"):
            w = sorted(wall[name])
            line = dict(route=name, fasta_bytes=size, contigs=contigs.n, gaps=len(c["rec"]), reps=args.reps, wall_ms=[round(x, 2) for x in wall[name]],
                        wall_ms_median=round(w[len(w) // 2], 2), wall_ms_min=round(w[0], 2), wall_ms_max=round(w[-1], 2), byte_identical=True,
                        chunk_mb=os.environ.get("DH_OUT_CHUNK_MB", "256"))
            if name == "device":
                for k in ("kernel", "copy", "fwrite", "total"):
                    v = sorted(p[k] for p in parts)
                    line[f"{k}_ms_median"], line[f"{k}_ms_min"], line[f"{k}_ms_max"] = round(v[len(v) // 2], 3), round(v[0], 3), round(v[-1], 3)
            print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
