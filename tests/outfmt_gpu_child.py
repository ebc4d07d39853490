"""Child process of tests/test_parity_outfmt_gpu.py: every case of tests/outfmt_cases.py through Context.output_db at one
chunking (DH_OUT_CHUNK_MB is set before the library formats anything; the chunking "record" sets it per case to a chunk that
ends exactly on a record boundary).  Usage: outfmt_gpu_child.py <chunking> <dir>; writes <dir>/<case>.{fasta,agp,bed,dropped}."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import dentist_amd  # noqa: E402
import outfmt_cases as oc  # noqa: E402


def chunk_mb(nbytes):
    return repr(nbytes / 1048576.0)   # (a power of two in the divisor: the decimal is exact)


def main(chunking, out_dir):
    if chunking in ("64", "112"):
        os.environ["DH_OUT_CHUNK_MB"] = chunk_mb(int(chunking))
    else:
        os.environ.pop("DH_OUT_CHUNK_MB", None)
    ctx = dentist_amd.Context(0)
    for name, c in oc.ALL.items():
        if chunking == "record":
            q = oc.chunk_at_record_boundary(oc.plan_of(c))
            if q is None:
                continue
            os.environ["DH_OUT_CHUNK_MB"] = chunk_mb(q)
        db = os.path.join(out_dir, name + ".insertions.db")
        oc.write_db(c, db)
        A = ctx.db(oc.seqdb(c))
        base = os.path.join(out_dir, name)
        dropped = ctx.output_db(base + ".fasta", A, c["scaffold_of"], c["headers"], c["gap_len"], db, bed_path=base + ".bed",
                                agp_path=base + ".agp", agp_dazzler=True, **c["opts"])
        open(base + ".dropped", "w").write(str(dropped))
    ctx.close()
    print("done")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
