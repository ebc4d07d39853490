"""Context.output_db (dh_output_db: the FASTA text formatted by k_outfmt, AGP and BED on the host) against the host writer
dentist_amd.output_assembly on every case of tests/outfmt_cases.py, written as insertions.db and read back, at every chunking
(a fresh child process per chunking); the filter against the host writer called without the filtered records.  Every
comparison is byte equality."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dentist_amd

import outfmt_cases as oc

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the host writer's three files of every case, on the records dh_insertions_from_db reads back from the case's file"""
    d = tmp_path_factory.mktemp("host")
    out = {}
    for name, c in oc.ALL.items():
        db = str(d / (name + ".db"))
        oc.write_db(c, db)
        off = np.cumsum([0] + [len(x) for x in c["contigs"]])
        rec, bases, ids = dentist_amd.insertions_from_db(db, off)
        ok = c["rec"][c["rec"]["status"] == 0]
        for f in ("contig_left", "contig_right", "join", "left_aepos", "right_abpos", "ins_begin", "ins_end", "comp", "cons_len"):
            assert np.array_equal(rec[f], ok[f]), (name, f)     # the file holds the case
        base = str(d / name)
        dropped = oc.host_fasta(c, base + ".fasta", rec=rec, bases=bases, ids=ids, bed_path=base + ".bed", agp_path=base + ".agp")
        out[name] = (open(base + ".fasta", "rb").read(), open(base + ".agp", "rb").read(), open(base + ".bed", "rb").read(), dropped)
        # ... and on these the host writer writes what it writes on the case itself
        oc.host_fasta(c, base + ".direct.fasta")
        assert open(base + ".direct.fasta", "rb").read() == out[name][0], name
    return out


@pytest.mark.parametrize("chunking", ["default", "64", "112", "record"])
def test_every_case_is_byte_identical_to_the_host_writer(tmp_path, host, chunking):
    r = subprocess.run([sys.executable, os.path.join(HERE, "outfmt_gpu_child.py"), chunking, str(tmp_path)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.strip().endswith("done"), (r.returncode, r.stderr[-2000:])
    seen = 0
    for name in oc.ALL:
        base = str(tmp_path / name)
        if chunking == "record" and not os.path.exists(base + ".fasta"):
            continue
        seen += 1
        fa, agp, bed, dropped = host[name]
        assert open(base + ".fasta", "rb").read() == fa, name
        assert open(base + ".agp", "rb").read() == agp, name
        assert open(base + ".bed", "rb").read() == bed, name
        assert int(open(base + ".dropped").read()) == dropped, name
    assert seen >= (1 if chunking == "record" else len(oc.ALL))


def run_filtered(gpu_ctx, tmp_path, c, diffs, tag, **flt):
    db = str(tmp_path / (tag + ".db"))
    oc.write_db(c, db, diffs=diffs)
    base = str(tmp_path / tag)
    gpu_ctx.output_db(base + ".fasta", gpu_ctx.db(oc.seqdb(c)), c["scaffold_of"], c["headers"], c["gap_len"], db, bed_path=base + ".bed",
                      agp_path=base + ".agp", agp_dazzler=True, **flt, **c["opts"])
    return tuple(open(base + e, "rb").read() for e in (".fasta", ".agp", ".bed"))


def host_without(tmp_path, c, gone, tag):
    rec = c["rec"].copy()
    rec["status"][list(gone)] = 4   # (a record that is not DH_PILE_OK takes no part)
    base = str(tmp_path / tag)
    oc.host_fasta(c, base + ".fasta", rec=rec, bed_path=base + ".bed", agp_path=base + ".agp")
    return tuple(open(base + e, "rb").read() for e in (".fasta", ".agp", ".bed"))


def test_the_filter_gives_the_host_writers_files_without_the_filtered_records(gpu_ctx, tmp_path):
    c = oc.ALL["basic_w50"]
    # insertion 0: its left overlap covers A [0, 110): 12 diffs are 0.109 > 0.1, 11 diffs are exactly 0.1 and stay
    # (averageErrorRate > maxInsertionError, output.d:392); insertion 2 closes the gap of contigs 2 | 3 (0-based)
    none = host_without(tmp_path, c, [], "h_none")
    assert run_filtered(gpu_ctx, tmp_path, c, {0: (12, 0)}, "d_off") == none                                # no filter given
    assert run_filtered(gpu_ctx, tmp_path, c, {0: (11, 0)}, "d_at", max_insertion_error=0.1) == none
    assert run_filtered(gpu_ctx, tmp_path, c, {0: (12, 0)}, "d_err", max_insertion_error=0.1) == host_without(tmp_path, c, [0], "h_err")
    assert run_filtered(gpu_ctx, tmp_path, c, {0: (0, 9)}, "d_right", max_insertion_error=0.1) == host_without(tmp_path, c, [0], "h_right")  # 9 / 75 of contig 1
    assert run_filtered(gpu_ctx, tmp_path, c, None, "d_skip", skip_gaps=[(2, 3)]) == host_without(tmp_path, c, [2], "h_skip")
    assert run_filtered(gpu_ctx, tmp_path, c, {0: (12, 0)}, "d_both", max_insertion_error=0.1, skip_gaps=[(2, 3), (0, 5)]) == \
        host_without(tmp_path, c, [0, 2], "h_both")
    assert host_without(tmp_path, c, [0, 2], "h_both2") != none


def test_no_device_route_and_refusals(gpu_ctx, tmp_path):
    c = oc.ALL["cyclic"]
    db = str(tmp_path / "c.db")
    oc.write_db(c, db)
    A = gpu_ctx.db(oc.seqdb(c))
    with pytest.raises(dentist_amd.DhError) as ei:
        gpu_ctx.output_db(str(tmp_path / "x.fasta"), A, c["scaffold_of"], c["headers"], c["gap_len"], db, skip_gaps=[(1, 1)], **c["opts"])
    assert ei.value.code == -1 and "skip_gaps2" in str(ei.value)
    with pytest.raises(dentist_amd.DhError) as ei:
        gpu_ctx.output_db(str(tmp_path / "no" / "x.fasta"), A, c["scaffold_of"], c["headers"], c["gap_len"], db, **c["opts"])
    assert ei.value.code == -5
    st = gpu_ctx.output_stats()
    assert set(st) == {"kernel", "copy", "fwrite", "total"}
