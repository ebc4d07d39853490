"""tools/output, the last command of the reference's integration script (tests/test-commands.sh:184-230), through the file
route: process_pileups -> insertions.db -> tools/merge-insertions -> tools/output on DBs made with tools/fasta2DAM, tools/fasta2DB
and tools/DBsplit.  The reference's own checksum of gap-closed.fasta (tests/test-commands.sh:62-65), --skip-gaps, stdout, and
a simulated assembly with several gaps against dentist_amd.output_assembly on the in-memory result."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool(name, *args, cwd=None, stdin=None, binary=False):
    r = subprocess.run([os.path.join(ROOT, "tools", name), *args], cwd=cwd, input=stdin, capture_output=True, text=not binary, timeout=300)
    assert r.returncode == 0, (name, args, r.stderr)
    return r.stdout


def wrapped(header, seq, width=50):
    return header + "\n" + "\n".join(seq[i:i + width] for i in range(0, len(seq), width)) + "\n"


def fasta_db(db):
    out = []
    for i in range(db.n):
        s = sim.decode(db.seq(i))
        out.append(f">sim/{i + 1}/0_{len(s)} RQ=0.850\n" + "\n".join(s[k:k + 100] for k in range(0, len(s), 100)))
    return "\n".join(out) + "\n"


def make_dbs(d, assembly_fasta, reads):
    tool("fasta2DAM", "-i", "ref.dam", cwd=d, stdin=assembly_fasta)
    tool("DBsplit", "-x20", "ref.dam", cwd=d)
    tool("fasta2DB", "-i", "reads.db", cwd=d, stdin=fasta_db(reads))
    tool("DBsplit", "-x20", "reads.db", cwd=d)


@pytest.fixture(scope="module")
def fixture_route(gpu_ctx, tmp_path_factory):
    """the fixture of test_process_reference_fixture_gap_is_closed_perfectly up to the merged insertions.db"""
    d = tmp_path_factory.mktemp("fixture")
    raw = open(os.path.join(os.path.dirname(__file__), "golden", "test_commands_assembly_reference.fasta")).read()
    header, seq = raw.split("\n")[0], "".join(raw.split("\n")[1:])
    codes = sim.encode(seq)
    contigs = sim.SeqDb.from_list([codes[:2000], codes[2097:]])
    reads, _ = sim.reads(1724161952, codes, 40, 3000, 0, min_len=500)
    A, B = gpu_ctx.db(contigs), gpu_ctx.db(reads)
    las, trace = gpu_ctx.align_db(A, B, dentist_amd.default_align_opts())
    po = dentist_amd.default_process_opts(rounds=2, flank_window=20000)
    piles = dentist_amd.Pileups(las, contigs.off, po)
    rec, bases, ids = dentist_amd.process_pileups(gpu_ctx, A, B, las, trace, piles, po, read_ids=True,
                                                  insertions_db=(str(d / "batch.db"), contigs.off, po.tspace_pile))
    assert len(rec) == 1 and rec[0]["status"] == 0
    tool("merge-insertions", "insertions.db", "batch.db", cwd=d)
    assembly = seq[:2000] + "n" * 97 + seq[2097:]
    make_dbs(d, wrapped(header, assembly, 80), reads)
    return d, header, seq, assembly, ids


def test_reference_fixture_through_the_file_route(fixture_route):
    d, header, seq, assembly, ids = fixture_route
    tool("output", "--agp=gap-closed.agp", "--agp-dazzler", "--closed-gaps-bed=closed-gaps.bed", "ref.dam", "reads.db", "insertions.db",
         "gap-closed.fasta", cwd=d)
    data = open(d / "gap-closed.fasta", "rb").read()
    assert hashlib.md5(data).hexdigest() == "c3836dc00a3f5e1e2aa8f2a802da4d67"   # tests/test-commands.sh:62-65
    idlist = "-".join(str(int(x) + 1) for x in sorted(ids[0].tolist()))
    assert open(d / "closed-gaps.bed").read() == f"{header[1:]}\t2000\t2098\tcontigs-1-2|reads-{idlist}\n"   # every read of the pile-up
    agp = [ln for ln in open(d / "gap-closed.agp").read().split("\n") if ln and not ln.startswith("#")]
    assert len(agp) == 3 and agp[1].split("\t")[4:6] == ["O", f"reads-{idlist}"]
    # the read names of the reads DB when the AGP asks for them
    tool("output", "--agp=names.agp", "ref.dam", "reads.db", "insertions.db", "again.fasta", cwd=d)
    assert open(d / "again.fasta", "rb").read() == data
    comp = [ln for ln in open(d / "names.agp").read().split("\n") if "\tO\t" in ln][0].split("\t")[5].split(" ")
    assert len(comp) == len(ids[0]) and all(x.startswith("sim/") for x in comp)


def test_skip_gaps_writes_the_input_assembly_back(fixture_route):
    d, header, seq, assembly, ids = fixture_route
    for spec in ("--skip-gaps=1-2", "--skip-gaps=2-1"):
        tool("output", spec, "--closed-gaps-bed=none.bed", "ref.dam", "reads.db", "insertions.db", "skipped.fasta", cwd=d)
        assert open(d / "skipped.fasta").read() == wrapped(header + "\tscaffold-1", assembly)
        assert open(d / "none.bed").read() == ""
    (d / "gaps.txt").write_text("# the only gap\n\n1-2\n")
    tool("output", "--skip-gaps-file=gaps.txt", "ref.dam", "reads.db", "insertions.db", "skipped2.fasta", cwd=d)
    assert open(d / "skipped2.fasta").read() == wrapped(header + "\tscaffold-1", assembly)


def test_without_a_result_file_the_fasta_goes_to_stdout(fixture_route):
    d, header, seq, assembly, ids = fixture_route
    tool("output", "ref.dam", "reads.db", "insertions.db", "file.fasta", cwd=d)
    out = tool("output", "ref.dam", "reads.db", "insertions.db", cwd=d, binary=True)
    assert out == open(d / "file.fasta", "rb").read() and hashlib.md5(out).hexdigest() == "c3836dc00a3f5e1e2aa8f2a802da4d67"


def test_simulated_assembly_with_several_gaps(gpu_ctx, tmp_path):
    w = sim.Workload(160_000, 4, 1200, 4000, seed=5, spacing=10000, gap_max=600)
    ngaps = len(w.gap_begin)
    assert ngaps >= 3
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    las, trace = gpu_ctx.align_db(A, B, dentist_amd.default_align_opts(algo=1, width=64))
    po = dentist_amd.default_process_opts(algo=1)
    piles = dentist_amd.Pileups(las, w.contigs.off, po)
    dbp = str(tmp_path / "insertions.db")
    rec, bases, ids = dentist_amd.process_pileups(gpu_ctx, A, B, las, trace, piles, po, read_ids=True,
                                                  insertions_db=(dbp, w.contigs.off, po.tspace_pile))
    ok = np.flatnonzero(rec["status"] == 0)
    assert len(ok) >= 3
    # the file gives the records of the process stage back
    rec2, bases2, ids2 = dentist_amd.insertions_from_db(dbp, w.contigs.off)
    assert len(rec2) == len(ok)
    for f in ("left_aepos", "right_abpos", "ins_begin", "ins_end", "comp", "cons_len", "join", "contig_left", "left_diffs", "right_diffs"):
        assert np.array_equal(rec2[f], rec[f][ok]), f
    right = np.where((rec["join"][ok] == 0) & (rec["contig_right"][ok] == 0), rec["contig_left"][ok] + 1, rec["contig_right"][ok])
    assert np.array_equal(rec2["contig_right"], right)
    for k, i in enumerate(ok):
        assert np.array_equal(bases2[rec2[k]["cons_off"]:rec2[k]["cons_off"] + rec2[k]["cons_len"]],
                              bases[rec[i]["cons_off"]:rec[i]["cons_off"] + rec[i]["cons_len"]])
        assert sorted(ids2[0][ids2[1][k]:ids2[1][k + 1]].tolist()) == sorted(ids[0][ids[1][i]:ids[1][i + 1]].tolist())
    # the tool's three files equal the host writer's on the in-memory result
    text = sim.decode(w.truth)
    asm, at = "", 0
    for b, e in zip(w.gap_begin, w.gap_end):
        asm += text[at:b] + "n" * int(e - b)
        at = int(e)
    asm += text[at:]
    make_dbs(tmp_path, wrapped(">scaf some words", asm, 80), w.reads)
    dz = dentist_amd.DazzDb(str(tmp_path / "ref.dam"))
    assert np.array_equal(dz.off, w.contigs.off) and np.array_equal(dz.bases, w.contigs.bases)
    tool("output", "--agp=tool.agp", "--agp-dazzler", "--closed-gaps-bed=tool.bed", "--fasta-line-width=60", "ref.dam", "reads.db",
         "insertions.db", "tool.fasta", cwd=tmp_path)
    gaps = [int(e - b) for b, e in zip(w.gap_begin, w.gap_end)] + [0]
    host = [str(tmp_path / n) for n in ("host.fasta", "host.bed", "host.agp")]
    dentist_amd.output_assembly(host[0], w.contigs, [0] * w.contigs.n, [dz.headers[0].lstrip(">")], gaps, rec, bases, read_ids=ids,
                                bed_path=host[1], agp_path=host[2], agp_dazzler=True, line_width=60, input_assembly="ref.dam")
    for mine, theirs in zip(("tool.fasta", "tool.bed", "tool.agp"), host):
        assert open(tmp_path / mine, "rb").read() == open(theirs, "rb").read(), mine
    assert open(host[1]).read().count("\n") == len(ok)
