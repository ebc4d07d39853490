"""The validation half of the workflow on this project's executables: the tail of the reference's command sequence
(tests/test-commands.sh:212-229) -- output --closed-gaps-bed, fasta2DAM + DBsplit of the preliminary assembly, bed2mask
--data-comments, damapper of the reads on it, LAmerge, LAsplit, validate-regions, the skip-gaps file made from its report, and
the final output --skip-gaps-file -- on a simulated assembly of about 60 kb: one scaffold with two gaps, a second one that no
read touches, reads of 4 kb at 20x."""
import json
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from test_tools_gpu import fasta_db
import validate_ref as vr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREADS = 300
VALIDATE = ["--read-coverage=20", "--ploidy=2"]    # min coverage reads (int)(0.5 * 20 / 2) = 5; defaults 3, 1000, 500
MIN_COV, MIN_SPAN, CONTEXT, WINDOW = 5, 3, 1000, 500


def tool(d, name, *args, stdin=None):
    r = subprocess.run([os.path.join(ROOT, "tools", name), *args], cwd=d, stdin=stdin, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (name, args, r.stderr)
    return r.stdout


def wrapped(header, seq, width=80):
    return header + "\n" + "\n".join(seq[i:i + width] for i in range(0, len(seq), width)) + "\n"


def records(fasta_text):
    """[(header up to its first tab, sequence)]"""
    out = []
    for rec in fasta_text.split(">")[1:]:
        lines = rec.split("\n")
        out.append((lines[0].split("\t")[0], "".join(lines[1:])))
    return out


@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("validation_loop"))
    w = sim.Workload(60_000, 2, NREADS, 4000, seed=7, spacing=10000, gap_max=600)
    text = sim.decode(w.truth)
    first, at = "", 0
    for b, e in zip(w.gap_begin, w.gap_end):
        first += text[at:b] + "n" * int(e - b)
        at = int(e)
    first += text[at:]
    second = sim.decode(sim.genome(99, 8000))
    assembly = wrapped(">scaf1 with two gaps", first) + wrapped(">scaf2 untouched", second)
    open(os.path.join(d, "assembly.fasta"), "w").write(assembly)
    open(os.path.join(d, "reads.fasta"), "w").write(fasta_db(w.reads))
    tool(d, "fasta2DB", "reads.db", "reads.fasta")
    tool(d, "DBsplit", "-x20", "reads.db")
    tool(d, "fasta2DAM", "assembly.dam", "assembly.fasta")
    tool(d, "DBsplit", "-x20", "assembly.dam")
    dentist_amd.dazz_write_mask(os.path.join(d, "assembly.dam"), "rep", np.zeros(5, np.int64), np.zeros(2, np.int32))
    tool(d, "damapper", "-C", "-T1", "-e0.7", "assembly", "reads.1")
    tool(d, "LAmerge", "-v", "assembly.reads.las", "assembly.reads.1.las")
    tool(d, "collect", "--mask=rep", "assembly.dam", "reads.db", "assembly.reads.las", "pile-ups.db")
    tool(d, "process", "--mask=rep", "--batch=0..$", "assembly.dam", "reads.db", "pile-ups.db", "batch.0.db")
    tool(d, "merge-insertions", "insertions.db", "batch.0.db")
    # tests/test-commands.sh:212-214
    tool(d, "output", "--agp=pre.agp", "--closed-gaps-bed=pre.bed", "--revert=scaffolding,skip-gaps,skip-gaps-file,agp-dazzler", "--agp-dazzler",
         "assembly.dam", "reads.db", "insertions.db", "pre.fasta")
    tool(d, "fasta2DAM", "pre.dam", "pre.fasta")
    tool(d, "DBsplit", "-x20", "pre.dam")
    tool(d, "bed2mask", "--config=dentist.json", "--data-comments", "--bed=pre.bed", "pre.dam", "closed-gaps")
    # :222-224 (the masks of :215-221 are not needed by a mapping this small)
    tool(d, "damapper", "-C", "-T1", "-e0.7", "pre", "reads.1")
    tool(d, "LAmerge", "-v", "pre.reads.las", "pre.reads.1.las")
    with open(os.path.join(d, "pre.reads.las"), "rb") as f:
        tool(d, "LAsplit", "pre.@.reads.las", "1", stdin=f)
    bed = [ln.split("\t") for ln in open(os.path.join(d, "pre.bed")).read().split("\n") if ln]
    assert len(bed) == 2, bed    # both gaps were closed
    gaps = []
    for scaffold, begin, end, comment in bed:
        contigs, reads = comment.split("|")
        assert scaffold == "scaf1 with two gaps" and contigs.startswith("contigs-") and reads.startswith("reads-")
        gaps.append((int(begin), int(end), [int(x) for x in contigs.split("-")[1:]], [int(x) for x in reads.split("-")[1:]]))
    assert [g[2] for g in gaps] == [[1, 2], [2, 3]] and all(len(g[3]) >= 3 for g in gaps)
    return dict(d=d, gaps=gaps, assembly=assembly)


def validate(x, *args, mask="closed-gaps"):
    return tool(x["d"], "validate-regions", "--config=dentist.json", "--threads=1", *args, "pre.dam", "reads.db", "pre.1.reads.las", mask).splitlines()


def test_a_every_report_line_carries_the_ids_of_its_bed_line(loop):
    x = loop
    lines = validate(x, *VALIDATE, "--report-all", "--weak-coverage-mask=dentist-weak-coverage")
    assert len(lines) == 2
    for line, (begin, end, contig_ids, read_ids) in zip(lines, x["gaps"]):
        rep = json.loads(line)
        # the gaps are closed: scaf1 is one contig of pre.dam, contig and scaffold coordinates are the same
        assert rep["region"] == {"contigId": 1, "begin": begin, "end": end}
        assert rep["contigIds"] == contig_ids and rep["consensusReadIds"] == read_ids
        assert list(rep)[-3:] == ["weakCoverageMaskBps", "contigIds", "consensusReadIds"]
    # the mask of the same command can be read back
    ptr, _ = dentist_amd.DazzDb(os.path.join(x["d"], "pre.dam")).read_mask("dentist-weak-coverage")
    assert len(ptr) == 3


def test_b_invalid_regions_become_skipped_gaps(loop):
    x = loop
    d = x["d"]
    lines = validate(x, *VALIDATE, f"--min-spanning-reads={NREADS + 1}")     # no region can have that many: all are reported
    assert len(lines) == 2 and all(json.loads(ln)["isValid"] is False for ln in lines)
    # jq -r 'select(.isValid // false | not) | .contigIds | map(tostring) | join("-")' (tests/test-commands.sh:228)
    skip = ["-".join(str(c) for c in rep["contigIds"]) for rep in map(json.loads, lines) if not rep.get("isValid", False)]
    assert skip == ["1-2", "2-3"]
    open(os.path.join(d, "skip-gaps.txt"), "w").write("".join(s + "\n" for s in skip))
    tool(d, "output", "--config=dentist.json", "--agp=gap-closed.agp", "--closed-gaps-bed=gap-closed.closed-gaps.bed", "--skip-gaps-file=skip-gaps.txt",
         "assembly.dam", "reads.db", "insertions.db", "gap-closed.fasta")
    assert open(os.path.join(d, "gap-closed.closed-gaps.bed")).read() == ""      # no gap is closed
    assert records(open(os.path.join(d, "gap-closed.fasta")).read()) == records(x["assembly"])
    # the same run without the file closes both
    tool(d, "output", "--config=dentist.json", "--agp=all.agp", "--closed-gaps-bed=all.bed", "assembly.dam", "reads.db", "insertions.db", "all.fasta")
    assert open(os.path.join(d, "all.bed")).read() == open(os.path.join(d, "pre.bed")).read()
    assert open(os.path.join(d, "all.fasta")).read() == open(os.path.join(d, "pre.fasta")).read()
    closed = records(open(os.path.join(d, "all.fasta")).read())
    assert [h for h, _ in closed] == ["scaf1 with two gaps", "scaf2 untouched"] and "n" not in closed[0][1]
    assert closed[1] == records(x["assembly"])[1]


def test_c_a_mask_without_extras_prints_what_it_printed_before(loop):
    x = loop
    path = os.path.join(x["d"], "pre.dam")
    dz = dentist_amd.DazzDb(path)
    ptr, iv = dz.read_mask("closed-gaps")
    assert ptr.tolist() == [0, 2, 2] and iv.reshape(-1, 2).tolist() == [[b, e] for b, e, _, _ in x["gaps"]]
    dentist_amd.dazz_write_mask(path, "plain", ptr, iv)
    assert dentist_amd.read_mask_extra(path, "plain", "contigs") is None
    las, _, _ = dentist_amd.las_read(os.path.join(x["d"], "pre.1.reads.las"))
    case = dict(las=las, contig_off=dz.off, regions=[(0, b, e) for b, e, _, _ in x["gaps"]], min_cov=MIN_COV, min_span=MIN_SPAN, context=CONTEXT,
                window=WINDOW)
    plain = validate(x, *VALIDATE, "--report-all", mask="plain")
    assert plain == vr.json_lines(case, vr.validate(case), True)
    assert all("contigIds" not in ln and "consensusReadIds" not in ln for ln in plain)
    # with the extras the same lines, the two keys behind them
    with_ids = validate(x, *VALIDATE, "--report-all")
    for a, c, (_, _, contig_ids, read_ids) in zip(with_ids, plain, x["gaps"]):
        assert a == c[:-1] + ',"contigIds":[%d,%d],"consensusReadIds":[%s]}' % (*contig_ids, ",".join(map(str, read_ids)))
