"""tools/collect: a reference DAM of two scaffolds with gaps, a reads DB, a mapping and two mask tracks; the written pile-ups.db
against the file the library route writes from the same inputs -- dentist_amd.collect_filter (the host function), the resolved
scaffold pile-ups, all pile-ups, Pileups.write_db -- and the stage lines against dropped6."""
import os
import re
import subprocess

import numpy as np
import pytest

import dentist_amd
import propagate_cases as pc
from test_tools_editpath_gpu import tool
from test_tools_propagate_gpu import fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "collect")
CLEN, RLEN, TS, NREADS = 3000, 2000, 100, 24
STAGES = ("LQ", "Improper", "WeaklyAnchored", "Contained", "Ambiguous", "Redundant")


def reference():
    """scaffold A of three contigs, scaffold B of two, runs of n between them"""
    rng = np.random.default_rng(1)
    seq = lambda: "".join("acgt"[c] for c in rng.integers(0, 4, CLEN))   # noqa: E731
    return f">scafA\n{seq()}{'n' * 50}{seq()}{'n' * 70}{seq()}\n>scafB\n{seq()}{'n' * 40}{seq()}\n"


def mapping():
    """four reads across every gap of the assembly, and one read for every filter to drop"""
    b = pc.Builder(TS)
    r = 0
    for c in (0, 1, 3):
        for _ in range(4):
            b.record(c, r, CLEN - 900, CLEN, 0, [100] * 9)
            b.record(c + 1, r, 0, 1100, 900, [100] * 11)
            r += 1
    b.record(0, r, CLEN - 900, CLEN, 0, [100] * 9)                  # LQ (diffs set below)
    lq = len(b.rows) - 1
    b.record(1, r + 1, 1000, 1900, 500, [100] * 9)                  # Improper
    b.record(4, r + 2, 0, 900, 1100, [100] * 9)                     # WeaklyAnchored: 500 of its 900 bases are masked
    b.record(2, r + 3, CLEN - 900, CLEN, 0, [100] * 9)              # Contained: the second lies inside the first
    b.record(2, r + 3, CLEN - 800, CLEN - 100, 100, [100] * 7)
    b.record(0, r + 4, CLEN - 900, CLEN, 0, [100] * 9)              # Ambiguous: both cover the read's bases 500 .. 900
    b.record(1, r + 4, 0, 1500, 500, [100] * 15)
    b.record(3, r + 5, 500, 2500, 0, [100] * 20)                    # Redundant: the read fits inside the contig
    case = b.case(ncontigs=5, nreads=NREADS)
    las = case["las"].copy()
    las["diffs"] = 20
    las["diffs"][lq] = 400
    return las, case["trace"]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("collect")
    tool("fasta2DAM", "-i", str(d / "ref.dam"), stdin=reference())
    tool("fasta2DB", "-i", str(d / "reads.db"), stdin=fasta(NREADS, RLEN, lambda i: f"sim/{i + 1}/0_{RLEN} RQ=0.850", 2))
    tool("DBsplit", "-x20", str(d / "ref.dam"))
    tool("DBsplit", "-x20", str(d / "reads.db"))
    ptr = np.asarray([0, 0, 0, 0, 0, 1])
    dentist_amd.dazz_write_mask(str(d / "ref.dam"), "rep", ptr, np.asarray([0, 450], dtype=np.int32))
    dentist_amd.dazz_write_mask(str(d / "ref.dam"), "tan", ptr, np.asarray([400, 500], dtype=np.int32))
    las, trace = mapping()
    dentist_amd.las_write(str(d / "ref.reads.las"), las, trace, TS)
    dentist_amd.las_write(str(d / "empty.las"), las[:0], trace[:0], TS)
    bad = las.copy()
    bad["diffs"] = (bad["aepos"] - bad["abpos"]) // 2
    dentist_amd.las_write(str(d / "bad.las"), bad, trace, TS)
    return d, las, trace


def run(d, *args):
    return subprocess.run([TOOL, *args], cwd=d, capture_output=True, text=True, timeout=300)


def library_route(gpu_ctx, d, las, trace, path, allowance=TS, **scaffold):
    ref, reads = dentist_amd.DazzDb(str(d / "ref.dam")), dentist_amd.DazzDb(str(d / "reads.db"))
    mask = (np.asarray([0, 0, 0, 0, 0, 1]), np.asarray([0, 500], dtype=np.int32))   # the union of the two tracks
    po = dentist_amd.default_process_opts(max_align_err_ppm=300000, allowance=allowance, min_anchor=500)
    flt, dropped, used = dentist_amd.collect_filter(las, ref.off, reads.off, po, repeat_mask=mask)
    gaps = [(c, c + 1) for c in range(ref.n - 1) if ref.origin[c + 1] > ref.origin[c]]
    assert gaps == [(0, 1), (1, 2), (3, 4)]
    opts = dict(min_spanning_reads=3, merge_extensions=1, best_pile_up_margin=3.0, existing_gap_bonus=6.0)
    opts.update(scaffold)
    resolve = dict(ctx=gpu_ctx, contigs=gpu_ctx.db(ref), reads=gpu_ctx.db(reads), map_opts=dentist_amd.default_align_opts(tspace=TS),
                   allowance=allowance, trace=trace)
    piles, skipped, all_las, all_trace, _ = dentist_amd.scaffold_all_pileups(flt, ref.off, reads.off, gaps, only="both", resolve=resolve, **opts)
    piles.write_db(str(path), all_las, np.concatenate([all_trace, [0]]), ref.off, reads.off, tspace=TS)
    return dropped, len(piles)


def test_pile_ups_db_is_that_of_the_library_route(gpu_ctx, files):
    d, las, trace = files
    dropped, npiles = library_route(gpu_ctx, d, las, trace, d / "expected.db")
    assert dropped.tolist() == [1, 1, 1, 1, 2, 1] and npiles >= 3
    r = run(d, "--mask=rep,tan", "ref.dam", "reads.db", "ref.reads.las", "pile-ups.db")
    assert r.returncode == 0, r.stderr
    assert (d / "pile-ups.db").read_bytes() == (d / "expected.db").read_bytes() and (d / "expected.db").stat().st_size > 100
    lines = {m.group(1): int(m.group(2)) for m in re.finditer(r"collect: filter (\w+) dropped (\d+) alignment chains", r.stderr)}
    assert [lines[s] for s in STAGES] == dropped.tolist()
    # the short forms, the options without effect, and every option at a value of its own
    dropped2, _ = library_route(gpu_ctx, d, las, trace, d / "expected2.db", allowance=50, min_spanning_reads=4, merge_extensions=0,
                                best_pile_up_margin=2.0, existing_gap_bonus=5.0)
    r = run(d, "-m", "rep", "-mtan", "-e0.3", "--min-anchor-length=500", "--proper-alignment-allowance=50", "--min-spanning-reads=4",
            "--best-pile-up-margin=2.0", "--existing-gap-bonus=5.0", "--no-merge-extension", "-v", "-T4", "--tmpdir=/nowhere", "ref.dam",
            "reads.db", "ref.reads.las", "pile-ups2.db")
    assert r.returncode == 0 and r.stderr.count("no effect") == 1, r.stderr
    assert (d / "pile-ups2.db").read_bytes() == (d / "expected2.db").read_bytes()


def test_exit_codes(files):
    d, _, _ = files
    r = run(d, "ref.dam", "reads.db", "ref.reads.las", "x.db")
    assert r.returncode == 1 and "usage" in r.stderr                      # a mask is required
    r = run(d, "--mask=rep", "--debug-pile-ups=x", "ref.dam", "reads.db", "ref.reads.las", "x.db")
    assert r.returncode == 1 and "usage" in r.stderr
    r = run(d, "--mask=rep", "ref.dam", "reads.db", "empty.las", "x.db")
    assert r.returncode == 2 and "empty ref vs. reads alignment" in r.stderr
    r = run(d, "--mask=rep", "ref.dam", "reads.db", "bad.las", "x.db")
    assert r.returncode == 2 and "no alignment chains left after filtering" in r.stderr
    r = run(d, "--mask=absent", "ref.dam", "reads.db", "ref.reads.las", "x.db")
    assert r.returncode == 2 and "absent" in r.stderr
    r = run(d, "--mask=rep", "--max-alignment-error=0.5", "ref.dam", "reads.db", "ref.reads.las", "x.db")
    assert r.returncode == 2 and "(0, 0.3]" in r.stderr
    assert not (d / "x.db").exists()
