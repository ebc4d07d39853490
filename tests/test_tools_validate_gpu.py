"""tools/validate-regions: the regions of a mask track of a reference DAM validated against a .las of reads, the JSON lines
and the written weak-coverage mask against the restatement of the contract (tests/validate_ref.py)."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
import validate_ref as vr
from test_tools_editpath_gpu import tool
from test_tools_propagate_gpu import fasta, random_mask, read_mask, records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "validate-regions")
NREF, NREADS, REF_LEN, READ_LEN, TS = 4, 12, 2400, 900, 100


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("vreg")
    tool("fasta2DAM", "-i", str(d / "ref.dam"), stdin=fasta(NREF, REF_LEN, lambda i: f"scaf{i}", 1))
    tool("fasta2DB", "-i", str(d / "reads.db"), stdin=fasta(NREADS, READ_LEN, lambda i: f"sim/{i + 1}/0_{READ_LEN} RQ=0.850", 2))
    tool("DBsplit", "-x20", str(d / "ref.dam"))
    tool("DBsplit", "-x20", str(d / "reads.db"))
    mask = random_mask(3, NREF, REF_LEN, 5)
    dentist_amd.dazz_write_mask(str(d / "ref.dam"), "gaps", *mask)
    # records on contigs 1 and 2 only: the regions of contigs 0 and 3 are not the file's
    las, trace = [], []
    for seed in (5, 6, 7):
        l, t = records(seed, NREF, REF_LEN, NREADS, READ_LEN)
        l = l.copy()
        l["toff"] += len(trace)
        las.append(l)
        trace = np.concatenate([trace, t]) if len(trace) else t
    las = np.concatenate(las)
    las = las[(las["aread"] == 1) | (las["aread"] == 2)]
    las = las[np.lexsort((las["abpos"], las["bread"], las["aread"]))]
    dentist_amd.las_write(str(d / "ref.reads.las"), las, trace, TS)
    dentist_amd.las_write(str(d / "empty.las"), las[:0], trace[:0], TS)
    regions = [(c, int(b), int(e)) for c in (1, 2) for b, e in mask[1][mask[0][c]:mask[0][c + 1]]]
    return d, las, regions


def expect(las, regions, min_cov, min_span, context, window):
    case = dict(las=las, contig_off=np.arange(NREF + 1, dtype=np.int64) * REF_LEN, regions=regions, min_cov=min_cov, min_span=min_span,
                context=context, window=window)
    return case, vr.validate(case)


def test_report_lines_and_the_mask(files):
    d, las, regions = files
    case, exp = expect(las, regions, 2, 1, 100, 50)
    opts = ["--read-coverage=8", "--ploidy=2", "--min-spanning-reads=1", "--region-context=100", "--weak-coverage-window=50"]
    out = tool("validate-regions", *opts, "--report-all", "--weak-coverage-mask=weak", "ref.dam", "reads.db", "ref.reads.las", "gaps", cwd=d)
    lines = out.splitlines()
    assert len(lines) == len(regions) == 10 and lines == vr.json_lines(case, exp, True)
    assert any('"isValid":true' in x for x in lines) and any('"isValid":false' in x for x in lines)
    assert any('"spanningReadIds":[]' not in x for x in lines)
    ptr, iv = read_mask(d / "ref.dam", "weak")
    assert len(exp["mask"][1]) > 0 and np.array_equal(ptr, exp["mask"][0]) and np.array_equal(iv, exp["mask"][1])
    out = tool("validate-regions", *opts, "-v", "-T4", "ref.dam", "reads.db", "ref.reads.las", "gaps", cwd=d)
    assert out.splitlines() == vr.json_lines(case, exp, False) and 0 < len(out.splitlines()) < len(regions)


def test_defaults_and_min_coverage_reads(files):
    d, las, regions = files
    case, exp = expect(las, regions, 1, 3, 1000, 500)
    out = tool("validate-regions", "--min-coverage-reads=1", "--report-all", "ref.dam", "reads.db", "ref.reads.las", "gaps", cwd=d)
    assert out.splitlines() == vr.json_lines(case, exp, True)


def test_empty_las(files):
    d, _, _ = files
    r = subprocess.run([TOOL, "--min-coverage-reads=1", "--report-all", "ref.dam", "reads.db", "empty.las", "gaps"], cwd=d,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout == "" and "empty reads-alignment" in r.stderr


def test_exit_codes(files):
    d, _, _ = files

    def run(*args):
        return subprocess.run([TOOL, *args], cwd=d, capture_output=True, text=True, timeout=300)
    r = run("--min-coverage-reads=1", "--report-everything", "ref.dam", "reads.db", "ref.reads.las", "gaps")
    assert r.returncode == 1 and "usage" in r.stderr
    r = run("--min-coverage-reads=1", "ref.dam", "reads.db", "ref.reads.las", "absent")
    assert r.returncode == 2 and "absent" in r.stderr
    r = run("ref.dam", "reads.db", "ref.reads.las", "gaps")
    assert r.returncode == 2 and "exactly one" in r.stderr
    r = run("--min-coverage-reads=1", "--read-coverage=8", "--ploidy=2", "ref.dam", "reads.db", "ref.reads.las", "gaps")
    assert r.returncode == 2 and "exactly one" in r.stderr
    r = run("--read-coverage=8", "ref.dam", "reads.db", "ref.reads.las", "gaps")
    assert r.returncode == 2 and "ploidy" in r.stderr
