"""tools/mask-repetitive-regions: the self and the reads case on a small simulated DB; the written mask tracks (with
--debug-repeat-masks all three) read back and compared with the library route (Context.repeat_mask) and with the restatement of
the contract (tests/repeat_ref.py); both ways of giving the bounds; the option validation; the empty .las."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
import repeat_cases as rc
import repeat_ref as rr
from test_tools_editpath_gpu import tool
from test_tools_propagate_gpu import fasta, read_mask, records

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "mask-repetitive-regions")
NREF, NREADS, REF_LEN, READ_LEN, TS = 4, 12, 2400, 900, 100


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("rmask")
    tool("fasta2DAM", "-i", str(d / "ref.dam"), stdin=fasta(NREF, REF_LEN, lambda i: f"scaf{i}", 1))
    tool("fasta2DB", "-i", str(d / "reads.db"), stdin=fasta(NREADS, READ_LEN, lambda i: f"sim/{i + 1}/0_{READ_LEN} RQ=0.850", 2))
    tool("DBsplit", "-x20", str(d / "ref.dam"))
    tool("DBsplit", "-x20", str(d / "reads.db"))
    las, trace = [], []
    for seed in (5, 6, 7):   # records on contigs 0..2: contig 3 has none
        l, t = records(seed, NREF - 1, REF_LEN, NREADS, READ_LEN)
        l = l.copy()
        l["toff"] += len(trace)
        las.append(l)
        trace = np.concatenate([trace, t]) if len(trace) else t
    las = np.concatenate(las)
    las = las[np.lexsort((las["abpos"], las["bread"], las["aread"]))]
    dentist_amd.las_write(str(d / "ref.reads.las"), las, trace, TS)
    dentist_amd.las_write(str(d / "empty.las"), las[:0], trace[:0], TS)
    self_las = las.copy()   # a self alignment: the B side are contigs as well
    self_las["bread"] %= NREF
    dentist_amd.las_write(str(d / "ref.ref.las"), self_las, trace, TS)
    return d, las, self_las


CO = np.arange(NREF + 1, dtype=np.int64) * REF_LEN
RO = np.arange(NREADS + 1, dtype=np.int64) * READ_LEN


def same(path, name, lib, ref):
    ptr, iv = read_mask(path, name)
    got = rc.triples((ptr, iv))
    return got == rc.triples(lib) == ref


def test_self_case(files, gpu_ctx):
    d, _, self_las = files
    tool("mask-repetitive-regions", "ref.dam", "ref.ref.las", "rep-self", cwd=d)   # --max-coverage-self defaults to 4
    tool("mask-repetitive-regions", "--max-coverage-self=2", "ref.dam", "ref.ref.las", "rep-self2", cwd=d)
    for name, upper in (("rep-self", 4), ("rep-self2", 2)):
        lib = gpu_ctx.repeat_mask(self_las, CO, None, 0, upper)
        ref = rr.repeat_mask(self_las, CO, None, 0, upper)
        assert same(d / "ref.dam", name, lib.mask, ref["mask"])
    loose, tight = rr.repeat_mask(self_las, CO, None, 0, 4)["mask"], rr.repeat_mask(self_las, CO, None, 0, 2)["mask"]
    assert len(loose) > 0 and len(tight) > 0 and loose != tight


def test_reads_case_with_all_three_masks(files, gpu_ctx):
    d, las, _ = files
    tool("mask-repetitive-regions", "--max-coverage-reads=3", "--max-improper-coverage-reads=1", "--debug-repeat-masks", "ref.dam", "reads.db",
         "ref.reads.las", "rep", cwd=d)
    kw = dict(lower=0, upper=3, improper=(0, 1), allowance=TS)   # the allowance defaults to the trace spacing
    lib, ref = gpu_ctx.repeat_mask(las, CO, RO, **kw), rr.repeat_mask(las, CO, RO, **kw)
    assert same(d / "ref.dam", "rep", lib.mask, ref["mask"])
    assert same(d / "ref.dam", "rep-all", lib.all, ref["all"])
    assert same(d / "ref.dam", "rep-improper", lib.improper, ref["improper"])
    assert len(ref["all"]) > 0 and len(ref["improper"]) > 0 and ref["mask"] != ref["all"]
    # another allowance: other improper units
    tool("mask-repetitive-regions", "--max-coverage-reads=3", "--max-improper-coverage-reads=1", "--proper-alignment-allowance=700", "-v", "-T4",
         "ref.dam", "reads.db", "ref.reads.las", "rep700", cwd=d)
    kw["allowance"] = 700
    lib, ref2 = gpu_ctx.repeat_mask(las, CO, RO, **kw), rr.repeat_mask(las, CO, RO, **kw)
    assert same(d / "ref.dam", "rep700", lib.mask, ref2["mask"]) and ref2["improper_units"] < ref["improper_units"]
    assert not os.path.exists(d / ".ref.rep700-all.anno")   # only on request


def test_bounds_from_the_read_coverage(files, gpu_ctx):
    d, las, _ = files
    tool("mask-repetitive-regions", "--read-coverage=2.5", "ref.dam", "reads.db", "ref.reads.las", "rep-cov", cwd=d)
    upper, iupper = dentist_amd.max_coverage_reads(2.5), dentist_amd.max_improper_coverage_reads(2.5)
    kw = dict(lower=0, upper=upper, improper=(0, iupper), allowance=TS)
    lib, ref = gpu_ctx.repeat_mask(las, CO, RO, **kw), rr.repeat_mask(las, CO, RO, **kw)
    assert same(d / "ref.dam", "rep-cov", lib.mask, ref["mask"])


def test_empty_las(files):
    d, _, _ = files
    r = subprocess.run([TOOL, "--read-coverage=8", "--debug-repeat-masks", "ref.dam", "reads.db", "empty.las", "rep-empty"], cwd=d,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "empty reads-alignment" in r.stderr
    for name in ("rep-empty", "rep-empty-all", "rep-empty-improper"):
        ptr, iv = read_mask(d / "ref.dam", name)
        assert len(iv) == 0 and len(ptr) == NREF + 1 and not ptr.any()
    r = subprocess.run([TOOL, "ref.dam", "empty.las", "rep-empty-self"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "empty self-alignment" in r.stderr


def test_option_validation_and_exit_codes(files):
    d, _, _ = files

    def run(*args):
        return subprocess.run([TOOL, *args], cwd=d, capture_output=True, text=True, timeout=300)
    tail = ("ref.dam", "reads.db", "ref.reads.las", "rep-x")
    for args, words in ((("--max-improper-coverage-reads=1",), "must provide either --read-coverage or --max-coverage-reads"),
                        (("--read-coverage=8", "--max-coverage-reads=3"), "must not provide both --read-coverage and --max-coverage-reads"),
                        (("--max-coverage-reads=3",), "must provide either --read-coverage or --max-improper-coverage-reads"),
                        (("--read-coverage=8", "--max-improper-coverage-reads=1"),
                         "must not provide both --read-coverage and --max-improper-coverage-reads")):
        r = run(*args, *tail)
        assert r.returncode == 1 and words in r.stderr, (args, r.stderr)
    r = run("--max-coverage-self=0", "ref.dam", "ref.ref.las", "rep-x")
    assert r.returncode == 1 and "must be positive" in r.stderr
    r = run("--mask-everything", *tail)
    assert r.returncode == 1 and "usage" in r.stderr
    r = run("ref.dam", "rep-x")
    assert r.returncode == 1 and "usage" in r.stderr
    r = run("--read-coverage=8", "-v", "ref.dam", "reads.db", "absent.las", "rep-x")
    assert r.returncode == 2 and "absent.las" in r.stderr and r.stderr.count("have no effect here") == 1
    r = run("--read-coverage=8", "reads.db", "ref.dam", "ref.reads.las", "rep-x")   # the DBs exchanged: ids and ends out of range
    assert r.returncode == 2 and "dh_la_repeat_mask: record" in r.stderr
    assert not os.path.exists(d / ".ref.rep-x.anno")
