"""tools/merge-masks and tools/filter-mask on a small .dam built with fasta2DAM whose masks are written through the binding: the
written tracks, byte for byte, against write_mask applied to the restatement's result (tests/maskops_ref.py); a `<block>.<mask>`
input on a DB of two blocks; both filter options alone and together; the empty mask; the options that are accepted and
ignored; the usage and exit 1 for an unknown option; exit 2 for a missing mask."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
import maskops_cases as mc
import maskops_ref as mr
from test_tools_editpath_gpu import tool
from test_tools_propagate_gpu import fasta

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NREF, REF_LEN = 5, 2400
CO = np.arange(NREF + 1, dtype=np.int64) * REF_LEN
MASKS = {"a": [(0, 100, 300), (0, 250, 400), (2, 0, 50), (2, 2390, 2400), (4, 7, 7)],
         "b": [(0, 400, 500), (2, 60, 70), (2, 40, 45), (3, 1000, 1200)],
         "c": [(3, 1100, 1300), (3, 1306, 1400), (0, 0, 10), (2, 75, 77)]}


def track_bytes(d, db, name):
    return tuple(open(d / f".{db}.{name}.{ext}", "rb").read() for ext in ("anno", "data"))


def expect_bytes(d, triples, n=NREF, db="ref"):
    """the files write_mask makes of the restatement's result"""
    ptr, iv = mc.mask(n, triples)
    dentist_amd.dazz_write_mask(str(d / f"{db}.dam"), "expected", ptr, iv.reshape(-1) if len(iv) else np.zeros(2, np.int32))
    return track_bytes(d, db, "expected")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("maskops")
    tool("fasta2DAM", "-i", str(d / "ref.dam"), stdin=fasta(NREF, REF_LEN, lambda i: f"scaf{i}", 1))
    tool("DBsplit", "-x20", str(d / "ref.dam"))
    for name, t in MASKS.items():
        ptr, iv = mc.mask(NREF, t)
        dentist_amd.dazz_write_mask(str(d / "ref.dam"), name, ptr, iv.reshape(-1))
    dentist_amd.dazz_write_mask(str(d / "ref.dam"), "none", np.zeros(NREF + 1, np.int64), np.zeros(2, np.int32))
    return d


def test_merge_three_masks(files):
    d = files
    tool("merge-masks", "ref.dam", "merged", "a", "b", "c", cwd=d)
    exp = mr.combine_intervals([mc.mask(NREF, MASKS[k]) for k in "abc"], CO)
    assert len(exp) == 8 and (0, 0, 10) in exp and (0, 100, 500) in exp and (3, 1000, 1300) in exp
    assert track_bytes(d, "ref", "merged") == expect_bytes(d, exp)
    tool("merge-masks", "ref.dam", "merged-1", "b", cwd=d)       # one input: normalised
    assert track_bytes(d, "ref", "merged-1") == expect_bytes(d, sorted(MASKS["b"]))
    tool("merge-masks", "ref.dam", "merged-0", "none", "none", cwd=d)
    assert track_bytes(d, "ref", "merged-0") == expect_bytes(d, [])


def test_merge_a_block_mask(tmp_path):
    """`<block>.<mask>` is the track of DB block <block>: its reads are shifted by the block's first id (Snakefile:583-584, 1490)"""
    d, n, length = tmp_path, 6, 300_000
    rng = np.random.default_rng(3)
    text = "".join(f">scaf{i}\n{np.frombuffer(b'acgt', np.uint8)[rng.integers(0, 4, length)].tobytes().decode()}\n" for i in range(n))
    tool("fasta2DAM", "-i", str(d / "big.dam"), stdin=text)
    tool("DBsplit", "-x20", "-s1", str(d / "big.dam"))
    b1, b2 = dentist_amd.DazzDb(str(d / "big.1.dam")), dentist_amd.DazzDb(str(d / "big.2.dam"))
    assert b1.n + b2.n == n and b1.n > 0 and b2.n > 1 and b2.first_id == b1.n
    whole = [(0, 5, 50), (n - 1, 0, 100)]
    in_block = [(0, 10, 20), (1, 299_000, 300_000), (1, 15, 25)]         # reads of block 2
    ptr, iv = mc.mask(n, whole)
    dentist_amd.dazz_write_mask(str(d / "big.dam"), "weak", ptr, iv.reshape(-1))
    ptr, iv = mc.mask(b2.n, in_block)
    # a block's track: `.big.2.weak.anno` with one entry per read of the block (write_mask takes no dots: renamed)
    dentist_amd.dazz_write_mask(str(d / "big.dam"), "weakblock", ptr, iv.reshape(-1))
    for ext in ("anno", "data"):
        os.rename(d / f".big.weakblock.{ext}", d / f".big.2.weak.{ext}")
    tool("merge-masks", "big.dam", "merged", "weak", "2.weak", cwd=d)
    shifted = [(c + b2.first_id, b, e) for c, b, e in in_block]
    exp = mr.combine_intervals([mc.mask(n, whole), mc.mask(n, shifted)], np.arange(n + 1, dtype=np.int64) * length)
    assert track_bytes(d, "big", "merged") == expect_bytes(d, exp, n, "big") and (b2.first_id, 10, 20) in exp


@pytest.mark.parametrize("gap,size", [(6, 0), (0, 51), (6, 51), (0, 0), (5, 50)])
def test_filter_options(files, gap, size):
    d = files
    tool("merge-masks", "ref.dam", "all", "a", "b", "c", cwd=d)
    opts = ([f"--min-gap-size={gap}"] if gap else []) + ([f"--min-interval-size={size}"] if size else [])
    name = f"filtered-{gap}-{size}"
    tool("filter-mask", *opts, "ref.dam", "all", name, cwd=d)
    masks = [mc.mask(NREF, MASKS[k]) for k in "abc"]
    exp = mr.combine_intervals(masks, CO, min_gap=gap, min_interval=size)
    assert track_bytes(d, "ref", name) == expect_bytes(d, exp)
    united = mr.combine_intervals(masks, CO)
    assert (exp != united) == bool(gap or size)
    if (gap, size) == (6, 51):      # [1100, 1300) and [1306, 1400) are 6 apart; [2, 0, 50) is 50 long
        assert (3, 1000, 1400) in exp and (2, 0, 50) not in exp
    if (gap, size) == (5, 50):
        assert (3, 1000, 1300) in exp and (2, 0, 50) in exp


def test_filter_the_empty_mask(files):
    d = files
    tool("filter-mask", "--min-gap-size=10", "--min-interval-size=10", "ref.dam", "none", "none-filtered", cwd=d)
    assert track_bytes(d, "ref", "none-filtered") == expect_bytes(d, [])


@pytest.mark.parametrize("name,args", [("merge-masks", ["ref.dam", "ignored-m", "a", "b"]), ("filter-mask", ["--min-gap-size=3", "ref.dam", "a", "ignored-f"])])
def test_accepted_and_ignored_options(files, name, args):
    d = files
    r = subprocess.run([os.path.join(ROOT, "tools", name), "--config=x.yml", "-v", "--quiet", "-T4", "--threads=2", *args], cwd=d, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and r.stderr.count("have no effect here") == 1, r.stderr
    tool(name, *[a.replace("ignored", "plain") for a in args], cwd=d)
    out = args[1] if name == "merge-masks" else args[-1]
    assert track_bytes(d, "ref", out) == track_bytes(d, "ref", out.replace("ignored", "plain"))


@pytest.mark.parametrize("name,args", [("merge-masks", ["--frobnicate", "ref.dam", "x", "a"]), ("filter-mask", ["--min-gap=3", "ref.dam", "a", "x"]),
                                       ("filter-mask", ["--min-gap-size=-3", "ref.dam", "a", "x"]), ("merge-masks", ["ref.dam", "x"])])
def test_usage_and_exit_1(files, name, args):
    r = subprocess.run([os.path.join(ROOT, "tools", name), *args], cwd=files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 1 and f"usage: {name}" in r.stderr and not os.path.exists(files / ".ref.x.anno")


@pytest.mark.parametrize("name,args,words", [("merge-masks", ["ref.dam", "x", "a", "missing"], "mask track not found: missing"),
                                             ("filter-mask", ["ref.dam", "missing", "x"], "mask track not found: missing"),
                                             ("merge-masks", ["nowhere.dam", "x", "a"], "cannot open nowhere.dam")])
def test_exit_2_with_the_library_message(files, name, args, words):
    r = subprocess.run([os.path.join(ROOT, "tools", name), *args], cwd=files, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and words in r.stderr and not os.path.exists(files / ".ref.x.anno"), r.stderr
