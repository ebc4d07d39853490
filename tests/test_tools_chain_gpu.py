"""tools/chain-local-alignments: the chained .las as a file, against Context.chain(...).to_set on the same records."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
import chain_cases as cc
from test_tools_editpath_gpu import tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "chain-local-alignments")


def fasta(n, header):
    rng = np.random.default_rng(1)
    return "".join(f">{header(i)}\n{''.join('acgt'[c] for c in rng.integers(0, 4, 120))}\n" for i in range(n))


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain")
    tool("fasta2DAM", "-i", str(d / "ref.dam"), stdin=fasta(6, lambda i: f"scaf{i}"))
    tool("fasta2DB", "-i", str(d / "reads.db"), stdin=fasta(20, lambda i: f"sim/{i + 1}/0_120 RQ=0.850"))
    tool("DBsplit", "-x20", str(d / "ref.dam"))
    tool("DBsplit", "-x20", str(d / "reads.db"))
    las, trace = cc.with_traces(cc.random_case(seed=11, sizes=(1, 2, 3, 9, 65)))
    assert int(las["aread"].max()) < 6 and int(las["bread"].max()) < 20
    dentist_amd.las_write(str(d / "in.las"), las, trace, cc.TSPACE)
    return d, las, trace


@pytest.mark.parametrize("args,opts", [((), {}), (("--min-relative-score=0.5",), dict(min_relative_score=0.5))], ids=["default", "0.5"])
def test_tool_writes_what_the_library_chains(gpu_ctx, files, args, opts):
    d, las, trace = files
    tool("chain-local-alignments", *args, "ref.dam", "reads.db", "in.las", "out.las", cwd=d)
    rec, tr = gpu_ctx.chain(las, cc.TSPACE, **opts).to_set(las, trace, cc.TSPACE)
    assert len(rec) > 0
    dentist_amd.las_write(str(d / "expected.las"), rec, tr, cc.TSPACE)
    with open(d / "out.las", "rb") as f, open(d / "expected.las", "rb") as g:
        assert f.read() == g.read()


def test_bad_option_and_missing_input(files):
    d, _, _ = files
    r = subprocess.run([TOOL, "--min-relative-scores=0.5", "ref.dam", "reads.db", "in.las", "out2.las"], cwd=d, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 1 and "usage" in r.stderr and not os.path.exists(d / "out2.las")
    r = subprocess.run([TOOL, "ref.dam", "reads.db", "absent.las", "out2.las"], cwd=d, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "absent.las" in r.stderr
