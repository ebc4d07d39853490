"""tools/stretcher: the call of `dentist check-results` (commands/checkResults.d:2091-2100) on FASTA files named the way it
names them, read back the way it reads them (:2113-2162), against Context.nw_affine_batch on the same sequences."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
import nwa_ref as ar
from test_pair_format import read_like_check_results

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STRETCHER = os.path.join(ROOT, "tools", "stretcher")


def write_fasta(path, header, seq, letters="acgt"):
    t = "".join(letters[c] if c < 4 else "n" for c in seq)
    with open(path, "w") as f:
        f.write(f">{header}\n" + "\n".join(t[k:k + 50] for k in range(0, len(t), 50)) + "\n")
        f.write(">a-second-record that is not read\nacgtacgt\n")


def run(*args, cwd):
    return subprocess.run([STRETCHER, *args], cwd=cwd, capture_output=True, text=True, timeout=300)


def ops_of_lines(ref_line, edit, qry_line):
    ops = []
    for x, y, z in zip(ref_line, edit, qry_line):
        if x == "-":
            assert y == "-" and z != "-"
            ops.append(2)
        elif z == "-":
            assert y == "-"
            ops.append(1)
        else:
            assert (y == "|") == (x == z) and y in "|."
            ops.append(0 if y == "|" else 3)
    return np.asarray(ops, np.uint8)


@pytest.mark.parametrize("rev", [False, True], ids=["forward", "sreverse2"])
def test_stretcher_as_check_results_calls_it(gpu_ctx, tmp_path, rev):
    rng = np.random.default_rng(31 + rev)
    r = rng.integers(0, 4, 900).astype(np.uint8)
    q = ar.mutate(rng, np.concatenate([r[:300], r[380:]]), 0.04)  # a missing stretch of 80 bases and some noise
    q[17] = 4                                                     # a letter outside ACGT
    stored = (3 - q[::-1]).astype(np.uint8) if rev else q.copy()  # --sreverse2 turns the file's sequence back into q
    stored[stored > 250] = 4                                      # (3 - 4 wraps: n stays n)
    write_fasta(tmp_path / "true.fasta", "true-1-2@1-2 [contig-1@10, contig-1@60)", r, "ACGT")
    write_fasta(tmp_path / "inserted.fasta", "inserted-1-2@1-2 [contig-1@10, contig-1@60)", stored)
    flags = ["--sreverse2"] if rev else []
    res = run("--auto", "--stdout", "--aformat=pair", "--awidth=4294967295", *flags, "true.fasta", "inserted.fasta", cwd=tmp_path)
    assert res.returncode == 0, res.stderr
    n, m, ref_line, edit, qry_line = read_like_check_results(res.stdout)
    ep, status = gpu_ctx.nw_affine_batch([r], [q])
    assert status[0] == 0
    assert np.array_equal(ops_of_lines(ref_line, edit, qry_line), ep.ops)
    assert (n, m) == (int(np.count_nonzero(ep.ops == 0)), len(ep.ops))
    assert ref_line.replace("-", "") == "".join("acgtn"[c] for c in r) and qry_line.replace("-", "") == "".join("acgtn"[c] for c in q)
    assert f"# Score: {int(ep.score[0])}" in res.stdout.split("\n")
    # one dash, other penalties, a file instead of stdout
    res2 = run("-auto", "-aformat=pair", "-awidth=60", "-gapopen=12", "-gapextend=3", "-outfile=out.pair", *flags, "true.fasta",
               "inserted.fasta", cwd=tmp_path)
    assert res2.returncode == 0 and res2.stdout == ""
    ep2, _ = gpu_ctx.nw_affine_batch([r], [q], scoring=(5, -4, 12, 3))
    text = open(tmp_path / "out.pair").read()
    assert text == dentist_amd.format_pair("true-1-2@1-2", r, "inserted-1-2@1-2", q, ep2.ops, int(ep2.score[0]), (5, -4, 12, 3), 60)
    assert "# Gap_penalty: 12" in text and "# Extend_penalty: 3" in text


def test_refusals_and_the_band_limit(tmp_path):
    rng = np.random.default_rng(37)
    a, b = rng.integers(0, 4, 3000).astype(np.uint8), rng.integers(0, 4, 3000).astype(np.uint8)
    write_fasta(tmp_path / "true.fasta", "true-1-2@1-2", a)
    write_fasta(tmp_path / "inserted.fasta", "inserted-1-2@1-2", b)
    res = run("--auto", "--stdout", "--aformat=pair", "true.fasta", "inserted.fasta", cwd=tmp_path)  # unrelated sequences
    assert res.returncode != 0 and res.stdout == "" and str(dentist_amd.NWA_MAX_BAND) in res.stderr
    res = run("--auto", "--stdout", "--aformat=srspair", "true.fasta", "inserted.fasta", cwd=tmp_path)
    assert res.returncode != 0 and res.stdout == "" and "srspair" in res.stderr
    res = run("--auto", "--stdout", "--frobnicate", "true.fasta", "inserted.fasta", cwd=tmp_path)
    assert res.returncode != 0 and res.stdout == ""
    res = run("--auto", "--stdout", "true.fasta", cwd=tmp_path)
    assert res.returncode != 0 and "usage" in res.stderr
