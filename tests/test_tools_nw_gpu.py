"""tools/DBnw: read i of one DB against read i of another end to end, against Context.nw_batch on the same sequences."""
import os
import re
import subprocess

import numpy as np
import pytest

import dentist_amd
import nw_ref as nr
from test_tools_editpath_gpu import ops_of_block, tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fasta(seqs, name):
    out = []
    for i, s in enumerate(seqs):
        t = "".join("acgt"[c] for c in s)
        out.append(f">{name}{i}\n" + "\n".join(t[k:k + 80] for k in range(0, len(t), 80)))
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("fs", [False, True], ids=["global", "free-shift"])
def test_dbnw_matches_the_library(gpu_ctx, tmp_path, fs):
    rng = np.random.default_rng(29)
    pairs = [nr.pair_of(rng, int(n), int(n) + int(rng.integers(-40, 41)), float(d))
             for n, d in zip(rng.integers(150, 1200, 12), rng.choice([0.0, 0.05, 0.2], 12))]
    refs, qrys = [p[0] for p in pairs], [p[1] for p in pairs]
    tool("fasta2DAM", "-i", str(tmp_path / "a.dam"), stdin=fasta(refs, "a"))
    tool("fasta2DAM", "-i", str(tmp_path / "b.dam"), stdin=fasta(qrys, "b"))
    ep, status = gpu_ctx.nw_batch(refs, qrys, free_shift=fs)
    assert not status.any()
    flags = ["-f"] if fs else []
    out = tool("DBnw", *flags, "-a", "-w60", "a.dam", "b.dam", cwd=tmp_path).split("\n")
    assert out[-1] == ""
    recs, blocks = [], []
    for line in out[:-1]:
        if line.startswith("#"):
            blocks[-1].append(line[1:])
        else:
            recs.append(line.split("\t"))
            blocks.append([])
    assert len(recs) == len(pairs)
    for i, f in enumerate(recs):
        ops = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        assert len(f) == 7
        assert [int(x) for x in f[:6]] == [i + 1, len(refs[i]), len(qrys[i]), int(ep.score[i]), int(np.count_nonzero(ops == 0)), len(ops)]
        assert f[6] == dentist_amd.format_cigar(ops, extended=True)
        runs = [(int(n), c) for n, c in re.findall(r"(\d+)([=XID])", f[6])]
        assert sum(n for n, c in runs if c in "=XD") == len(refs[i]) and sum(n for n, c in runs if c in "=XI") == len(qrys[i])
        assert np.array_equal(ops_of_block(blocks[i]), ops)
        assert all(len(l) <= 60 for l in blocks[i])
        assert "\n".join(blocks[i]) == dentist_amd.format_alignment(refs[i], qrys[i], ops, 60)
    # a range, without -a: the same lines
    part = tool("DBnw", *flags, "a.dam", "b.dam", "3-7", cwd=tmp_path).split("\n")[:-1]
    assert [l.split("\t") for l in part] == recs[2:7]
    r = subprocess.run([os.path.join(ROOT, "tools", "DBnw"), "a.dam", "b.dam", f"1-{len(pairs) + 1}"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "range" in r.stderr
