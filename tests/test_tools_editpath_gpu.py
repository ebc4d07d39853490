"""tools/LApaf: PAF with an extended cigar from a .las, against Context.edit_paths on the same inputs."""
import os
import re
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fasta_dam(db, name="scaf"):
    out = []
    for i in range(db.n):
        s = sim.decode(db.seq(i))
        out.append(f">{name}{i}\n" + "\n".join(s[k:k + 80] for k in range(0, len(s), 80)))
    return "\n".join(out) + "\n"


def fasta_db(db):
    out = []
    for i in range(db.n):
        s = sim.decode(db.seq(i))
        out.append(f">sim/{i + 1}/0_{len(s)} RQ=0.850\n" + "\n".join(s[k:k + 100] for k in range(0, len(s), 100)))
    return "\n".join(out) + "\n"


def tool(name, *args, cwd=None, stdin=None):
    r = subprocess.run([os.path.join(ROOT, "tools", name), *args], cwd=cwd, input=stdin, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr
    return r.stdout


def ops_of_block(lines):
    """the ops a `-a` block shows: three lines per chunk (A line, compare line, B line), chunks separated by an empty line"""
    ops = []
    for k in range(0, len(lines), 4):
        a, c, b = lines[k:k + 3]
        assert len(a) == len(c) == len(b) and (k + 3 >= len(lines) or lines[k + 3] == "")
        for x, y, z in zip(a, c, b):
            if x == "-":
                assert y == " "
                ops.append(2)
            elif z == "-":
                assert y == " "
                ops.append(1)
            else:
                assert (y == "|") == (x == z) and y in "|*"
                ops.append(0 if y == "|" else 3)
    return np.asarray(ops, dtype=np.uint8)


def test_lapaf_matches_the_library(gpu_ctx, tmp_path):
    w = sim.Workload(120_000, 2, 60, 3000, seed=41, spacing=15000)
    tool("fasta2DAM", "-i", str(tmp_path / "ref.dam"), stdin=fasta_dam(w.contigs))
    tool("fasta2DB", "-i", str(tmp_path / "reads.db"), stdin=fasta_db(w.reads))
    tool("DBsplit", "-x20", str(tmp_path / "ref.dam"))
    tool("DBsplit", "-x20", str(tmp_path / "reads.db"))
    tool("damapper", "-T1", "-e0.7", "ref", "reads.1", cwd=tmp_path)
    las_path = str(tmp_path / "ref.reads.1.las")
    las, trace, ts = dentist_amd.las_read(las_path)
    assert len(las) >= w.reads.n and set((las["flags"] & 1).tolist()) == {0, 1}
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    out = tool("LApaf", "-a", "-w60", "ref.dam", "reads.db", "ref.reads.1.las", cwd=tmp_path).split("\n")
    assert out[-1] == ""
    out = out[:-1]
    recs, blocks = [], []
    for line in out:
        if line.startswith("#"):
            blocks[-1].append(line[1:])
        else:
            recs.append(line.split("\t"))
            blocks.append([])
    assert len(recs) == len(las)
    for i, (f, la) in enumerate(zip(recs, las)):
        assert len(f) == 15
        ops = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        blen, alen = w.reads.length(int(la["bread"])), w.contigs.length(int(la["aread"]))
        comp = bool(la["flags"] & 1)
        assert f[0] == f"sim/{la['bread'] + 1}" and f[5] == f"scaf{la['aread']}/{la['aread'] + 1}"
        assert (int(f[1]), int(f[6])) == (blen, alen)
        qb, qe = (blen - la["bepos"], blen - la["bbpos"]) if comp else (la["bbpos"], la["bepos"])
        assert (int(f[2]), int(f[3]), f[4]) == (qb, qe, "-" if comp else "+")
        assert (int(f[7]), int(f[8])) == (la["abpos"], la["aepos"])
        assert f[11] == "255"
        tags = dict((t[:4], t[5:]) for t in f[12:])
        cg = tags["cg:Z"]
        assert cg == dentist_amd.format_cigar(ops, extended=True)
        assert int(tags["NM:i"]) == ep.score[i]
        assert int(tags["tp:i"]) == int(trace[la["toff"]:la["toff"] + la["tlen"]:2].sum()) >= ep.score[i]
        runs = [(int(n), c) for n, c in re.findall(r"(\d+)([=XID])", cg)]
        assert int(f[9]) == sum(n for n, c in runs if c == "=")       # residue matches
        assert int(f[10]) == sum(n for n, _ in runs) == len(ops)      # alignment block length
        assert sum(n for n, c in runs if c in "=XD") == int(f[8]) - int(f[7])
        assert sum(n for n, c in runs if c in "=XI") == int(f[3]) - int(f[2])
        assert np.array_equal(ops_of_block(blocks[i]), ops)
        assert all(len(l) <= 60 for l in blocks[i])
    # a record range, without -a: the same lines
    part = tool("LApaf", "ref.dam", "reads.db", "ref.reads.1.las", "3-7", cwd=tmp_path).split("\n")[:-1]
    assert [l.split("\t") for l in part] == recs[2:7]
    r = subprocess.run([os.path.join(ROOT, "tools", "LApaf"), "ref.dam", "reads.db", "ref.reads.1.las", f"1-{len(las) + 1}"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "range" in r.stderr
