"""tools/LApaf -c: one PAF line per chain of a .las, against Context.chain_paths on the same inputs; without -c the tool prints
what it printed before, one line per record from Context.edit_paths."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from test_tools_editpath_gpu import fasta_dam, fasta_db, ops_of_block, tool

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def expected_lines(ctx, w, las, trace, ts):
    """the -c lines formatted from chain_paths, one call per chain for its own filler count"""
    A, B = ctx.db(w.contigs), ctx.db(w.reads)
    op_off, ops, score, status, _ = ctx.chain_paths(A, B, las, trace, ts)
    off = [i for i in range(len(las)) if i == 0 or not (las[i]["flags"] & 8)] + [len(las)]
    lines = []
    for i in range(len(off) - 1):
        ch = las[off[i]:off[i + 1]]
        f, l = ch[0], ch[-1]
        nf = ctx.chain_paths(A, B, ch, trace, ts, chain_off=[0, len(ch)])[4]
        blen, alen = w.reads.length(int(f["bread"])), w.contigs.length(int(f["aread"]))
        comp = bool(f["flags"] & 1)
        qb, qe = (blen - l["bepos"], blen - f["bbpos"]) if comp else (f["bbpos"], l["bepos"])
        o = ops[op_off[i]:op_off[i + 1]]
        nested = status[i] == dentist_amd.CP_NESTED
        tags = [f"NM:i:{score[i]}", f"nl:i:{len(ch)}", f"nf:i:{nf}", "cg:Z:" + ("*" if nested else dentist_amd.format_cigar(o, extended=True))]
        if status[i] == dentist_amd.CP_FAKED:
            tags.append("fk:i:1")
        if nested:
            tags.append("st:Z:nested")
        lines.append("\t".join([f"sim/{f['bread'] + 1}", str(blen), str(qb), str(qe), "-" if comp else "+", f"scaf{f['aread']}/{f['aread'] + 1}",
                                str(alen), str(f["abpos"]), str(l["aepos"]), str(int(np.count_nonzero(o == 0))), str(len(o)), "255"] + tags))
    return lines, (op_off, ops)


def test_lapaf_chains_match_the_library(gpu_ctx, tmp_path):
    w = sim.Workload(120_000, 2, 60, 3000, seed=41, spacing=15000)
    tool("fasta2DAM", "-i", str(tmp_path / "ref.dam"), stdin=fasta_dam(w.contigs))
    tool("fasta2DB", "-i", str(tmp_path / "reads.db"), stdin=fasta_db(w.reads))
    tool("DBsplit", "-x20", str(tmp_path / "ref.dam"))
    tool("DBsplit", "-x20", str(tmp_path / "reads.db"))
    tool("damapper", "-T1", "-e0.7", "ref", "reads.1", cwd=tmp_path)
    las, trace, ts = dentist_amd.las_read(str(tmp_path / "ref.reads.1.las"))
    exp, (op_off, ops) = expected_lines(gpu_ctx, w, las, trace, ts)
    assert 0 < len(exp) <= len(las)
    out = tool("LApaf", "-c", "-a", "-w60", "ref.dam", "reads.db", "ref.reads.1.las", cwd=tmp_path).split("\n")
    assert out[-1] == ""
    lines, blocks = [], []
    for line in out[:-1]:
        if line.startswith("#"):
            blocks[-1].append(line[1:])
        else:
            lines.append(line)
            blocks.append([])
    assert lines == exp
    for i, b in enumerate(blocks):
        if "st:Z:nested" not in lines[i]:
            assert np.array_equal(ops_of_block(b), ops[op_off[i]:op_off[i + 1]])
    # first-last counts chains
    part = tool("LApaf", "-c", "ref.dam", "reads.db", "ref.reads.1.las", "2-4", cwd=tmp_path).split("\n")[:-1]
    assert part == exp[1:4]
    r = subprocess.run([os.path.join(ROOT, "tools", "LApaf"), "-c", "ref.dam", "reads.db", "ref.reads.1.las", f"1-{len(exp) + 1}"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "range" in r.stderr
    # without -c: a line per record, as before
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    plain = tool("LApaf", "ref.dam", "reads.db", "ref.reads.1.las", cwd=tmp_path).split("\n")[:-1]
    assert len(plain) == len(las)
    for i, (line, la) in enumerate(zip(plain, las)):
        f = line.split("\t")
        o = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        assert len(f) == 15 and f[12] == f"NM:i:{ep.score[i]}" and f[14] == "cg:Z:" + dentist_amd.format_cigar(o, extended=True)
        assert f[13] == f"tp:i:{int(trace[la['toff']:la['toff'] + la['tlen']:2].sum())}" and (int(f[7]), int(f[8])) == (la["abpos"], la["aepos"])
