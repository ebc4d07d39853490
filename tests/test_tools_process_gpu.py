"""The workflow's chain on the project's own executables: damapper -> collect -> process -> merge-insertions -> output.
tools/process writes the insertions.db the library route (Context.process_pileups_db + write_db) writes for the same
pile-ups.db, byte for byte; two batches give the bytes of one; --only=extending on a file of gap pile-ups writes an empty
insertions.db; process-pile-ups is the same tool."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from test_tools_gpu import fasta_db
import test_pileups_from_db as tp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tool(d, name, *args):
    r = subprocess.run([os.path.join(ROOT, "tools", name)] + list(args), cwd=d, capture_output=True, text=True)
    assert r.returncode == 0, (name, args, r.stderr)
    return r


@pytest.fixture(scope="module")
def chain(gpu_ctx, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("process_tools"))
    w = sim.Workload(120_000, 2, 600, 4000, seed=5, spacing=10000, gap_max=600)
    # one scaffold with its gaps as runs of n, as the workflow's reference is
    text = ">scaf\n"
    for c in range(w.contigs.n):
        text += sim.decode(w.contigs.seq(c)) + ("n" * 500 if c + 1 < w.contigs.n else "") + "\n"
    dentist_amd.dazz_create_dam(os.path.join(d, "ref.dam"), text)
    dentist_amd.dazz_split(os.path.join(d, "ref.dam"), cutoff=20)
    dentist_amd.dazz_create_db(os.path.join(d, "reads.db"), fasta_db(w.reads))
    dentist_amd.dazz_split(os.path.join(d, "reads.db"), cutoff=20)
    dentist_amd.dazz_write_mask(os.path.join(d, "ref.dam"), "rep", np.zeros(w.contigs.n + 1, np.int64), np.zeros(2, np.int32))
    tool(d, "damapper", "-T1", "-e0.7", "ref", "reads.1")
    tool(d, "collect", "--mask=rep", "ref.dam", "reads.db", "ref.reads.1.las", "pile-ups.db")
    n = len(dentist_amd.pileupdb_read(os.path.join(d, "pile-ups.db"))["pile_counts"])
    assert n >= 2
    r = tool(d, "process", "--mask=rep", "--batch=0..$", "ref.dam", "reads.db", "pile-ups.db", "insertions.db")
    return dict(d=d, w=w, n=n, stderr=r.stderr)


def data(x, name):
    return open(os.path.join(x["d"], name), "rb").read()


def test_process_writes_what_the_library_route_writes(gpu_ctx, chain):
    x = chain
    d = x["d"]
    ref = dentist_amd.DazzDb(os.path.join(d, "ref.dam"))
    A = gpu_ctx.db(ref)
    po = dentist_amd.default_process_opts(max_reads=0)
    rec, bases = gpu_ctx.process_pileups_db(A, os.path.join(d, "reads.db"), os.path.join(d, "pile-ups.db"), po,
                                            insertions_db=(os.path.join(d, "library.db"), ref.off, po.tspace_pile))
    assert (rec["status"] == 0).sum() >= 2
    assert data(x, "insertions.db") == data(x, "library.db")
    assert len(dentist_amd.insertiondb_read(os.path.join(d, "insertions.db"))["insertions"]) == (rec["status"] == 0).sum()
    # one line per pile-up that was not closed, with its index in the file
    assert x["stderr"].count("not closed") == (rec["status"] != 0).sum()
    # the rest of the chain: merge-insertions and output on either file give the same assembly
    tool(d, "merge-insertions", "merged.db", "insertions.db")
    assert data(x, "merged.db") == data(x, "insertions.db")
    tool(d, "output", "ref.dam", "reads.db", "merged.db", "tools.fasta")
    tool(d, "output", "ref.dam", "reads.db", "library.db", "library.fasta")
    assert data(x, "tools.fasta") == data(x, "library.fasta") and data(x, "tools.fasta").count(b">") >= 1
    assert b"n" * 500 not in data(x, "tools.fasta")   # the gaps are closed


def test_two_batches_give_the_bytes_of_one(chain):
    x = chain
    d = x["d"]
    tool(d, "process", "--mask=rep", "--batch=0..1", "--batch=1..$", "ref.dam", "reads.db", "pile-ups.db", "two.db")
    assert data(x, "two.db") == data(x, "insertions.db")
    # ... and as two jobs merged by merge-insertions, up to the running ids of the overlaps, which count inside a file
    tool(d, "process", "--mask=rep", "--batch=0..1", "ref.dam", "reads.db", "pile-ups.db", "b0.db")
    tool(d, "process", "--mask=rep", "--batch=1..$", "ref.dam", "reads.db", "pile-ups.db", "b1.db")
    tool(d, "merge-insertions", "b.db", "b0.db", "b1.db")
    one, two = (dentist_amd.insertiondb_read(os.path.join(d, f)) for f in ("insertions.db", "b.db"))
    for k in ("insertions", "bases", "read_ids", "las", "trace"):
        assert np.array_equal(one[k], two[k]), k
    for f in one["seeded"].dtype.names:
        assert f == "id" or np.array_equal(one["seeded"][f], two["seeded"][f]), f


def test_both_names_give_the_same_bytes(chain):
    x = chain
    tool(x["d"], "process-pile-ups", "--mask=rep", "ref.dam", "reads.db", "pile-ups.db", "other-name.db")
    assert data(x, "other-name.db") == data(x, "insertions.db")


def test_only_extending_on_gap_pile_ups_writes_an_empty_file(chain):
    x = chain
    d = x["d"]
    ref = dentist_amd.DazzDb(os.path.join(d, "ref.dam"))
    piles, _, _, _, file_index = dentist_amd.pileups_from_db(os.path.join(d, "pile-ups.db"), 0, -1, ref.off)
    gaps = sorted(int(file_index[i]) for i in range(len(piles)) if piles.get_join(i)[2] >= 0)
    assert gaps
    split = tp.split_piles(os.path.join(d, "pile-ups.db"))
    tp.write_piles(os.path.join(d, "gaps.db"), [split[g] for g in gaps])
    r = tool(d, "process", "--mask=rep", "--only=extending", "ref.dam", "reads.db", "gaps.db", "none.db")
    assert len(dentist_amd.insertiondb_read(os.path.join(d, "none.db"))["insertions"]) == 0
    assert r.stderr.count("skipped by --only=extending") == len(gaps)
