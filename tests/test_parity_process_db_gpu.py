"""dh_process_pileups_db, the file route of the process stage (pile-ups.db -> dh_pileups_from_db -> the reads the pile-ups
name through dh_dazz_load_reads -> dh_process_pileups_masked), against process_pileups on the whole reads DB with the same
pile-ups: records, consensus bases and read ids are equal, bit for bit -- for the whole file, for a first / count selection,
with a repeat mask and with the smallest DH_LOAD_CHUNK_MB."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import Pileups, sim
from test_tools_gpu import fasta_db

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(gpu_ctx, tmp_path_factory):
    """three contigs, two gaps, the reads mapped with the library; every pile-up of the scaffold graph written to pile-ups.db
    and the reads to a DAZZ_DB"""
    d = tmp_path_factory.mktemp("process_db")
    w = sim.Workload(120_000, 2, 600, 4000, seed=5, spacing=10000, gap_max=600)
    po = dentist_amd.default_process_opts(rounds=2, algo=1, max_reads=0)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    las, trace = gpu_ctx.align_db(A, B, dentist_amd.default_align_opts(algo=1, width=64), select_best=True)
    las, _, _ = dentist_amd.collect_filter(las, w.contigs.off, w.reads.off, po, inplace=True)
    gaps_in = np.stack([np.arange(w.contigs.n - 1), np.arange(1, w.contigs.n)], axis=1)
    piles, _ = dentist_amd.scaffold_all_pileups(las, w.contigs.off, w.reads.off, gaps_in, only="both", min_spanning_reads=po.min_reads)
    assert len(piles) >= 2
    sizes = [len(piles.get(i)[1]) for i in range(len(piles))]
    assert any(piles.get_join(i)[2] >= 0 and n >= 6 for i, n in enumerate(sizes)), sizes   # gap pile-ups of several reads
    pdb, rdb = str(d / "pile-ups.db"), str(d / "reads.db")
    piles.write_db(pdb, las, trace, w.contigs.off, w.reads.off, 100)
    dentist_amd.dazz_create_db(rdb, fasta_db(w.reads))
    return dict(w=w, po=po, A=A, B=B, las=las, trace=trace, piles=piles, pdb=pdb, rdb=rdb)


def subset(piles, first, count):
    idx = range(first, first + count)
    return Pileups.from_joins([piles.get_join(i) for i in idx], [piles.get(i)[1] for i in idx])


def same(got, want):
    (rec, bases, (ids, off)), (rec2, bases2, (ids2, off2)) = got, want
    assert len(rec) == len(rec2)
    for f in rec.dtype.names:
        assert np.array_equal(rec[f], rec2[f]), f
    assert rec.tobytes() == rec2.tobytes()
    assert np.array_equal(bases, bases2)
    assert np.array_equal(off, off2) and np.array_equal(ids, ids2)


def test_the_whole_file(gpu_ctx, world):
    x = world
    want = dentist_amd.process_pileups(gpu_ctx, x["A"], x["B"], x["las"], x["trace"], x["piles"], x["po"], read_ids=True)
    assert (want[0]["status"] == 0).sum() >= 2   # both gaps are closed
    got = gpu_ctx.process_pileups_db(x["A"], x["rdb"], x["pdb"], x["po"], read_ids=True)
    same(got, want)
    assert (got[0]["ref_read_id"][got[0]["status"] == 0] >= 0).all() and got[2][0].max() < x["w"].reads.n
    st = dentist_amd.load_stats(gpu_ctx)
    used = np.unique(np.concatenate([x["piles"].get(i)[1][:, 0] for i in range(len(x["piles"]))]))
    assert st["bases"] == sum(x["w"].reads.length(int(r)) for r in used) < x["w"].reads.off[-1] // 4   # a fraction of the reads DB


def test_a_selection_in_file_order(gpu_ctx, world):
    x = world
    n = len(x["piles"])
    for first, count in ((1, n - 1), (0, 1), (n - 1, -1)):
        k = n - first if count < 0 else count
        want = dentist_amd.process_pileups(gpu_ctx, x["A"], x["B"], x["las"], x["trace"], subset(x["piles"], first, k), x["po"], read_ids=True)
        same(gpu_ctx.process_pileups_db(x["A"], x["rdb"], x["pdb"], x["po"], first=first, count=count, read_ids=True), want)
    rec, bases, (ids, off) = gpu_ctx.process_pileups_db(x["A"], x["rdb"], x["pdb"], x["po"], first=n, count=-1, read_ids=True)
    assert len(rec) == 0 and len(bases) == 0 and len(ids) == 0
    with pytest.raises(dentist_amd.DhError) as e:
        gpu_ctx.process_pileups_db(x["A"], x["rdb"], x["pdb"], x["po"], first=1, count=n)
    assert "outside the file's %d pile-ups" % n in str(e.value)


def test_with_a_repeat_mask(gpu_ctx, world):
    """the contigs' ends masked where the reads' common trace points would fall: the cropper moves, on both routes alike"""
    x = world
    w = x["w"]
    iv, ptr = [], [0]
    for c in range(w.contigs.n):
        L = w.contigs.length(c)
        iv += [300, 1500, L - 1500, L - 300]
        ptr.append(len(iv) // 2)
    mask = (np.array(ptr, np.int64), np.array(iv, np.int32))
    want = dentist_amd.process_pileups(gpu_ctx, x["A"], x["B"], x["las"], x["trace"], x["piles"], x["po"], read_ids=True, repeat_mask=mask)
    plain = dentist_amd.process_pileups(gpu_ctx, x["A"], x["B"], x["las"], x["trace"], x["piles"], x["po"], read_ids=True)
    assert want[0].tobytes() != plain[0].tobytes()   # the mask bites
    same(gpu_ctx.process_pileups_db(x["A"], x["rdb"], x["pdb"], x["po"], read_ids=True, repeat_mask=mask), want)


def test_with_one_read_per_chunk(gpu_ctx, world, monkeypatch):
    x = world
    want = dentist_amd.process_pileups(gpu_ctx, x["A"], x["B"], x["las"], x["trace"], x["piles"], x["po"], read_ids=True)
    monkeypatch.setenv("DH_LOAD_CHUNK_MB", "0.0000001")
    same(gpu_ctx.process_pileups_db(x["A"], x["rdb"], x["pdb"], x["po"], read_ids=True), want)
    assert dentist_amd.load_stats(gpu_ctx)["chunks"] == dentist_amd.load_stats(gpu_ctx)["runs"] > 10


def test_a_read_length_that_contradicts_the_reads_db(gpu_ctx, world, tmp_path):
    import test_pileups_from_db as tp
    x = world
    piles = tp.split_piles(x["pdb"])
    piles[0][0][0][0]["contig_b_len"] += 1
    if len(piles[0][0]) > 1:
        piles[0][0][1][0]["contig_b_len"] += 1
    bad = str(tmp_path / "bad.db")
    tp.write_piles(bad, piles)
    with pytest.raises(dentist_amd.DhError) as e:
        gpu_ctx.process_pileups_db(x["A"], x["rdb"], bad, x["po"])
    assert "dh_process_pileups_db" in str(e.value) and ("the pile-ups say" in str(e.value) or "has two lengths" in str(e.value))
