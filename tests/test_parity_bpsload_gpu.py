"""dh_dazz_load_reads (the sparse packed read loader, kernel k_bps_unpack) against dh_dazz_open: the bases of the loaded DB
equal the slices of the host view, for a .db, a .dam and a trimmed copy with two blocks, with the padding bits of the .bps
set, for every selection and every chunking; its refusals by their message."""
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import DhError, load_reads, load_stats

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(1, 10)) + [15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 257, 1000]
CUTOFF = 8
# DH_LOAD_CHUNK_MB: the default, a value that holds one read (less than a byte), a value that splits a run of reads in its middle
CHUNKS = {"default": None, "one read": "0.0000001", "mid-run": "0.0001"}


def tool(name, *args, stdin=None, cwd=None):
    r = subprocess.run([os.path.join(ROOT, "tools", name)] + list(args), input=stdin, capture_output=True, text=True, cwd=cwd)
    assert r.returncode == 0, r.stderr


def set_padding_bits(db_path, lengths):
    """ones behind the last base of every read whose length is no multiple of four"""
    d, base = os.path.split(db_path)
    bps = os.path.join(d, "." + os.path.splitext(base)[0] + ".bps")
    raw = bytearray(open(bps, "rb").read())
    at = 0
    for l in lengths:
        at += (l + 3) // 4
        if l % 4:
            raw[at - 1] |= (1 << (8 - 2 * (l % 4))) - 1
    assert at == len(raw)
    open(bps, "wb").write(bytes(raw))


@pytest.fixture(scope="module")
def dbs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bpsload")
    rng = np.random.default_rng(11)
    order = [int(x) for x in rng.permutation(LENGTHS)]
    seqs = ["".join("acgt"[c] for c in rng.integers(0, 4, l)) for l in order]
    reads = "".join(">sim/%d/0_%d RQ=0.850\n%s\n" % (i + 1, len(s), s) for i, s in enumerate(seqs))
    contigs = "".join(">scaf%d\n%s\n" % (i, s) for i, s in enumerate(seqs))
    paths = {"db": str(d / "reads.db"), "dam": str(d / "ref.dam"), "trimmed": str(d / "trimmed.db")}
    tool("fasta2DB", paths["db"], "-i", stdin=reads)
    tool("fasta2DAM", paths["dam"], "-i", stdin=contigs)
    tool("fasta2DB", paths["trimmed"], "-i", stdin=reads)
    tool("DBsplit", "-x%d" % CUTOFF, paths["trimmed"])
    # two blocks: the table DBsplit writes for a block size between the halves (its -s counts whole megabases)
    stub = open(paths["trimmed"]).read().splitlines(keepends=True)
    at = next(i for i, l in enumerate(stub) if l.startswith("blocks ="))
    kept = [i for i, l in enumerate(order) if l >= CUTOFF]
    mid = kept[len(kept) // 2]
    stub[at] = "blocks = %9d\n" % 2
    stub[at + 2:] = [" %9d %9d\n" % (0, 0), " %9d %9d\n" % (mid, len(kept) // 2), " %9d %9d\n" % (len(order), len(kept))]
    open(paths["trimmed"], "w").writelines(stub)
    for p in paths.values():
        set_padding_bits(p, order)
    paths["trimmed.2"] = str(d / "trimmed.2")
    views = {k: dentist_amd.DazzDb(p) for k, p in paths.items()}
    assert views["db"].n == views["dam"].n == len(LENGTHS) and views["trimmed"].n == len(kept) < len(LENGTHS)
    assert views["trimmed.2"].n == len(kept) - len(kept) // 2 and views["trimmed.2"].first_id == len(kept) // 2
    return paths, views, order


def selections(n):
    yield "all", list(range(n))
    yield "first", [0]
    yield "last", [n - 1]
    yield "every other", list(range(0, n, 2))
    yield "two runs", [1, 2, n - 3, n - 2]


def expected(view, ids):
    return np.concatenate([view.seq(i) for i in ids]) if len(ids) else np.zeros(0, np.uint8)


@pytest.mark.parametrize("chunk", list(CHUNKS))
@pytest.mark.parametrize("which", ["db", "dam", "trimmed", "trimmed.2"])
def test_loaded_bases_equal_the_host_view(gpu_ctx, dbs, monkeypatch, which, chunk):
    paths, views, order = dbs
    view = views[which]
    if CHUNKS[chunk] is None:
        monkeypatch.delenv("DH_LOAD_CHUNK_MB", raising=False)
    else:
        monkeypatch.setenv("DH_LOAD_CHUNK_MB", CHUNKS[chunk])
    for name, ids in selections(view.n):
        db = load_reads(gpu_ctx, paths[which], ids)
        want = expected(view, ids)
        assert np.array_equal(db.off, np.concatenate([[0], np.cumsum([len(view.seq(i)) for i in ids])])), name
        got = db.bases()
        assert got.dtype == np.uint8 and np.array_equal(got, want), (which, chunk, name)
        st = load_stats(gpu_ctx)
        packed = sum((len(view.seq(i)) + 3) // 4 for i in ids)
        assert st["packed_bytes"] == packed and st["bases"] == len(want), name   # not a byte of the .bps beyond the reads
        if chunk == "default":
            assert st["chunks"] == 1
        elif chunk == "one read":
            assert st["chunks"] == len(ids)
        elif name == "all":
            assert 1 < st["chunks"] <= len(ids) and (which not in ("db", "dam") or st["chunks"] < len(ids))
        if chunk == "default" and which in ("db", "dam"):
            assert st["runs"] == {"all": 1, "first": 1, "last": 1, "every other": len(ids), "two runs": 2}[name], name
        # a slice of the loaded DB, from the device
        if len(ids) > 2:
            assert np.array_equal(db.bases(1, len(ids) - 2), expected(view, ids[1:-1]))
        db.close()


def test_trimmed_ids_differ_from_untrimmed_ones(gpu_ctx, dbs):
    paths, views, order = dbs
    first_kept = next(i for i, l in enumerate(order) if l >= CUTOFF)
    db = load_reads(gpu_ctx, paths["trimmed"], [0])
    assert len(db.bases()) == order[first_kept] and np.array_equal(db.bases(), views["db"].seq(first_kept))
    db.close()


def test_refusals(gpu_ctx, dbs):
    paths, views, order = dbs
    n = views["db"].n
    for ids, what in (([3, 2], "unsorted"), ([0, 5, 4, 9], "unsorted"), ([2, 2], "duplicate"), ([0, n], "outside"), ([-1, 0], "outside"), ([], "at least one")):
        with pytest.raises(DhError) as e:
            load_reads(gpu_ctx, paths["db"], ids)
        assert "dh_dazz_load_reads" in str(e.value) and what in str(e.value), (ids, str(e.value))
    with pytest.raises(DhError) as e:   # ids are those of the view: the block has fewer reads than the DB
        load_reads(gpu_ctx, paths["trimmed.2"], [views["trimmed.2"].n])
    assert "outside" in str(e.value)
    with pytest.raises(DhError):
        load_reads(gpu_ctx, os.path.join(os.path.dirname(paths["db"]), "none.db"), [0])
