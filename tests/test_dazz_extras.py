"""Track extras of a mask (dh_dazz_read_extra / dh_dazz_write_extra; source/dentist/dazzler.d:5173-5379): the reference's own
round-trip vector, the bytes behind the pointers of the .anno, the refusals, and every reader of the mask itself before and
after extras were appended.  Host only."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dentist_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK = "test-mask"
# the DB of the reference's unit test (dazzler.d:5359-5362)
READS = ">Sim/1/0_14 RQ=0.975\nggcccacccaggcagccc\n>Sim/3/0_11 RQ=0.975\ngagtgcgtgcagtgg\n"
NOT_FOUND = -7   # DH_ENOTFOUND


@pytest.fixture()
def db(tmp_path):
    path = str(tmp_path / "test.db")
    dentist_amd.dazz_create_db(path, READS)
    dentist_amd.dazz_split(path, cutoff=0)
    dentist_amd.dazz_write_mask(path, MASK, np.zeros(3, np.int64), np.zeros(2, np.int32))   # an empty mask
    return path


def anno(path, mask=MASK):
    return os.path.join(os.path.dirname(path), f".test.{mask}.anno")


def test_reference_unit_vector(db):
    ints, floats = np.arange(1024, dtype=np.int64), np.arange(1024, dtype=np.float64)
    dentist_amd.write_mask_extra(db, MASK, "int-extra", ints, accum="sum")
    dentist_amd.write_mask_extra(db, MASK, "float-extra", floats)
    got = dentist_amd.read_mask_extra(db, MASK, "int-extra", np.int64)
    assert got.data.dtype == np.int64 and np.array_equal(got.data, ints) and got.accum == "sum"
    got = dentist_amd.read_mask_extra(db, MASK, "float-extra", np.float64)    # the second, found by skipping the first
    assert got.data.dtype == np.float64 and np.array_equal(got.data, floats) and got.accum == "exact"
    # without a type asked for, the stored one comes back
    assert dentist_amd.read_mask_extra(db, MASK, "int-extra").data.dtype == np.int64
    assert dentist_amd.read_mask_extra(db, MASK, "float-extra").data.dtype == np.float64


def test_exact_bytes_behind_the_pointers(db):
    head = open(anno(db), "rb").read()
    assert head == struct.pack("<iiqqq", 2, 0, 0, 0, 0)
    dentist_amd.write_mask_extra(db, MASK, "abc", [5, -1, 1 << 40], accum="sum")
    assert open(anno(db), "rb").read() == head + struct.pack("<iiii", 0, 3, 1, 3) + b"abc" + struct.pack("<qqq", 5, -1, 1 << 40)
    dentist_amd.write_mask_extra(db, MASK, "d", [0.5])
    assert open(anno(db), "rb").read()[len(head) + 16 + 3 + 24:] == struct.pack("<iiii", 1, 1, 0, 1) + b"d" + struct.pack("<d", 0.5)


def test_wrong_vtype_and_absent_name(db):
    dentist_amd.write_mask_extra(db, MASK, "ints", [1, 2, 3])
    with pytest.raises(dentist_amd.DhError, match=r"current extra index 0\): vtype does not match: expected 1 but got 0") as ei:
        dentist_amd.read_mask_extra(db, MASK, "ints", np.float64)
    assert ei.value.code == -1 and anno(db) in str(ei.value)
    assert dentist_amd.read_mask_extra(db, MASK, "absent") is None
    assert dentist_amd.read_mask_extra(db, MASK, "int") is None        # a prefix of a name is another name
    # the status itself, through the C ABI
    import ctypes
    vtype = ctypes.c_int32(0)
    L = dentist_amd.lib()
    assert L.dh_dazz_read_extra(db.encode(), MASK.encode(), b"absent", ctypes.byref(vtype), None, None, 0) == NOT_FOUND
    assert L.dh_dazz_read_extra(db.encode(), MASK.encode(), b"ints", ctypes.byref(vtype), None, None, 0) == 3   # sized without an array
    # a mask that does not exist is an error, not an absent extra
    with pytest.raises(dentist_amd.DhError, match="mask track not found"):
        dentist_amd.read_mask_extra(db, "no-such-mask", "ints")
    with pytest.raises(dentist_amd.DhError, match="mask track not found"):
        dentist_amd.write_mask_extra(db, "no-such-mask", "ints", [1])


def test_appending_never_looks_for_an_existing_name(db):
    dentist_amd.write_mask_extra(db, MASK, "x", [1, 2])
    dentist_amd.write_mask_extra(db, MASK, "x", [3])
    assert dentist_amd.read_mask_extra(db, MASK, "x").data.tolist() == [1, 2]     # the first of that name
    assert os.path.getsize(anno(db)) == 32 + (16 + 1 + 16) + (16 + 1 + 8)


def test_a_file_cut_anywhere_names_the_index_of_the_extra(db):
    dentist_amd.write_mask_extra(db, MASK, "first", [1, 2])
    dentist_amd.write_mask_extra(db, MASK, "second", [7.5, 8.5, 9.5])
    whole = open(anno(db), "rb").read()
    first_end = 32 + 16 + 5 + 16
    assert len(whole) == first_end + 16 + 6 + 24
    cases = [(32 + 7, "first", 0, "header data"), (32 + 16 + 2, "first", 0, "name"), (32 + 16 + 5 + 9, "first", 0, "data"),
             (32 + 16 + 5 + 9, "second", 0, "data"),                                  # skipping runs into the cut, too
             (first_end + 15, "second", 1, "header data"), (first_end + 16 + 5, "second", 1, "name"),
             (first_end + 16 + 6 + 23, "second", 1, "data"), (first_end + 16 + 6, "second", 1, "data")]
    for cut, name, index, what in cases:
        open(anno(db), "wb").write(whole[:cut])
        with pytest.raises(dentist_amd.DhError) as ei:
            dentist_amd.read_mask_extra(db, MASK, name)
        msg = str(ei.value)
        assert ei.value.code == -1 and f"(current extra index {index}): unexpected end of file while reading {what}" in msg, (cut, msg)
        assert anno(db) in msg
    # cut between the extras: the first is whole, the second is absent
    open(anno(db), "wb").write(whole[:first_end])
    assert dentist_amd.read_mask_extra(db, MASK, "first").data.tolist() == [1, 2]
    assert dentist_amd.read_mask_extra(db, MASK, "second") is None
    # cut inside the pointers of the mask
    open(anno(db), "wb").write(whole[:20])
    with pytest.raises(dentist_amd.DhError, match="mask pointers"):
        dentist_amd.read_mask_extra(db, MASK, "first")


def test_readers_of_the_mask_do_not_see_extras_and_write_mask_drops_them(tmp_path):
    path = str(tmp_path / "ref.dam")
    rng = np.random.default_rng(11)
    seqs = ["".join("acgt"[x] for x in rng.integers(0, 4, n)) for n in (300, 200, 250, 100)]
    dentist_amd.dazz_create_dam(path, "".join(f">s{i}\n{s}\n" for i, s in enumerate(seqs)))
    dentist_amd.dazz_split(path, cutoff=20)
    ptr, iv = np.asarray([0, 2, 2, 3, 4], np.int64), np.asarray([5, 20, 40, 90, 0, 250, 7, 8], np.int32)
    dentist_amd.dazz_write_mask(path, "m", ptr, iv)
    dz = dentist_amd.DazzDb(path)
    before = dz.read_mask("m")
    plain = open(tmp_path / ".ref.m.anno", "rb").read()
    dentist_amd.write_mask_extra(path, "m", "contigs", np.arange(8))
    dentist_amd.write_mask_extra(path, "m", "weights", np.arange(4) / 4, accum="sum")
    after = dz.read_mask("m")
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and np.array_equal(after[1], iv)
    # ... nor does a block view of the DB, which takes a slice of the pointers
    dentist_amd.dazz_split(path, cutoff=20, size_mb=1)
    assert np.array_equal(dentist_amd.DazzDb(str(tmp_path / "ref.1.dam")).read_mask("m")[1], iv)
    # rewriting the mask truncates the .anno: the extras are gone (the reference's writeMask does the same)
    dentist_amd.dazz_write_mask(path, "m", ptr, iv)
    assert open(tmp_path / ".ref.m.anno", "rb").read() == plain
    assert dentist_amd.read_mask_extra(path, "m", "contigs") is None


def test_catrack_reads_block_tracks_with_extras(tmp_path):
    """Catrack takes the intervals of the block tracks as before; their extras are not carried over (out of scope)."""
    path = str(tmp_path / "ref.dam")
    rng = np.random.default_rng(12)
    dentist_amd.dazz_create_dam(path, "".join(f">s{i}\n" + "".join("acgt"[x] for x in rng.integers(0, 4, 200)) + "\n" for i in range(3)))
    dentist_amd.dazz_split(path, cutoff=20)   # one block
    ptr, iv = np.asarray([0, 1, 1, 2], np.int64), np.asarray([5, 20, 0, 150], np.int32)
    dentist_amd.dazz_write_mask(path, "tmp", ptr, iv)
    for ext in ("anno", "data"):
        os.rename(tmp_path / f".ref.tmp.{ext}", tmp_path / f".ref.1.tan.{ext}")
    dentist_amd.write_mask_extra(path, "1.tan", "x", [1, 2, 3])      # the block's track, named as merge-masks names it
    assert dentist_amd.read_mask_extra(path, "1.tan", "x").data.tolist() == [1, 2, 3]
    r = subprocess.run([os.path.join(ROOT, "tools", "Catrack"), "-v", path, "tan"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    got = dentist_amd.DazzDb(path).read_mask("tan")
    assert np.array_equal(got[0], ptr) and np.array_equal(got[1], iv)
    assert dentist_amd.read_mask_extra(path, "tan", "x") is None
