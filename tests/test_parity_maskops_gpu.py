"""Context.combine_masks and Context.tandem_mask (dh_mask_combine, dh_la_tandem_mask: two keys per interval, a device-wide radix
sort, a device-wide sweep, gap and size filters by flag, scan and compaction) against the contract (tests/maskops_ref.py) on
every case of tests/maskops_cases.py: at the default knobs, at the smallest sort tile and with one launch group per contig; the
counters; run-to-run identity; the union against Context.repeat_mask's own; the tandem rule against the host tool TANmask; the
refusals.  Every comparison is equality."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib

import maskops_cases as mc
import maskops_ref as mr
import repeat_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = {"default": {}, "min_tile": {"DH_MASKOPS_TILE_KEYS": str(mc.TILE_MIN)}, "many_groups": {"DH_MASKOPS_CHUNK_MB": "0.000001"}}


def call(ctx, c):
    return ctx.combine_masks(c["masks"], c["contig_off"], **mc.args_of(c))


def set_knobs(monkeypatch, knobs):
    for k in ("DH_MASKOPS_TILE_KEYS", "DH_MASKOPS_CHUNK_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("name", list(mc.ALL))
def test_every_case_equals_the_contract(gpu_ctx, monkeypatch, name, knobs):
    set_knobs(monkeypatch, KNOBS[knobs])
    c = mc.ALL[name]
    got = call(gpu_ctx, c)
    assert mc.triples(got.ptr, got.iv) == mc.expected_of(name), (name, knobs)
    assert got.events == 2 * mr.count_nonempty(c["masks"], c["subtract"])
    assert got.groups == (mc.groups_of(c) if knobs == "many_groups" else min(1, mc.groups_of(c)))


def test_the_digits_in_use_decide_the_passes(gpu_ctx, monkeypatch):
    set_knobs(monkeypatch, {})
    small = call(gpu_ctx, mc.ALL["one_interval"]).sort_passes          # 1 contig of 10 bases: 4 + 2 bits
    assert small == 1
    assert call(gpu_ctx, mc.ALL["tile"]).sort_passes == 2              # 5000 bases: 13 + 2 bits
    assert call(gpu_ctx, mc.ALL["longest_contig"]).sort_passes == 5    # 1 + 31 + 2 bits
    many = call(gpu_ctx, mc.ALL["many_contigs"]).sort_passes           # 17 + 6 + 2 bits: the contig takes part in three digits
    assert many == 4 and many > small
    assert call(gpu_ctx, mc.ALL["three_masks_min_2"]).sort_passes == 2   # the masks on their own first (2 + 4 + 2 bits), then 4 + 2 bits
    assert call(gpu_ctx, mc.ALL["nothing"]).sort_passes == 0


@pytest.mark.parametrize("name", ["random_or", "random_min_2_filtered", "all_keys_equal", "many_contigs"])
def test_two_runs_are_byte_identical(gpu_ctx, monkeypatch, name):
    set_knobs(monkeypatch, {})
    a, b = call(gpu_ctx, mc.ALL[name]), call(gpu_ctx, mc.ALL[name])
    assert a.ptr.tobytes() == b.ptr.tobytes() and a.iv.tobytes() == b.iv.tobytes()


@pytest.mark.parametrize("name", ["reference_vector", "random_12"])
def test_union_of_all_and_improper_is_the_repeat_mask(gpu_ctx, monkeypatch, name):
    """mask = all | improper (maskRepetitiveRegions.d): the union of this call against the one pinned to oracle/maskcov.py"""
    set_knobs(monkeypatch, {})
    c = dict(rc.ALL[name])
    if c["improper"] is None:
        c["improper"] = (1, 2)
    rm = gpu_ctx.repeat_mask(c["las"], c["contig_off"], c["read_off"], c["lower"], c["upper"], c["improper"], c["allowance"])
    got = gpu_ctx.combine_masks([rm.all, rm.improper], c["contig_off"])
    assert len(rm.mask[1]) > 0 and got.ptr.tobytes() == rm.mask[0].tobytes() and got.iv.tobytes() == rm.mask[1].tobytes()


@pytest.mark.parametrize("first", [0, 5])
def test_tandem_rule(gpu_ctx, monkeypatch, first):
    set_knobs(monkeypatch, {})
    las, read_off, first, min_len = mc.tandem_case(first)
    got = gpu_ctx.tandem_mask(las, read_off, first, min_len)
    assert mc.triples(got.ptr, got.iv) == mr.tandem(las, read_off, first, min_len) == [(0, 100, 1300), (2, 50, 1100), (3, 0, 2000)]
    assert got.events == 2 * 5 and got.groups == 1
    none = gpu_ctx.tandem_mask(las[1:3], read_off, first, min_len)
    assert len(none.iv) == 0 and not none.ptr.any() and none.groups == 0


def test_tandem_mask_equals_the_host_tool(gpu_ctx, monkeypatch, tmp_path):
    """datander's .las of a DB block: Context.tandem_mask == the track tools/TANmask (host only) writes"""
    from test_tools_gpu import fasta_dam, tandem_reads
    set_knobs(monkeypatch, {})
    db, _ = tandem_reads()
    ref = str(tmp_path / "asm.dam")
    dentist_amd.dazz_create_dam(ref, fasta_dam(db))
    dentist_amd.dazz_split(ref, cutoff=20)
    for tool, args in (("datander", ["-T1", "-s126", "-l500", "-e0.7", "asm.1"]), ("TANmask", ["-ntan", ref, "TAN.asm.1.las"]),
                       ("Catrack", [ref, "tan"])):     # (Catrack: the block tracks into the DB's, which read_mask reads)
        r = subprocess.run([os.path.join(ROOT, "tools", tool), *args], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
    las, _, _ = dentist_amd.las_read(str(tmp_path / "TAN.asm.1.las"))
    block = dentist_amd.DazzDb(str(tmp_path / "asm.1.dam"))
    ptr, iv = block.read_mask("tan")
    got = gpu_ctx.tandem_mask(las, block.off, block.first_id, 500)
    assert len(iv) > 0 and got.ptr.tobytes() == np.asarray(ptr, dtype=np.int64).tobytes()
    assert got.iv.reshape(-1).tobytes() == np.asarray(iv, dtype=np.int32).reshape(-1).tobytes()


@pytest.mark.parametrize("name,case,words", mc.refusals(), ids=[r[0] for r in mc.refusals()])
def test_refusals_name_the_lowest_index(gpu_ctx, name, case, words):
    with pytest.raises(dentist_amd.DhError) as e:
        call(gpu_ctx, case)
    assert words in str(e.value) and "dh_mask_combine" in str(e.value)


def test_tandem_refusals(gpu_ctx):
    las, read_off, first, min_len = mc.tandem_case(5)
    for change, words in (({"aread": 9, "bread": 9}, "record 3: aread outside the reads"), ({"aread": 4, "bread": 4}, "record 3: aread outside the reads"),
                          ({"aepos": 1601}, "record 3: end behind the read's end")):
        bad = las.copy()
        for k, v in change.items():
            bad[3][k] = v
        with pytest.raises(dentist_amd.DhError) as e:
            gpu_ctx.tandem_mask(bad, read_off, first, min_len)
        assert words in str(e.value) and "dh_la_tandem_mask" in str(e.value)
    bad = las.copy()
    bad[1]["aread"] = 99       # not counted (aread != bread): not looked at
    assert len(gpu_ctx.tandem_mask(bad, read_off, first, min_len).iv) == 3


def test_bad_arguments(gpu_ctx):
    L = _lib.lib()
    c = mc.ALL["three_masks_min_2"]
    ptrs = (ctypes.c_void_p * 3)(*[m[0].ctypes.data for m in c["masks"]])
    ivs = (ctypes.c_void_p * 3)(*[m[1].ctypes.data for m in c["masks"]])
    o = _lib.MaskOpts(0, 0, 0, 0)
    L.dh_default_mask_opts(ctypes.byref(o))
    assert (o.min_count, o.min_gap, o.min_interval) == (1, 0, 0)
    h = ctypes.c_void_p()
    co = c["contig_off"]
    args = [gpu_ctx._h, ptrs, ivs, 3, None, None, co.ctypes.data, 1, ctypes.byref(o), ctypes.byref(h)]
    assert L.dh_mask_combine(*args) == 0 and L.dh_mask_set_count(h) == 1
    L.dh_mask_set_destroy(h)
    for k, v in ((0, None), (1, None), (2, None), (6, None), (8, None), (9, None), (3, 0), (3, -1), (7, -1), (4, co.ctypes.data)):
        bad = list(args)
        bad[k] = v
        assert L.dh_mask_combine(*bad) == -1 and "bad argument" in L.dh_last_error().decode(), k
    ptrs[1] = None       # a NULL mask
    assert L.dh_mask_combine(*args) == -1 and "bad argument" in L.dh_last_error().decode()
    las, ro, first, min_len = mc.tandem_case()
    targs = [gpu_ctx._h, las.ctypes.data, len(las), ro.ctypes.data, len(ro) - 1, first, min_len, ctypes.byref(h)]
    for k, v in ((0, None), (1, None), (3, None), (7, None), (2, -1), (4, -1)):
        bad = list(targs)
        bad[k] = v
        assert L.dh_la_tandem_mask(*bad) == -1 and "bad argument" in L.dh_last_error().decode(), k
