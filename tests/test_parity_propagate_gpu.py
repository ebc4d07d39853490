"""Context.propagate_mask (dh_la_propagate_mask / dh_la_set_propagate_mask: the mask propagation with the union taken on a
bitmap of the destination bases) against the restatement of the contract (tests/propagate_ref.py) on the shapes of
tests/propagate_cases.py, and against the host function on a real mapping.  Every comparison is equality.  A record of one
tile holds tspace bases at most, so the shape (1 tile, 200 intervals) takes the tspace intervals that fit."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim

import propagate_cases as pc
import propagate_ref as pr

pytestmark = pytest.mark.gpu


def device(ctx, case):
    return ctx.propagate_mask(case["las"], case["trace"], case["tspace"], case["mask"], case["ncontigs"], case["read_off"])


def expect(case):
    exp, stats = pr.propagate(case["las"], case["trace"], case["tspace"], case["mask"][0], case["mask"][1], pc.read_len(case))
    return pr.arrays(exp, len(case["read_off"]) - 1), stats


def same(got, exp, stats):
    ptr, iv = exp
    return (np.array_equal(got.ptr, ptr) and np.array_equal(got.iv, iv) and got.ptr.dtype == ptr.dtype and got.iv.dtype == iv.dtype
            and got.iv.shape == iv.shape and got.raw == stats["raw"] and got.hit == stats["hit"])


@pytest.mark.parametrize("name", list(pc.HAND))
def test_hand_worked_cases(gpu_ctx, name):
    case, expected = pc.HAND[name]
    got = device(gpu_ctx, case)
    assert pr.as_dict(got.ptr, got.iv) == expected and got.passes == 1


@pytest.mark.parametrize("tspace", [100, 126])
def test_trace_shapes(gpu_ctx, tspace):
    case = pc.trace_shapes(tspace)
    exp, stats = expect(case)
    assert stats["raw"] > len(exp[1]) > 0 and stats["empty"] > 0  # (the restatement gives exactly that)
    got = device(gpu_ctx, case)
    assert got.raw > len(got) > 0
    assert same(got, exp, stats)


def test_bitmap_edges(gpu_ctx):
    case, expected = pc.bitmap_edges()
    exp, stats = expect(case)
    got = device(gpu_ctx, case)
    assert same(got, exp, stats) and pr.as_dict(got.ptr, got.iv) == expected
    lens = pc.read_len(case)
    full = [r for r, v in expected.items() if v == [(0, int(lens[r]))]]
    assert any(r + 1 in full for r in full)  # neighbours masked in full: two intervals, not one


def test_long_record(gpu_ctx):
    case = pc.long_record()
    exp, stats = expect(case)
    assert int(case["las"][0]["tlen"]) == 40_000 and stats["raw"] + stats["empty"] >= 3000
    assert same(device(gpu_ctx, case), exp, stats)


def test_many_raw_intervals_into_one_sequence(gpu_ctx):
    case = pc.many_into_one()
    exp, stats = expect(case)
    assert stats["raw"] + stats["empty"] == 100_000 and len(case["read_off"]) == 2
    assert same(device(gpu_ctx, case), exp, stats)


def test_destination_ranges(gpu_ctx, monkeypatch):
    case = pc.wide_destination()
    exp, stats = expect(case)
    one = device(gpu_ctx, case)
    monkeypatch.setenv("DH_PMASK_BITMAP_MB", "1")
    got = device(gpu_ctx, case)
    assert one.passes == 1 and got.passes >= 3
    assert same(got, exp, stats) and same(one, exp, stats)


def test_launch_groups(gpu_ctx, monkeypatch):
    """records cut into launch groups of at most 300 raw intervals (by default a group holds up to 2^31): the same result"""
    case = pc.trace_shapes(100)
    exp, stats = expect(case)
    monkeypatch.setenv("DH_PMASK_GROUP_RAW", "300")
    assert same(device(gpu_ctx, case), exp, stats)
    case = pc.many_into_one(nrec=500)
    exp, stats = expect(case)
    assert same(device(gpu_ctx, case), exp, stats)


def test_volume(gpu_ctx):
    case = pc.volume()
    exp, stats = expect(case)
    got = device(gpu_ctx, case)
    assert len(case["las"]) == 200_000 and 0 < got.hit < len(case["las"]) // 4
    assert same(got, exp, stats)


def test_a_real_mapping_equals_the_host_function(gpu_ctx):
    """the workload, options and mask of tests/test_maskcov.py::test_propagate_mask_matches_the_oracle_on_a_mapping"""
    w = sim.Workload(400_000, 4, 3000, 6000, seed=5)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    las, trace = gpu_ctx.align_db(A, B, dentist_amd.default_align_opts(kmer_mod=4, k=20), select_best=True)
    rng = np.random.default_rng(9)
    ptr, iv = [0], []
    for c in range(w.contigs.n):
        n = int(w.contigs.off[c + 1] - w.contigs.off[c])
        cuts = np.sort(rng.choice(np.arange(1, n), size=24, replace=False))
        for b, e in cuts.reshape(-1, 2):
            iv.append((int(b), int(min(e, b + 900))))
        ptr.append(len(iv))
    mask = (np.array(ptr, dtype=np.int64), np.array(iv, dtype=np.int32))
    optr, oiv = dentist_amd.propagate_mask(las, trace, 100, mask, w.contigs.n, w.reads.off)
    got = gpu_ctx.propagate_mask(las, trace, 100, mask, w.contigs.n, w.reads.off)
    assert np.array_equal(got.ptr, optr) and np.array_equal(got.iv, oiv) and got.iv.dtype == oiv.dtype
    assert len(got) > 100 and len(pr.as_dict(got.ptr, got.iv)) > 100


def test_set_path_uses_the_trace_on_the_device(gpu_ctx):
    w = sim.Workload(300_000, 3, 600, 5000, seed=21, spacing=20000, gap_max=1500)
    mo = dentist_amd.default_align_opts(kmer_mod=4, k=20, width=64, xdrop=60, algo=1)
    po = dentist_amd.default_process_opts(algo=1)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    las, dtrace, _ = gpu_ctx.map_reads(A, B, mo, po, trace_on_device=True)[:3]
    assert isinstance(dtrace, dentist_amd.DeviceTrace) and dtrace.on_device() and len(las) > 100
    rng = np.random.default_rng(2)
    ptr, iv = [0], []
    for c in range(w.contigs.n):
        n = int(w.contigs.off[c + 1] - w.contigs.off[c])
        cuts = np.sort(rng.choice(np.arange(1, n), size=40, replace=False))
        iv += [(int(b), int(e)) for b, e in cuts.reshape(-1, 2)]
        ptr.append(len(iv))
    mask = (np.array(ptr, dtype=np.int64), np.array(iv, dtype=np.int32))
    on_dev = gpu_ctx.propagate_mask(las, dtrace, mo.tspace, mask, w.contigs.n, w.reads.off)
    assert dtrace.on_device()  # used where it is, and still there
    trace = dtrace.numpy()
    arrays = gpu_ctx.propagate_mask(las, trace, mo.tspace, mask, w.contigs.n, w.reads.off)
    assert len(on_dev) > 10 and np.array_equal(on_dev.ptr, arrays.ptr) and np.array_equal(on_dev.iv, arrays.iv)
    assert (on_dev.raw, on_dev.hit) == (arrays.raw, arrays.hit)
    hptr, hiv = dentist_amd.propagate_mask(las, trace, mo.tspace, mask, w.contigs.n, w.reads.off)
    assert np.array_equal(arrays.ptr, hptr) and np.array_equal(arrays.iv, hiv)


@pytest.mark.parametrize("name,case,names", pc.refusals(), ids=[r[0] for r in pc.refusals()])
def test_refusals(gpu_ctx, name, case, names):
    with pytest.raises(dentist_amd.DhError) as ei:
        device(gpu_ctx, case)
    assert ei.value.code == -1 and names in str(ei.value)
    good, expected = pc.HAND["header_example"]
    got = device(gpu_ctx, good)  # the context is usable afterwards
    assert pr.as_dict(got.ptr, got.iv) == expected


def test_empty_inputs(gpu_ctx):
    case = pc.HAND["header_example"][0]
    for change in (dict(las=case["las"][:0]), dict(mask=(np.zeros(2, np.int64), np.zeros((0, 2), np.int32))),
                   dict(las=case["las"][:0], read_off=np.zeros(1, np.int64))):
        c = dict(case)
        c.update(change)
        got = device(gpu_ctx, c)
        assert len(got.ptr) == len(c["read_off"]) and not got.ptr.any() and len(got) == 0
