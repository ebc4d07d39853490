"""Context.repeat_mask (dh_la_repeat_mask: chains by a scan, two keys per chain, a sort per contig in three tiers, a walk with
two running sums, a merge per contig) against the contract (tests/repeat_ref.py over oracle/maskcov.py) on every case of
tests/repeat_cases.py, for all three masks: at the default knobs, at the lowest LDS cap and in many launch groups; the counters;
run-to-run identity; dh_db_mask_coverage on units of one record and where the two differ on chains; the set form; the refusals.
Every comparison is equality."""
import ctypes

import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib, sim

import repeat_cases as rc

pytestmark = pytest.mark.gpu

KNOBS = {"default": {}, "low_cap": {"DH_RMASK_LDS_EVENTS": str(rc.LOW_CAP)}, "many_groups": {"DH_RMASK_CHUNK_MB": "0.000001"}}


def call(ctx, case):
    return ctx.repeat_mask(case["las"], case["contig_off"], case["read_off"], case["lower"], case["upper"], case["improper"], case["allowance"])


def set_knobs(monkeypatch, knobs):
    for k in ("DH_RMASK_LDS_EVENTS", "DH_RMASK_CHUNK_MB"):
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("name", list(rc.ALL))
def test_every_case_equals_the_contract(gpu_ctx, monkeypatch, name, knobs):
    set_knobs(monkeypatch, KNOBS[knobs])
    case, exp = rc.ALL[name], rc.expected_of(name)
    got = call(gpu_ctx, case)
    for which in ("mask", "all", "improper"):
        assert rc.triples(getattr(got, which)) == exp[which], (name, which, knobs)
    ncontigs = len(case["contig_off"]) - 1
    assert (got.units, got.improper_units) == (exp["units"], exp["improper_units"]) and sum(got.tier_contigs) == ncontigs
    assert got.groups == (ncontigs if knobs == "many_groups" else 1)


def test_every_tier_and_more_than_one_group_ran(gpu_ctx, monkeypatch):
    set_knobs(monkeypatch, KNOBS["low_cap"])
    assert call(gpu_ctx, rc.ALL["edges"]).tier_contigs == [1, 3, 3, 1]    # 0 | 2, 62, 64 | 66, cap - 2, cap | cap + 2 events
    set_knobs(monkeypatch, {})
    assert call(gpu_ctx, rc.ALL["edges"]).tier_contigs == [1, 3, 4, 0]
    assert call(gpu_ctx, rc.ALL["above_default_cap"]).tier_contigs == [1, 1, 0, 1]
    set_knobs(monkeypatch, KNOBS["many_groups"])
    got = call(gpu_ctx, rc.ALL["random_12"])
    assert got.groups == 40 and got.tier_contigs[0] > 0 and got.tier_contigs[2] > 0


@pytest.mark.parametrize("name", ["random_12", "above_default_cap", "all_equal"])
def test_two_runs_are_byte_identical(gpu_ctx, monkeypatch, name):
    set_knobs(monkeypatch, {})
    a, b = call(gpu_ctx, rc.ALL[name]), call(gpu_ctx, rc.ALL[name])
    for which in ("mask", "all", "improper"):
        for x, y in zip(getattr(a, which), getattr(b, which)):
            assert x.tobytes() == y.tobytes()


def db_mask(ctx, case, **kw):
    """the parent's route: dh_db_mask_coverage on a fresh DB, dh_db_get_mask"""
    lens = np.diff(case["contig_off"]).tolist()
    db = ctx.db(sim.SeqDb.from_list([np.zeros(n, dtype=np.uint8) for n in lens]))
    db.mask_coverage(case["las"], case["lower"], case["upper"], **kw)
    ptr, iv = db.get_mask()
    return rc.triples((ptr, iv))


@pytest.mark.parametrize("name", ["reference_vector", "edges", "overhang_at_zero", "cov_equals_bounds", "gaps_lower_1"])
def test_single_record_units_equal_db_mask_coverage(gpu_ctx, monkeypatch, name):
    set_knobs(monkeypatch, {})
    case = rc.ALL[name]
    got = call(gpu_ctx, case)
    assert got.units == len(case["las"]) > 0
    assert rc.triples(got.all) == db_mask(gpu_ctx, case)


def test_chains_differ_from_db_mask_coverage_where_the_contract_says(gpu_ctx, monkeypatch):
    set_knobs(monkeypatch, {})
    # the gaps between the members of a chain: covered by the command, not by the per-record kernel
    case = rc.ALL["gaps_covered"]
    assert rc.triples(call(gpu_ctx, case).all) == [(0, 100, 700)]
    assert db_mask(gpu_ctx, case) == [(0, 100, 200), (0, 300, 400), (0, 600, 700)]
    # a chain that is end-to-end as a whole is proper; its members alone are not
    case = rc.ALL["proper_whole_improper_members"]
    got = call(gpu_ctx, case)
    assert got.improper_units == 0 and rc.triples(got.improper) == []
    per_record = db_mask(gpu_ctx, dict(case, lower=0, upper=0), read_off=case["read_off"], improper_only=True, allowance=0)
    assert per_record == [(0, 500, 700), (0, 800, 1000)]


def test_raw_handle_of_a_real_mapping(gpu_ctx, monkeypatch):
    """dh_la_set_repeat_mask: the records of a result set, as the arrays taken from it; both against the contract"""
    set_knobs(monkeypatch, {})
    w = sim.Workload(120_000, 2, 600, 4000, seed=5, spacing=10000, gap_max=600)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    h = gpu_ctx.align_db_block(A, B, 0, w.reads.n, dentist_amd.default_align_opts(kmer_mod=4, k=20), raw=True)
    kw = dict(lower=0, upper=12, improper=(0, 3), allowance=100)
    got = gpu_ctx.repeat_mask(h, w.contigs.off, w.reads.off, **kw)
    las = _lib._take_la_set(h)[0]  # (owns the handle from here on)
    assert len(las) > 100 and np.all(np.diff(las["aread"]) >= 0)
    exp = gpu_ctx.repeat_mask(las, w.contigs.off, w.reads.off, **kw)
    ref = rc.rr.repeat_mask(las, w.contigs.off, w.reads.off, **kw)
    for which in ("mask", "all", "improper"):
        assert rc.triples(getattr(got, which)) == rc.triples(getattr(exp, which)) == ref[which]
    assert got.units == exp.units == ref["units"] and len(ref["mask"]) > 0


@pytest.mark.parametrize("name,case,words", rc.refusals(), ids=[r[0] for r in rc.refusals()])
def test_refusals_name_the_lowest_index(gpu_ctx, name, case, words):
    with pytest.raises(dentist_amd.DhError) as e:
        call(gpu_ctx, case)
    assert words in str(e.value) and "dh_la_repeat_mask" in str(e.value)


def test_bad_arguments_and_no_records(gpu_ctx):
    L = _lib.lib()
    case = rc.reference_vector()
    las, co, ro = case["las"], case["contig_off"], case["read_off"]
    o = _lib.RepeatOpts(0, 4, 0, 0, 0, 0)
    h = ctypes.c_void_p()
    args = [gpu_ctx._h, las.ctypes.data, len(las), co.ctypes.data, 3, ro.ctypes.data, len(ro) - 1, ctypes.byref(o), ctypes.byref(h)]
    for k in (0, 1, 3, 7, 8):   # a NULL pointer, opts missing
        bad = list(args)
        bad[k] = None
        assert L.dh_la_repeat_mask(*bad) == -1 and "bad argument" in L.dh_last_error().decode()
    for k, v in ((2, -1), (4, -3), (6, -1)):   # a negative count
        bad = list(args)
        bad[k] = v
        assert L.dh_la_repeat_mask(*bad) == -1 and "bad argument" in L.dh_last_error().decode()
    bad = list(args)   # read_off may be missing iff with_improper == 0
    bad[5] = None
    assert L.dh_la_repeat_mask(*bad) == 0
    L.dh_repeat_result_destroy(h)
    o.with_improper = 1
    assert L.dh_la_repeat_mask(*bad) == -1 and "bad argument" in L.dh_last_error().decode()
    got = gpu_ctx.repeat_mask(las[:0], co, ro, 1, 2, improper=(1, 2))   # no records: three empty masks, no launch
    assert all(len(getattr(got, w)[1]) == 0 and not getattr(got, w)[0].any() for w in ("mask", "all", "improper")) and got.groups == 0
