"""Context.validate_regions (dh_la_validate_regions: every record bound to the regions it touches, a workgroup per region)
against the restatement of the contract (tests/validate_ref.py) on the shapes of tests/validate_cases.py, and against the host
function on a real mapping.  Every comparison is equality."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib, sim

import validate_cases as vc
import validate_ref as vr

pytestmark = pytest.mark.gpu


def device(ctx, case):
    return ctx.validate_regions(case["las"], case["contig_off"], case["regions"], **vc.args(case))


@pytest.mark.parametrize("name", list(vc.HAND))
def test_hand_worked_cases(gpu_ctx, name):
    case, expected = vc.HAND[name]
    got = device(gpu_ctx, case)
    rep = got.reports[0]
    assert got.span_ids.tolist() == expected["span"] and [tuple(x) for x in got.weak.tolist()] == expected["weak"]
    assert (rep["num_spanning_reads"], rep["weak_bp"], bool(rep["is_valid"])) == (len(expected["span"]), expected["weak_bp"], expected["valid"])
    assert vr.same(got, vr.validate(case))


@pytest.mark.parametrize("name", list(vc.SHAPES))
def test_shapes(gpu_ctx, name):
    case = vc.SHAPES[name]
    exp = vr.validate(case)
    got = device(gpu_ctx, case)
    assert vr.same(got, exp) and got.pairs == exp["pairs"] and got.big_regions == 0
    assert got.reports.dtype == dentist_amd.REGION_REPORT_DTYPE


def test_global_tier(gpu_ctx, monkeypatch):
    """DH_VREG_LDS_WINDOWS lowered: regions take the slab of global memory, the result is the same"""
    monkeypatch.setenv("DH_VREG_LDS_WINDOWS", str(vc.LOW_CAP))
    for k in (-1, 0, 1):
        case = vc.SHAPES[f"tier_cap{k:+d}"]
        got = device(gpu_ctx, case)
        assert vr.same(got, vr.validate(case)) and got.big_regions == (1 if k > 0 else 0)
    monkeypatch.setenv("DH_VREG_LDS_WINDOWS", "2")
    for name in ("weak_run_across_chunks", "regions_shuffled", "runs_exactly_wlen_apart", "runs_wlen_plus_one_apart", "window_of_one_base"):
        case = vc.SHAPES[name]
        got = device(gpu_ctx, case)
        assert got.big_regions > 0 and vr.same(got, vr.validate(case))


def test_launch_groups(gpu_ctx, monkeypatch):
    """DH_VREG_SLAB_MB at its minimum: every region of this shape is a launch group of its own, the result is the same"""
    case = vc.group_case()
    exp = vr.validate(case)
    one = device(gpu_ctx, case)
    monkeypatch.setenv("DH_VREG_SLAB_MB", "1")
    cut = device(gpu_ctx, case)
    assert one.groups == 1 and cut.groups >= 3 and one.big_regions == cut.big_regions == 4
    assert vr.same(one, exp) and vr.same(cut, exp)


def test_many_regions_on_one_contig(gpu_ctx):
    """expectation: the host function, which tests/test_maskcov.py pins to the literal loop (the loop is too slow here)"""
    case = vc.many_regions()
    exp = vr.from_host(case)
    got = device(gpu_ctx, case)
    assert vr.same(got, exp) and got.pairs == exp["pairs"]


def test_two_calls_give_identical_arrays(gpu_ctx):
    case = vc.SHAPES["spanning_65"]
    a, b = device(gpu_ctx, case), device(gpu_ctx, case)
    for x, y in ((a.reports, b.reports), (a.weak, b.weak), (a.span_off, b.span_off), (a.span_ids, b.span_ids), (a.mask[0], b.mask[0]),
                 (a.mask[1], b.mask[1])):
        assert x.tobytes() == y.tobytes()
    case = vc.SHAPES["regions_shuffled"]
    a, b = device(gpu_ctx, case), device(gpu_ctx, case)
    assert a.weak.tobytes() == b.weak.tobytes() and a.span_ids.tobytes() == b.span_ids.tobytes() and len(a.span_ids) > 0


@pytest.mark.parametrize("name,case,words", vc.refusals(), ids=[r[0] for r in vc.refusals()])
def test_refusals(gpu_ctx, name, case, words):
    with pytest.raises(dentist_amd.DhError) as ei:
        device(gpu_ctx, case)
    assert ei.value.code == -1 and words in str(ei.value)
    good, expected = vc.HAND["one_spanning_read"]
    got = device(gpu_ctx, good)  # the context is usable afterwards
    assert got.span_ids.tolist() == expected["span"] and bool(got.reports[0]["is_valid"])


def test_a_real_mapping_equals_the_host_function(gpu_ctx):
    """the workload of tests/test_maskcov.py's mapping tests; 24 random intervals per contig as regions"""
    w = sim.Workload(400_000, 4, 3000, 6000, seed=5)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    las, _ = gpu_ctx.align_db(A, B, dentist_amd.default_align_opts(kmer_mod=4, k=20), select_best=True)
    las = las[np.argsort(las["aread"], kind="stable")]
    rng = np.random.default_rng(9)
    regions = []
    for c in range(w.contigs.n):
        n = int(w.contigs.off[c + 1] - w.contigs.off[c])
        cuts = np.sort(rng.choice(np.arange(1, n), size=48, replace=False))
        regions += [(c, int(b), int(min(e, b + 900))) for b, e in cuts.reshape(-1, 2)]
    case = dict(las=las, contig_off=w.contigs.off, regions=regions, min_cov=3, min_span=3, context=1000, window=500)
    exp = vr.from_host(case)
    got = device(gpu_ctx, case)
    assert vr.same(got, exp) and got.pairs == exp["pairs"] > 0
    assert len(got.span_ids) > 100 and 0 < int(got.reports["is_valid"].sum())


def test_raw_handle(gpu_ctx):
    """dh_la_set_validate_regions: the records of a result set, as the arrays taken from it"""
    w = sim.Workload(120_000, 2, 600, 4000, seed=5, spacing=10000, gap_max=600)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    h = gpu_ctx.align_db_block(A, B, 0, w.reads.n, dentist_amd.default_align_opts(kmer_mod=4, k=20), raw=True)
    regions = [(c, 2000 * k, 2000 * k + 300) for c in range(w.contigs.n) for k in range(1, 4)]
    got = gpu_ctx.validate_regions(h, w.contigs.off, regions, 2, min_spanning_reads=1, region_context=500, weak_coverage_window=200)
    las = _lib._take_la_set(h)[0]  # (owns the handle from here on)
    exp = gpu_ctx.validate_regions(las, w.contigs.off, regions, 2, min_spanning_reads=1, region_context=500, weak_coverage_window=200)
    assert got.pairs == exp.pairs > 0 and len(got.span_ids) > 0
    assert vr.same(got, dict(reports=exp.reports, weak=exp.weak, span_off=exp.span_off, span_ids=exp.span_ids, mask=exp.mask))
