"""Chaining on the GPU (dh_la_chain / Context.chain: k_chain_single, k_chain_wave, k_chain_lds, k_chain_global and the
emission kernels of dh_chain.hip) against the restatement of the contract (tests/chain_ref.py) on the shapes of
tests/chain_cases.py: off, score, src_index and flags, in the order of the contract.  Every comparison is equality."""
import functools

import numpy as np
import pytest

import dentist_amd
import chain_cases as cc
import chain_ref as cr

pytestmark = pytest.mark.gpu
GPU_SIZES = (1, 2, 63, 64, 65, 200)


@functools.lru_cache(maxsize=None)
def random_las():
    las = cc.random_case(seed=11, sizes=GPU_SIZES)
    las.setflags(write=False)
    return las


@functools.lru_cache(maxsize=None)
def expected(rel, min_score):
    return cr.arrays(cr.chain(random_las(), **cc.opts_of(rel, min_score)))


def same(ch, exp):
    got = (ch.off, ch.score, ch.src_index, ch.flags)
    return all(np.array_equal(g, e) and g.dtype == e.dtype for g, e in zip(got, exp))


def test_opts_are_the_headers():
    o = dentist_amd.default_chain_opts(126)
    assert (o.max_indel, o.max_chain_gap, o.min_score, o.max_relative_overlap, o.min_relative_score) == (1000, 10000, 126, 0.3, 1.0)


@pytest.mark.parametrize("name", list(cc.HAND))
def test_hand_worked_cases(gpu_ctx, name):
    las, opts, exp = cc.HAND[name]
    assert same(gpu_ctx.chain(las, cc.TSPACE, **opts), cr.arrays(exp))


@pytest.mark.parametrize("rel,min_score", cc.OPTION_SETS)
def test_random_shapes_equal_the_restatement(gpu_ctx, monkeypatch, rel, min_score):
    exp = expected(rel, min_score)
    ch = gpu_ctx.chain(random_las(), cc.TSPACE, **cc.opts_of(rel, min_score))
    assert same(ch, exp) and ch.big_pairs == 0
    # once more with the pairs of 129-200 nodes in the global-memory tier, a launch group each
    monkeypatch.setenv("DH_CHAIN_LDS_NODES", "128")
    monkeypatch.setenv("DH_CHAIN_CHUNK_KB", "9")
    big = gpu_ctx.chain(random_las(), cc.TSPACE, **cc.opts_of(rel, min_score))
    assert same(big, exp) and big.big_pairs == 2


def test_flat_kernel_and_mixed_tiers_in_one_call(gpu_ctx):
    rng = np.random.default_rng(7)
    las = np.concatenate([cc.make_pair(rng, i // 50, i % 50, 1) for i in range(20000)] + [cc.make_pair(rng, 1000, 0, 65)])
    ch = gpu_ctx.chain(las, cc.TSPACE, min_score=1500)
    assert same(ch, cr.arrays(cr.chain(las, min_score=1500)))
    assert 0 < len(ch) < 20001  # some of the single records score below 1500


def test_unordered_input_is_refused_by_name(gpu_ctx):
    bad = random_las().copy()
    k = len(bad) - 1
    bad[k]["aread"] = int(bad[0]["aread"]) - 1
    bad[k]["flags"] &= ~np.uint32(cc.DISABLED)
    with pytest.raises(dentist_amd.DhError) as e:
        gpu_ctx.chain(bad, cc.TSPACE)
    assert e.value.code == -1 and f"record {k} " in str(e.value)


def test_empty_all_disabled_and_bad_options(gpu_ctx):
    for las in (np.zeros(0, dtype=dentist_amd.LA_DTYPE), None):
        if las is None:
            las = random_las().copy()
            las["flags"] |= np.uint32(cc.DISABLED)
        ch = gpu_ctx.chain(las, cc.TSPACE)
        assert same(ch, cr.arrays([])) and len(ch) == 0
    for bad in (dict(max_relative_overlap=0.0), dict(max_relative_overlap=1.0), dict(min_relative_score=-0.1), dict(min_relative_score=1.5),
                dict(min_score=0), dict(max_indel=-1), dict(max_chain_gap=-1), dict(min_relative_score=float("nan"))):
        with pytest.raises(dentist_amd.DhError) as e:
            gpu_ctx.chain(random_las(), cc.TSPACE, **bad)
        assert e.value.code == -1, bad


def test_to_set_gathers_records_and_traces_per_occurrence(gpu_ctx, tmp_path):
    las, trace = cc.with_traces(random_las())
    ch = gpu_ctx.chain(las, cc.TSPACE, min_relative_score=0.0)
    assert same(ch, expected(0.0, 100))
    src = ch.src_index
    assert len(src) > len(set(src.tolist()))  # records shared between chains
    rec, tr = ch.to_set(las, trace, cc.TSPACE)
    assert len(rec) == len(src) and np.array_equal(rec["flags"], ch.flags)
    for f in ("tlen", "diffs", "abpos", "bbpos", "aepos", "bepos", "aread", "bread"):
        assert np.array_equal(rec[f], las[f][src]), f
    # the traces lie one behind the other in output order, a shared record's once per occurrence
    assert np.array_equal(rec["toff"], np.concatenate([[0], np.cumsum(rec["tlen"])[:-1]])) and len(tr) == int(rec["tlen"].sum())
    for i in (0, len(rec) // 2, len(rec) - 1, int(np.flatnonzero(src == np.flatnonzero(np.bincount(src) > 1)[0])[0])):
        for j in np.flatnonzero(src == src[i]):
            assert np.array_equal(tr[rec[j]["toff"]:rec[j]["toff"] + rec[j]["tlen"]],
                                  trace[las[src[i]]["toff"]:las[src[i]]["toff"] + las[src[i]]["tlen"]])
    # every chain is one contiguous run: START opens it, NEXT continues it, the pair and the strand stay
    starts = np.flatnonzero(rec["flags"] & cc.START)
    assert np.array_equal(starts, ch.off[:-1]) and np.all((rec["flags"] & cc.NEXT != 0) == (rec["flags"] & cc.START == 0))
    for a, b in zip(ch.off[:-1], ch.off[1:]):
        run = rec[a:b]
        assert len(set(zip(run["aread"].tolist(), run["bread"].tolist(), (run["flags"] & cc.COMP).tolist()))) == 1
        assert np.all(np.diff(run["abpos"]) > 0) and np.all(np.diff(run["bbpos"]) > 0)
    # the file round-trips
    path = str(tmp_path / "chained.las")
    dentist_amd.las_write(path, rec, tr, cc.TSPACE)
    back, btr, ts = dentist_amd.las_read(path)
    assert ts == cc.TSPACE and back.tobytes() == rec.tobytes() and np.array_equal(btr, tr)
