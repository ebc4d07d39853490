"""The pile-up join sizes its hit buffer by pile-up depth and runs k_join once (dh_get_join_counts tells); a context
learns the rate of data the model does not fit, so that such data costs it one rerun, not one per call.  Results never
depend on the capacity: forced rerun, learned capacity and the directory path give the same records and trace values."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim

pytestmark = pytest.mark.gpu

FIELDS = ("tlen", "diffs", "abpos", "bbpos", "aepos", "bepos", "flags", "aread", "bread")


def pile_ups(npiles, nreads, rl, err, seed):
    """`npiles` groups of `nreads` reads, every read a copy of its group's template of `rl` bases with `err` errors."""
    ps = []
    for g in range(npiles):
        rd, _ = sim.reads(seed + 2 * g + 1, sim.genome(seed + 2 * g, rl), nreads, rl, err=err)
        ps.append(rd)
    off = [np.zeros(1, dtype=np.int64)]
    for p in ps:
        off.append(p.off[1:] + off[-1][-1])
    return sim.SeqDb(np.concatenate([p.bases for p in ps]), np.concatenate(off),
                     group=np.concatenate([np.full(p.n, g, dtype=np.int32) for g, p in enumerate(ps)]))


def canon(res):
    """(record fields, every record's trace values in record order) -- independent of where a record's values lie."""
    las, trace = res
    tlen, toff = las["tlen"].astype(np.int64), las["toff"].astype(np.int64)
    start = np.cumsum(tlen) - tlen
    idx = np.repeat(toff - start, tlen) + np.arange(int(tlen.sum()), dtype=np.int64)
    return [las[f].copy() for f in FIELDS], np.asarray(trace)[idx]


def assert_same(a, b):
    (fa, ta), (fb, tb) = a, b
    for f, x, y in zip(FIELDS, fa, fb):
        assert np.array_equal(x, y), f
    assert np.array_equal(ta, tb)


def sym_opts():
    # daligner -s126 -l500 on a grouped DB against itself, every unordered pair aligned once, by the tiled band (DH-2) as
    # in the process stage
    return dentist_amd.default_align_opts(tspace=126, skip_self=2, min_len=500, max_la=256, max_cand=256, algo=1, width=64)


def align(ctx, both, g):
    d = ctx.db(both)
    res = ctx.align_db(d, d, g)
    d.close()
    return canon(res)


def test_deep_pile_ups_fit_the_first_attempt(monkeypatch):
    """8 pile-ups of 160 reads of 1 000 bp at 13 %: about 2 hits per base, above the 1.25 per base every call got before
    depth was looked at -- one launch of k_join, no rerun; the forced rerun (DH_JOIN_HITCAP) and the directory path
    (DH_NO_JOIN) give the same records and trace values."""
    both = pile_ups(8, 160, 1000, 0.13, seed=100)
    total = int(both.off[-1])
    g = sym_opts()
    ctx = dentist_amd.Context(0)
    try:
        got = align(ctx, both, g)
        launches, reruns, hits, cap = ctx.join_counts(reset=True)
        print(f"bases {total}, hits {hits} ({hits / total:.2f} per base), first capacity {cap}, launches {launches}, reruns {reruns}")
        assert hits > 1.25 * total, "precondition: the earlier constant would have overflowed"
        assert (launches, reruns) == (1, 0)
        assert cap >= hits and len(got[0][0]) > both.n
        monkeypatch.setenv("DH_JOIN_HITCAP", "1000")
        forced = align(ctx, both, g)
        assert ctx.join_counts(reset=True) == (2, 1, hits, 1000)
        monkeypatch.delenv("DH_JOIN_HITCAP")
        assert_same(got, forced)
        monkeypatch.setenv("DH_NO_JOIN", "1")
        directory = align(ctx, both, g)
        assert ctx.join_counts()[:2] == (0, 0)
        assert_same(got, directory)
    finally:
        ctx.close()


def test_a_context_learns_the_rate_of_low_error_reads():
    """8 pile-ups of 40 reads of 1 000 bp at 1 %: nearly every k-mer survives, about 15 hits per base against a first
    capacity at its floor -- one rerun on a fresh context, none from then on, the same results both times."""
    both = pile_ups(8, 40, 1000, 0.01, seed=300)
    g = sym_opts()
    ctx = dentist_amd.Context(0)
    try:
        first = align(ctx, both, g)
        launches, reruns, hits, cap = ctx.join_counts(reset=True)
        print(f"bases {int(both.off[-1])}, hits {hits}, first capacity {cap}, launches {launches}, reruns {reruns}")
        assert hits > cap, "precondition: the model does not fit this data"
        assert (launches, reruns) == (2, 1)
        second = align(ctx, both, g)
        launches, reruns, hits2, cap2 = ctx.join_counts()
        assert (launches, reruns) == (1, 0)
        assert hits2 == hits and cap2 >= hits
        assert_same(first, second)
    finally:
        ctx.close()


def test_process_parts_learn_on_their_own_and_report_to_the_parent():
    """process_pileups on 64 or more pile-ups runs as concurrent parts, each on a context of its own that persists: the
    parent's counters show one k_join per part and no rerun on the second call, and the same insertions."""
    w = sim.Workload(780_000, 70, 3900, 4000, seed=11, spacing=10000, gap_max=600)
    mo = dentist_amd.default_align_opts(algo=1, width=64)
    po = dentist_amd.default_process_opts(algo=1)
    ctx = dentist_amd.Context(0)
    try:
        A, B = ctx.db(w.contigs), ctx.db(w.reads)
        las, trace = ctx.align_db(A, B, mo)
        piles = dentist_amd.Pileups(las, w.contigs.off, po)
        assert len(piles) >= 64
        nparts = min(3, len(piles) // 16)
        ctx.join_counts(reset=True)
        rec, bases = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po)
        launches, reruns, hits, cap = ctx.join_counts(reset=True)
        print(f"{len(piles)} pile-ups, first call: launches {launches}, reruns {reruns}, hits {hits}, first capacities {cap}")
        assert launches == nparts + reruns and hits > 0
        rec2, bases2 = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po)
        launches, reruns, hits2, cap2 = ctx.join_counts()
        assert (launches, reruns) == (nparts, 0)
        assert hits2 == hits and cap2 >= hits
        assert np.array_equal(rec2, rec) and np.array_equal(bases2, bases) and np.any(rec["status"] == 0)
    finally:
        ctx.close()
