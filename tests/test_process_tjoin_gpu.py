"""process_pileups with the re-alignment rounds seeded by the per-group k-mer table (csrc/dh_tjoin.h) against the same
call by the directory lookups (DH_NO_TJOIN=1): records, consensus bases and read ids are identical, and
dh_get_tjoin_counts shows the re-alignment calls of rounds 2 and 3 seeded by the table."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim

pytestmark = pytest.mark.gpu


def process_both_ways(ctx, w, algo, monkeypatch, parts=None):
    """((calls, fall-backs, hits, reruns) of the run as it is, number of pile-ups); asserts the two runs agree"""
    mo = dentist_amd.default_align_opts(**(dict(algo=1, width=64) if algo else {}))
    po = dentist_amd.default_process_opts(rounds=3, algo=algo)
    A, B = ctx.db(w.contigs), ctx.db(w.reads)
    las, trace = ctx.align_db(A, B, mo)
    piles = dentist_amd.Pileups(las, w.contigs.off, po)
    if parts:
        monkeypatch.setenv("DH_PROCESS_PARTS", str(parts))
    ctx.tjoin_counts(reset=True)
    got = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po, read_ids=True)
    counts = ctx.tjoin_counts(reset=True)
    monkeypatch.setenv("DH_NO_TJOIN", "1")
    exp = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po, read_ids=True)
    monkeypatch.delenv("DH_NO_TJOIN")
    assert ctx.tjoin_counts() == (0, 0, 0, 0)
    assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
    assert np.array_equal(got[2][0], exp[2][0]) and np.array_equal(got[2][1], exp[2][1])
    assert (got[0]["status"] == 0).sum() >= 2
    return counts, len(piles)


@pytest.mark.parametrize("algo", [0, 1])
def test_small_gaps_three_rounds(gpu_ctx, monkeypatch, algo):
    """The shape of test_process_small_gaps.  The re-alignment calls of rounds 2 and 3 are seeded by the table, none of them
    falls back.  The one call counted as fallen back is the flank alignment: its A side are the flanks (two stretches of up to
    20 000 bases of contig per pile-up, more index entries than the table is planned for), so it keeps the directory."""
    w = sim.Workload(300_000, 3, 1200, 6000, seed=17, spacing=20000, gap_max=800)
    (calls, fallbacks, hits, reruns), _ = process_both_ways(gpu_ctx, w, algo, monkeypatch)
    print(f"table join: calls {calls}, fall-backs {fallbacks}, hits of the last call {hits}, reruns {reruns}")
    assert calls == 2 and fallbacks == 1 and hits > 0


def test_concurrent_parts_report_to_the_parent(monkeypatch):
    """64 or more pile-ups as four concurrent parts (DH_PROCESS_PARTS=4): the parent's counters are the sums over the
    parts -- two re-alignment calls per part seeded by the table, one flank call per part that keeps the directory."""
    w = sim.Workload(780_000, 70, 3900, 4000, seed=11, spacing=10000, gap_max=600)
    ctx = dentist_amd.Context(0)
    try:
        (calls, fallbacks, hits, reruns), npiles = process_both_ways(ctx, w, 1, monkeypatch, parts=4)
        assert npiles >= 64
        print(f"{npiles} pile-ups, table join: calls {calls}, fall-backs {fallbacks}, hits {hits}, reruns {reruns}")
        assert calls == 2 * 4 and fallbacks == 4 and hits > 0
    finally:
        ctx.close()
