"""The pieces tests/test_parity_fullsize_gpu.py is built from, checked without a GPU on oracle results alone: the two
restrictions that make the oracle affordable at full size are exact (the collect filters on a subset of the reads, the
scaffold-graph builder on a window of contigs), the strata land where the arithmetic says, and the comparisons raise on
a single altered value."""
import os

import numpy as np
import pytest

from dentist_amd import sim
from dentist_amd._lib import INSERTION_DTYPE
import helpers as hp
from oracle import collect_filters as cf
from oracle import process as pr
from oracle import pyoracle as oz
from oracle import scaffold as sc

NTHREADS = min(16, os.cpu_count() or 1)
MAP = dict(kmer_mod=8, k=20, width=64, xdrop=60, algo=1)


class Small:
    """The 2 Mb workload of test_the_benched_chain_against_the_oracle, mapped and filtered by the oracle."""

    def __init__(self):
        self.w = sim.Workload(2_000_000, 20, 20_000, 10_000, seed=20260929)
        self.opts = oz.default_opts(**MAP)
        self.olas, self.otrace, _ = oz.align_db(self.w.contigs, self.w.reads, self.opts, nthreads=NTHREADS, sort=False,
                                                select_best=True)
        self.flas, _, _ = cf.collect_filter(self.olas, self.w.contigs.off, self.w.reads.off)


@pytest.fixture(scope="module")
def small():
    return Small()


@pytest.fixture(scope="module")
def subset(small):
    """1 500 seeded reads of the small workload mapped on their own and filtered on their own."""
    w = small.w
    ids = np.sort(np.random.default_rng(5).choice(w.reads.n, size=1500, replace=False)).astype(np.int64)
    sub = hp.sub_db(w.reads, ids)
    slas, strace, _ = oz.align_db(w.contigs, sub, small.opts, nthreads=NTHREADS, sort=False, select_best=True)
    sflas, _, _ = cf.collect_filter(slas, w.contigs.off, sub.off)
    return ids, sub, sflas, strace


def test_filtering_a_subset_of_the_reads_equals_the_subset_of_the_filtered_whole(small, subset):
    w = small.w
    ids, sub, sflas, strace = subset
    # the filters alone: the records of the sampled reads cut out of the mapping of all reads
    rows = np.flatnonzero(np.isin(small.olas["bread"], ids))
    cut = small.olas[rows].copy()
    cut["bread"] = np.searchsorted(ids, cut["bread"])
    fcut, _, _ = cf.collect_filter(cut, w.contigs.off, sub.off)
    assert np.array_equal(fcut["flags"], small.flas["flags"][rows])
    assert np.any(fcut["flags"] & cf.DISABLED) and not np.all(fcut["flags"] & cf.DISABLED)
    # ... and the sampled reads mapped on their own, then filtered: what the full-size test does
    nrec, ntr = hp.assert_same_las_of_reads((small.flas, small.otrace), (sflas, strace), ids)
    assert nrec == len(rows) and ntr == int(cut["tlen"].sum())


def test_the_graph_builder_on_a_window_of_contigs_equals_the_global_build(small):
    w = small.w
    gaps_in = [(c, c + 1) for c in range(1, w.contigs.n)]
    whole = hp.oracle_gap_entries(sc.build(w.contigs.n, hp.la_chains(small.flas, w.contigs, w.reads), gaps_in, min_spanning_reads=3))
    assert sorted(whole) == list(range(w.contigs.n - 1))
    with_ext = 0
    for g in range(w.contigs.n - 1):
        exp = hp.batch_order(whole[g])
        assert hp.restricted_gap_entries(small.flas, w.contigs, w.reads, g, 3, window=1) == exp, g
        assert len(exp) > 60
        with_ext += any(t[1] < 0 or t[2] < 0 for t in exp)
    assert with_ext > 0, "the case must contain extension entries"


def test_chunk_edges_and_offset_wraps_on_synthetic_offsets():
    # 1 000 003 reads of 15 000 bases: offsets only, 15 Gbp that are never allocated
    n, ln = 1_000_003, 15_000
    off = np.arange(n + 1, dtype=np.int64) * ln
    assert hp.chunk_bounds(n) == [(0, 1 << 19), (1 << 19, n)]
    edges = hp.chunk_edge_reads(n)
    assert len(edges) == 4 * 64 and edges[0] == 0 and edges[-1] == n - 1
    assert all(r in edges for r in ((1 << 19) - 64, (1 << 19) - 1, 1 << 19, (1 << 19) + 63, n - 64))
    assert (1 << 19) - 65 not in edges and (1 << 19) + 64 not in edges and n - 65 not in edges
    hit, around = hp.offset_wrap_reads(off)
    # from the start of the DB: 2^32, 2 * 2^32, 3 * 2^32; from the start of chunk 1 (read 2^19): one more
    base = (1 << 19) * ln
    assert hit.tolist() == sorted([(1 << 32) // ln, (2 << 32) // ln, (3 << 32) // ln, (base + (1 << 32)) // ln])
    assert hit.tolist() == [286331, 572662, 810619, 858993]
    for r in hit:
        assert any(off[r] <= m < off[r + 1] for m in (1 << 32, 2 << 32, 3 << 32, base + (1 << 32)))
    assert len(around) == 4 * 17 and all(r - 8 in around and r + 8 in around for r in hit)
    # a read that STARTS on a multiple holds it, the read before it does not; offset 0 is no wrap; the DB's end is outside
    off = np.arange(13, dtype=np.int64) * 250
    hit, around = hp.offset_wrap_reads(off, chunk_items=12, wrap=1000, span=1)
    # DB: 1000, 2000 -> reads 4, 8; chunks of 6 reads start at 0 and 1500: 2500 -> read 10
    assert hit.tolist() == [4, 8, 10] and around.tolist() == [3, 4, 5, 7, 8, 9, 10, 11]
    # odd read counts and short last chunks
    assert hp.chunk_bounds(7, chunk_items=4) == [(0, 2), (2, 4), (4, 6), (6, 7)]
    assert hp.chunk_edge_reads(7, chunk_items=4, edge=1).tolist() == [0, 1, 2, 3, 4, 5, 6]
    assert hp.chunk_edge_reads(11, chunk_items=16, edge=2).tolist() == [0, 1, 6, 7, 8, 9, 10]


def test_the_read_sample_on_a_small_mapping(small):
    w = small.w
    pile_reads = [5000, 5001, 5002, 4095, 19_999]
    kw = dict(pile_reads=pile_reads, size=1500, chunk_items=1 << 13, wrap=1 << 25)
    ids, counts, wrapped = hp.fullsize_read_sample(w, small.flas, np.random.default_rng(3), **kw)
    assert np.all(np.diff(ids) > 0) and ids[0] == 0 and ids[-1] == w.reads.n - 1
    assert tuple(counts) == hp.STRATA and sum(counts.values()) == len(ids)
    assert len(ids) == 1500 + counts["pile-up members"] and all(counts[s] > 0 for s in hp.STRATA)
    assert counts["chunk edges"] == 2 * 64 * len(hp.chunk_bounds(w.reads.n, 1 << 13))
    assert 1 <= counts["pile-up members"] <= 3    # 4095 and 19 999 are chunk edges already
    assert set(pile_reads) <= set(ids.tolist()) and set(wrapped.tolist()) <= set(ids.tolist())
    nwraps = int(w.reads.off[-1]) >> 25
    assert nwraps >= 3 and len(wrapped) >= nwraps
    # strata 3 and 4 against their definitions
    cnt = np.bincount(small.flas["bread"], minlength=w.reads.n)
    assert cnt[ids].max() == cnt.max() and (cnt[ids] == 0).sum() >= min(200, int((cnt == 0).sum()))
    for c, field, best in ((0, "abpos", min), (w.contigs.n - 1, "aepos", max)):
        on = small.flas[small.flas["aread"] == c]
        assert int(on["bread"][on[field] == best(on[field])][0]) in ids
    ext = hp.contig_extreme_reads(w, small.flas)
    over = [max(int(e - b) if s < b < e else 0 for b in w.gap_begin) for s, e, _ in w.read_truth[ext]]
    assert max(over) > 0.9 * 10_000    # a read that barely touches the contig before a gap, and is mapped
    # the same seed gives the same sample, another seed another random stratum
    again = hp.fullsize_read_sample(w, small.flas, np.random.default_rng(3), **kw)
    other = hp.fullsize_read_sample(w, small.flas, np.random.default_rng(4), **kw)
    assert np.array_equal(again[0], ids) and again[1] == counts
    assert len(other[0]) == len(ids) and not np.array_equal(other[0], ids)


def test_the_pile_up_sample_and_the_cuts_between_the_concurrent_parts():
    rng = np.random.default_rng(11)
    counts = rng.integers(40, 200, size=1000)
    cut = hp.process_part_cuts(counts)
    cost = counts.astype(np.float64) ** 2
    assert cut[0] == 0 and cut[-1] == 1000 and len(cut) == 4 and np.all(np.diff(cut) > 0)
    for k in (1, 2):   # part k ends with the last pile-up that keeps the parts before the cut within k thirds of the cost
        assert cost[:cut[k]].sum() <= cost.sum() * k / 3 * (1 + 1e-12) < cost[:cut[k] + 1].sum() * (1 + 1e-12)
    assert hp.process_part_cuts([50] * 63) == [0, 63]               # fewer than 64 pile-ups: one piece
    assert hp.process_part_cuts([50] * 64) == [0, 21, 42, 64]
    assert hp.process_part_cuts([1000] + [1] * 99) == [0, 1, 2, 100]   # no part is empty
    gap_len = rng.integers(50, 5000, size=1000)
    s = hp.fullsize_pile_sample(counts, gap_len, np.random.default_rng(1))
    assert (s["first"], s["last"]) == (0, 999)
    assert counts[s["most entries"]] == counts.max() and counts[s["fewest entries"]] == counts.min()
    assert gap_len[s["longest gap"]] == gap_len.max() and gap_len[s["shortest gap"]] == gap_len.min()
    assert (s["last of part 1"], s["first of part 2"], s["last of part 2"], s["first of part 3"]) == \
           (cut[1] - 1, cut[1], cut[2] - 1, cut[2])
    assert len(s) == 12 and len({s["random 1"], s["random 2"]} - {v for k, v in s.items() if not k.startswith("random")}) == 2
    assert hp.fullsize_pile_sample(counts, gap_len, np.random.default_rng(1)) == s


def test_the_mapping_comparison_raises_on_one_altered_value(small, subset):
    ids, sub, sflas, strace = subset
    got = (small.flas, small.otrace)
    hp.assert_same_las_of_reads(got, (sflas, strace), ids)
    victim = int(np.flatnonzero(sflas["tlen"] > 4)[len(sflas) // 2])
    # one trace value
    tr = strace.copy()
    tr[sflas[victim]["toff"] + 3] += 1
    with pytest.raises(AssertionError, match=f"read {int(ids[sflas[victim]['bread']])}:"):
        hp.assert_same_las_of_reads(got, (sflas, tr), ids)
    # one flag bit: DISABLED, a chain flag, the strand
    for bit in (0x20, 0x4, 0x1):
        alt = sflas.copy()
        alt["flags"][victim] ^= bit
        with pytest.raises(AssertionError):
            hp.assert_same_las_of_reads(got, (alt, strace), ids)
    # one record dropped: the only record of a read, and one of several
    only = int(np.flatnonzero(np.bincount(sflas["bread"])[sflas["bread"]] == 1)[0])
    several = int(np.flatnonzero(np.bincount(sflas["bread"])[sflas["bread"]] > 1)[0])
    for x in (only, several):
        with pytest.raises(AssertionError, match="LA count differs"):
            hp.assert_same_las_of_reads(got, (np.delete(sflas, x), strace), ids)
    # ... and a record too many on the side under test
    with pytest.raises(AssertionError, match="LA count differs"):
        hp.assert_same_las_of_reads((np.delete(small.flas, int(np.flatnonzero(small.flas["bread"] == ids[7])[0])), small.otrace),
                                    (sflas, strace), ids)
    # one coordinate
    alt = sflas.copy()
    alt["bepos"][victim] -= 1
    with pytest.raises(AssertionError):
        hp.assert_same_las_of_reads(got, (alt, strace), ids)


def test_the_process_comparison_raises_on_one_altered_value(small):
    w = small.w
    g = 7
    ent = hp.cap_entries(hp.restricted_gap_entries(small.flas, w.contigs, w.reads, g, 3), small.flas, 60)
    assert len(ent) == 60
    ex = pr.process_pile(ent, small.flas, small.otrace, w.contigs, w.reads, g, rounds=3, nthreads=NTHREADS, algo=1)
    assert ex["status"] == "ok"
    # the record dh_process_pileups would return for this pile-up, with its consensus behind another one's bases
    r = np.zeros(1, dtype=INSERTION_DTYPE)[0]
    r["contig_left"], r["status"], r["nreads"], r["ref_read"] = g, 0, ex["pile"].n, ex["ref_idx"]
    r["ref_read_id"], r["crop_left"], r["crop_right"] = ex["read_ids"][ex["ref_idx"]], ex["cropL"], ex["cropR"]
    for f in ("left_aepos", "right_abpos", "ins_begin", "ins_end", "comp"):
        r[f] = ex[f]
    r["cons_off"], r["cons_len"] = 100, len(ex["consensus"])
    bases = np.concatenate([np.zeros(100, np.uint8), ex["consensus"], np.zeros(50, np.uint8)])
    assert hp.assert_same_insertion(r, bases, ex) == "ok"
    # one consensus base
    for at in (0, len(ex["consensus"]) // 2, len(ex["consensus"]) - 1):
        alt = dict(ex, consensus=ex["consensus"].copy())
        alt["consensus"][at] ^= 1
        with pytest.raises(AssertionError, match="consensus differs"):
            hp.assert_same_insertion(r, bases, alt)
    # one inserted base, one coordinate, the reference read, the status
    alt = dict(ex, insertion=ex["insertion"].copy())
    alt["insertion"][len(alt["insertion"]) // 2] ^= 1
    with pytest.raises(AssertionError, match="inserted bases differ"):
        hp.assert_same_insertion(r, bases, alt)
    for key in ("cropL", "cropR", "ref_idx", "left_aepos", "right_abpos", "ins_begin", "ins_end"):
        with pytest.raises(AssertionError):
            hp.assert_same_insertion(r, bases, dict(ex, **{key: ex[key] + 1}))
    with pytest.raises(AssertionError):
        hp.assert_same_insertion(r, bases, dict(ex, status="pile too small"))
    failed = r.copy()
    failed["status"] = 3
    with pytest.raises(AssertionError):
        hp.assert_same_insertion(failed, bases, ex)
    with pytest.raises(AssertionError):
        hp.assert_same_insertion(failed, bases, dict(ex, status="pile too small"))
    assert hp.assert_same_insertion(failed, bases, dict(ex, status=hp.PROCESS_STATUS[3])) == hp.PROCESS_STATUS[3]
