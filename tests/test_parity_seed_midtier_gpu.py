"""The middle tier of the segment-fed seed back end -- k_seed<2048, JOIN, 256 threads, 64 candidate band pairs>, the first
tier of a chunk of the mapping join or the table join whose reads have 342 to 1 365 hits on average (an unsampled mapping)
-- against the CPU oracle, against the same call with the 512-thread block in its place (DH_SEED_NO_MID_TIER=1) and against
the directory lookups (DH_NO_MJOIN=1): bit exact, whichever tier sorted a read's hits.  dh_get_seed_tier_counts tells
whether the tier ran and how many reads were redone behind it.

DH_MJOIN_MIN=0 sends the small inputs of these tests through the mapping join.

The candidates themselves, item by item: tests/test_parity_seedstage_gpu.py."""
import ctypes
import os

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from helpers import assert_same_las
from oracle import pyoracle as oz
from test_parity_map_gpu import both_opts

pytestmark = pytest.mark.gpu

KW = dict(k=20, kmer_mod=1, algo=1, width=64, xdrop=60)
MID_HITS = 2048        # hits the tier holds per read (both strands)
MID_PAIRS = 2 * 64     # candidate band pairs it holds per read (both strands)


@pytest.fixture(autouse=True)
def _join_for_small_inputs(monkeypatch):
    monkeypatch.setenv("DH_MJOIN_MIN", "0")


def oracle_hits_and_pairs(contigs, reads, **kw):
    """(hits, candidate band pairs) of every read by the oracle's seed stage, both strands together, the candidates before
    the cut at max_cand -- what decides whether the tier holds a read."""
    _, o = both_opts(**kw)
    o.max_cand = 4096
    L = oz.lib()
    L.oz_index_build.restype = ctypes.c_void_p
    L.oz_index_build.argtypes = [ctypes.POINTER(oz.Db), ctypes.POINTER(oz.Opts)]
    L.oz_index_free.argtypes = [ctypes.c_void_p]
    L.oz_seed_candidates.restype = ctypes.c_int
    L.oz_seed_candidates.argtypes = [ctypes.c_void_p, ctypes.POINTER(oz.Db), ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(oz.Opts), ctypes.c_void_p, ctypes.c_void_p]
    da = oz._db(contigs)
    ix = L.oz_index_build(ctypes.byref(da), ctypes.byref(o))
    row = np.zeros(o.max_cand + 1, dtype=oz.CAND_DTYPE)
    hits = np.zeros(reads.n, dtype=np.int64)
    pairs = np.zeros(reads.n, dtype=np.int64)
    nh = ctypes.c_int32(0)
    for r in range(reads.n):
        for s in range(2):
            b = np.ascontiguousarray(reads.seq(r) if s == 0 else sim.revcomp(reads.seq(r)))
            pairs[r] += L.oz_seed_candidates(ix, ctypes.byref(da), b.ctypes.data, len(b), 0, r, 0, ctypes.byref(o),
                                             row.ctypes.data, ctypes.byref(nh))
            hits[r] += nh.value
    L.oz_index_free(ix)
    assert pairs.max() < o.max_cand
    return hits, pairs


def map_and_compare(ctx, contigs, reads, monkeypatch, exp=None, **kw):
    """One mapping call: bit exact against the oracle (`exp`: its result, when a test before computed it), identical under
    DH_SEED_NO_MID_TIER=1 and DH_NO_MJOIN=1 -- neither of which counts a chunk for the tier.  Returns ((records, trace),
    (chunks seeded by the tier, reads redone behind it), chunks of the mapping join)."""
    g, o = both_opts(**kw)
    if exp is None:
        exp = oz.align_db(contigs, reads, o, nthreads=os.cpu_count() or 1)
    A, B = ctx.db(contigs), ctx.db(reads)
    ctx.seed_tier_counts(reset=True)
    ctx.mjoin_counts(reset=True)
    got = ctx.align_db(A, B, g)
    counts = ctx.seed_tier_counts(reset=True)
    chunks, fallbacks = ctx.mjoin_counts(reset=True)
    assert chunks > 0 and fallbacks == 0
    st = ctx.align_stats()
    assert (st.hits, st.cands, st.alignments, st.wave_cells) == tuple(int(x) for x in exp[2])
    assert_same_las(got, exp[:2])
    for env in ("DH_SEED_NO_MID_TIER", "DH_NO_MJOIN"):
        monkeypatch.setenv(env, "1")
        other = ctx.align_db(A, B, g)
        monkeypatch.delenv(env)
        assert ctx.seed_tier_counts(reset=True) == (0, 0), env
        assert_same_las(got, other)
    return got, counts, chunks


@pytest.fixture(scope="module")
def unsampled_12kb():
    """500 unsampled reads of 12 kb on a 2 Mb assembly (the shape of test_the_round_6_paths_against_their_switches: ~700 true
    hits per read on a few hundred neighbouring diagonals, reads spanning two contigs bring two clusters) and the oracle's
    result at KW, computed once."""
    w = sim.Workload(2_000_000, 6, 500, 12000, seed=77, spacing=300_000)
    _, o = both_opts(**KW)
    return w, oz.align_db(w.contigs, w.reads, o, nthreads=os.cpu_count() or 1)


def test_tier_chosen_and_holds_every_read(unsampled_12kb, monkeypatch):
    """1.5 x the host's mean of 12 000 x 0.075 hits lies in (512, 2 048]: the tier seeds the chunk, no read is redone."""
    w, exp = unsampled_12kb
    ctx = dentist_amd.Context(0)
    try:
        _, counts, chunks = map_and_compare(ctx, w.contigs, w.reads, monkeypatch, exp=exp, **KW)
        assert ctx.align_stats().hits / w.reads.n > 400
        assert counts == (chunks, 0)
    finally:
        ctx.close()


def test_heavy_buckets_through_the_network(unsampled_12kb, monkeypatch):
    """DH_SEED_NO_REFINE=1: the reads whose hits fill one diagonal bucket (nearly all of them) take the bitonic network of
    the 256-thread block instead of the second counting pass -- the same order, the same output."""
    w, exp = unsampled_12kb
    monkeypatch.setenv("DH_SEED_NO_REFINE", "1")
    ctx = dentist_amd.Context(0)
    try:
        _, counts, chunks = map_and_compare(ctx, w.contigs, w.reads, monkeypatch, exp=exp, **KW)
        assert counts == (chunks, 0)
    finally:
        ctx.close()


def long_tailed_reads():
    """Log-normal read lengths (mean 11 kb, sd 8 kb) with a tail to 35 - 40 kb and beyond on a 3 Mb assembly."""
    g = sim.genome(31, 3_000_000)
    contigs = sim.SeqDb.from_list([g[:1_400_000], g[1_410_000:]])
    rd, _ = sim.reads(32, g, 700, 11000, 8000, min_len=1000)
    return contigs, rd


def test_reads_with_more_hits_than_the_tier_holds(monkeypatch):
    """At least 20 reads of the long tail bring more than 2 048 hits while the mean stays in the tier's range: exactly those
    are redone from the list (by the 8 192-entry tier), the rest stay."""
    contigs, rd = long_tailed_reads()
    lens = rd.off[1:] - rd.off[:-1]
    assert 4600 < lens.mean() < 18000 and lens.max() > 35000
    hits, pairs = oracle_hits_and_pairs(contigs, rd, **KW)
    over = int((hits > MID_HITS).sum())
    assert over >= 20 and over * 4 < rd.n and hits.max() <= 8192 and pairs.max() <= MID_PAIRS, (over, hits.max(), pairs.max())
    ctx = dentist_amd.Context(0)
    try:
        _, counts, chunks = map_and_compare(ctx, contigs, rd, monkeypatch, **KW)
        assert counts == (chunks, over)
    finally:
        ctx.close()


def repeat_unit_assembly():
    """A unit of 3 kb on each of 150 contigs of the assembly (alternating strands) next to the 1 Mb the reads come from, in
    which 180 bases of the unit stand at twelve places: a read over one of them collects ~10 hits and one candidate band
    pair per copy of the unit -- more than 128 pairs from fewer than 2 048 hits.  (A read over the whole unit would bring
    25 000 hits and leave the tier by its hit count.)"""
    rng = np.random.default_rng(53)
    unit = rng.integers(0, 4, 3000).astype(np.uint8)
    g = sim.genome(54, 1_000_000)
    for i in range(12):
        at = 40_000 + i * 80_000
        g[at:at + 180] = unit[1400:1580]
    seqs = [g[:495_000], g[500_000:]]
    for c in range(150):
        u = unit if c % 2 == 0 else sim.revcomp(unit)
        seqs.append(np.concatenate([rng.integers(0, 4, 1500).astype(np.uint8), u, rng.integers(0, 4, 1500).astype(np.uint8)]))
    rd, _ = sim.reads(55, g, 400, 7000, 0, min_len=7000)
    return sim.SeqDb.from_list(seqs), rd


def test_reads_with_more_band_pairs_than_the_tier_holds(monkeypatch):
    """Some reads collect more than 2 x 64 candidate band pairs from fewer than 2 048 hits: they are marked like reads with
    too many hits and redone by the 512-thread block of the same capacity (256 band pairs per strand); identical records."""
    contigs, rd = repeat_unit_assembly()
    kw = dict(KW, tcap=400)
    hits, pairs = oracle_hits_and_pairs(contigs, rd, **kw)
    by_pairs = int(((pairs > MID_PAIRS) & (hits <= MID_HITS)).sum())
    over = int(((pairs > MID_PAIRS) | (hits > MID_HITS)).sum())
    assert by_pairs >= 3 and over * 4 < rd.n, (by_pairs, over)
    ctx = dentist_amd.Context(0)
    try:
        _, counts, chunks = map_and_compare(ctx, contigs, rd, monkeypatch, **kw)
        assert counts[0] == chunks and counts[1] >= 1
        assert counts[1] == over
    finally:
        ctx.close()


def test_sampled_reads_take_the_wavefront_tier(unsampled_12kb, monkeypatch):
    """kmer_mod 8 on the first data set: ~90 hits per read, the wavefront-per-read tier seeds the chunk and the counter stays 0."""
    w, _ = unsampled_12kb
    ctx = dentist_amd.Context(0)
    try:
        _, counts, _ = map_and_compare(ctx, w.contigs, w.reads, monkeypatch, **dict(KW, kmer_mod=8))
        assert counts == (0, 0)
    finally:
        ctx.close()


def test_long_reads_take_the_4096_entry_tier(monkeypatch):
    """30 kb reads: 1.5 x 30 000 x 0.075 hits is above 2 048, the chunk starts with the 4 096-entry tier and the counter stays 0."""
    w = sim.Workload(1_000_000, 3, 100, 30000, seed=61, spacing=300_000)
    ctx = dentist_amd.Context(0)
    try:
        _, counts, _ = map_and_compare(ctx, w.contigs, w.reads, monkeypatch, **KW)
        assert counts == (0, 0)
    finally:
        ctx.close()


def test_context_stops_using_the_tier_after_a_chunk_of_overflows(monkeypatch):
    """Two thirds of the reads are 2 kb long, one third 20 kb at 5 % error (0.36 hits per base: ~7 000 hits): the mean length
    selects the tier, more than a quarter of the chunk overflows it, and the context does not use it again."""
    g = sim.genome(71, 1_500_000)
    contigs = sim.SeqDb.from_list([g[:700_000], g[705_000:]])
    short, _ = sim.reads(72, g, 200, 2000, 0, min_len=2000, err=0.05)
    long_, _ = sim.reads(73, g, 100, 20000, 0, min_len=20000, err=0.05)
    rd = sim.SeqDb.from_list([short.seq(i) for i in range(short.n)] + [long_.seq(i) for i in range(long_.n)])
    hits, pairs = oracle_hits_and_pairs(contigs, rd, **KW)
    over = int(((hits > MID_HITS) | (pairs > MID_PAIRS)).sum())
    assert over * 4 > rd.n and hits.max() <= 16384, (over, hits.max())
    ctx = dentist_amd.Context(0)
    try:
        (las, trace), counts, chunks = map_and_compare(ctx, contigs, rd, monkeypatch, **KW)
        assert counts == (chunks, over) and chunks == 1
        A, B = ctx.db(contigs), ctx.db(rd)
        again = ctx.align_db(A, B, dentist_amd.default_align_opts(**KW))
        assert ctx.seed_tier_counts() == (0, 0)
        assert_same_las((las, trace), again)
    finally:
        ctx.close()


def test_realignment_rounds_fed_by_the_table_join(monkeypatch):
    """process_pileups over ~70 small pile-ups in four concurrent parts: where the re-alignment rounds (seeded by the
    per-group k-mer table) select the tier, the records, consensus bases and read ids are those of the call without it."""
    w = sim.Workload(780_000, 70, 3900, 4000, seed=11, spacing=10000, gap_max=600)
    ctx = dentist_amd.Context(0)
    try:
        mo = dentist_amd.default_align_opts(algo=1, width=64)
        po = dentist_amd.default_process_opts(rounds=3, algo=1)
        A, B = ctx.db(w.contigs), ctx.db(w.reads)
        las, trace = ctx.align_db(A, B, mo)
        piles = dentist_amd.Pileups(las, w.contigs.off, po)
        assert len(piles) >= 64
        monkeypatch.setenv("DH_PROCESS_PARTS", "4")
        ctx.seed_tier_counts(reset=True)
        ctx.tjoin_counts(reset=True)
        got = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po, read_ids=True)
        counts = ctx.seed_tier_counts(reset=True)
        assert ctx.tjoin_counts(reset=True)[0] > 0
        print(f"{len(piles)} pile-ups: {counts[0]} chunks of the re-alignment rounds seeded by the middle tier, {counts[1]} reads redone")
        monkeypatch.setenv("DH_SEED_NO_MID_TIER", "1")
        exp = dentist_amd.process_pileups(ctx, A, B, las, trace, piles, po, read_ids=True)
        monkeypatch.delenv("DH_SEED_NO_MID_TIER")
        assert ctx.seed_tier_counts() == (0, 0)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
        assert np.array_equal(got[2][0], exp[2][0]) and np.array_equal(got[2][1], exp[2][1])
        assert (got[0]["status"] == 0).sum() >= 2
    finally:
        ctx.close()
