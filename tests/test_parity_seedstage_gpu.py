"""The seed stage by itself -- dh_seed_candidates: the fat directory, the pile-up join, the partitioned mapping join, the
per-group table join and behind them every tier of k_seed -- against the oracle's seed stage (oz.seed_candidates_all), item
by item: the hits, the number of candidates and every candidate field by field in the order the extension takes them.  The
mapping tests (test_parity_map_gpu, test_parity_mjoin_gpu, test_parity_tjoin_gpu, test_parity_seed_midtier_gpu) compare
finished alignments, which a seed moved along its diagonal or a mis-scored band pair leaves untouched; a mismatch here names
the item, the rank and the field.  Every test shows with the context's counters (or the library's trace) which path and
tier ran.  Constructed inputs: tests/seed_cases.py (what they claim is checked on the oracle by tests/test_seed_cases.py)."""
import re

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from oracle import pyoracle as oz
import seed_cases as sc
from test_parity_map_gpu import both_opts, grouped_piles
from test_parity_tjoin_gpu import BASE as TJ_BASE, base_case as tj_base_case, copies, grouped

pytestmark = pytest.mark.gpu

FIELDS = ("score", "aseq", "apos", "bpos")
KW = dict(k=20, kmer_mod=1, algo=1, width=64)
CASES = sc.all_cases()
MAPPING_CASES = [c for c in CASES if c["mapping"]]


def ids(cases):
    return [c["name"] for c in cases]


def where(it):
    return f"item {it} (read {it // 2}, strand {it & 1})"


def assert_same_seeds(got, exp, what):
    """ncand, nhits and the first ncand candidates of every item, field by field in stored order"""
    cand, ncand, nhits = got
    ecand, encand, enhits = exp
    assert len(ncand) == len(encand) and cand.shape == ecand.shape, what
    for name, a, b in (("nhits", nhits, enhits), ("ncand", ncand, encand)):
        bad = np.flatnonzero(a != b)
        assert not len(bad), f"{what}: {where(int(bad[0]))} {name} {a[bad[0]]}, oracle {b[bad[0]]} ({len(bad)} items differ)"
    live = np.arange(cand.shape[1])[None, :] < ncand[:, None]
    for f in FIELDS:
        bad = np.argwhere(live & (cand[f] != ecand[f]))
        if len(bad):
            it, r = int(bad[0][0]), int(bad[0][1])
            raise AssertionError(f"{what}: {where(it)} rank {r} field {f}: {cand[it][r][f]}, oracle {ecand[it][r][f]} "
                                 f"(candidate {cand[it][r]}, oracle {ecand[it][r]}; {len(bad)} candidates differ in {f})")


def assert_well_formed(got, kw, what):
    """what the extension relies on, whatever the oracle says: at most max_cand candidates; symmetric mode: the candidates
    of one partner stand together (k_units_fat and k_tile_units make one work unit of each run of equal aseq)"""
    cand, ncand, _ = got
    assert (ncand <= cand.shape[1]).all() and (ncand >= 0).all(), what
    if kw.get("skip_self", 0) == 2:
        for it in np.flatnonzero(ncand > 1):
            aseq = cand["aseq"][it][:ncand[it]]
            runs = 1 + int((aseq[1:] != aseq[:-1]).sum())
            assert runs == len(set(aseq.tolist())), f"{what}: {where(int(it))} candidates of one partner are apart: {aseq.tolist()}"


def oracle_seeds(A, B, **kw):
    _, o = both_opts(**kw)
    return oz.seed_candidates_all(A, B, o, with_nhits=True)


def gpu_seeds(ctx, A, B, **kw):
    """dh_seed_candidates on fresh device DBs (nothing cached from a call under other switches)"""
    g, _ = both_opts(**kw)
    dA = ctx.db(A)
    dB = dA if B is A else ctx.db(B)
    try:
        return ctx.seed_candidates(dA, dB, g)
    finally:
        dA.close()
        if dB is not dA:
            dB.close()


def check(ctx, A, B, exp, what, **kw):
    got = gpu_seeds(ctx, A, B, **kw)
    assert_well_formed(got, kw, what)
    assert_same_seeds(got, exp, what)
    st = ctx.align_stats()
    assert (st.hits, st.cands) == (int(exp[2].sum()), int(exp[1].sum())), what
    return got


def reset(ctx):
    for f in (ctx.mjoin_counts, ctx.join_counts, ctx.tjoin_counts, ctx.seed_tier_counts):
        f(reset=True)


def per_read(x):
    return x[0::2].astype(np.int64) + x[1::2]


@pytest.fixture(scope="module")
def ctx():
    """a context of this module's own: what a context learns about the tiers stays out of the other modules' counters"""
    c = dentist_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def case_oracle():
    return {c["name"]: oracle_seeds(c["A"], c["B"], **c["kw"]) for c in CASES}


# ------------------------------------------------------------------------------------------------------ constructed cases
@pytest.mark.parametrize("c", CASES, ids=ids(CASES))
def test_constructed_case_by_the_directory(ctx, case_oracle, c):
    reset(ctx)
    check(ctx, c["A"], c["B"], case_oracle[c["name"]], c["name"], **c["kw"])
    assert ctx.mjoin_counts() == (0, 0) and ctx.join_counts()[0] == 0 and ctx.tjoin_counts()[0] == 0
    assert ctx.seed_tier_counts() == (0, 0)


FIRST_TIERS = {"wavefront": (), "middle": ("DH_SEED_NO_WAVE_TIER",), "512-thread": ("DH_SEED_NO_WAVE_TIER", "DH_SEED_NO_MID_TIER")}


@pytest.fixture
def fresh_ctx():
    """a context that has learned nothing: a read of a case before that overflowed the wavefront-per-read tier or the middle
    tier (one read is more than a quarter of these chunks) would switch the tier off for the cases after it"""
    c = dentist_amd.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("tier", list(FIRST_TIERS))
@pytest.mark.parametrize("c", MAPPING_CASES, ids=ids(MAPPING_CASES))
def test_constructed_case_by_the_mapping_join(fresh_ctx, case_oracle, monkeypatch, c, tier):
    """every first tier of a chunk of the mapping join: the wavefront per read (what these few hits select), the 256-thread
    tier and the 512-thread block with 2 048 entries"""
    monkeypatch.setenv("DH_MJOIN_MIN", "0")
    for env in FIRST_TIERS[tier]:
        monkeypatch.setenv(env, "1")
    check(fresh_ctx, c["A"], c["B"], case_oracle[c["name"]], f"{c['name']}, mapping join, {tier} tier", **c["kw"])
    assert fresh_ctx.mjoin_counts() == (1, 0)
    assert fresh_ctx.seed_tier_counts()[0] == (1 if tier == "middle" else 0)


@pytest.mark.parametrize("c", MAPPING_CASES, ids=ids(MAPPING_CASES))
def test_constructed_case_in_chunks_of_three_reads(case_oracle, monkeypatch, c):
    """DH_ALIGN_CHUNK=6: chunk edges inside the DB, the candidate rows of a chunk shifted by its first item"""
    monkeypatch.setenv("DH_MJOIN_MIN", "0")
    monkeypatch.setenv("DH_ALIGN_CHUNK", "6")
    for no_mjoin in (False, True):
        if no_mjoin:
            monkeypatch.setenv("DH_NO_MJOIN", "1")
        ctx = dentist_amd.Context(0)
        try:
            check(ctx, c["A"], c["B"], case_oracle[c["name"]], f"{c['name']}, chunks of 6 items{' by the directory' * no_mjoin}", **c["kw"])
            assert ctx.mjoin_counts() == ((0 if no_mjoin else (2 * c["B"].n + 5) // 6), 0)
        finally:
            ctx.close()


# --------------------------------------------------------------------------------------------------- directory capacities
@pytest.fixture(scope="module")
def long_tailed():
    """160 unsampled reads at 5 % error with log-normal lengths (mean 9 kb, a tail beyond 50 kb: 0.36 hits per base) on a
    0.9 Mb assembly, and the oracle's seeds"""
    g = sim.genome(301, 900_000)
    contigs = sim.SeqDb.from_list([g[:440_000], g[445_000:]])
    rd, _ = sim.reads(302, g, 160, 9000, 9000, min_len=800, err=0.05)
    return contigs, rd, oracle_seeds(contigs, rd, **KW)


def expected_caps(hits, cap, nitems, big_pct=None):
    """the capacities the directory path tries (seed_chunk: the whole chunk again with twice the capacity when more reads
    overflow than HBM staging is worth) as [(capacity, reads above it), ...]"""
    out = []
    while True:
        over = int((hits > cap).sum())
        if over:
            out.append((cap, over))
        redo_all = nitems // 4 if cap >= 8192 else nitems // 50 + 8
        if big_pct is not None:
            redo_all = int(nitems * big_pct / 200.0)
        if over > redo_all and cap < 16384:
            cap *= 2
            continue
        return out


@pytest.mark.parametrize("cap,switch", [("1024", None), ("2048", None), ("4096", None), ("8192", None), ("16384", None),
                                        ("1024", ("DH_SEED_BIG_PCT", "100")), ("4096", ("DH_SEED_BIG_PCT", "100")),
                                        (None, ("DH_SEED_BLOCKS_PER_CU", "1")), ("2048", ("DH_SEED_BLOCKS_PER_CU", "1"))])
def test_directory_capacities(ctx, long_tailed, monkeypatch, capfd, cap, switch):
    """Every LDS capacity of the directory path's k_seed, the reads above it redone by the HBM-staged k_seed<0> -- after the
    capacity was doubled while many overflowed, or (DH_SEED_BIG_PCT=100) all of them straight away"""
    contigs, rd, exp = long_tailed
    hits = per_read(exp[2])
    for c in (1024, 2048, 4096, 8192):
        assert (hits > c).sum() >= 5, c
    if cap:
        monkeypatch.setenv("DH_SEED_CAP", cap)
    if switch:
        monkeypatch.setenv(*switch)
    monkeypatch.setenv("DH_TRACE", "1")
    reset(ctx)
    capfd.readouterr()
    check(ctx, contigs, rd, exp, f"DH_SEED_CAP={cap} {switch}", **KW)
    err = capfd.readouterr().err
    assert ctx.mjoin_counts() == (0, 0)
    tried = [(int(c), int(n)) for c, n in re.findall(r"\[seeds\] cap (\d+): (\d+) of \d+ reads overflow", err)]
    print(tried, "big_items", ctx.align_stats().big_items)
    if cap:
        want = expected_caps(hits, int(cap), 2 * rd.n, 100 if switch and switch[0] == "DH_SEED_BIG_PCT" else None)
        assert tried == want
    assert tried and ctx.align_stats().big_items == 2 * tried[-1][1] > 0


# ----------------------------------------------------------------------------------------------------- mapping join tiers
def join_tiers(err):
    """{entries: reads redone from the list by that tier} of the library's trace"""
    out = {}
    for n, t in re.findall(r"join tiers: (\d+) reads redone with (\d+) entries", err):
        if int(n):
            out[int(t)] = out.get(int(t), 0) + int(n)
    return out


def mapping_three_ways(A, B, exp, monkeypatch, capfd, what, expect_mid=None, env=(), **kw):
    """The call as it is, with DH_SEED_NO_REFINE=1 and with DH_NO_MJOIN=1, each against the oracle.  Returns the tier counts,
    the trace's list tiers and big_items of the first."""
    monkeypatch.setenv("DH_MJOIN_MIN", "0")
    monkeypatch.setenv("DH_TRACE", "1")
    for k, v in env:
        monkeypatch.setenv(k, v)
    out = None
    for extra in (None, "DH_SEED_NO_REFINE", "DH_NO_MJOIN"):
        if extra:
            monkeypatch.setenv(extra, "1")
        ctx = dentist_amd.Context(0)  # (a context learns from its chunks: each run starts from scratch)
        try:
            capfd.readouterr()
            check(ctx, A, B, exp, f"{what} {extra or ''}", **kw)
            err = capfd.readouterr().err
            counts, mj, big = ctx.seed_tier_counts(), ctx.mjoin_counts(), ctx.align_stats().big_items
        finally:
            ctx.close()
        if extra:
            monkeypatch.delenv(extra)
        assert mj == ((0, 0) if extra == "DH_NO_MJOIN" else (1, 0)), (what, extra)
        if extra != "DH_NO_MJOIN":
            if expect_mid is not None:
                assert counts == expect_mid, (what, extra)
            if out is None:
                out = counts, join_tiers(err), big
            else:
                assert (counts, join_tiers(err), big) == out, (what, extra)
        else:
            assert counts == (0, 0)
    return out


@pytest.fixture(scope="module")
def reads_6kb():
    w = sim.Workload(800_000, 3, 150, 6000, seed=311, spacing=200_000)
    return w, oracle_seeds(w.contigs, w.reads, **KW)


def test_wavefront_tier(reads_6kb, monkeypatch, capfd):
    """kmer_mod 8: ~57 hits per read, the wavefront-per-read tier (512 hits, 32 band pairs); DH_SEED_NO_WAVE_TIER=1 puts the
    middle tier in its place, DH_SEED_NO_MID_TIER=1 on top of it the 512-thread block"""
    w, _ = reads_6kb
    kw = dict(KW, kmer_mod=8)
    exp = oracle_seeds(w.contigs, w.reads, **kw)
    assert per_read(exp[2]).max() < 512 / 1.5
    assert mapping_three_ways(w.contigs, w.reads, exp, monkeypatch, capfd, "wavefront tier", expect_mid=(0, 0), **kw) == ((0, 0), {}, 0)
    mapping_three_ways(w.contigs, w.reads, exp, monkeypatch, capfd, "the middle tier in its place", expect_mid=(1, 0),
                       env=(("DH_SEED_NO_WAVE_TIER", "1"),), **kw)
    mapping_three_ways(w.contigs, w.reads, exp, monkeypatch, capfd, "the 512-thread block in its place", expect_mid=(0, 0),
                       env=(("DH_SEED_NO_WAVE_TIER", "1"), ("DH_SEED_NO_MID_TIER", "1")), **kw)


def test_middle_tier(reads_6kb, monkeypatch, capfd):
    """unsampled reads of 6 kb: ~450 hits per read, the 256-thread tier seeds the chunk and holds every read"""
    w, exp = reads_6kb
    hits = per_read(exp[2])
    assert 512 / 1.5 < hits.mean() and hits.max() <= 2048
    assert mapping_three_ways(w.contigs, w.reads, exp, monkeypatch, capfd, "middle tier", expect_mid=(1, 0), **KW) == ((1, 0), {}, 0)


def test_2048_entry_first_tier(reads_6kb, monkeypatch, capfd):
    w, exp = reads_6kb
    mapping_three_ways(w.contigs, w.reads, exp, monkeypatch, capfd, "2048-entry tier", expect_mid=(0, 0),
                       env=(("DH_SEED_NO_MID_TIER", "1"),), **KW)


def test_4096_entry_first_tier(monkeypatch, capfd):
    """reads of 30 kb: 1.5 x 30 000 x 0.075 hits is above 2 048, the chunk starts with the 4 096-entry tier"""
    w = sim.Workload(900_000, 3, 40, 30000, seed=312, spacing=250_000)
    exp = oracle_seeds(w.contigs, w.reads, **KW)
    hits = per_read(exp[2])
    assert 2048 < 1.5 * hits.mean() and hits.max() <= 4096
    for env in ((), (("DH_SEED_NO_MID_TIER", "1"),)):
        assert mapping_three_ways(w.contigs, w.reads, exp, monkeypatch, capfd, f"4096-entry tier {env}", expect_mid=(0, 0), env=env,
                                  **KW) == ((0, 0), {}, 0)


@pytest.fixture(scope="module")
def with_low_error_reads(reads_6kb):
    """the 6 kb reads and, at 5 % error, six reads of 20 kb (~7 500 hits) and six of 40 kb (~15 000)"""
    w, _ = reads_6kb
    lo20, _ = sim.reads(313, w.truth, 6, 20000, 0, min_len=20000, err=0.05)
    lo40, _ = sim.reads(314, w.truth, 6, 40000, 0, min_len=40000, err=0.05)
    rd = sim.SeqDb.from_list([w.reads.seq(i) for i in range(w.reads.n)] + [lo20.seq(i) for i in range(6)] + [lo40.seq(i) for i in range(6)])
    exp = oracle_seeds(w.contigs, rd, **KW)
    hits = per_read(exp[2])
    assert ((hits > 2048) & (hits <= 8192)).sum() == 6 and ((hits > 8192) & (hits <= 16384)).sum() == 6 and (hits > 2048).sum() == 12
    return w.contigs, rd, exp


def test_reads_redone_from_the_list(with_low_error_reads, monkeypatch, capfd):
    """behind the middle tier six reads are redone by the 8 192-entry tier and six by the 16 384-entry one; behind the
    2 048-entry 512-thread tier (DH_SEED_NO_MID_TIER=1) the same"""
    contigs, rd, exp = with_low_error_reads
    assert mapping_three_ways(contigs, rd, exp, monkeypatch, capfd, "list tiers", **KW) == ((1, 12), {8192: 6, 16384: 6}, 0)
    assert mapping_three_ways(contigs, rd, exp, monkeypatch, capfd, "list tiers behind the 512-thread tier",
                              env=(("DH_SEED_NO_MID_TIER", "1"),), **KW) == ((0, 0), {8192: 6, 16384: 6}, 0)


def test_reads_redone_by_the_hbm_staged_join_variant(with_low_error_reads, monkeypatch, capfd):
    """DH_SEED_NO16K=1: the six reads above 8 192 hits go to dhk_seed_big_join"""
    contigs, rd, exp = with_low_error_reads
    assert mapping_three_ways(contigs, rd, exp, monkeypatch, capfd, "without the 16384-entry tier", env=(("DH_SEED_NO16K", "1"),),
                              **KW) == ((1, 12), {8192: 6}, 12)


def test_more_band_pairs_than_the_middle_tier_holds(monkeypatch, capfd):
    """150 bases of a unit that stands on each of 140 small contigs (alternating strands) at six places of the 400 kb the
    reads come from: a read over one of them has a candidate band pair per copy -- more than 2 x 64, some from fewer than
    2 048 hits: those are redone by the 512-thread block of the same capacity, the others by the 8 192-entry tier"""
    rng = np.random.default_rng(53)
    unit = rng.integers(0, 4, 600).astype(np.uint8)
    g = sim.genome(54, 400_000)
    for i in range(6):
        at = 30_000 + i * 60_000
        g[at:at + 150] = unit[200:350]
    seqs = [g[:195_000], g[200_000:]]
    for c in range(140):
        u = unit if c % 2 == 0 else sim.revcomp(unit)
        seqs.append(np.concatenate([rng.integers(0, 4, 300).astype(np.uint8), u, rng.integers(0, 4, 300).astype(np.uint8)]))
    contigs = sim.SeqDb.from_list(seqs)
    rd, _ = sim.reads(55, g, 150, 5000, 0, min_len=5000)
    kw = dict(KW, tcap=400, max_cand=256)
    exp = oracle_seeds(contigs, rd, **kw)
    hits, pairs = per_read(exp[2]), per_read(exp[1])
    assert exp[1].max() < 256  # (nothing cut: the candidates are the band pairs)
    by_pairs = int(((pairs > 128) & (hits <= 2048)).sum())
    over = int(((pairs > 128) | (hits > 2048)).sum())
    assert by_pairs >= 3 and hits.max() <= 8192 and over * 4 < rd.n, (by_pairs, over)
    counts, tiers, big = mapping_three_ways(contigs, rd, exp, monkeypatch, capfd, "band pairs", **kw)
    assert counts == (1, over) and tiers == {2048: by_pairs, 8192: over - by_pairs} and big == 0


# ------------------------------------------------------------------------------------------------------------ pile-up join
@pytest.fixture(scope="module")
def deep_piles():
    """four pile-ups of 1 to 14 reads and a fifth one, 260 reads of 1 kb over 1.3 kb: an item meets more than 64 partners"""
    g = sim.genome(81, 1300)
    deep, _ = sim.reads(82, g, 260, 1000, 0, min_len=1000)
    return grouped_piles(extra=(deep, 5))


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("is_grouped", [True, False], ids=["grouped", "ungrouped"])
def test_pile_up_join(ctx, deep_piles, monkeypatch, algo, is_grouped):
    """A == B, skip_self 2: the per-pile-up k-mer join (a grouped DB) against the directory lookups (DH_NO_JOIN=1, and the
    same sequences without groups, where the reads of different pile-ups share what chance gives them)"""
    p = deep_piles if is_grouped else sim.SeqDb(deep_piles.bases, deep_piles.off)
    kw = dict(k=14, algo=algo, width=64 if algo else 30, skip_self=2, max_cand=48, tcap=400)
    exp = oracle_seeds(p, p, **kw)
    uncut = oracle_seeds(p, p, **dict(kw, max_cand=256))
    assert (uncut[1] > 64).sum() >= 20 and uncut[1].max() < 256 and (exp[1] == 48).sum() >= 20
    reset(ctx)
    check(ctx, p, p, exp, f"pile-up join, algo {algo}", **kw)
    assert (ctx.join_counts()[0] >= 1) == is_grouped
    monkeypatch.setenv("DH_NO_JOIN", "1")
    reset(ctx)
    check(ctx, p, p, exp, f"pile-up DB by the directory, algo {algo}", **kw)
    assert ctx.join_counts()[0] == 0


# -------------------------------------------------------------------------------------------------------------- table join
def tj_palindromes():
    """test_parity_tjoin_gpu.test_the_t_cap_and_palindromes: a unit repeated 8 times and AAAAAAATTTTTTT 3 and 6 times at tcap 4"""
    pal = sim.encode("AAAAAAATTTTTTT")
    t0 = sim.genome(42, 2000)
    t0[600:920] = np.tile(sim.genome(41, 40), 8)
    t1 = sim.genome(43, 2000)
    for p in (300, 900, 1500):
        t1[p:p + 14] = pal
    t2 = sim.genome(44, 2000)
    for p in (200, 500, 800, 1100, 1400, 1700):
        t2[p:p + 14] = pal
    tseq, rseq, rgrp = [t0, t1, t2], [], []
    for g, t in enumerate(tseq):
        rs, _ = copies(50 + g, t, 8, 0.05)
        rseq += rs
        rgrp += [g] * len(rs)
    return grouped(tseq, [0, 1, 2]), grouped(rseq, rgrp)


@pytest.mark.parametrize("which,kw", [("base", dict(k=14)), ("base", dict(k=16)), ("base", dict(k=14, kmer_mod=4)),
                                      ("base", dict(k=14, strands=1)), ("base", dict(k=14, strands=2)),
                                      ("n", dict(k=14, algo=0, width=30)), ("palindromes", dict(k=14, tcap=4))])
def test_table_join(fresh_ctx, monkeypatch, which, kw):
    ctx = fresh_ctx
    A, B = tj_palindromes() if which == "palindromes" else tj_base_case(with_n=which == "n")
    kw = dict(TJ_BASE, **kw)
    exp = oracle_seeds(A, B, **kw)
    assert exp[1].sum() > B.n // 4
    reset(ctx)
    check(ctx, A, B, exp, f"table join, {which}", **kw)
    calls, fallbacks, hits, _ = ctx.tjoin_counts()
    assert (calls, fallbacks, hits) == (1, 0, int(exp[2].sum()))
    monkeypatch.setenv("DH_NO_TJOIN", "1")
    reset(ctx)
    check(ctx, A, B, exp, f"grouped DBs by the directory, {which}", **kw)
    assert ctx.tjoin_counts() == (0, 0, 0, 0)


# ------------------------------------------------------------------------------------------------------------ index shapes
@pytest.mark.parametrize("pbits", ["10", None])
def test_directory_with_long_buckets(ctx, monkeypatch, pbits):
    """DH_INDEX_PBITS=10: 1 024 buckets for 150 000 k-mers -- nearly every fat word names a bucket of several entries that
    the lookup walks -- and the default (about a bucket per k-mer) on the same input"""
    w = sim.Workload(150_000, 2, 60, 3000, seed=321, spacing=60_000)
    kw = dict(k=14, algo=1, width=64)
    exp = oracle_seeds(w.contigs, w.reads, **kw)
    assert exp[1].sum() >= w.reads.n
    if pbits:
        monkeypatch.setenv("DH_INDEX_PBITS", pbits)
    reset(ctx)
    check(ctx, w.contigs, w.reads, exp, f"DH_INDEX_PBITS={pbits}", **kw)
    assert ctx.mjoin_counts() == (0, 0)
    check(ctx, w.contigs, w.reads, oracle_seeds(w.contigs, w.reads, **dict(kw, kmer_mod=4)), f"DH_INDEX_PBITS={pbits}, kmer_mod 4",
          **dict(kw, kmer_mod=4))


@pytest.mark.parametrize("switch", ["DH_INDEX_LDS_MIN", "DH_INDEX_ATOMICS"])
def test_grouped_index(ctx, monkeypatch, switch):
    """the index of a grouped DB counted group by group in LDS (DH_INDEX_LDS_MIN=0) and by the generic passes (DH_INDEX_ATOMICS=1)"""
    p = grouped_piles()
    kw = dict(k=14, algo=1, width=64, skip_self=2, max_cand=128)
    monkeypatch.setenv("DH_NO_JOIN", "1")
    monkeypatch.setenv(switch, "0" if switch == "DH_INDEX_LDS_MIN" else "1")
    reset(ctx)
    check(ctx, p, p, oracle_seeds(p, p, **kw), switch, **kw)
    assert ctx.join_counts()[0] == 0
