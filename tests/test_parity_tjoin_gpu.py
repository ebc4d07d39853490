"""The per-group k-mer table join that seeds a grouped template DB against a grouped read DB (csrc/dh_tjoin.h; the
consensus re-alignment of `dentist process`) against the directory lookups it replaces (DH_NO_TJOIN=1) and against the
CPU oracle -- bit exact: the same hits per read, hence the same candidates, records and trace values.
dh_get_tjoin_counts tells which path ran.

The candidates themselves, item by item: tests/test_parity_seedstage_gpu.py."""
import os
import re

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from oracle import pyoracle as oz
from test_join_capacity_gpu import canon, assert_same
from test_parity_map_gpu import both_opts

pytestmark = pytest.mark.gpu

BASE = dict(algo=1, width=64, tspace=126, min_len=500, max_la=4, max_cand=32)


def copies(seed, template, n, err):
    """n reads that are copies of `template` with `err` errors, both orientations; (list of reads, strands)"""
    rd, truth = sim.reads(seed, template, n, len(template), err=err)
    return [rd.bases[rd.off[i]:rd.off[i + 1]].copy() for i in range(rd.n)], truth[:, 2]


def grouped(seqs, groups):
    order = np.argsort(np.asarray(groups), kind="stable")
    return sim.SeqDb.from_list([seqs[i] for i in order], group=np.asarray(groups, dtype=np.int32)[order])


def three_ways(ctx, A, B, monkeypatch, expect=(1, 0), reruns=None, **kw):
    """a = the call as it is (expect: calls seeded by the table, calls that fell back), b = DH_NO_TJOIN=1, c = the oracle.
    reruns: None = the hit buffer may have been too small once (the context learns the hits per base as it goes)."""
    g, o = both_opts(**dict(BASE, **kw))
    dA, dB = ctx.db(A), ctx.db(B)
    try:
        ctx.tjoin_counts(reset=True)
        a = canon(ctx.align_db(dA, dB, g))
        calls, fallbacks, hits, rr = ctx.tjoin_counts(reset=True)
        st = ctx.align_stats()
        print(f"reads {B.n}, records {len(a[0][0])}, table join: calls {calls}, fall-backs {fallbacks}, hits {hits}, reruns {rr}")
        assert (calls, fallbacks) == expect and (rr in (0, 1) if reruns is None else rr == reruns)
        assert hits == (st.hits if calls else 0)
        monkeypatch.setenv("DH_NO_TJOIN", "1")
        b = canon(ctx.align_db(dA, dB, g))
        monkeypatch.delenv("DH_NO_TJOIN")
        assert ctx.tjoin_counts() == (0, 0, 0, 0)
        assert ctx.align_stats().hits == st.hits
    finally:
        dA.close()
        dB.close()
    c = canon(oz.align_db(A, B, o, nthreads=os.cpu_count() or 1)[:2])
    assert_same(a, b)
    assert_same(a, c)
    return a, hits


def base_case(with_n=False):
    """groups 0, 1, 3, 4 (no group 2; group 3 has reads and no template); templates of 1 000 - 3 000 bp, group 1 has two;
    6 - 14 reads per group at 13 %; a read shorter than k; a read and a template with a run of N"""
    tlen = {0: 1000, 1: 3000, 3: 1700, 4: 2300}
    nreads = {0: 6, 1: 14, 3: 8, 4: 11}
    tseq, tgrp, rseq, rgrp, strands = [], [], [], [], []
    for g in (0, 1, 3, 4):
        t = sim.genome(500 + g, tlen[g])
        rs, sd = copies(600 + g, t, nreads[g], 0.13)
        if g == 4 and with_n:
            t[1200:1230] = 4
        if g != 3:
            tseq.append(t)
            tgrp.append(g)
        if g == 1:  # the second template of the group and reads of it
            t2 = sim.genome(777, 1500)
            tseq.append(t2)
            tgrp.append(g)
            more, sd2 = copies(778, t2, 5, 0.13)
            rs, sd = rs + more, np.concatenate([sd, sd2])
        if g == 0:
            if with_n:
                rs[2][400:425] = 4
            rs.append(sim.genome(9, 9))  # shorter than k
            sd = np.concatenate([sd, [0]])
        rseq += rs
        rgrp += [g] * len(rs)
        strands.append(sd)
    strands = np.concatenate(strands)
    assert (strands == 0).sum() >= 5 and (strands != 0).sum() >= 5
    return grouped(tseq, tgrp), grouped(rseq, rgrp)


@pytest.mark.parametrize("k,kmer_mod,strands", [(14, 1, 3), (16, 1, 3), (14, 4, 3), (14, 1, 1), (14, 1, 2)])
def test_base_shapes(gpu_ctx, monkeypatch, k, kmer_mod, strands):
    A, B = base_case()
    a, _ = three_ways(gpu_ctx, A, B, monkeypatch, k=k, kmer_mod=kmer_mod, strands=strands)
    las = a[0]
    assert len(las[0]) >= (B.n - 9) // (2 if strands != 3 else 1) // 2
    grpA, grpB = A.group[las[7]], B.group[las[8]]
    assert np.array_equal(grpA, grpB) and 3 not in grpB  # a read only meets the templates of its own group


@pytest.mark.parametrize("k,kmer_mod,strands", [(14, 1, 3), (16, 1, 3), (14, 4, 3), (14, 1, 1), (14, 1, 2)])
def test_runs_of_n(gpu_ctx, monkeypatch, k, kmer_mod, strands):
    """The base shapes with a run of N in a template and in a read: a k-mer with an N is neither indexed nor probed.  The
    tiled band (algo 1) takes sequences of a, c, g, t only, so this case runs the wave extension (algo 0) behind the same
    seeds; everything else as above."""
    A, B = base_case(with_n=True)
    assert (A.bases == 4).sum() == 30 and (B.bases == 4).sum() == 25
    three_ways(gpu_ctx, A, B, monkeypatch, k=k, kmer_mod=kmer_mod, strands=strands, algo=0,
               width=dentist_amd.default_align_opts().width)


def test_the_t_cap_and_palindromes(gpu_ctx, monkeypatch):
    """tcap = 4: a 40-base unit repeated 8 times (k-mers with 8 copies in one orientation: skipped), AAAAAAATTTTTTT (its own
    reverse complement at k = 14: it counts and emits on both strands) planted 3 times (under the cap) and 6 times (above);
    reads at 5 %"""
    pal = sim.encode("AAAAAAATTTTTTT")
    unit = sim.genome(41, 40)
    t0 = sim.genome(42, 2000)
    t0[600:920] = np.tile(unit, 8)
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
    three_ways(gpu_ctx, grouped(tseq, [0, 1, 2]), grouped(rseq, rgrp), monkeypatch, k=14, tcap=4)


def test_tiers(monkeypatch, capfd):
    """a 6 000 bp template with 8 reads at 1 % (thousands of hits per read) next to groups at 13 %: the mean selects the
    wavefront-per-read tier (512 entries), the reads above it go through the 2 048- and the 8 192-entry tiers from lists
    (the library's trace says how many went where).  A context of its own: the first tier is switched off per context when
    a quarter of a chunk overflows it."""
    tseq, rseq, rgrp = [], [], []
    for g in range(9):
        t = sim.genome(70 + g, 6000 if g == 0 else (1000 if g < 7 else 4000))
        rs, _ = copies(80 + g, t, 8 if g == 0 else (50 if g < 7 else 4), 0.01 if g == 0 else 0.13)
        tseq.append(t)
        rseq += rs
        rgrp += [g] * len(rs)
    A, B = grouped(tseq, list(range(9))), grouped(rseq, rgrp)
    ctx = dentist_amd.Context(0)
    try:
        three_ways(ctx, A, B, monkeypatch, k=14)
        g, _ = both_opts(**dict(BASE, k=14))
        dA, dB = ctx.db(A), ctx.db(B)
        try:
            monkeypatch.setenv("DH_TRACE", "1")
            capfd.readouterr()
            ctx.align_db(dA, dB, g)
            err = capfd.readouterr().err
            monkeypatch.delenv("DH_TRACE")
            st = ctx.align_stats()
            hits = ctx.tjoin_counts()[2]
        finally:
            dA.close()
            dB.close()
        assert 1.5 * hits / B.n <= 512, "precondition: the mean selects the 512-entry tier"
        assert st.hits == hits and hits > 8 * 8192 // 2  # the low-error reads bring several thousand hits each
        first = re.search(r"\[seeds\] cap \d+: (\d+) of (\d+) reads overflow", err)
        tiers = {int(t): int(n) for n, t in re.findall(r"join tiers: (\d+) reads redone with (\d+) entries", err)}
        print(f"hits {hits}, overflowed the first tier: {first.group(1) if first else None}, tiers {tiers}")
        assert first and int(first.group(2)) == B.n and int(first.group(1)) >= 9
        assert tiers.get(2048, 0) >= 1 and tiers.get(8192, 0) == 8  # the 4 000 bp reads at 13 %; the eight reads at 1 %
        assert int(first.group(1)) == tiers[2048] + tiers[8192] and st.big_items == 0
    finally:
        ctx.close()


def test_soft_masks(gpu_ctx, monkeypatch):
    """a masked stretch on a template and on a read: a k-mer touching it is neither indexed nor probed"""
    tseq, rseq, rgrp = [], [], []
    for g in range(3):
        t = sim.genome(90 + g, 2000)
        rs, _ = copies(95 + g, t, 8, 0.13)
        tseq.append(t)
        rseq += rs
        rgrp += [g] * len(rs)
    A, B = grouped(tseq, [0, 1, 2]), grouped(rseq, rgrp)
    _, free_hits = three_ways(gpu_ctx, A, B, monkeypatch, k=14)

    def with_mask(db, ivs):
        ptr = np.zeros(db.n + 1, dtype=np.int64)
        iv = []
        for s in range(db.n):
            iv += ivs.get(s, [])
            ptr[s + 1] = len(iv) // 2
        db.mask = (ptr, np.asarray(iv + [0, 0], dtype=np.int32))
        return db

    Am = with_mask(sim.SeqDb(A.bases, A.off, A.group), {1: [300, 1700]})
    Bm = with_mask(sim.SeqDb(B.bases, B.off, B.group), {2: [0, 1500], 20: [100, 1900]})
    _, masked_hits = three_ways(gpu_ctx, Am, Bm, monkeypatch, k=14)
    assert 0 < masked_hits < free_hits


def test_hit_buffer_rerun(gpu_ctx, monkeypatch):
    """DH_TJOIN_HITCAP=1024: the first attempt's buffer is too small, the cursor says what is needed, one rerun, same results"""
    A, B = base_case()
    monkeypatch.setenv("DH_TJOIN_HITCAP", "1024")
    three_ways(gpu_ctx, A, B, monkeypatch, reruns=1, k=14)


def test_capacity_fall_back(gpu_ctx, monkeypatch):
    """DH_TJOIN_CAP below the entries of the largest group: the call keeps the directory and is counted, same results"""
    A, B = base_case()
    monkeypatch.setenv("DH_TJOIN_CAP", "2000")
    three_ways(gpu_ctx, A, B, monkeypatch, expect=(0, 1), k=14)
