"""BASELINE configs[2] -- the size bench.py times: 100 Mb assembly, 1 000 gaps, 1 M x 15 kb reads, 15.7 Gbp -- against the
oracle, bit-exact, on a sample.  The code that runs only at this size (the partitioned mapping join above DH_MJOIN_MIN,
the index of 10^8 entries with real multi-entry buckets, two chunks of 2^20 items whose host filters overlap the next
chunk's kernels, read offsets beyond 2^32, k_tile's queue over 2 M items, three concurrent parts of 1 000 pile-ups, the
overflow limits of k_pile_funnel) is otherwise seen by property checks only (test_config2_full_size_properties,
test_config2_bench_chain_at_the_reference_behaviour, test_config3_...): a few hundred reads with one wrong trace pair stay
inside every tolerance there.

Mapping: bench.py's one dh_map_reads call over all reads; the oracle maps a stratified sample of about 4 000 reads
(helpers.fullsize_read_sample: chunk edges, offset wraps, contig extremes, record-count extremes, the members of the
sampled pile-ups, seeded random) against all contigs and filters them -- the six collect filters look at one read at a
time, so filtering a subset is exact.  Every record of every sampled read: nine fields, chain and DISABLED flags, every
trace value.  Process: about 12 pile-ups of the batch of 1 000 (helpers.fullsize_pile_sample: the ends of the batch, the
extremes of entries and gap length, both sides of the cuts between the concurrent parts, seeded random): membership
against oracle/scaffold.py:build on the contigs around the gap, then status, crop points, reference read, every consensus
base and the splice against oracle/process.py on the product's records.  Both identities that make the oracle affordable
here are checked on a small workload in test_fullsize_helpers.py, which also shows each comparison failing on one
altered value.

Property-only at full size after this: the other 99.6 % of the reads, the other 988 pile-ups, and configs[4] (no oracle at
that size: test_configs_gpu.py).

Measured on one MI355X with 16 CPU threads for the oracle: 43 s for the four tests when the file runs alone (10 s of
that the workload, the mapping and the pile-ups of the shared fixture), about 33 s inside the whole `-m gpu` run, which
then takes 224 s for 194 tests (219 s for 190 before).  Mapping, kmer_mod 1: 4 696 reads, 7 066 records, 1.34 M trace
values; oracle index of the 100 Mb assembly 3.8 - 4.1 s, index + sample 5.3 - 5.7 s.  kmer_mod 8: index 1.3 s, index + sample
2.2 s.  Process, uncapped: 12 pile-ups of 121 .. 228 entries in 12 s of oracle time; at 60 reads: 10 pile-ups in 2.4 s.  The GPU
side of every leg is well under a second once its buffers exist.  (The oracle is far quicker than its rate on 256 cores
suggested, so nothing of the sample had to be halved: the sample is not the
cost, the workload is.)"""
import os
import time
from types import SimpleNamespace

import numpy as np
import pytest

import dentist_amd
import helpers as hp
from oracle import collect_filters as cf
from oracle import process as pr
from oracle import pyoracle as oz

pytestmark = pytest.mark.gpu

NTHREADS = min(16, os.cpu_count() or 1)     # what a command on a GPU box may use, not the machine's core count
MAP = dict(k=20, width=64, xdrop=60, algo=1)   # bench.py's mapping options; kmer_mod 1 is the headline, 8 the fast mode
SEED = 20261016
SAMPLE = 2000                                # reads beyond the members of the sampled pile-ups
CAPS = (0, 60)                               # dh_process_opts.max_reads: the reference's behaviour, bench.py's fast mode


def gap_inputs(w):
    return np.stack([np.arange(w.contigs.n - 1), np.arange(1, w.contigs.n)], axis=1).astype(np.int32)


@pytest.fixture(scope="module")
def mapped(gpu_ctx, cfg2_workload):
    """The mapping at kmer_mod 1 (one dh_map_reads call, as bench.py), its scaffold-graph pile-ups at both read caps and
    the pile-ups sampled from them: shared by the mapping test and the process test."""
    w = cfg2_workload
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    mo = dentist_amd.default_align_opts(kmer_mod=1, **MAP)
    po = dentist_amd.default_process_opts(algo=1, max_reads=0, max_partners=0)
    gpu_ctx.mjoin_counts(reset=True)
    t0 = time.perf_counter()
    las, trace = gpu_ctx.map_reads(A, B, mo, po, sorted=False, candidates=False)[:2]
    t_map = time.perf_counter() - t0
    st = gpu_ctx.align_stats()
    # the chunk edges of the sample follow align_range's rule (2^20 items, two per read): one k_tile launch per chunk
    assert st.wave_launches == len(hp.chunk_bounds(w.reads.n)) == 2, st.as_dict()
    assert gpu_ctx.mjoin_counts()[0] > 0, "the partitioned join did not run"
    gp, _ = dentist_amd.scaffold_spanning_pileups(las, w.contigs.off, w.reads.off, gap_inputs(w), with_extensions=True,
                                                  min_spanning_reads=po.min_reads)
    m = SimpleNamespace(A=A, B=B, las=las, trace=trace, t_map=t_map, piles={}, entries={}, sample={})
    glen = np.asarray(w.gap_end - w.gap_begin)
    for cap in CAPS:
        piles = gp.select(las, dentist_amd.default_process_opts(algo=1, max_reads=cap, max_partners=0))
        cl, cnt, tri = piles.flat()
        assert len(cl) == 1000 and np.array_equal(cl, np.arange(1000))
        at = np.concatenate([[0], np.cumsum(cnt)])
        m.piles[cap] = piles
        m.entries[cap] = [[tuple(int(x) for x in t) for t in tri[at[p]:at[p + 1]].tolist()] for p in range(len(cl))]
        m.sample[cap] = hp.fullsize_pile_sample(cnt, glen[cl], np.random.default_rng(SEED + cap))
    # stratum 5 of the read sample: every entry of a sampled pile-up, before the cap (the capped entries are among them)
    m.pile_reads = np.unique([t[0] for cap in CAPS for p in m.sample[cap].values() for t in m.entries[0][p]])
    yield m
    del m.A, m.B


@pytest.mark.parametrize("kmer_mod", [1, 8])
def test_sampled_reads_of_the_full_size_mapping_equal_the_oracle(gpu_ctx, cfg2_workload, mapped, kmer_mod, capsys):
    w = cfg2_workload
    if kmer_mod == 1:
        las, trace, t_map = mapped.las, mapped.trace, mapped.t_map
    else:
        mo = dentist_amd.default_align_opts(kmer_mod=kmer_mod, **MAP)
        po = dentist_amd.default_process_opts(algo=1)
        mapped.A.drop_cache()
        mapped.B.drop_cache()
        t0 = time.perf_counter()
        las, trace = gpu_ctx.map_reads(mapped.A, mapped.B, mo, po, sorted=False, candidates=False)[:2]
        t_map = time.perf_counter() - t0
        assert gpu_ctx.align_stats().wave_launches == 2
        mapped.A.drop_cache()    # (the process test runs on the index of kmer_mod 1)
    ids, counts, wrapped = hp.fullsize_read_sample(w, las, np.random.default_rng(SEED), pile_reads=mapped.pile_reads, size=SAMPLE)
    assert len(ids) == SAMPLE + counts["pile-up members"] and set(mapped.pile_reads.tolist()) <= set(ids.tolist())
    for s in hp.STRATA:
        assert counts[s] > 0 or s == "record count", counts
    # the reads that hold byte 2^32, 2 * 2^32 and 3 * 2^32 of the DB
    assert int(w.reads.off[-1]) > 3 << 32
    straddle = [int(np.searchsorted(w.reads.off, m << 32, side="right")) - 1 for m in (1, 2, 3)]
    assert set(straddle) <= set(wrapped.tolist()) <= set(ids.tolist()), (straddle, wrapped)
    # ---- the oracle on the sample: every contig, the sampled reads, then the six filters
    sub = hp.sub_db(w.reads, ids)
    oo = oz.default_opts(kmer_mod=kmer_mod, **MAP)
    t0 = time.perf_counter()
    oz.align_db(w.contigs, hp.sub_db(w.reads, ids[:1]), oo, nthreads=NTHREADS, sort=False, select_best=True)
    t_index = time.perf_counter() - t0    # a call with a single read is the index build plus one alignment
    t0 = time.perf_counter()
    olas, otrace, _ = oz.align_db(w.contigs, sub, oo, nthreads=NTHREADS, sort=False, select_best=True)
    t_oracle = time.perf_counter() - t0
    flas, _, _ = cf.collect_filter(olas, w.contigs.off, sub.off)
    nrec, ntr = hp.assert_same_las_of_reads((las, trace), (flas, otrace), ids)
    assert nrec > len(ids) // 2
    with capsys.disabled():
        print(f"\n[configs[2], kmer_mod {kmer_mod}] {len(ids)} of {w.reads.n} reads against the oracle: "
              + ", ".join(f"{s} {c}" for s, c in counts.items())
              + f"; offset wraps in reads {wrapped.tolist()}; {nrec} records ({int((flas['flags'] & 0x20 != 0).sum())} DISABLED, "
              f"{int(np.bincount(flas['bread'], minlength=len(ids)).max())} at most per read) and {ntr} trace values equal; "
              f"GPU mapping of all reads {t_map:.1f} s incl. first-use allocations; oracle on {NTHREADS} threads: index "
              f"{t_index:.1f} s, sample {t_oracle:.1f} s incl. index")


@pytest.mark.parametrize("max_reads", CAPS)
def test_sampled_pile_ups_of_the_full_size_run_equal_the_oracle(gpu_ctx, cfg2_workload, mapped, max_reads, capsys):
    w = cfg2_workload
    las, trace = mapped.las, mapped.trace
    po = dentist_amd.default_process_opts(algo=1, max_reads=max_reads, max_partners=0)
    assert po.rounds == 3
    piles, sample = mapped.piles[max_reads], mapped.sample[max_reads]
    assert len(set(sample.values())) >= 6
    t0 = time.perf_counter()
    rec, bases = dentist_amd.process_pileups(gpu_ctx, mapped.A, mapped.B, las, trace, piles, po)
    t_gpu = time.perf_counter() - t0
    assert len(rec) == len(piles) == 1000
    lines, ok, t_oracle = [], 0, 0.0
    for p in sorted(set(sample.values())):
        g, tri = piles.get(p)
        got = [tuple(int(x) for x in t) for t in tri.tolist()]
        assert got == mapped.entries[max_reads][p] and rec[p]["contig_left"] == g
        assert set(t[0] for t in got) <= set(mapped.pile_reads.tolist())   # (their records are pinned by the mapping test)
        # ---- membership: the oracle's graph builder on the contigs around the gap, then the cap
        exp = hp.cap_entries(hp.restricted_gap_entries(las, w.contigs, w.reads, g, po.min_reads, window=1), las, max_reads)
        assert got == exp, f"pile-up {p} (gap {g}): entries differ"
        # ---- process: the oracle's driver on the product's records
        t0 = time.perf_counter()
        ex = pr.process_pile(got, las, trace, w.contigs, w.reads, g, rounds=po.rounds, nthreads=NTHREADS, algo=1)
        t_oracle += time.perf_counter() - t0
        status = hp.assert_same_insertion(rec[p], bases, ex)
        ok += status == "ok"
        lines.append(f"  pile-up {p:3d} ({', '.join(k for k, v in sample.items() if v == p)}): {len(got)} entries, "
                     f"{ex['pile'].n if 'pile' in ex else 0} reads, gap of {int(w.gap_end[g] - w.gap_begin[g])}: {status}")
    with capsys.disabled():
        print(f"\n[configs[2], max_reads {max_reads}] {len(lines)} of 1 000 pile-ups against the oracle (process on the GPU "
              f"{t_gpu:.1f} s, oracle on {NTHREADS} threads {t_oracle:.1f} s):\n" + "\n".join(lines))
    assert ok >= len(lines) - 1, "the sample must end in insertions"
