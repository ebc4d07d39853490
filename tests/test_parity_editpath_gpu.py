"""Base-level alignments from trace points (dh_la_edit_paths: k_edit_fast / k_edit_general, dh_editpath.hip) against the
oracle: every record is cut into its trace tiles in plain Python and every tile aligned by oracle/nw.c (findAlignment with
indel 1, no free shift, and its traceback rule: util/string.d:478-520, 775-831; getExactAlignment's per-trace-point part,
dazzler.d:2405-2426).  Bit-exact: every op, every tile score, every record score."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib, sim
from oracle import pyoracle as oz

pytestmark = pytest.mark.gpu

T = dict(algo=1, width=64)


def oracle_record(la, trace, ts, A, B, rc_cache):
    """(ops 0/1/2/3, tile scores) of one record from the oracle, tile by tile"""
    a = A.seq(int(la["aread"]))
    br = int(la["bread"])
    if la["flags"] & 1:
        if br not in rc_cache:
            rc_cache[br] = sim.revcomp(B.seq(br))
        b = rc_cache[br]
    else:
        b = B.seq(br)
    tr = trace[la["toff"]:la["toff"] + la["tlen"]].reshape(-1, 2)
    ap, bp, aepos = int(la["abpos"]), int(la["bbpos"]), int(la["aepos"])
    ops, scores = [], []
    for _, bb in tr:
        a1 = min((ap // ts + 1) * ts, aepos)
        b1 = bp + int(bb)
        at, bt = a[ap:a1], b[bp:b1]
        score, o = oz.nw(at, bt, 1, False)
        o = o.copy()
        i = j = 0
        for k, op in enumerate(o):  # OZ_OP_SUB -> match (0) / mismatch (3) by base equality
            if op == 0:
                if at[i] != bt[j]:
                    o[k] = 3
                i, j = i + 1, j + 1
            elif op == 1:
                i += 1
            else:
                j += 1
        ops.append(o)
        scores.append(score)
        ap, bp = a1, b1
    assert ap == aepos and bp == int(la["bepos"])
    return (np.concatenate(ops) if ops else np.zeros(0, np.uint8)), scores


def check_against_oracle(ep, las, trace, ts, A, B, first=0):
    rc_cache = {}
    assert len(ep) == len(las) - first
    for i in range(len(ep)):
        la = las[first + i]
        exp_ops, exp_scores = oracle_record(la, trace, ts, A, B, rc_cache)
        got = ep.ops[ep.op_off[i]:ep.op_off[i + 1]]
        assert np.array_equal(got, exp_ops), f"record {first + i}: ops differ"
        assert ep.tile_score[ep.tile_off[i]:ep.tile_off[i + 1]].tolist() == exp_scores, f"record {first + i}: tile scores"
        assert ep.score[i] == sum(exp_scores) == int(np.count_nonzero(got))
        assert int(np.count_nonzero(got != 2)) == la["aepos"] - la["abpos"]
        assert int(np.count_nonzero(got != 1)) == la["bepos"] - la["bbpos"]


def tile_diffs(las, trace):
    return np.concatenate([trace[l["toff"]:l["toff"] + l["tlen"]:2] for l in las]) if len(las) else np.zeros(0, np.uint16)


def same_result(x, y):
    return (x.ops.tobytes() == y.ops.tobytes() and np.array_equal(x.op_off, y.op_off) and np.array_equal(x.score, y.score)
            and np.array_equal(x.tile_off, y.tile_off) and np.array_equal(x.tile_score, y.tile_score))


def mapped(ctx, contigs, reads, same=False, **kw):
    A = ctx.db(contigs)
    B = A if same else ctx.db(reads)
    g = dentist_amd.default_align_opts(**kw, **T)
    las, trace = ctx.align_db(A, B, g)
    return A, B, las, trace, g.tspace


@pytest.fixture(scope="module")
def mapping_workload():
    return sim.Workload(150_000, 2, 250, 3000, seed=61, spacing=15000)


@pytest.fixture(scope="module")
def mapping100(gpu_ctx, mapping_workload):
    """the mapping case at tspace 100, its edit paths (computed once, never modified) and the oracle check done"""
    w = mapping_workload
    A, B, las, trace, ts = mapped(gpu_ctx, w.contigs, w.reads, tspace=100)
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    return w, A, B, las, trace, ep


@pytest.mark.parametrize("ts", [100, 126, 64])
def test_mapping_every_record_of_both_strands(gpu_ctx, mapping_workload, ts):
    w = mapping_workload
    A, B, las, trace, _ = mapped(gpu_ctx, w.contigs, w.reads, tspace=ts)
    assert len(las) >= w.reads.n and set((las["flags"] & 1).tolist()) == {0, 1}
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    check_against_oracle(ep, las, trace, ts, w.contigs, w.reads)
    assert np.all(ep.tile_score <= tile_diffs(las, trace))
    assert ep.general_tiles == 0, "a trace of DH-2 understated a tile's edit distance"


def test_band_classes_high_error_reads(gpu_ctx):
    w = sim.Workload(250_000, 3, 250, 4000, seed=13, err=0.20, spacing=15000)
    A, B, las, trace, ts = mapped(gpu_ctx, w.contigs, w.reads, tspace=100)
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    check_against_oracle(ep, las, trace, ts, w.contigs, w.reads)
    d = tile_diffs(las, trace)
    assert np.all(ep.tile_score <= d) and ep.general_tiles == 0
    assert np.count_nonzero((d + 1 > 31) & (d + 1 <= 63)) > 0, "no tile took the two-word class"


def test_band_classes_ont_like_profile(gpu_ctx):
    g = sim.genome(97, 600_000)
    gb, ge = sim.gaps(98, len(g), 3, 50, 3000, 20000)
    contigs, _ = sim.contigs_from_gaps(g, gb, ge)
    reads, _ = sim.reads(99, g, 240, 20000, 0, err=0.10, p_ins=0.30, p_del=0.40)
    A, B, las, trace, ts = mapped(gpu_ctx, contigs, reads, k=20, kmer_mod=4)
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    check_against_oracle(ep, las, trace, ts, contigs, reads)
    d = tile_diffs(las, trace)
    assert np.all(ep.tile_score <= d) and ep.general_tiles == 0
    assert np.count_nonzero(d + 1 <= 31) > 0


def test_short_and_ragged_inputs(gpu_ctx):
    """One-tile records, a first tile of a few bases, a read equal to its contig, tiles that end at a sequence end (the
    kernel's unaligned 8-byte loads rely on the DBs' padding there)."""
    rng = np.random.default_rng(11)
    g = rng.integers(0, 4, 6000).astype(np.uint8)
    contigs = sim.SeqDb.from_list([g[:3000], g[3100:3160], g[3200:6000], g[100:140]])
    reads = sim.SeqDb.from_list([g[2900:3000], g[2950:3160], g[0:3000], g[3150:3300], g[10:70], sim.revcomp(g[3300:5900]),
                                 g[3100:3160], g[2990:3110], g[20:52], g[0:0], g[5:12]])
    A, B, las, trace, ts = mapped(gpu_ctx, contigs, reads, k=12, hmin=20, min_len=20)
    assert len(las) >= 8
    ntiles = las["tlen"] // 2
    assert np.any(ntiles == 1) and np.any(las["aepos"] == contigs.off[las["aread"] + 1] - contigs.off[las["aread"]])
    ep = gpu_ctx.edit_paths(A, B, las, trace, ts)
    check_against_oracle(ep, las, trace, ts, contigs, reads)
    assert ep.general_tiles == 0


def test_symmetric_pile_up_both_records_of_a_pair(gpu_ctx):
    g = sim.genome(21, 20000)
    reads, _ = sim.reads(22, g, 30, 6000)
    A, _, las, trace, ts = mapped(gpu_ctx, reads, reads, same=True, tspace=126, skip_self=2, min_len=500, max_la=64,
                                  max_cand=128)
    key = set(zip(las["aread"].tolist(), las["bread"].tolist(), (las["flags"] & 1).tolist()))
    assert len(las) > reads.n and all((b, a, c) in key for a, b, c in key) and any(c for _, _, c in key)
    ep = gpu_ctx.edit_paths(A, A, las, trace, ts)
    check_against_oracle(ep, las, trace, ts, reads, reads)
    assert ep.general_tiles == 0


def test_general_path_understated_diffs_give_identical_results(gpu_ctx, mapping100):
    w, A, B, las, trace, ep = mapping100
    check_against_oracle(ep, las, trace, 100, w.contigs, w.reads)
    zero = trace.copy()
    zero[0::2] = 0  # (every record's toff is even: pairs start at even indices)
    assert np.all(las["toff"] % 2 == 0)
    ep0 = gpu_ctx.edit_paths(A, B, las, zero, 100)
    assert same_result(ep0, ep)
    assert ep0.general_tiles == int(np.count_nonzero(ep.tile_score)) > 0 and ep.general_tiles == 0


def _one_record(aread, bread, alen, blen, diffs, toff):
    la = np.zeros(1, dtype=dentist_amd.LA_DTYPE)
    la[0]["aread"], la[0]["bread"] = aread, bread
    la[0]["aepos"], la[0]["bepos"] = alen, blen
    la[0]["tlen"], la[0]["toff"], la[0]["diffs"] = 2, toff, diffs
    return la


def test_general_path_hand_made_tiles(gpu_ctx):
    rng = np.random.default_rng(5)
    a100 = rng.integers(0, 4, 100).astype(np.uint8)
    b180 = a100.tolist()
    for _ in range(80):
        b180.insert(int(rng.integers(0, len(b180) + 1)), int(rng.integers(0, 4)))
    b180 = np.asarray(b180, dtype=np.uint8)
    u100, v100 = rng.integers(0, 4, 100).astype(np.uint8), rng.integers(0, 4, 100).astype(np.uint8)
    a250, b1000 = rng.integers(0, 4, 250).astype(np.uint8), rng.integers(0, 4, 1000).astype(np.uint8)
    adb, bdb = sim.SeqDb.from_list([a100, u100, a250]), sim.SeqDb.from_list([b180, v100, b1000])
    A, B = gpu_ctx.db(adb), gpu_ctx.db(bdb)
    # band 81 fits no class; a band of 6 that the tile's ~50 differences do not fit
    las = np.concatenate([_one_record(0, 0, 100, 180, 80, 0), _one_record(1, 1, 100, 100, 5, 2)])
    las[1]["flags"] = 1  # ... against the reverse complement
    trace = np.asarray([80, 180, 5, 100], dtype=np.uint16)
    ep = gpu_ctx.edit_paths(A, B, las, trace, 100)
    check_against_oracle(ep, las, trace, 100, adb, bdb)
    assert ep.general_tiles == 2 and ep.score[0] == 80 and ep.score[1] > 5
    # a tile at the caps: tspace = 250, 1 000 B bases
    las = _one_record(2, 2, 250, 1000, 750, 0)
    trace = np.asarray([750, 1000], dtype=np.uint16)
    ep = gpu_ctx.edit_paths(A, B, las, trace, 250)
    check_against_oracle(ep, las, trace, 250, adb, bdb)
    assert ep.general_tiles == 1 and 750 <= ep.score[0] <= 1000


def test_refusals_without_a_launch(gpu_ctx, mapping100):
    w, A, B, las, trace, ep = mapping100

    def refused(l, t, ts=100, a=A, b=B, match=None):
        with pytest.raises(dentist_amd.DhError, match=match) as ei:
            gpu_ctx.edit_paths(a, b, l, t, ts)
        assert ei.value.code == -1  # DH_EINVAL
        again = gpu_ctx.edit_paths(A, B, las, trace, 100, first=0, count=1)  # the context is usable afterwards
        assert again.ops.tobytes() == ep.ops[:ep.op_off[1]].tobytes() and again.score[0] == ep.score[0]

    k = int(np.argmax(las["tlen"] >= 4))
    one = las[k:k + 1].copy()
    bad = trace.copy()
    bad[one[0]["toff"] + 1] += 1  # the B bases no longer sum to bepos - bbpos
    refused(one, bad, match="LA 0")
    odd = one.copy()
    odd[0]["tlen"] -= 1
    refused(odd, trace, match="tlen")
    far = one.copy()
    far[0]["aepos"] = w.contigs.length(int(one[0]["aread"])) + 1  # past the sequence
    refused(far, trace, match="outside")
    fewer = one.copy()
    fewer[0]["tlen"] -= 2  # a tile count that disagrees with abpos / aepos
    refused(fewer, trace, match="trace points")
    rng = np.random.default_rng(6)
    adb = sim.SeqDb.from_list([rng.integers(0, 4, 100).astype(np.uint8)])
    bdb = sim.SeqDb.from_list([rng.integers(0, 4, 500).astype(np.uint8)])
    refused(_one_record(0, 0, 100, 401, 300, 0), np.asarray([300, 401], dtype=np.uint16), a=gpu_ctx.db(adb), b=gpu_ctx.db(bdb),
            match="LA 0 tile 0")
    refused(one, trace, ts=251, match="tspace")


def test_handle_range_and_chunk_size(gpu_ctx, mapping100, monkeypatch):
    w, A, B, las, trace, ep = mapping100
    g = dentist_amd.default_align_opts(tspace=100, **T)
    h = gpu_ctx.align_db_block(A, B, 0, w.reads.n, g, raw=True)
    eph = gpu_ctx.edit_paths(A, B, h)
    part = gpu_ctx.edit_paths(A, B, h, first=3, count=5)
    hl, ht, hts = _lib._take_la_set(h)  # (owns the handle from here on)
    assert hts == 100 and same_result(eph, gpu_ctx.edit_paths(A, B, hl, ht, hts))
    check_against_oracle(eph, hl, ht, 100, w.contigs, w.reads)
    assert part.ops.tobytes() == eph.ops[eph.op_off[3]:eph.op_off[8]].tobytes() and np.array_equal(part.score, eph.score[3:8])
    # first / count: the slices of the whole
    n = len(las)
    for first, count in ((0, 1), (n // 3, n // 2), (n - 1, 1), (n, 0)):
        s = gpu_ctx.edit_paths(A, B, las, trace, 100, first=first, count=count)
        assert s.ops.tobytes() == ep.ops[ep.op_off[first]:ep.op_off[first + count]].tobytes()
        assert np.array_equal(s.op_off, ep.op_off[first:first + count + 1] - ep.op_off[first])
        assert np.array_equal(s.score, ep.score[first:first + count])
        assert np.array_equal(s.tile_score, ep.tile_score[ep.tile_off[first]:ep.tile_off[first + count]])
    monkeypatch.setenv("DH_EDIT_CHUNK", "37")
    assert same_result(gpu_ctx.edit_paths(A, B, las, trace, 100), ep)
    zero = trace.copy()
    zero[0::2] = 0
    assert same_result(gpu_ctx.edit_paths(A, B, las, zero, 100), ep)  # both kernels in every chunk
