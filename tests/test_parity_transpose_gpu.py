"""Exact transposition of local alignments (dh_la_transpose: k_trace_transpose / k_trace_pairs, dh_editpath.hip) against the
plain restatement in tests/transpose_ref.py, which walks the ops of Context.edit_paths (pinned to the oracle op for op by
tests/test_parity_editpath_gpu.py) record by record.  Bit-exact: all nine record fields, every trace value, src_index."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import _lib, sim
from helpers import FIELDS, check_trace_invariants

import transpose_ref as tr

pytestmark = pytest.mark.gpu

T = dict(algo=1, width=64)
CHAIN = 0x4 | 0x8 | 0x10  # START, NEXT, BEST
CONDITIONS = ("abpos_on_grid", "aepos_on_grid", "code2_after_crossing", "single_tile")


def lengths(db):
    return np.diff(np.asarray(db.off, dtype=np.int64))


def mapped(ctx, contigs, reads, same=False, **kw):
    A = ctx.db(contigs)
    B = A if same else ctx.db(reads)
    g = dentist_amd.default_align_opts(**kw, **T)
    las, trace = ctx.align_db(A, B, g)
    return A, B, las, trace, g.tspace


def assert_same_set(got, exp):
    (gl, gt, gs), (el, et, es) = got, exp
    assert len(gl) == len(el)
    for f in FIELDS:
        assert np.array_equal(gl[f], el[f]), f
    assert np.array_equal(gs, es)
    for i, (x, y) in enumerate(zip(gl, el)):
        assert np.array_equal(gt[x["toff"]:x["toff"] + x["tlen"]], et[y["toff"]:y["toff"] + y["tlen"]]), f"record {i}: trace"


def check_transposed(ctx, A, B, adb, bdb, las, trace, ts):
    """transpose, compare with the restatement; returns (las', trace', src, ep of the sources, the restatement's counts)"""
    ep = ctx.edit_paths(A, B, las, trace, ts)
    exp_las, exp_trace, exp_src, stats = tr.transpose_set(las, ep, ts, lengths(adb), lengths(bdb), dentist_amd.LA_DTYPE)
    got = ctx.transpose(A, B, las, trace, ts)
    assert_same_set(got, (exp_las, exp_trace, exp_src))
    check_trace_invariants(got[0], got[1], ts)
    assert np.all(got[0]["flags"] & (CHAIN | 0x20) == 0)
    return got[0], got[1], got[2], ep, stats


def boundary_case(ts):
    """One contig of 2 kb and reads cut from it whose only differences sit at multiples of ts of the READ: a contig base
    left out right behind read position k * ts (in the transposed path a code-2 op directly behind a grid crossing), a
    foreign base put in at read position k * ts; forward and reverse-complemented (a reverse-complemented read carries
    its edits at multiples of ts counted from its own start, which is where the transposed grid lies).  Reads 0 and 1 are
    exact pieces of 4 * ts bases: their mappings start and end on a grid point of the read.  The last two reads are
    shorter than ts: a single tile."""
    rng = np.random.default_rng(1000 + ts)
    g = rng.integers(0, 4, 2000).astype(np.uint8)

    def edited(start, fwd):
        src = g[start:start + 8 * ts + 8]
        src = src if fwd else sim.revcomp(src)
        read, s = [], 0
        for k in range(1, 7):
            need = k * ts - len(read)  # up to read position k * ts
            read += src[s:s + need].tolist()
            s += need
            if k % 2:
                s += 1  # the contig base behind read position k * ts has no read base
            else:
                read.append((int(src[s]) + 1) % 4)  # read base k * ts has no contig base
        read += src[s:s + ts + 3].tolist()
        return np.asarray(read, dtype=np.uint8)

    reads = [g[300:300 + 4 * ts], sim.revcomp(g[700:700 + 4 * ts]), edited(100, True), edited(500, False), edited(901, True),
             edited(333, False), g[1205:1200 + ts - 7], sim.revcomp(g[1503:1500 + ts - 9])]
    return sim.SeqDb.from_list([g]), sim.SeqDb.from_list(reads)


@pytest.fixture(scope="module")
def mapping_workload():
    return sim.Workload(150_000, 2, 250, 3000, seed=61, spacing=15000)


@pytest.fixture(scope="module")
def mapping100(gpu_ctx, mapping_workload):
    """the mapping at tspace 100 with its transposed set (computed once, never modified)"""
    w = mapping_workload
    A, B, las, trace, ts = mapped(gpu_ctx, w.contigs, w.reads, tspace=100)
    tl, tt, src = gpu_ctx.transpose(A, B, las, trace, ts)
    return w, A, B, las, trace, (tl, tt, src)


@pytest.mark.parametrize("ts", [100, 126, 64])
def test_mapping_both_strands(gpu_ctx, mapping_workload, ts):
    w = mapping_workload
    A, B, las, trace, _ = mapped(gpu_ctx, w.contigs, w.reads, tspace=ts)
    assert len(las) >= w.reads.n and set((las["flags"] & 1).tolist()) == {0, 1}
    _, _, _, _, stats = check_transposed(gpu_ctx, A, B, w.contigs, w.reads, las, trace, ts)
    # what the mapping lacks of the four conditions, the crafted case at the same tspace supplies
    cdb, rdb = boundary_case(ts)
    A2, B2, las2, trace2, _ = mapped(gpu_ctx, cdb, rdb, tspace=ts, k=12, hmin=20, min_len=20)
    _, _, _, _, stats2 = check_transposed(gpu_ctx, A2, B2, cdb, rdb, las2, trace2, ts)
    for c in CONDITIONS:
        print(f"tspace {ts}: {c}: mapping {stats[c]}, crafted {stats2[c]}")
        assert stats[c] + stats2[c] > 0, c


@pytest.mark.parametrize("ts", [100, 64])
def test_crafted_boundary_cases(gpu_ctx, ts):
    cdb, rdb = boundary_case(ts)
    A, B, las, trace, _ = mapped(gpu_ctx, cdb, rdb, tspace=ts, k=12, hmin=20, min_len=20)
    assert set((las["flags"] & 1).tolist()) == {0, 1} and len(las) >= rdb.n
    tl, _, src, _, stats = check_transposed(gpu_ctx, A, B, cdb, rdb, las, trace, ts)
    for c in CONDITIONS:
        print(f"tspace {ts}: {c}: {stats[c]}")
        assert stats[c] > 0, c
    both = tl[(tl["abpos"] % ts == 0) & (tl["aepos"] % ts == 0)]
    assert len(both) > 0 and set((both["flags"] & 1).tolist()) == {0, 1}, "no mapping that starts and ends on the read's grid"


def test_output_is_a_real_alignment_and_an_involution(gpu_ctx, mapping100):
    w, A, B, las, trace, (tl, tt, src) = mapping100
    ep = gpu_ctx.edit_paths(A, B, las, trace, 100)
    # the transposed set read as alignments of (B, A): accepted record by record, so its bases sum and its tile counts agree
    ep2 = gpu_ctx.edit_paths(B, A, tl, tt, 100)
    d2 = np.concatenate([tt[l["toff"]:l["toff"] + l["tlen"]:2] for l in tl])
    assert np.all(ep2.tile_score <= d2)
    assert ep2.general_tiles == int(np.count_nonzero(d2.astype(np.int64) + 1 > 63))  # none where the band class fits
    assert np.array_equal(tl["diffs"], ep.score[src])
    assert np.all(ep2.score <= tl["diffs"])
    # transposing the transposed set gives the coordinates back; diffs may only fall
    bl, bt, bsrc = gpu_ctx.transpose(B, A, tl, tt, 100)
    back = src[bsrc]  # source record of every record of the second transposition
    for f in ("aread", "bread", "abpos", "aepos", "bbpos", "bepos"):
        assert np.array_equal(bl[f], las[f][back]), f
    assert np.array_equal(bl["flags"] & 1, las["flags"][back] & 1)
    assert np.all(bl["diffs"] <= tl["diffs"][bsrc]) and np.all(tl["diffs"] <= las["diffs"][src])
    assert sorted(back.tolist()) == list(range(len(las)))
    check_trace_invariants(bl, bt, 100)


def test_chunking_at_record_boundaries(gpu_ctx, mapping100, monkeypatch):
    w, A, B, las, trace, (tl, tt, src) = mapping100
    tiles = las["tlen"] // 2
    assert tiles.max() > 7
    for chunk in (7, int(tiles[:3].sum()), int(tiles.max()) + 1):  # below the largest record; between records; a few records
        monkeypatch.setenv("DH_EDIT_CHUNK", str(chunk))
        got = gpu_ctx.transpose(A, B, las, trace, 100)
        assert got[0].tobytes() == tl.tobytes() and np.array_equal(got[1], tt) and np.array_equal(got[2], src), chunk
    monkeypatch.delenv("DH_EDIT_CHUNK")
    gpu_ctx.release_scratch()  # the scratch of the transposition goes back with the rest
    got = gpu_ctx.transpose(A, B, las, trace, 100)
    assert got[0].tobytes() == tl.tobytes() and np.array_equal(got[1], tt)


def test_long_record_several_passes(gpu_ctx):
    g = sim.genome(71, 12000)
    rng = np.random.default_rng(72)
    read = g[1500:10500].copy()
    hit = rng.random(len(read)) < 0.04
    read[hit] = (read[hit] + 1 + rng.integers(0, 3, int(hit.sum()))) % 4
    read = np.delete(read, rng.choice(len(read), 150, replace=False))
    cdb = sim.SeqDb.from_list([g])
    for rdb in (sim.SeqDb.from_list([read]), sim.SeqDb.from_list([sim.revcomp(read)])):
        A, B, las, trace, ts = mapped(gpu_ctx, cdb, rdb, tspace=100)
        _, _, _, ep, _ = check_transposed(gpu_ctx, A, B, cdb, rdb, las, trace, ts)
        assert int(np.diff(ep.op_off).max()) > 4096, "no path long enough for a second pass of the wavefront"


def test_chain_flags_and_refusals(gpu_ctx, mapping100):
    w, A, B, las, trace, (tl, tt, src) = mapping100
    assert np.all(tl["flags"] & CHAIN == 0)
    bl, bt, bsrc = gpu_ctx.transpose(A, B, las, trace, 100, select_best=True)
    assert np.all((bl["flags"] & (0x4 | 0x8)) != 0) and np.any(bl["flags"] & 0x10)
    assert sorted(bsrc.tolist()) == list(range(len(las)))
    plain = bl.copy()
    plain["flags"] &= ~np.uint32(CHAIN | 0x20)
    order = np.argsort(bsrc)
    assert plain[order].tobytes() == tl[np.argsort(src)].tobytes()  # the same records, flags and order apart

    def refused(l, t, match):
        with pytest.raises(dentist_amd.DhError, match=match) as ei:
            gpu_ctx.transpose(A, B, l, t, 100)
        assert ei.value.code == -1  # DH_EINVAL
        again = gpu_ctx.transpose(A, B, las[:4], trace, 100)  # the context is usable afterwards
        exp = gpu_ctx.edit_paths(A, B, las[:4], trace, 100)
        assert np.array_equal(np.sort(again[0]["diffs"]), np.sort(exp.score))

    empty = las[:1].copy()
    empty[0]["bepos"] = empty[0]["bbpos"]
    empty[0]["aepos"] = empty[0]["abpos"]
    empty[0]["tlen"] = 0
    refused(empty, trace, "no B bases")
    k = int(np.argmax(las["tlen"] >= 4))
    bad = trace.copy()
    bad[las[k]["toff"] + 1] += 1  # the B bases no longer sum to bepos - bbpos
    refused(las[k:k + 1], bad, "LA 0")


def test_raw_handle(gpu_ctx, mapping100):
    w, A, B, las, trace, (tl, tt, src) = mapping100
    g = dentist_amd.default_align_opts(tspace=100, **T)
    h = gpu_ctx.align_db_block(A, B, 0, w.reads.n, g, raw=True)
    got = gpu_ctx.transpose(A, B, h)
    hl, ht, hts = _lib._take_la_set(h)  # (owns the handle from here on)
    exp = gpu_ctx.transpose(A, B, hl, ht, hts)
    assert got[0].tobytes() == exp[0].tobytes() and np.array_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    assert len(got[0]) == len(hl) > 0


def test_same_db_symmetric_pile_up(gpu_ctx):
    g = sim.genome(21, 20000)
    reads, _ = sim.reads(22, g, 30, 6000)
    A, _, las, trace, ts = mapped(gpu_ctx, reads, reads, same=True, tspace=126, skip_self=2, min_len=500, max_la=64, max_cand=128)
    assert len(las) > reads.n and set((las["flags"] & 1).tolist()) == {0, 1}
    check_transposed(gpu_ctx, A, A, reads, reads, las, trace, ts)
