"""The extension stage by itself -- dh_extend_candidates: k_wave, k_wave2<32>, k_wave2<16> and k_tile with what stands around
them (work units, records in place, the compactions, the per-chunk packed and plane copies) -- against the oracle's
extension of the same PLANTED candidates (oz.extend_candidates).  The parity tests of whole dh_align_db calls feed these
kernels whatever the k-mers of simulated reads produce; the cases of tests/extend_cases.py put every rule of the candidate
loop, the acceptance and the two extensions on both sides of its boundary (their claims are shown on the oracle by
tests/test_extend_cases.py).  Exact integer equality: every record field, every trace value, attempts and cells.  A
mismatch names the case, the item, the rank of the record, the fields and the candidate the expected record came from.

Every case runs under every path its options allow.  Which kernel a call takes is shown from its options and switches only:
kernel_of restates the choice of prepare_dbs / alloc_scratch / extend_chunk, and the tests check that restatement against
the kernel they are named after -- a check of the test's own selection of cases, which cannot notice a library that takes
another path.  What is read from the library: stats.wave_launches (one launch for a plain call, ceil(items / chunk) for the
chunked runs).  For DH_WAVE_SINGLE, DH_WAVE_BYTES, DH_TILE_QBATCH and DH_TILE_BOOK_MIN the path is inferred from the
environment alone.

The two pflags cases (symmetric DH-2, records wanted on one side only) are left out here by name: the binding has no call
that sets pflags on a device DB (dh_db_set_pflags is internal to the library, reached through dh_process_* only), so
dh_extend_candidates cannot be given them.  They run on the oracle and through the lane code on the host
(tests/test_extend_cases_host.py)."""
import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim
from helpers import FIELDS, la_rows
from oracle import pyoracle as oz
import extend_cases as ec
from test_parity_map_gpu import OPT_FIELDS

pytestmark = pytest.mark.gpu

CASES = tuple(c for c in ec.all_cases() if not c["pflags"])   # (see the docstring)
SWITCHES = ("DH_WAVE_SINGLE", "DH_WAVE_BYTES", "DH_TILE_QBATCH", "DH_TILE_BOOK_MIN", "DH_ALIGN_CHUNK", "DH_WAVE_G32")


def dev_opts(kw):
    g = dentist_amd.default_align_opts()
    o = ec.oracle_opts(kw)
    for f in OPT_FIELDS:
        setattr(g, f, getattr(o, f))
    return g


def dev_cand(cand):
    dc = np.zeros(cand.shape, dtype=dentist_amd.SEED_CAND_DTYPE)
    for f in ("score", "aseq", "apos", "bpos"):
        dc[f] = cand[f]
    return dc


def kernel_of(kw, env=()):
    """the extension kernel a call with these options and switches takes"""
    if kw["algo"] == 1:
        return f"k_tile<{kw['width']}>"
    if kw["width"] <= 30 and "DH_WAVE_SINGLE" not in env:
        return "k_wave2<16>" if kw["width"] <= 14 else "k_wave2<32>"
    return "k_wave"


def is_sym(c):
    return c["kw"].get("skip_self", 0) == 2


def has_n(c):
    return bool((c["A"].bases > 3).any() or (c["B"].bases > 3).any())


@pytest.fixture(scope="module")
def ctx():
    c = dentist_amd.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def run_gpu(ctx, c, sort=False):
    """dh_extend_candidates on fresh device DBs; returns ((las, trace), (las2, trace2) or None, stats)"""
    dA = ctx.db(c["A"])
    dB = dA if c["B"] is c["A"] else ctx.db(c["B"])
    try:
        out = ctx.extend_candidates(dA, dB, dev_opts(c["kw"]), dev_cand(c["cand"]), c["ncand"], sort=sort, transposed=c["transposed"])
        st = ctx.align_stats()
        if c["transposed"]:
            return out[0], out[1], st
        return out, None, st
    finally:
        dA.close()
        if dB is not dA:
            dB.close()


def source_of(c, exp, item, rank):
    """the candidate the rank-th record of an item came from, by the oracle's attempts log"""
    acc = np.flatnonzero(exp.att[item, :, 0] == 3)
    if is_sym(c) or rank >= len(acc):
        return "candidates " + ", ".join(f"{int(s)}: {tuple(int(c['cand'][item][s][f]) for f in ('aseq', 'apos', 'bpos'))}" for s in acc[:4])
    s = int(acc[rank])
    return f"candidate {s} (aseq, apos, bpos) = {tuple(int(c['cand'][item][s][f]) for f in ('aseq', 'apos', 'bpos'))}, box and diffs {exp.att[item, s, 1:6].tolist()}"


def explain(c, exp, x, y, what, rank_of):
    """x: the record we got (or None), y: the record the oracle has (or None)"""
    ref = y if y is not None else x
    item = 2 * ref[FIELDS.index("bread")] + (ref[FIELDS.index("flags")] & 1)
    rank = rank_of(item)
    bad = [f for f, u, v in zip(FIELDS + ("trace",), x or (), y or ()) if u != v]
    return (f"{what}: case {c['name']} ({c['claim']}), item {item} (read {item // 2}, strand {item & 1}), record rank {rank}, "
            f"fields {bad or 'record missing or extra'}\n got {x}\n exp {y}\n from {source_of(c, exp, item, rank)}")


def compare_rows(c, exp, got, want, what):
    """got / want: rows in comparable order; the first difference is explained"""
    per_item = {}

    def rank_of(item):
        return per_item.get(item, 0)
    for x, y in zip(got, want):
        assert x == y, explain(c, exp, x, y, what, rank_of)
        item = 2 * y[FIELDS.index("bread")] + (y[FIELDS.index("flags")] & 1)
        per_item[item] = per_item.get(item, 0) + 1
    if len(got) != len(want):
        n = min(len(got), len(want))
        raise AssertionError(explain(c, exp, got[n] if len(got) > n else None, want[n] if len(want) > n else None,
                                     f"{what}: {len(got)} records, oracle {len(want)}", rank_of))


def check(ctx, c, what, launches=None):
    exp = ec.oracle(c)
    try:
        (las, trace), second, st = run_gpu(ctx, c)
    except dentist_amd.DhError as e:
        raise AssertionError(f"{what}: case {c['name']} ({c['claim']}): {e}") from e
    got, want = la_rows(las, trace), la_rows(exp.las, exp.trace)
    if c["overflow"]:
        # more records than slots: which pairs are dropped depends on the arrival order; what arrives is the oracle's
        assert set(got) <= set(want) and len(got) < len(want) and st.overflow_items > 0, f"{what}: case {c['name']}"
    else:
        if is_sym(c):   # slots are claimed in arrival order: the sorted set per A read
            key = lambda r: (r[FIELDS.index("aread")],) + r  # noqa: E731
            got, want = sorted(got, key=key), sorted(want, key=key)
        compare_rows(c, exp, got, want, what)
        assert st.las == len(want) and st.overflow_items == 0, f"{what}: case {c['name']}"
    assert (st.alignments, st.wave_cells) == (int(exp.stats[2]), int(exp.stats[3])), \
        f"{what}: case {c['name']}: attempts and cells {(st.alignments, st.wave_cells)}, oracle {(int(exp.stats[2]), int(exp.stats[3]))}"
    assert (st.hits, st.cands) == (0, int(c["ncand"].sum())), f"{what}: case {c['name']}"
    if second is not None:
        compare_rows(c, exp, sorted(la_rows(*second)), sorted(la_rows(exp.las2, exp.trace2)), what + " (transposed file)")
    if launches is not None:
        assert st.wave_launches == launches(c), f"{what}: case {c['name']}: {st.wave_launches} launches"
    return st


def config_cases(algo, width):
    t = ec.tag(algo, width)
    return [c for c in CASES if c["name"].endswith(t)]


def ids(cfgs):
    return [ec.tag(*c) for c in cfgs]


DH1 = [cfg for cfg in ec.CONFIGS if cfg[0] == 0]
DH2 = [cfg for cfg in ec.CONFIGS if cfg[0] == 1]
OWN_WIDTH = [c for c in CASES if not any(c["name"].endswith(ec.tag(*cfg)) for cfg in ec.CONFIGS)]   # the DH-1-only cases


# ------------------------------------------------------------------------------------------- every case, plain call
@pytest.mark.parametrize("algo,width", ec.CONFIGS, ids=ids(ec.CONFIGS))
def test_cases_by_the_kernel_of_their_width(ctx, algo, width):
    cases = config_cases(algo, width)
    assert len(cases) > 80
    want = {(1, 64): "k_tile<64>", (1, 32): "k_tile<32>", (0, 62): "k_wave", (0, 30): "k_wave2<32>", (0, 14): "k_wave2<16>"}[(algo, width)]
    for c in cases:
        assert kernel_of(c["kw"]) == want
        check(ctx, c, want, launches=lambda c: 1)


def test_dh1_cases_of_a_width_of_their_own(ctx):
    """dmax, the width pairs 1 ... 62 (14 | 15 and 30 | 31 change the kernel), N against N and N against a base"""
    kernels = set()
    for c in OWN_WIDTH:
        kernels.add(kernel_of(c["kw"]))
        check(ctx, c, kernel_of(c["kw"]))
    assert kernels == {"k_wave", "k_wave2<32>", "k_wave2<16>"}


# ------------------------------------------------------------------------------------------------- the switches
@pytest.mark.parametrize("algo,width", [(0, 30), (0, 14)], ids=["dh1w30", "dh1w14"])
def test_narrow_waves_by_k_wave(ctx, monkeypatch, algo, width):
    monkeypatch.setenv("DH_WAVE_SINGLE", "1")
    for c in config_cases(algo, width) + [c for c in OWN_WIDTH if c["kw"]["width"] <= 30 and (c["kw"]["width"] <= 14) == (width == 14)]:
        assert kernel_of(c["kw"], ("DH_WAVE_SINGLE",)) == "k_wave"
        check(ctx, c, "k_wave (DH_WAVE_SINGLE=1)")


@pytest.mark.parametrize("algo,width", DH1, ids=ids(DH1))
def test_byte_path(ctx, monkeypatch, algo, width):
    """the wave kernels over the byte arrays, 8 bases per load (the packed copies are what the plain runs above slide over)"""
    monkeypatch.setenv("DH_WAVE_BYTES", "1")
    for c in config_cases(algo, width) + ([c for c in OWN_WIDTH if not has_n(c)] if width == 62 else []):
        check(ctx, c, f"{kernel_of(c['kw'])} on bytes (DH_WAVE_BYTES=1)")


@pytest.mark.parametrize("algo,width", DH2, ids=ids(DH2))
@pytest.mark.parametrize("switch,value", [("DH_TILE_QBATCH", "1"), ("DH_TILE_BOOK_MIN", "64")])
def test_tile_switches(ctx, monkeypatch, switch, value, algo, width):
    """work fetched one item at a time; bookkeeping only when all 64 lanes wait for it"""
    monkeypatch.setenv(switch, value)
    for c in config_cases(algo, width):
        check(ctx, c, f"k_tile<{width}> ({switch}={value})")


@pytest.mark.parametrize("algo,width", ec.CONFIGS, ids=ids(ec.CONFIGS))
@pytest.mark.parametrize("chunk", [2, 6])
def test_chunk_edges_inside_the_db(ctx, monkeypatch, chunk, algo, width):
    """chunks of 2 and of 6 items: candidate rows, records and the derived copies of B relative to the chunk (the neighbour,
    run and phase cases start their chunks on every phase of a packed word).  Symmetric calls are one chunk by definition."""
    monkeypatch.setenv("DH_ALIGN_CHUNK", str(chunk))
    cases = [c for c in config_cases(algo, width) if not is_sym(c)]
    assert any(2 * c["B"].n > chunk for c in cases)
    for c in cases:
        check(ctx, c, f"{kernel_of(c['kw'])} (DH_ALIGN_CHUNK={chunk})", launches=lambda c: -(-2 * c["B"].n // chunk))


# ----------------------------------------------------------------------------- all cases of one mode in one call
def concatenated(cases, name):
    """one DB pair and one call: the sequences of every case behind each other, aseq and items shifted"""
    kw = dict(cases[0]["kw"], max_cand=max(c["kw"]["max_cand"] for c in cases))
    As, Bs, plants, a0, b0 = [], [], {}, 0, 0
    for c in cases:
        As += [c["A"].seq(i) for i in range(c["A"].n)]
        Bs += [c["B"].seq(i) for i in range(c["B"].n)]
        for it in np.flatnonzero(c["ncand"]):
            plants[2 * b0 + int(it)] = [(int(q["aseq"]) + a0, int(q["apos"]), int(q["bpos"])) for q in c["cand"][it][:c["ncand"][it]]]
        a0 += c["A"].n
        b0 += c["B"].n
    return ec.case(name, "all cases of one mode in one call", f"{len(cases)} cases in one DB", ec.db(As), ec.db(Bs), kw, plants)


def groups(algo, width):
    by_kw = {}
    for c in config_cases(algo, width):
        if c["B"] is c["A"] or c["transposed"]:
            continue
        key = tuple(sorted((k, v) for k, v in c["kw"].items() if k != "max_cand"))
        by_kw.setdefault(key, []).append(c)
    return [g for g in by_kw.values() if len(g) > 1]


@pytest.mark.parametrize("algo,width", ec.CONFIGS, ids=ids(ec.CONFIGS))
def test_all_cases_of_a_mode_in_one_call(ctx, algo, width):
    """the lanes of a wavefront hold different cases at once; the expected records are those of the cases by themselves
    (a pair of sequences does not see what else is in the DB), which the oracle confirms on the concatenated input"""
    gs = groups(algo, width)
    assert max(len(g) for g in gs) >= 40
    for n, g in enumerate(gs):
        big = concatenated(g, f"concat-{n}-{ec.tag(algo, width)}")
        exp = ec.oracle(big)
        rows, a0, b0 = [], 0, 0
        for c in g:
            r = ec.oracle(c)
            for row in la_rows(r.las, r.trace):
                row = list(row)
                row[FIELDS.index("aread")] += a0
                row[FIELDS.index("bread")] += b0
                rows.append(tuple(row))
            a0 += c["A"].n
            b0 += c["B"].n
        assert rows == la_rows(exp.las, exp.trace) and exp.stats[2] == sum(ec.oracle(c).stats[2] for c in g)
        check(ctx, big, f"{kernel_of(big['kw'])}, {len(g)} cases in one call", launches=lambda c: 1)


# --------------------------------------------------------------------------------------------------- rejections
def test_planted_candidates_out_of_range_are_refused_on_the_host(ctx):
    """nothing a candidate says may take a kernel out of bounds: DH_EINVAL before anything is launched"""
    a, b = ec.island(7)
    A, B = ec.db([a, a[:500]]), ec.db([b, b[:300]])
    dA, dB = ctx.db(A), ctx.db(B)
    other = dentist_amd.Context(0)
    dO = other.db(B)
    g = dev_opts(dict(ec.BASE_KW, algo=1, width=64))
    good = ec.case("ok", "", "", A, B, dict(algo=1, width=64), {0: [(0, 600, 460)], 2: [(1, 300, 160)]})

    def refused(cand, ncand, opts=g, dbs=(dA, dB)):
        before = ctx.cum_stats().wave_launches
        with pytest.raises(dentist_amd.DhError) as e:
            ctx.extend_candidates(dbs[0], dbs[1], opts, cand, ncand)
        assert e.value.code == -1 and ctx.cum_stats().wave_launches == before, str(e.value)

    try:
        (las, _) = ctx.extend_candidates(dA, dB, g, dev_cand(good["cand"]), good["ncand"])
        assert len(las) == 2
        for item, field, value in ((0, "aseq", -1), (0, "aseq", 2), (0, "apos", -1), (0, "apos", 1201), (2, "apos", 501), (0, "bpos", -1),
                                   (0, "bpos", 921), (2, "bpos", 301)):
            cand = dev_cand(good["cand"])
            cand[item][0][field] = value
            refused(cand, good["ncand"])
        for item, value in ((0, -1), (0, 9), (3, -2)):
            ncand = good["ncand"].copy()
            ncand[item] = value
            refused(dev_cand(good["cand"]), ncand)
        # the edges themselves are inside: apos = alen, bpos = blen
        cand = dev_cand(good["cand"])
        cand[2][0]["apos"], cand[2][0]["bpos"] = 500, 300
        ctx.extend_candidates(dA, dB, g, cand, good["ncand"])
        refused(dev_cand(good["cand"]), good["ncand"], dbs=(dA, dO))
        # what the seed stage never says under the skip_self rules; a strand the options leave out
        same = ec.case("same", "", "", A, A, dict(algo=1, width=64), {0: [(0, 600, 460)]})
        for skip, cnd in ((1, (0, 600, 460)), (2, (0, 600, 460)), (3, (1, 300, 100)), (3, (0, 100, 100)), (3, (0, 100, 300))):
            c = ec.case("s", "", "", A, A, dict(algo=1, width=64), {0: [cnd]})
            refused(dev_cand(c["cand"]), c["ncand"], dev_opts(dict(ec.BASE_KW, algo=1, width=64, skip_self=skip, strands=1)), (dA, dA))
        c = ec.case("s", "", "", A, B, dict(algo=1, width=64), {1: [(0, 600, 460)]})
        refused(dev_cand(c["cand"]), c["ncand"], dev_opts(dict(ec.BASE_KW, algo=1, width=64, strands=1)))
        assert same["ncand"][0] == 1
    finally:
        for d in (dA, dB, dO):
            d.close()
        other.close()


# -------------------------------------------------------------------------------------------------- composition
@pytest.mark.parametrize("mode", ["mapping", "pile-up"])
def test_the_two_stages_compose_to_the_whole_call(ctx, mode):
    """extend_candidates(seed_candidates(...)) is align_db: records, trace values and counters"""
    if mode == "mapping":
        w = sim.Workload(120_000, 2, 120, 3000, seed=23, spacing=10000, gap_max=500)
        A, B, kw = w.contigs, w.reads, dict(algo=1, width=64)
    else:
        g0 = sim.genome(29, 12000)
        reads, _ = sim.reads(30, g0, 24, 4000)
        A = B = reads
        kw = dict(algo=1, width=64, tspace=126, skip_self=2, max_la=64, max_cand=128)
    g = dentist_amd.default_align_opts(**kw)
    dA = ctx.db(A)
    dB = dA if B is A else ctx.db(B)
    try:
        whole = ctx.align_db(dA, dB, g)
        st = ctx.align_stats()
        cand, ncand, _ = ctx.seed_candidates(dA, dB, g)
        assert (ncand >= 0).all() and ncand.sum() == st.cands
        parts = ctx.extend_candidates(dA, dB, g, cand, ncand, sort=True)
        st2 = ctx.align_stats()
    finally:
        dA.close()
        if dB is not dA:
            dB.close()
    assert len(whole[0]) > (100 if mode == "mapping" else 2 * B.n)
    assert la_rows(*parts) == la_rows(*whole)
    assert (st2.alignments, st2.wave_cells, st2.las, st2.cands) == (st.alignments, st.wave_cells, st.las, st.cands)


def test_no_shared_kmer_is_needed(ctx):
    """the stage does not look at k-mers: two sequences that share no 14-mer (a substitution every 9 bases) still align
    through a planted candidate, while the whole call finds nothing between them"""
    a = ec.rnd(301, 900)
    b = ec.subs(a, range(4, 900, 9))
    A, B = ec.db([a]), ec.db([b])
    c = ec.case("no-kmer", "", "", A, B, dict(algo=1, width=64), {0: [(0, 450, 450)]})
    exp = ec.oracle(c)
    assert exp.a(0, 0, "state") == 3 and exp.box(0, 0)[1] - exp.box(0, 0)[0] > 800
    dA, dB = ctx.db(A), ctx.db(B)
    try:
        assert len(ctx.align_db(dA, dB, dev_opts(c["kw"]))[0]) == 0
    finally:
        dA.close()
        dB.close()
    check(ctx, c, "no shared k-mer")
    check(ctx, dict(c, kw=dict(c["kw"], algo=0, width=30), name="no-kmer-dh1"), "no shared k-mer")
