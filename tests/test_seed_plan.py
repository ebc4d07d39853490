"""The plan of the seed stage (dentist_amd/csrc/dh_seed_plan.h: every decision plan_seeds, plan_mj_chunk and seed_chunk
take, as functions of numbers) compiled for the CPU (tests/native/seedplan_host.cpp) against tests/seed_plan_ref.py, the
restatement of those functions' earlier text: the anchors the code's comments give, worked by hand, and a seeded sweep of
random arguments under every combination of the development switches.  Equality, doubles included: both sides do the
same operations in the same order.  No GPU needed."""
import ctypes
import os
import random
import re
import subprocess

import pytest

import seed_plan_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECTORY, PILEUP_JOIN, MAPPING_JOIN, TABLE_JOIN = 0, 1, 2, 3

i32, i64, u64, f64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
P = ctypes.POINTER


def consts():
    """the constants the library hands the plan, from the headers that define them"""
    C = {}
    for h in ("dh_mjoin.h", "dh_tjoin.h", "dh_device.h", "dh_internal.h"):
        text = open(os.path.join(ROOT, "dentist_amd", "csrc", h)).read()
        for m in re.finditer(r"^#define ((?:MJ|TJ|DH_SEED_FSCR|DH_TJ_HIT)_\w+) +(.+?) *(?:/\*.*)?$", text, re.M):
            C[m.group(1)] = m.group(2).strip()
    out = {}
    for name in ("MJ_PBITS", "MJ_CAP", "MJ_THREADS", "MJ_POSBITS", "MJ_GROUP", "MJ_BATCH", "MJ_PAGE", "MJ_PROBE_THREADS", "TJ_CAP",
                 "TJ_THREADS", "DH_SEED_FSCR_WORDS", "DH_SEED_FSCR_WORDS16", "DH_SEED_FSCR_BLOCKS_PER_CU"):
        out[name] = int(C[name])
    out["MJ_P"] = 1 << out["MJ_PBITS"]
    assert C["MJ_P"] == "(1 << MJ_PBITS)" and C["TJ_RUN"] == "(TJ_THREADS / 64)"
    out["TJ_RUN"] = out["TJ_THREADS"] // 64
    out["DH_TJ_HIT_RATE0"] = float(C["DH_TJ_HIT_RATE0"])
    return out


C = consts()
K = (i64 * 13)(*[C[n] for n in ("MJ_P", "MJ_CAP", "MJ_THREADS", "MJ_POSBITS", "MJ_GROUP", "MJ_BATCH", "MJ_PAGE", "MJ_PROBE_THREADS",
                                "TJ_CAP", "TJ_RUN", "DH_SEED_FSCR_WORDS", "DH_SEED_FSCR_WORDS16", "DH_SEED_FSCR_BLOCKS_PER_CU")])
RATE0 = C["DH_TJ_HIT_RATE0"]


def knobs(env):
    """the switches as the library's reader turns the environment into a SeedKnobs (atoi / atoll / atof of the value)"""
    def num(name):
        return (1, int(env[name])) if name in env else (0, 0)
    v = [*num("DH_SEED_CAP"), int("DH_SEED_NO16K" in env), int("DH_SEED_NO_WAVE_TIER" in env), int("DH_SEED_NO_MID_TIER" in env),
         int("DH_SEED_BIG_PCT" in env), *num("DH_MJOIN_MIN"), *num("DH_MJOIN_PAGES"), int("DH_NO_MJOIN" in env), int("DH_NO_TJOIN" in env),
         *num("DH_TJOIN_CAP"), *num("DH_TJOIN_HITCAP")]
    return (i64 * 16)(*v), float(env.get("DH_SEED_BIG_PCT", 0))


@pytest.fixture(scope="module")
def host():
    subprocess.run(["make", "-C", ROOT, "-s", "tests/native/libseedplan_host.so"], check=True)
    L = ctypes.CDLL(os.path.join(ROOT, "tests", "native", "libseedplan_host.so"))
    KN, KC = [P(i64), f64], [P(i64), f64]
    sig = {
        "sp_chance_density": (f64, [i64, i32, i32, i32]),
        "sp_first_cap": (i32, [i32, i32, f64, i32, i32, P(ctypes.c_uint32), i32] + KN),
        "sp_mj_min_bases": (i64, KN),
        "sp_mj_chunk_size_ok": (i32, [i64, i64]),
        "sp_tj_cap_entries": (i64, KN + KC),
        "sp_mj_geometry": (None, [i64, i32, i32, f64, f64, i32] + KN + KC + [P(i64)]),
        "sp_mj_pool_regrow": (i32, [i64, i64, u64, u64, f64] + KC + [P(f64)]),
        "sp_tj_units": (i32, [P(i32), i32, i32] + KC + [P(i32)]),
        "sp_tj_first_hitcap": (i64, [f64, i64] + KN),
        "sp_tj_learned_rate": (f64, [f64, u64, i64] + KC),
        "sp_mean_hits_expected": (f64, [i64, i32, i32, f64]),
        "sp_mean_hits_counted": (f64, [u64, i32]),
        "sp_first_tier": (None, [i32, i32, f64, i32, i32, i32] + KN + KC + [P(i64)]),
        "sp_tier_fscr_words": (i64, [i32] + KC),
        "sp_fscr_total_words": (i64, [i64, i32] + KC),
        "sp_tier_ladder": (i32, [i32] + KN + [P(i32)]),
        "sp_split_rung": (i32, [P(i32), i32, P(i32), i64, i32, P(i32), P(i32), P(i32)]),
        "sp_list_overflowed": (i32, [P(i32), P(i32), i32, i64, P(i32), P(i32)]),
        "sp_quarter_overflowed": (i32, [i64, i32]),
        "sp_redo_all_above": (i64, [i32, i32] + KN),
        "sp_cap_doubles": (i32, [i32, i64, i64, i32]),
        "sp_hbm_pass": (i32, [i32, P(i64)]),
    }
    for name, (res, args) in sig.items():
        getattr(L, name).restype = res
        getattr(L, name).argtypes = args
    return L


# ---- the library's side of every function, in the shape the reference returns
def first_tier(L, kind, cap, mean, nseg=1, ctx_wave=True, ctx_mid=True, env={}):
    out = (i64 * 4)()
    L.sp_first_tier(kind, cap, mean, nseg, int(ctx_wave), int(ctx_mid), *knobs(env), K, RATE0, out)
    return list(out)


def ref_first_tier(kind, cap, mean, nseg=1, ctx_wave=True, ctx_mid=True, env={}):
    return ref.first_tier(kind == PILEUP_JOIN, kind == MAPPING_JOIN, kind == TABLE_JOIN, cap, mean, nseg, ctx_wave, ctx_mid, env, C)


def ladder(L, held, env={}):
    out = (i32 * 4)()
    n = L.sp_tier_ladder(held, *knobs(env), out)
    return list(out)[:n]


def first_cap(L, max_len, kmer_mod, dens, same, joined, jhist, nreads, env={}):
    return L.sp_first_cap(max_len, kmer_mod, dens, int(same), int(joined), (ctypes.c_uint32 * 4)(*jhist), nreads, *knobs(env))


def geometry(L, bases, max_len, kmer_mod, hit_frac=0.2, dens=0.0, ncu=256, env={}):
    out = (i64 * 8)()
    L.sp_mj_geometry(bases, max_len, kmer_mod, hit_frac, dens, ncu, *knobs(env), K, RATE0, out)
    return list(out)


def regrow(L, npages, exp_ent, hits, unplaced, hit_frac):
    out = (f64 * 3)()
    again = L.sp_mj_pool_regrow(npages, exp_ent, hits, unplaced, hit_frac, K, RATE0, out)
    return out[0], out[1], out[2], bool(again)


def units(L, group, cr0, cr1):
    out = (i32 * (3 * max(1, cr1 - cr0)))()
    n = L.sp_tj_units((i32 * len(group))(*group), cr0, cr1, K, RATE0, out)
    return [tuple(out[3 * i:3 * i + 3]) for i in range(n)]


def hbm(L, gcap):
    out = (i64 * 3)()
    if L.sp_hbm_pass(gcap, out):
        return True, None, None, None
    return False, out[0], out[1], out[2]


def split(L, big, nhits, item0, tier):
    n = len(big)
    fits, left, cnt = (i32 * max(1, n))(), (i32 * max(1, n))(), (i32 * 2)()
    gcap = L.sp_split_rung((i32 * max(1, n))(*big), n, (i32 * len(nhits))(*nhits), item0, tier, fits, left, cnt)
    return list(fits)[:cnt[0]], list(left)[:cnt[1]], gcap


def overflowed(L, ncand, nhits, item0):
    ni = len(ncand)
    big, gcap = (i32 * max(1, ni // 2))(), i32()
    n = L.sp_list_overflowed((i32 * max(1, ni))(*ncand), (i32 * max(1, ni))(*nhits), ni, item0, big, ctypes.byref(gcap))
    return list(big)[:n], gcap.value


# ---- (a) the anchors
W, W16 = C["DH_SEED_FSCR_WORDS"], C["DH_SEED_FSCR_WORDS16"]


def test_the_constants_the_anchors_are_worked_with():
    assert (C["MJ_CAP"], C["MJ_THREADS"], C["MJ_POSBITS"], C["MJ_GROUP"], C["MJ_BATCH"], C["TJ_RUN"]) == (8192, 512, 17, 16, 64, 16)
    assert (W, W16) == (6144, 24576)


@pytest.mark.parametrize("kind", [MAPPING_JOIN, TABLE_JOIN])
def test_first_tier_by_the_mean_hits_per_read(host, kind):
    cases = [
        (140.0, {}, [512, 1, 0, 0]),       # 1/8 sampling: the wavefront-per-read tier
        (925.0, {}, [2048, 0, 1, 0]),      # unsampled: 1.5 x 925 exceeds 512, the middle tier
        (1100.0, {}, [2048, 0, 1, 0]),
        (1365.0, {}, [2048, 0, 1, 0]),     # 2047.5
        (1366.0, {}, [4096, 0, 0, 0]),     # 2049
        (2730.0, {}, [4096, 0, 0, 0]),     # 4095
        (2731.0, {}, [8192, 0, 0, W]),     # 4096.5
        (5461.0, {}, [8192, 0, 0, W]),     # 8191.5
        (5462.0, {}, [16384, 0, 0, W16]),  # 8193
        (5462.0, {"DH_SEED_NO16K": "1"}, [8192, 0, 0, W]),
        (140.0, {"DH_SEED_NO_WAVE_TIER": "1"}, [2048, 0, 1, 0]),
        (925.0, {"DH_SEED_NO_MID_TIER": "1"}, [2048, 0, 0, 0]),
    ]
    for mean, env, want in cases:
        assert first_tier(host, kind, 4096, mean, env=env) == want == ref_first_tier(kind, 4096, mean, env=env), (mean, env)
    # the context has given a tier up
    assert first_tier(host, kind, 4096, 140.0, ctx_wave=False) == [2048, 0, 1, 0]
    assert first_tier(host, kind, 4096, 925.0, ctx_mid=False) == [2048, 0, 0, 0]
    # a block gathers one segment per thread: 257 segments per read are no work for 256 threads -- of the mapping join
    assert first_tier(host, kind, 4096, 925.0, nseg=256) == [2048, 0, 1, 0]
    assert first_tier(host, kind, 4096, 925.0, nseg=257) == [2048, 0, int(kind == TABLE_JOIN), 0]


def test_first_tier_slab_scratch(host):
    """the directory's kernel takes scratch between 4096 and 8192 entries only; a join path's goes by its own capacity"""
    for cap, want in ((2048, 0), (4096, 0), (8192, W), (16384, 0)):
        assert first_tier(host, DIRECTORY, cap, 0.0)[3] == want == ref_first_tier(DIRECTORY, cap, 0.0)[3]
    for cap, capj, want in ((1024, 2048, 0), (4096, 4096, 0), (8192, 8192, W), (16384, 16384, W16)):
        assert first_tier(host, PILEUP_JOIN, cap, 0.0) == [capj, 0, 0, want] == ref_first_tier(PILEUP_JOIN, cap, 0.0)
    assert first_tier(host, PILEUP_JOIN, 16384, 0.0, env={"DH_SEED_NO16K": "1"}) == [8192, 0, 0, W]
    # (a mapping chunk of a call whose cap is 8192: the pointer is handed on, the small tiers do not look at it)
    assert first_tier(host, MAPPING_JOIN, 8192, 140.0) == [512, 1, 0, W] == ref_first_tier(MAPPING_JOIN, 8192, 140.0)
    assert first_tier(host, MAPPING_JOIN, 8192, 5462.0) == [16384, 0, 0, W16]
    assert host.sp_tier_fscr_words(8192, K, RATE0) == W and host.sp_tier_fscr_words(16384, K, RATE0) == W16
    assert host.sp_fscr_total_words(W, 256, K, RATE0) == 256 * 4 * W


def test_tier_ladder(host):
    for held, want in ((0, [2048, 8192, 16384]), (512, [2048, 8192, 16384]), (2048, [8192, 16384]), (4096, [8192, 16384]),
                       (8192, [16384]), (16384, [])):
        assert ladder(host, held) == want == ref.tier_ladder(held, 16384), held
    no16k = {"DH_SEED_NO16K": "1"}
    for held, want in ((0, [2048, 8192]), (2048, [8192]), (8192, [])):
        assert ladder(host, held, no16k) == want == ref.tier_ladder(held, ref.tier_max(no16k)), held


def test_split_of_a_rung_and_the_list_of_overflowed_reads(host):
    item0 = 10                          # reads 5 .. 9
    ncand = [3, 0, -1, -1, -1, 5, 7, 7, -1, -1]
    nhits = [9, 9, 3000, 1000, 5000, 4000, 1, 1, 2048, 0]
    assert overflowed(host, ncand, nhits, item0) == ([6, 7, 9], 9000) == ref.list_overflowed(ncand, nhits, len(ncand), item0)
    assert split(host, [6, 7, 9], nhits, item0, 2048) == ([9], [6, 7], 9000) == ref.split_rung([6, 7, 9], nhits, item0, 2048)
    assert split(host, [6, 7], nhits, item0, 8192) == ([6], [7], 9000)
    assert split(host, [7], nhits, item0, 16384) == ([7], [], 0)
    assert overflowed(host, [-1], [5], 0) == ([], 0)  # (an odd item at the end is no read)


def test_first_capacity_of_the_call(host):
    n = 1000                            # 0.3 n = 300 reads may overflow a tier
    for jhist, want in (([300, 999, 999, 0], 2048), ([301, 300, 999, 0], 4096), ([301, 301, 300, 0], 8192), ([301, 301, 301, 0], 16384)):
        assert first_cap(host, 15000, 8, 0.01, True, True, jhist, n) == want == ref.plan_cap(15000, 8, 0.01, True, True, jhist, n, {})
    assert first_cap(host, 15000, 8, 0.01, True, True, [999, 999, 999, 0], n, {"DH_SEED_CAP": "1024"}) == 1024
    # all-vs-all without the join: 0.6 hits per base of the longest read, up to 8192
    for max_len, want in ((1706, 1024), (1707, 2048), (13653, 8192), (13654, 8192), (100000, 8192)):
        assert first_cap(host, max_len, 1, 0.0, True, False, [0] * 4, n) == want == ref.plan_cap(max_len, 1, 0.0, True, False, [0] * 4, n, {})
    # a mapping: 1.5 x max_len / kmer_mod x (2 dens + 0.1)
    for max_len, want in ((6826, 1024), (6827, 2048), (200000, 16384)):
        assert first_cap(host, max_len, 1, 0.0, False, False, [0] * 4, n) == want == ref.plan_cap(max_len, 1, 0.0, False, False, [0] * 4, n, {})
    assert host.sp_chance_density(1 << 27, 8, 14, 1) == 4.0 == ref.dens(1 << 27, 8, 14, 1)


def test_whole_chunk_again_and_the_quarter(host):
    for ni, cap, env, want in ((1000, 2048, {}, 28), (1000, 4096, {}, 28), (1000, 8192, {}, 250), (1000, 16384, {}, 250),
                               (1000, 2048, {"DH_SEED_BIG_PCT": "10"}, 50), (1001, 8192, {"DH_SEED_BIG_PCT": "0.5"}, 2)):
        assert host.sp_redo_all_above(ni, cap, *knobs(env)) == want == ref.redo_all(ni, cap, env)
    assert host.sp_cap_doubles(DIRECTORY, 29, 28, 2048) == 1 and host.sp_cap_doubles(DIRECTORY, 28, 28, 2048) == 0
    assert host.sp_cap_doubles(DIRECTORY, 999, 28, 16384) == 0 and host.sp_cap_doubles(PILEUP_JOIN, 999, 28, 2048) == 0
    # a quarter of the ni / 2 reads
    assert host.sp_quarter_overflowed(125, 1000) == 0 and host.sp_quarter_overflowed(126, 1000) == 1
    assert host.sp_quarter_overflowed(0, 1) == 0 and host.sp_quarter_overflowed(1, 3) == 1


def test_pool_regrowth_and_its_ceiling(host):
    # 1.2 x 160 hits over 3 expected k-mers is 64.0 exactly: the last rate a pool is planned for
    assert regrow(host, 0, 3, 160, 0, 0.2) == (0.0, 64.0, 64.0, True) == ref.mj_pool_regrow(0, 3, 160, 0, 0.2, C)
    got = regrow(host, 0, 3, 161, 0, 0.2)
    assert got == ref.mj_pool_regrow(0, 3, 161, 0, 0.2, C) and got[2] > 64.0 and not got[3]
    # half as much again when the count asks for less; the pages held plus what found none when that is more than the hits
    got = regrow(host, 134, 1 << 24, 1000, 0, 0.2)
    assert got == ref.mj_pool_regrow(134, 1 << 24, 1000, 0, 0.2, C) and got[2] == 0.2 * 1.5 and got[3]
    got = regrow(host, 134, 1 << 20, 1000, 5 << 20, 0.2)
    assert got == ref.mj_pool_regrow(134, 1 << 20, 1000, 5 << 20, 0.2, C) and got[1] == 1.2 * (134 * 16384 / 1.34 + (5 << 20)) / (1 << 20)


def test_hbm_pass_geometry(host):
    assert hbm(host, 1 << 22) == (False, 1 << 22, 10485760, 25) == ref.hbm_pass(1 << 22)
    assert hbm(host, (1 << 22) + 1)[0] and ref.hbm_pass((1 << 22) + 1)[0]
    for gcap, want in ((0, (False, 1, 3, 89478485)), (1, (False, 1, 3, 89478485)), (3, (False, 4, 10, 26843545)), (16385, (False, 32768, 81920, 3276))):
        assert hbm(host, gcap) == want == ref.hbm_pass(gcap)


def test_table_join_units_and_hit_buffer(host):
    run = C["TJ_RUN"]
    group = [0] * 5 + [2] * 3 + [3]     # a group change inside a run, a last read alone
    assert units(host, group, 0, 9) == [(0, 0, 5), (2, 5, 8), (3, 8, 9)] == ref.tj_units(group, 0, 9, C)
    assert units(host, [7] * run, 0, run) == [(7, 0, run)]
    assert units(host, [7] * (run + 1), 0, run + 1) == [(7, 0, run), (7, run, run + 1)] == ref.tj_units([7] * (run + 1), 0, run + 1, C)
    assert units(host, group, 3, 6) == [(0, 3, 5), (2, 5, 6)] and units(host, group, 4, 4) == []
    assert host.sp_tj_first_hitcap(0.14, 1000000, *knobs({})) == 179096 == ref.tj_first_hitcap(0.14, 1000000, {})
    assert host.sp_tj_first_hitcap(0.14, 1000000, *knobs({"DH_TJOIN_HITCAP": "0"})) == 1
    # the learned rate never falls below the starting figure, and a chunk without bases teaches nothing
    assert host.sp_tj_learned_rate(0.5, 10, 1000, K, RATE0) == RATE0 == ref.tj_learned_rate(0.5, 10, 1000, C)
    assert host.sp_tj_learned_rate(0.14, 870, 1000, K, RATE0) == 0.87 and host.sp_tj_learned_rate(0.5, 10, 0, K, RATE0) == 0.5
    assert host.sp_tj_cap_entries(*knobs({}), K, RATE0) == 8192 and host.sp_tj_cap_entries(*knobs({"DH_TJOIN_CAP": "100"}), K, RATE0) == 100
    assert host.sp_tj_cap_entries(*knobs({"DH_TJOIN_CAP": "-5"}), K, RATE0) == 0 and host.sp_tj_cap_entries(*knobs({"DH_TJOIN_CAP": "99999"}), K, RATE0) == 8192
    assert host.sp_mean_hits_counted(3000, 20) == 300.0 and host.sp_mean_hits_counted(5, 1) == 5.0


def test_mapping_join_geometry(host):
    # bases per tile: the tile's capacity unsampled, 13/16 of it times the sampling otherwise, in whole rolls of the block
    assert geometry(host, 1, 1000, 1)[:5] == [8192, 1, 64, 4, 2]
    assert geometry(host, 1, 1000, 8)[:5] == [53248, 1, 64, 4, 2]
    for kmer_mod, tb in ((1, 8192), (8, 53248)):
        for bases, ntiles in ((1, 1), (tb, 1), (tb + 1, 2), (64 * tb, 64), (64 * tb + 1, 65)):
            got = geometry(host, bases, 15000, kmer_mod)
            assert got == ref.mj_chunk(bases, 15000, kmer_mod, 0.2, 0.0, 256, {}, C)
            assert got[:4] == [tb, ntiles, (ntiles + 63) // 64 * 64, (ntiles + 63) // 64 * 4] and got[5] == bases // kmer_mod and got[7] == 1
    # a read spans at most 512 tile groups
    tbg = 8192 * 16
    assert geometry(host, 1 << 30, 511 * tbg, 1)[4::3] == [512, 1] and geometry(host, 1 << 30, 511 * tbg + 1, 1)[4::3] == [513, 0]
    # pages: 1.34 x (0.2 + 0.06) hits per sampled k-mer, a page per wavefront of the probe kernel, 64 on top
    assert geometry(host, 1 << 30, 15000, 1)[6] == int(1.34 * (0.2 + 0.06 + 0.0) * float(1 << 30)) // 16384 + 256 * 16 + 64
    assert geometry(host, 1 << 30, 15000, 1, env={"DH_MJOIN_PAGES": "3"})[6:] == [3, 1]
    assert geometry(host, 1 << 30, 15000, 1, env={"DH_MJOIN_PAGES": str(1 << 30)})[6:] == [1 << 30, 0]
    # 2^20 tiles are too many
    assert geometry(host, 8192 * ((1 << 20) - 1), 15000, 1)[7] == 1 and geometry(host, 8192 * (1 << 20), 15000, 1)[7] == 0
    assert host.sp_mj_min_bases(*knobs({})) == 64 << 20 and host.sp_mj_min_bases(*knobs({"DH_MJOIN_MIN": "0"})) == 0
    assert host.sp_mj_chunk_size_ok((64 << 20) - 1, 64 << 20) == 0 and host.sp_mj_chunk_size_ok(64 << 20, 64 << 20) == 1
    assert host.sp_mj_chunk_size_ok((1 << 40) - 1, 0) == 1 and host.sp_mj_chunk_size_ok(1 << 40, 0) == 0


# ---- (b) the sweep
SWITCHES = {
    "DH_SEED_CAP": lambda r: str(1024 << r.randrange(5)),
    "DH_SEED_NO16K": lambda r: "1",
    "DH_SEED_NO_WAVE_TIER": lambda r: "1",
    "DH_SEED_NO_MID_TIER": lambda r: "1",
    "DH_SEED_BIG_PCT": lambda r: r.choice(["0", "1", "2.5", "10", "50", "100"]),
    "DH_MJOIN_MIN": lambda r: str(r.choice([0, 1, 1 << 20, 1 << 33])),
    "DH_MJOIN_PAGES": lambda r: str(r.choice([-1, 0, 1, 100, 1 << 30, 1 << 31])),
    "DH_NO_MJOIN": lambda r: "1",
    "DH_NO_TJOIN": lambda r: "1",
    "DH_TJOIN_CAP": lambda r: str(r.choice([-1, 0, 100, 8192, 10000])),
    "DH_TJOIN_HITCAP": lambda r: str(r.choice([-1, 0, 1, 4096, 1 << 33])),
}


def random_env(rng, i):
    """every switch on its own and every pair in turn, then random subsets"""
    names = sorted(SWITCHES)
    if i < len(names):
        pick = [names[i]]
    elif i < len(names) + len(names) * (len(names) - 1) // 2:
        pairs = [(a, b) for k, a in enumerate(names) for b in names[k + 1:]]
        pick = pairs[i - len(names)]
    else:
        pick = [n for n in names if rng.random() < 0.4]
    return {n: SWITCHES[n](rng) for n in pick}


def test_sweep_of_random_arguments_under_every_switch(host):
    rng = random.Random(20261020)
    L = host
    for i in range(3000):
        env = random_env(rng, i)
        kn = knobs(env)
        edge = rng.choice([1, 2, 511, 512, 513, 1365, 1366, 2047, 2048, 2049, 2730, 2731, 4096, 5461, 5462, 8192, 8193, 16384, 16385])
        mean = rng.choice([float(edge), edge / 1.5, edge / 1.5 + 1e-9, rng.uniform(0, 20000), rng.uniform(0, 600)])
        cap = 1024 << rng.randrange(5)
        kind = rng.randrange(4)
        nseg = rng.choice([0, 1, 2, 255, 256, 257, 512])
        cw, cm = rng.random() < 0.7, rng.random() < 0.7
        assert first_tier(L, kind, cap, mean, nseg, cw, cm, env) == ref_first_tier(kind, cap, mean, nseg, cw, cm, env), (i, env)
        held = rng.choice([0, 512, 2048, 4096, 8192, 16384])
        assert ladder(L, held, env) == ref.tier_ladder(held, ref.tier_max(env))
        # the call
        ix_n, kmer_mod, k, ng = rng.randrange(1, 1 << 28), rng.choice([0, 1, 2, 4, 8, 64]), rng.randrange(8, 29), rng.choice([0, 1, 7, 5000])
        dens = L.sp_chance_density(ix_n, kmer_mod, k, ng)
        assert dens == ref.dens(ix_n, kmer_mod, k, ng)
        max_len, nreads = rng.choice([1, 100, 1706, 1707, 15000, 60000, 1 << 24]), rng.randrange(0, 200000)
        jhist = [rng.choice([0, int(0.3 * nreads), int(0.3 * nreads) + 1, nreads]) for _ in range(4)]
        same, joined = rng.random() < 0.5, rng.random() < 0.5
        assert first_cap(L, max_len, kmer_mod, dens, same, joined, jhist, nreads, env) == ref.plan_cap(max_len, kmer_mod, dens, same, joined, jhist, nreads, env)
        assert L.sp_mj_min_bases(*kn) == ref.mj_min_bases(env)
        assert L.sp_tj_cap_entries(*kn, K, RATE0) == ref.tj_cap_entries(env, C)
        # the mapping join of a chunk
        bases = rng.choice([1, 4096, 8192, 8193, 53248, 53249, rng.randrange(1, 1 << 34), rng.randrange(1 << 34, 1 << 40)])
        hit_frac, ncu = rng.choice([0.2, 0.3, rng.uniform(0.2, 64.0)]), rng.choice([1, 64, 256, 304])
        assert bool(L.sp_mj_chunk_size_ok(bases, ref.mj_min_bases(env))) == ref.mj_chunk_wanted(bases, ref.mj_min_bases(env))
        got = geometry(L, bases, max_len, kmer_mod, hit_frac, dens, ncu, env)
        assert got == ref.mj_chunk(bases, max_len, kmer_mod, hit_frac, dens, ncu, env, C), (i, env)
        hits, unplaced = rng.randrange(0, 1 << 36), rng.choice([0, rng.randrange(0, 1 << 30)])
        assert regrow(L, got[6] if got[6] > 0 else 1, got[5], hits, unplaced, hit_frac) == ref.mj_pool_regrow(got[6] if got[6] > 0 else 1, got[5], hits, unplaced, hit_frac, C)
        # the table join of a chunk
        nr = rng.randrange(0, 80)
        group, g = [], 0
        for _ in range(nr):
            g += rng.random() < 0.15
            group.append(g)
        cr0 = rng.randrange(0, nr + 1)
        cr1 = rng.randrange(cr0, nr + 1)
        assert units(L, group or [0], cr0, cr1) == ref.tj_units(group, cr0, cr1, C)
        rate, cbases = rng.uniform(0.0, 2.0), rng.choice([0, 1, rng.randrange(0, 1 << 36)])
        assert L.sp_tj_first_hitcap(rate, cbases, *kn) == ref.tj_first_hitcap(rate, cbases, env)
        assert L.sp_tj_learned_rate(rate, hits, cbases, K, RATE0) == ref.tj_learned_rate(rate, hits, cbases, C)
        ni = rng.choice([1, 2, 3, 100, 1 << 18, 1 << 20])
        assert L.sp_mean_hits_expected(bases, ni, kmer_mod, dens) == ref.mean_hits_expected(bases, ni, kmer_mod, dens)
        assert L.sp_mean_hits_counted(hits, ni) == ref.mean_hits_counted(hits, ni)
        # the reads that overflowed
        nbig = rng.choice([0, 1, ni // 8, ni // 8 + 1, ni // 50 + 8, ni // 50 + 9, ni // 4, ni // 4 + 1, ni // 2])
        assert bool(L.sp_quarter_overflowed(nbig, ni)) == ref.quarter_overflowed(nbig, ni)
        redo_all = L.sp_redo_all_above(ni, cap, *kn)
        assert redo_all == ref.redo_all(ni, cap, env)
        assert bool(L.sp_cap_doubles(kind, nbig, redo_all, cap)) == ref.cap_doubles(kind != DIRECTORY, nbig, redo_all, cap)
        nit, item0 = rng.randrange(0, 40), 2 * rng.randrange(0, 1 << 30)
        ncand = [rng.choice([-1, -1, -2, 0, 5]) for _ in range(nit)]
        nhits = [rng.choice([0, 1, 1024, 1025, 4096, 8192, 8193, rng.randrange(0, 1 << 21)]) for _ in range(nit)]
        big, gcap = overflowed(L, ncand, nhits, item0)
        assert (big, gcap) == ref.list_overflowed(ncand, nhits, nit, item0)
        tier = rng.choice([2048, 8192, 16384])
        assert split(L, big, nhits, item0, tier) == ref.split_rung(big, nhits, item0, tier)
        gcap = rng.choice([gcap, 0, 1, 2, 3, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, rng.randrange(0, 1 << 23)])
        assert hbm(L, gcap) == ref.hbm_pass(gcap)
