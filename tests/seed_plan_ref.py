"""The decisions of the seed stage of an alignment call restated in Python, from the text of plan_seeds, plan_mj_chunk and
seed_chunk as they stood in dentist_amd/csrc/dh_align.cpp before the seed plan became a header of its own -- statement
by statement, with the development switches read from an `env` dict where that text called getenv, and the constants
of the kernel headers from a `C` dict (their #define names).  tests/test_seed_plan.py holds dh_seed_plan.h against it.

C arithmetic is kept: a cast to an integer truncates (int()), integers divide downwards (all operands are >= 0 here),
doubles are Python floats and see the same operations in the same order."""


def atoi(s):
    return int(s)


def dens(ix_n, kmer_mod, k, ngroups):
    return float(ix_n) * max(1, kmer_mod) / 4.0 ** k / max(1, ngroups)


def plan_cap(max_len, kmer_mod, dens_, same_db, use_join, jhist, nreads, env):
    exp_hits = float(max_len) / max(1, kmer_mod) * (2.0 * dens_ + 0.1)
    cap = 1024
    while cap < 16384 and exp_hits * 1.5 >= cap:
        cap *= 2
    if same_db:
        cap = 1024
        while cap < 8192 and 0.6 * max_len > cap:
            cap *= 2
    if use_join:
        tol = int(0.3 * nreads)
        cap = 2048 if jhist[0] <= tol else (4096 if jhist[1] <= tol else (8192 if jhist[2] <= tol else 16384))
    if "DH_SEED_CAP" in env:
        cap = atoi(env["DH_SEED_CAP"])
    return cap


def mj_min_bases(env):
    m = 64 << 20
    if "DH_MJOIN_MIN" in env:
        m = atoi(env["DH_MJOIN_MIN"])
    return m


def mj_chunk_wanted(bases, min_bases):
    return not (bases < min_bases or bases >= (1 << 40))


def tj_cap_entries(env, C):
    tcap = C["TJ_CAP"]
    if "DH_TJOIN_CAP" in env:
        tcap = max(0, min(C["TJ_CAP"], atoi(env["DH_TJOIN_CAP"])))
    return tcap


def mj_chunk(bases, max_len, kmer_mod, hit_frac, dens_, ncu, env, C):
    """plan_mj_chunk's geometry: tb, ntiles, ntiles_pad, ngroups, nseg, exp_ent, npages, fits"""
    kmer_mod = max(1, kmer_mod)
    tb = (C["MJ_CAP"] // 16 * 13) * kmer_mod
    if kmer_mod == 1:
        tb = C["MJ_CAP"]
    tb = min(tb, (1 << C["MJ_POSBITS"]) - 64)
    tb = max(C["MJ_THREADS"] * 8, tb // (C["MJ_THREADS"] * 8) * (C["MJ_THREADS"] * 8))
    ntiles = (bases + tb - 1) // tb
    ntiles_pad = (ntiles + C["MJ_BATCH"] - 1) // C["MJ_BATCH"] * C["MJ_BATCH"]
    ngroups = ntiles_pad // C["MJ_GROUP"]
    tbg = tb * C["MJ_GROUP"]
    nseg = (max_len + tbg - 1) // tbg + 1
    exp_ent = bases // kmer_mod
    npages = int(1.34 * (hit_frac + 0.06 + 2.5 * dens_) * float(exp_ent)) // C["MJ_PAGE"] + ncu * (C["MJ_PROBE_THREADS"] // 64) + 64
    if "DH_MJOIN_PAGES" in env:
        npages = max(1, atoi(env["DH_MJOIN_PAGES"]))
    fits = not (ntiles >= (1 << 30) // C["MJ_P"] or npages >= (1 << 31) // 2 or nseg > 512)
    return [tb, ntiles, ntiles_pad, ngroups, nseg, exp_ent, npages, int(fits)]


def mj_pool_regrow(npages, exp_ent, hits, unplaced, hit_frac, C):
    """have, need, the new mj_hit_frac, and whether the chunk runs through the join again"""
    have = float(npages) * C["MJ_PAGE"] / 1.34
    need = 1.2 * max(have + float(unplaced), float(hits)) / max(1.0, float(exp_ent))
    hit_frac = max(hit_frac * 1.5, need)
    return have, need, hit_frac, hit_frac <= 64.0


def tj_units(group, cr0, cr1, C):
    units = []
    rd = cr0
    while rd < cr1:
        g = group[rd]
        e = rd + 1
        while e < cr1 and e - rd < C["TJ_RUN"] and group[e] == g:
            e += 1
        units.append((g, rd, e))
        rd = e
    return units


def tj_first_hitcap(rate, cbases, env):
    hcap = int(1.25 * rate * float(cbases)) + 4096
    if "DH_TJOIN_HITCAP" in env:
        hcap = max(1, atoi(env["DH_TJOIN_HITCAP"]))
    return hcap


def tj_learned_rate(rate, hits, cbases, C):
    if cbases > 0:
        rate = max(C["DH_TJ_HIT_RATE0"], float(hits) / float(cbases))
    return rate


def mean_hits_expected(bases, ni, kmer_mod, dens_):
    kmers_per_read = float(bases) / max(1, ni // 2) / max(1, kmer_mod)
    return kmers_per_read * (2.0 * dens_ + 0.075)


def mean_hits_counted(tj_hits, ni):
    return float(tj_hits) / max(1, ni // 2)


def tier_max(env):
    return 8192 if "DH_SEED_NO16K" in env else 16384


def first_tier(use_join, mj_chunk_, tj_chunk, cap, mean_hits, nseg, ctx_wave, ctx_mid, env, C):
    """capj, wave_tier, mid_tier and the words per block of the slab scratch the launch is handed (0: a null pointer)"""
    fscr = 0
    if cap > 4096 and cap <= 8192:
        fscr = C["DH_SEED_FSCR_WORDS"]
    jn = use_join or mj_chunk_ or tj_chunk
    tmax = tier_max(env)
    wave_tier = (mj_chunk_ or tj_chunk) and ctx_wave and 1.5 * mean_hits <= 512.0 and "DH_SEED_NO_WAVE_TIER" not in env
    capj = min(max(cap, 2048), tmax)
    if mj_chunk_ or tj_chunk:
        capj = 2048
        while capj < tmax and 1.5 * mean_hits > capj:
            capj *= 2
        if wave_tier:
            capj = 512
    mid_tier = ((mj_chunk_ or tj_chunk) and not wave_tier and capj == 2048 and ctx_mid and (not mj_chunk_ or nseg <= 256)
                and "DH_SEED_NO_MID_TIER" not in env)
    if jn and capj > 4096:
        fscr = C["DH_SEED_FSCR_WORDS16"] if capj > 8192 else C["DH_SEED_FSCR_WORDS"]
    return [capj, int(bool(wave_tier)), int(bool(mid_tier)), fscr]


def tier_fscr_words(tier, C):
    return C["DH_SEED_FSCR_WORDS16"] if tier > 8192 else C["DH_SEED_FSCR_WORDS"]


def fscr_total_words(per_block, ncu, C):
    return ncu * C["DH_SEED_FSCR_BLOCKS_PER_CU"] * per_block


def list_overflowed(ncand, nhits, ni, item0):
    big, gcap = [], 0
    for it in range(0, ni - 1, 2):
        if ncand[it] == -1:
            big.append((item0 + it) >> 1)
            gcap = max(gcap, nhits[it] + nhits[it + 1])
    return big, gcap


def quarter_overflowed(nbig, ni):
    return nbig * 4 > ni // 2


def redo_all(ni, cap, env):
    v = ni // 50 + 8
    if cap >= 8192:
        v = ni // 4
    if "DH_SEED_BIG_PCT" in env:
        v = int(float(ni) * float(env["DH_SEED_BIG_PCT"]) / 200.0)
    return v


def cap_doubles(jn, nbig, redo_all_, cap):
    return (not jn) and nbig > redo_all_ and cap < 16384


def tier_ladder(held, tmax):
    """the tiers the loop over the list tiers runs its body for (it is entered for held < tmax only)"""
    tiers = []
    if not held < tmax:
        return tiers
    tier = 2048 if held < 2048 else 8192
    while tier <= tmax:
        if not tier <= held:
            tiers.append(tier)
        tier = 8192 if tier < 8192 else tier * 2
    return tiers


def split_rung(big, nhits, item0, tier):
    mid, huge, gcap2 = [], [], 0
    for rd in big:
        it = 2 * rd - item0
        nh = nhits[it] + nhits[it + 1]
        if nh <= tier:
            mid.append(rd)
        else:
            huge.append(rd)
            gcap2 = max(gcap2, nh)
    return mid, huge, gcap2


def hbm_pass(gcap):
    """refused, pow2, slab_words, per_launch"""
    if gcap > (1 << 22):
        return True, None, None, None
    pow2 = 1
    while pow2 < gcap:
        pow2 <<= 1
    slab_words = 2 * pow2 + (pow2 + 1) // 2
    per_launch = max(1, (2 << 30) // (slab_words * 8))
    return False, pow2, slab_words, per_launch
