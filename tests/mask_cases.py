"""Inputs of the mask-layer tests (dh_db_dust, dh_db_mask_coverage, dh_db_set_mask, dh_db_get_mask): constructed shapes at
the sizes where the kernels take another path or meet an edge.  Everything is seeded; every builder is cached and returns
what the CPU tests (tests/test_mask_ref.py) and the GPU tests (tests/test_parity_masklayer_gpu.py) both consume.  What a
builder claims about its own case -- that a window really has the score it is named for, that a DB really has the size that
switches a regime -- it asserts itself, on tests/mask_ref.py, never on the code under test.

A DUST case is a dict(db=SeqDb, ...); a coverage case is a dict(lens=, las=, intervals= (sequence, begin, end) rows,
thresholds=[(lower, upper), ...], ...)."""
import functools

import numpy as np

from dentist_amd import sim

import mask_ref as mr

LA_DTYPE = np.dtype([("tlen", "<i4"), ("diffs", "<i4"), ("abpos", "<i4"), ("bbpos", "<i4"), ("aepos", "<i4"), ("bepos", "<i4"),
                     ("flags", "<u4"), ("aread", "<i4"), ("bread", "<i4"), ("pad", "<i4"), ("toff", "<i8")])

REPEAT_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 66)
CHUNK_SWITCH = 16384     # dh_db_dust: max_len below this -> chunks of 64 window starts, from it on chunks of 512
SLAB = 65535             # sequences per launch of the coverage classification
SCAN_TOP_SLOTS = 2048 * 1024  # above this many slots the top level of the scan has more than one block sum per thread


def mask_of(db):
    return mr.dust_mask(db.bases, db.off)


def per_seq(ptr, iv, s):
    return [tuple(x) for x in np.asarray(iv).reshape(-1, 2)[ptr[s]:ptr[s + 1]].tolist()]


def is_clean(seq):
    return not mr.dust_flags(seq, np.array([0, len(seq)])).any()


def clean_random(rng, n):
    """n random bases without a low-complexity window"""
    while True:
        s = rng.integers(0, 4, n).astype(np.uint8)
        if is_clean(s):
            return s


def repeat(unit, n):
    unit = np.asarray(unit, dtype=np.uint8)
    return np.tile(unit, n // len(unit) + 1)[:n]


# ------------------------------------------------------------------------------------------------------------------ DUST
@functools.lru_cache(maxsize=None)
def dust_repeats(seed=1):
    """homopolymers, di- and trinucleotide repeats of REPEAT_LENGTHS, each a sequence of its own followed by a clean
    sequence of random length: the repeats and their neighbours begin on every residue mod 32 of the bitmap"""
    rng = np.random.default_rng(seed)
    seqs, kinds = [], []
    at, i = 0, 0
    for unit in ([0], [3], [0, 2], [1, 3], [0, 1, 2], [3, 3, 1]):
        for n in REPEAT_LENGTHS:
            seqs.append(repeat(unit, n))
            kinds.append((len(unit), n))
            i += 1
            fill = int(rng.integers(17, 90))
            fill += (11 * i - (at + n + fill)) % 32  # the next repeat begins on residue 11 i mod 32: all of them in turn
            seqs.append(clean_random(rng, fill))
            kinds.append((0, fill))
            at += n + fill
    db = sim.SeqDb.from_list(seqs)
    ptr, iv = mask_of(db)
    assert set((db.off[:-1:2] % 32).tolist()) == set(range(32))
    for s, (u, n) in enumerate(kinds):
        got = per_seq(ptr, iv, s)
        if u == 0 or n < 16:
            assert got == [], (s, u, n)            # no neighbour gets a bit, nothing shorter than a window is masked
        elif u in (1, 2):
            assert got == [(0, n)], (s, u, n)      # masked whole
        elif n < 32:
            assert got == [], (s, u, n)            # 14 triplets of three kinds: 10 + 10 + 6 = 26 = 2 (16 - 3), not above
        else:
            assert got == [(0, n)], (s, u, n)
    return dict(db=db, kinds=kinds)


def _score(win):
    c = np.bincount(mr.triplet_codes(win), minlength=64)
    return int((c * (c - 1) // 2).sum())


@functools.lru_cache(maxsize=None)
def _two_letter_windows_16():
    """all 65 536 windows of 16 bases over two letters, and their scores"""
    w = (np.arange(1 << 16)[:, None] >> np.arange(16)[None, :] & 1).astype(np.uint8)
    code = w[:, :-2] * 4 + w[:, 1:-1] * 2 + w[:, 2:]
    S = np.zeros(len(w), dtype=np.int64)
    for t in range(8):
        c = (code == t).sum(axis=1)
        S += c * (c - 1) // 2
    return w, S


def _window_with_score(rng, L, target):
    """a window of L bases (codes 0..3) whose score is exactly target.  L = 32, 64: tandem repeats with random substitutions,
    drawn until one fits.  L = 16: a score of 27 over 14 triplets is so rare (about one such draw in a million) that the
    window is taken from the complete list of two-letter windows instead (twelve of them score 27)."""
    if L == 16:
        w, S = _two_letter_windows_16()
        hits = np.flatnonzero(S == target)
        letters = rng.choice(4, size=2, replace=False).astype(np.uint8)
        return letters[w[int(rng.choice(hits))]]
    while True:
        win = repeat(rng.integers(0, 4, int(rng.integers(1, 9))), L).copy()
        k = int(rng.integers(0, L // 2))
        win[rng.integers(0, L, k)] = rng.integers(0, 4, k)
        if _score(win) == target:
            return win


@functools.lru_cache(maxsize=None)
def dust_thresholds(seed=2):
    """per window length L two sequences: one whose only low-complexity window has S = 2 (L - 3) + 1 (masked, exactly that
    window), one with a window of S = 2 (L - 3) and no window above (clear)"""
    rng = np.random.default_rng(seed)
    seqs, want = [], []
    for L in mr.DUST_WINDOWS:
        T = mr.dust_threshold(L)
        for target in (T + 1, T):
            while True:
                left, right = int(rng.integers(20, 90)), int(rng.integers(20, 90))
                seq = np.concatenate([rng.integers(0, 4, left), _window_with_score(rng, L, target), rng.integers(0, 4, right)]).astype(np.uint8)
                sc = mr.window_scores(seq)
                low = [(M, int(a)) for M in mr.DUST_WINDOWS for a in np.flatnonzero(sc[M][0] > mr.dust_threshold(M))]
                if int(sc[L][0][left]) != target:
                    continue
                if target == T + 1 and low == [(L, left)]:
                    break
                if target == T and low == []:
                    break
            seqs.append(seq)
            want.append((L, target, left))
    db = sim.SeqDb.from_list(seqs)
    ptr, iv = mask_of(db)
    for s, (L, target, left) in enumerate(want):
        assert per_seq(ptr, iv, s) == ([(left, left + L)] if target > mr.dust_threshold(L) else []), (s, L, target)
    assert sorted((L, t - mr.dust_threshold(L)) for L, t, _ in want) == [(L, d) for L in mr.DUST_WINDOWS for d in (0, 1)]
    return dict(db=db, want=want)


@functools.lru_cache(maxsize=None)
def dust_nonbase(seed=3):
    """a dinucleotide run of 48 bases between clean flanks with one non-base code at its first base, at its last base, one
    base before it, one base after it and in its middle; codes 4, 5 and 255; a sequence of code 4 only"""
    rng = np.random.default_rng(seed)
    left, right, run = clean_random(rng, 85), clean_random(rng, 91), repeat([1, 2], 48)
    base = np.concatenate([left, run, right])
    r0, r1 = len(left), len(left) + len(run)
    places = {"first": r0, "last": r1 - 1, "before": r0 - 1, "after": r1, "middle": (r0 + r1) // 2}
    seqs, names = [base], ["plain"]
    for code in (4, 5, 255):
        for name, p in places.items():
            s = base.copy()
            s[p] = code
            seqs.append(s)
            names.append(f"{name}_{code}")
    seqs.append(np.full(70, 4, dtype=np.uint8))
    names.append("all_4")
    seqs.append(np.concatenate([repeat([0], 20), [4], repeat([0], 15)]).astype(np.uint8))  # 20 masked, 15 too short
    names.append("split_homopolymer")
    db = sim.SeqDb.from_list(seqs)
    ptr, iv = mask_of(db)
    m = {n: per_seq(ptr, iv, s) for s, n in enumerate(names)}
    # windows that hold a few flank bases beside the run are low-complexity too: the plain mask reaches into both flanks
    (pb, pe), = m["plain"]
    assert 0 < pb < r0 and r1 < pe < len(base)
    for code in (4, 5, 255):
        (b, e), = m[f"first_{code}"]
        assert b == r0 + 1 and r1 <= e <= pe
        (b, e), = m[f"before_{code}"]
        assert b == r0 and r1 <= e <= pe
        (b, e), = m[f"last_{code}"]
        assert e == r1 - 1 and pb <= b <= r0
        (b, e), = m[f"after_{code}"]
        assert e == r1 and pb <= b <= r0
        (b, e), (b2, e2) = m[f"middle_{code}"]
        assert e == places["middle"] and b2 == places["middle"] + 1 and b >= pb and e2 <= pe
        assert all(m[f"{n}_{code}"] == m[f"{n}_4"] for n in places)
    assert m["all_4"] == [] and m["split_homopolymer"] == [(0, 20)]
    return dict(db=db, names=names)


def _plant(seq, where, rng):
    """runs of 34 to 80 bases (homopolymer, di- or trinucleotide) at [begin, ...) or (..., end] positions"""
    for kind, p in where:
        n = int(rng.integers(34, 81))
        unit = rng.integers(0, 4, int(rng.integers(1, 4)))
        if len(unit) > 1 and len(set(unit.tolist())) == 1:
            unit = unit[:1]
        b = {"across": p - n // 2, "begin": p, "end": p - n}[kind]
        assert 0 <= b and b + n <= len(seq), (kind, p, n)
        seq[b:b + n] = repeat(unit, n)


@functools.lru_cache(maxsize=None)
def dust_borders(max_len, seed=4):
    """a DB whose longest sequence has max_len bases, with runs planted across, at and before the chunk borders (64 j below
    CHUNK_SWITCH, 512 j from it on), the tile border (256 chunks = 131 072 window starts in the 512 regime; in the 64 regime a
    tile is 16 384 starts and no sequence reaches a second one: the runs at 16 384 lie across the last base, and across
    and from bit 16 384 of the bitmap in the second sequence) and ending at the sequence end; then short sequences around
    the window lengths, a second planted sequence, and the reverse complement of the first"""
    rng = np.random.default_rng(seed + max_len)
    chunk = 64 if max_len < CHUNK_SWITCH else 512
    main = rng.integers(0, 4, max_len).astype(np.uint8)
    tile = 256 * chunk
    js = [j for j in (1, 2, 3, 7, 31, 100, 200, 255, 256, 257) if chunk * j + 45 < max_len]
    where = [("across", chunk * j) for j in js]
    where += [("begin", chunk * j) for j in (5, 50, 150) if chunk * j + 100 < max_len]
    where += [("end", chunk * j) for j in (9, 60, 170) if chunk * j + 100 < max_len]
    where.append(("end", max_len))
    _plant(main, where, rng)
    second = rng.integers(0, 4, tile + 1000 if max_len > tile + 1000 else 5000).astype(np.uint8)
    w2 = [("across", 1000), ("begin", chunk), ("end", len(second))]
    if len(second) > tile:
        w2.append(("begin", tile))                  # begins exactly at the tile border
    g = CHUNK_SWITCH - max_len                      # bit 16 384 of the bitmap, where the second sequence holds it
    if 40 <= g <= 4000:
        w2 += [("across", g), ("begin", g + 200)]
    _plant(second, w2, rng)
    shorts = [repeat([0], n) for n in (15, 16, 17)] + [clean_random(rng, 33), repeat([1, 0], 64)]
    seqs = [main, second] + shorts + [sim.revcomp(main)]
    db = sim.SeqDb.from_list(seqs)
    assert int(np.diff(db.off).max()) == max_len
    ptr, iv = mask_of(db)
    fwd = np.asarray(per_seq(ptr, iv, 0)).reshape(-1, 2)
    rev = np.asarray(per_seq(ptr, iv, db.n - 1)).reshape(-1, 2)
    assert len(fwd) >= 5 and np.array_equal((max_len - fwd[:, ::-1])[::-1], rev)  # the mirror image
    assert any(e == max_len for _, e in fwd.tolist())
    flags = mr.flags_of(ptr, iv, db.off)
    for j in js:  # a run really straddles the border: the last start of one chunk and the first of the next are masked
        assert flags[chunk * j - 1] and flags[chunk * j], j
    if max_len > tile + 1000:
        assert flags[tile - 1] and flags[tile] and flags[max_len + tile] and flags[max_len + tile + 33]
    return dict(db=db, chunk=chunk)


@functools.lru_cache(maxsize=None)
def short_db(seed=5, n=70_000):
    """n sequences of 20 to 70 bases, about a third of them repeats of a unit of one to three bases: more sequences than one
    launch of the coverage classification takes (SLAB), more slots than SCAN_TOP_SLOTS"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(20, 71, n)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    total = int(off[-1])
    bases = rng.integers(0, 4, total).astype(np.uint8)
    seq = np.repeat(np.arange(n), lens)
    pos = np.arange(total) - off[seq]
    ulen = rng.integers(1, 4, n)
    units = rng.integers(0, 4, (n, 3))
    low = rng.random(n) < 1 / 3
    rep = units[seq, pos % ulen[seq]].astype(np.uint8)
    bases = np.where(low[seq], rep, bases)
    db = sim.SeqDb(bases, off)
    assert db.n > SLAB + 2 and total + n + 2 > SCAN_TOP_SLOTS and 2_900_000 < total < 3_400_000
    return dict(db=db, lens=lens, low=low)


@functools.lru_cache(maxsize=None)
def short_dust():
    """the reference mask of short_db(), computed once for the tests that share it"""
    db = short_db()["db"]
    return mr.dust_mask(db.bases, db.off)


# -------------------------------------------------------------------------------------------------------------- coverage
def las_of(intervals, bread=None, bb=None, be=None):
    """records whose A side is the (sequence, begin, end) rows"""
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 3)
    las = np.zeros(len(iv), dtype=LA_DTYPE)
    las["aread"], las["abpos"], las["aepos"] = iv[:, 0], iv[:, 1], iv[:, 2]
    las["bread"] = np.arange(len(iv)) if bread is None else bread
    las["bbpos"] = 0 if bb is None else bb
    las["bepos"] = iv[:, 2] - iv[:, 1] if be is None else be
    return las


STACK = 70_000


@functools.lru_cache(maxsize=None)
def coverage_short(seed=6):
    """on short_db(): intervals at both ends of the first launch's last sequences and the second launch's first ones, whole
    sequences, last bases, first bases, an empty interval, a few thousand random ones, and sequence SLAB covered STACK deep"""
    rng = np.random.default_rng(seed)
    lens = short_db()["lens"]
    n = len(lens)
    L = lambda s: int(lens[s])
    rows = [(0, 0, L(0)), (1, L(1) - 1, L(1)), (SLAB - 2, 0, 1), (SLAB - 1, 5, 5), (SLAB - 1, 0, L(SLAB - 1)),
            (SLAB + 1, 0, L(SLAB + 1)), (SLAB + 1, 0, L(SLAB + 1)), (SLAB + 1, L(SLAB + 1) - 1, L(SLAB + 1)),
            (SLAB + 2, 0, 1), (SLAB + 2, 0, L(SLAB + 2)), (SLAB + 2, L(SLAB + 2), L(SLAB + 2)),
            (n - 1, L(n - 1) - 1, L(n - 1)), (n - 1, 0, L(n - 1)), (n - 1, 0, L(n - 1))]
    special = sorted({r[0] for r in rows} | {SLAB})
    assert special == [0, 1, SLAB - 2, SLAB - 1, SLAB, SLAB + 1, SLAB + 2, n - 1]
    for _ in range(4000):
        s = int(rng.integers(2, n - 1))
        if s in special:
            continue
        b = int(rng.integers(0, L(s)))
        rows.append((s, b, int(min(L(s), b + rng.integers(1, 40)))))
        if rng.random() < 0.5:  # pile a few more onto the same sequence: coverage 2, 3, 4 next to 1
            for _ in range(int(rng.integers(1, 5))):
                b2 = int(rng.integers(0, L(s)))
                rows.append((s, b2, int(min(L(s), b2 + rng.integers(1, 40)))))
    sb, se = 3, L(SLAB) - 2
    rows += [(SLAB, sb, se)] * STACK + [(SLAB, sb + 4, se - 3)]   # STACK on [sb, sb + 4) and [se - 3, se), STACK + 1 between
    iv = np.asarray(rows, dtype=np.int64)
    iv = iv[rng.permutation(len(iv))]
    thresholds = [(0, 1), (1, 3), (0, STACK - 1), (0, STACK), (2, 2 ** 31 - 1)]
    case = dict(lens=lens, intervals=iv, las=las_of(iv), thresholds=thresholds)
    # what the case is named for, on the reference
    off = short_db()["db"].off
    masks = [mr.coverage_flags(lens, iv, lo, up) for lo, up in thresholds]
    counts = [int(m.sum()) for m in masks]
    assert all(c > 0 for c in counts) and len(set(counts)) == len(counts), counts
    o = int(off[SLAB])
    assert masks[2][o + sb:o + se].all() and not masks[2][o:o + sb].any() and counts[2] == se - sb
    assert masks[3][o + sb + 4:o + se - 3].all() and counts[3] == se - sb - 7      # STACK met exactly on 7 bases: clear
    assert masks[1][o + sb:o + se].all() and not masks[4][o + sb:o + se].any()
    o1 = int(off[SLAB + 1])
    assert masks[0][o1:o1 + L(SLAB + 1)].all()                                                  # coverage 2 and 3: above upper 1
    assert not masks[1][o1:o1 + L(SLAB + 1)].any() and not masks[4][o1:o1 + L(SLAB + 1)].any()  # 2 and 3 inside [1, 3] and [2, ..]
    assert masks[4][off[0]:off[1]].all() and not masks[1][off[0]:off[1]].any()                  # coverage 1: below lower 2
    assert int(off[-1]) + len(lens) + 2 > SCAN_TOP_SLOTS
    return case


@functools.lru_cache(maxsize=None)
def coverage_tiny():
    """sequences of one and two bases, empty sequences between covered ones, intervals [0, len), [len - 1, len), [0, 1), b == e"""
    lens = np.array([1, 2, 5, 0, 5, 1, 2, 0, 0, 3, 1], dtype=np.int64)
    rows = [(0, 0, 1), (1, 0, 2), (1, 1, 2), (2, 0, 5), (2, 4, 5), (3, 0, 0), (4, 0, 1), (4, 2, 5), (4, 2, 2), (5, 0, 0), (5, 1, 1),
            (6, 0, 1), (6, 0, 1), (9, 0, 3), (9, 1, 2), (9, 1, 2), (10, 0, 1), (10, 0, 1), (10, 0, 1)]
    iv = np.asarray(rows, dtype=np.int64)
    case = dict(lens=lens, intervals=iv, las=las_of(iv), thresholds=[(0, 0), (1, 1), (1, 2), (2, 2), (0, 3), (3, 3), (4, 9)])
    ptr, m = mr.coverage_mask(lens, iv, 1, 2)
    assert [per_seq(ptr, m, s) for s in range(len(lens))] == [[], [], [], [], [(1, 2)], [(0, 1)], [(1, 2)], [], [], [(1, 2)], [(0, 1)]]
    return case


@functools.lru_cache(maxsize=None)
def improper_cases():
    """per allowance (0 and 7) sixteen records, each on a contig and a read of its own (all of differing lengths): the begin
    is within the allowance exactly or misses it by one, on A or on B; the same for the end.  Four of sixteen are proper."""
    rows, alens, blens, for_allowance = [], [], [], []
    i = 0
    for allowance in (0, 7):
        for bk in ("a_in", "a_out", "b_in", "b_out"):
            for ek in ("a_in", "a_out", "b_in", "b_out"):
                alen, blen = 800 + 13 * i, 300 + 7 * i
                ab, bb = {"a_in": (allowance, 50), "a_out": (allowance + 1, 50), "b_in": (100, allowance), "b_out": (100, allowance + 1)}[bk]
                ae, be = {"a_in": (alen - allowance, 200), "a_out": (alen - allowance - 1, 200), "b_in": (600, blen - allowance),
                          "b_out": (600, blen - allowance - 1)}[ek]
                rows.append((i, ab, ae, i, bb, be))
                alens.append(alen)
                blens.append(blen)
                for_allowance.append((allowance, bk.endswith("in") and ek.endswith("in")))
                i += 1
    r = np.asarray(rows, dtype=np.int64)
    las = las_of(r[:, :3], bread=r[:, 3], bb=r[:, 4], be=r[:, 5])
    alens, blens = np.asarray(alens, dtype=np.int64), np.asarray(blens, dtype=np.int64)
    for la, (allowance, proper) in zip(las, for_allowance):
        assert mr.improper(la, alens[la["aread"]], blens[la["bread"]], allowance) == (not proper)
    for allowance in (0, 7):
        n = sum(mr.improper(la, alens[la["aread"]], blens[la["bread"]], allowance) for la in las)
        assert n == (12 + 16 if allowance == 0 else 12), (allowance, n)  # of the other allowance's records: all / none
    return dict(lens=alens, las=las, read_off=np.concatenate([[0], np.cumsum(blens)]).astype(np.int64), read_len=blens,
                allowances=(0, 7), thresholds=[(0, 0), (1, 1)])


def improper_intervals(case, allowance):
    las = case["las"]
    keep = [mr.improper(la, case["lens"][la["aread"]], case["read_len"][la["bread"]], allowance) for la in las]
    return np.asarray([(int(la["aread"]), int(la["abpos"]), int(la["aepos"])) for la, k in zip(las, keep) if k], dtype=np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------- layers
@functools.lru_cache(maxsize=None)
def layers(seed=7):
    """a DB of sequences that share bitmap words with their neighbours; two user tracks whose intervals begin and end on
    every residue mod 32 of the bitmap, among them [0, len) of a sequence that shares its first and its last word; alignments
    for two coverage masks"""
    rng = np.random.default_rng(seed)
    lens = [40, 70, 33, 100, 64, 17, 200, 31, 90, 1, 0, 45, 129, 63, 32, 32, 77, 300, 5, 58]
    lens += [n + 3 for n in lens] + [150, 260]
    seqs = []
    for i, n in enumerate(lens):
        s = rng.integers(0, 4, n).astype(np.uint8)
        if i % 3 == 0 and n >= 40:
            s[n // 4:n // 4 + 24] = repeat([i % 4], 24)
        seqs.append(s)
    db = sim.SeqDb.from_list(seqs)
    off = db.off

    def track(shift):
        """begins walk through the residues in steps of 5, ends in steps of 7 (from `shift` on)"""
        ptr, iv, rb, re = [0], [], shift, shift
        for s, n in enumerate(lens):
            o = int(off[s])
            if s == 3:
                iv.append((0, n))
            else:
                at = 0
                while True:
                    b = at + (rb - (o + at)) % 32
                    e = b + 1 + (re - (o + b + 1)) % 32
                    if e > n:
                        break
                    iv.append((b, e))
                    rb, re, at = (rb + 5) % 32, (re + 7) % 32, e + 1
            ptr.append(len(iv))
        return np.asarray(ptr, dtype=np.int64), np.asarray(iv, dtype=np.int32).reshape(-1)
    user1, user2 = track(0), track(3)
    for ptr, iv in (user1, user2):
        v = iv.reshape(-1, 2)
        s = np.repeat(np.arange(len(lens)), np.diff(ptr))
        assert set(((off[s] + v[:, 0]) % 32).tolist()) == set(range(32)) and set(((off[s] + v[:, 1]) % 32).tolist()) == set(range(32))
    assert off[3] % 32 and off[4] % 32 and off[3] // 32 == (off[3] - 1) // 32 and (off[4] - 1) // 32 == off[4] // 32
    assert not np.array_equal(user1[1], user2[1])
    rows = []
    for s, n in enumerate(lens):
        for _ in range(3 if n >= 5 else 0):
            b = int(rng.integers(0, n))
            rows.append((s, b, int(min(n, b + rng.integers(1, 60)))))
    iv = np.asarray(rows, dtype=np.int64)
    case = dict(db=db, lens=np.asarray(lens, dtype=np.int64), user1=user1, user2=user2, intervals=iv, las=las_of(iv), cov1=(0, 1), cov2=(1, 5))
    d = mr.dust_flags(db.bases, off)
    c1, c2 = (mr.coverage_flags(case["lens"], iv, *t) for t in (case["cov1"], case["cov2"]))
    u1 = mr.flags_of(*user1, off)
    assert d.any() and (c1 & ~d & ~u1).any() and (c2 & ~c1 & ~d).any() and (u1 & ~d & ~c1).any() and (d & ~u1).any()
    return case


# ------------------------------------------------------------------------------------------------------- k-mer consumption
K = 14


@functools.lru_cache(maxsize=None)
def kmer_edges(seed=8, n=600):
    """A = one random sequence whose k-mers are unique on both strands, B = its copy; single masked bases at the positions
    where the set of k-mers that touch them changes shape, and an interval that ends at the sequence end"""
    rng = np.random.default_rng(seed)
    while True:
        a = rng.integers(0, 4, n).astype(np.uint8)
        kmers = {bytes(s[q:q + K]) for s in (a, sim.revcomp(a)) for q in range(n - K + 1)}
        if len(kmers) == 2 * (n - K + 1):
            break
    places = {"first": 0, "second": 1, "k-1": K - 1, "k": K, "len-k-1": n - K - 1, "len-k": n - K, "last": n - 1}
    masks = {name: (p, p + 1) for name, p in places.items()}
    masks["tail"] = (n - 5, n)
    return dict(seq=a, masks=masks, k=K, starts=n - K + 1)


def kmer_drop(case, b, e):
    """k-mer starts whose k bases touch [b, e)"""
    n, k = len(case["seq"]), case["k"]
    return min(e - 1, n - k) - max(0, b - k + 1) + 1


def masked_db(seq, iv):
    db = sim.SeqDb.from_list([seq])
    if iv is not None:
        db.mask = (np.array([0, 1], dtype=np.int64), np.array(list(iv) + [0, 0], dtype=np.int32))
    return db
