"""Constructed chains for the chain padder's tests: records WITH VALID TRACES cut out of one known edit script between A and
B at given A positions (a trace tile = the script's non-zero ops and B bases per A tile), shifted copies of them where a case
needs a tandem duplicate or an inserted stretch, COMP variants that store the reverse complement of B.  All at tspace 100.
Not a test module."""
import numpy as np

from dentist_amd import _lib, sim

TS = 100
OK, FAKED, NESTED = 0, 1, 2


class Script:
    """A0 (n random bases), B0 = A0 under a known edit script of divergence div; bm[a] = B bases in front of A base a,
    dz[a] = non-zero ops in front of the op that consumes A base a"""

    def __init__(self, seed, n, div=0.12, a0=None):
        rng = np.random.default_rng(seed)
        self.A0 = rng.integers(0, 4, n).astype(np.uint8) if a0 is None else np.asarray(a0, np.uint8)[:n]
        n = len(self.A0)
        x = rng.random(n)
        b, self.bm, self.dz = [], np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
        d = 0
        for i in range(n):
            if 2 * div / 3 <= x[i] < div:  # an insertion in front of the base
                b.append(int(rng.integers(0, 4)))
                d += 1
            self.bm[i], self.dz[i] = len(b), d
            if x[i] < div / 3:  # deletion
                d += 1
            elif x[i] < 2 * div / 3:  # substitution
                b.append((int(self.A0[i]) + 1 + int(rng.integers(0, 3))) % 4)
                d += 1
            else:
                b.append(int(self.A0[i]))
        self.bm[n], self.dz[n] = len(b), d
        self.B0 = np.asarray(b, np.uint8)


class Builder:
    def __init__(self):
        self.las, self.trace = [], []

    def rec(self, sc, a0, a1, aread=0, bread=0, ashift=0, bshift=0, comp=False, nxt=False):
        ab, ae = a0 + ashift, a1 + ashift
        cuts = [ab] + list(range((ab // TS + 1) * TS, ae, TS)) + [ae]
        toff = len(self.trace)
        diffs = 0
        for x, y in zip(cuts[:-1], cuts[1:]):
            d, nb = int(sc.dz[y - ashift] - sc.dz[x - ashift]), int(sc.bm[y - ashift] - sc.bm[x - ashift])
            self.trace += [d, nb]
            diffs += d
        la = np.zeros(1, _lib.LA_DTYPE)[0]
        la["tlen"], la["toff"], la["diffs"] = len(self.trace) - toff, toff, diffs
        la["abpos"], la["aepos"] = ab, ae
        la["bbpos"], la["bepos"] = int(sc.bm[a0]) + bshift, int(sc.bm[a1]) + bshift
        la["flags"] = (1 if comp else 0) | (8 if nxt else 4)
        la["aread"], la["bread"] = aread, bread
        self.las.append(la)

    def chain(self, sc, cuts, **kw):
        """records (a0, a1[, ashift, bshift]) of one chain"""
        for k, c in enumerate(cuts):
            a0, a1, ash, bsh = (list(c) + [0, 0])[:4]
            self.rec(sc, a0, a1, ashift=ash, bshift=bsh, nxt=k > 0, **kw)

    def case(self, A, B, comp=False, **extra):
        las = np.asarray(self.las, dtype=_lib.LA_DTYPE) if self.las else np.zeros(0, _lib.LA_DTYPE)
        Bs = [sim.revcomp(b) for b in B] if comp else B
        return dict(A=sim.SeqDb.from_list(A), B=sim.SeqDb.from_list(Bs), las=las, trace=np.asarray(self.trace, np.uint16), ts=TS,
                    chain_off=None, **extra)


def simple(sc, cuts, expect=OK, fillers=True, comp=False, A=None, B=None):
    b = Builder()
    b.chain(sc, cuts, comp=comp)
    return b.case([sc.A0 if A is None else A], [sc.B0 if B is None else B], comp=comp, expect=[expect], fillers=fillers)


def cat(*parts):
    return np.concatenate(parts).astype(np.uint8)


def build_cases():
    sc = Script(7, 3000)
    A0, B0, bm = sc.A0, sc.B0, sc.bm
    rng = np.random.default_rng(99)
    rnd = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    c = {}
    c["single"] = simple(sc, [(150, 2750)], fillers=False)
    c["gap_both"] = simple(sc, [(100, 1000), (1130, 2500)])
    d = int(bm[1130] - bm[1000])
    c["gap_a_only"] = simple(sc, [(100, 1000), (1130, 2500, 0, -d)], B=cat(B0[:bm[1000]], B0[bm[1130]:]), fillers=False)
    c["gap_b_only"] = simple(sc, [(100, 1000), (1000, 2500, 0, 57)], B=cat(B0[:bm[1000]], rnd(57), B0[bm[1000]:]), fillers=False)
    c["gap_none"] = simple(sc, [(100, 1000), (1000, 2500)], fillers=False)
    c["overlap_both_mid_tile"] = simple(sc, [(100, 1250), (1130, 2500)])
    c["overlap_both_on_grid"] = simple(sc, [(100, 1200), (1100, 2500)])
    # q's B frame is 60 bases in front of the script's: the A and the B resolution pick different trace points (the tail of p
    # no longer matches its trace's diffs, which sends its tiles to the full-matrix kernel)
    c["overlap_both_picks_differ"] = simple(sc, [(100, 1250), (1130, 2500, 0, -60)], B=cat(B0[:bm[1130] - 60], B0[bm[1130]:]))
    d = int(bm[1250] - bm[1190])
    c["overlap_a_only_tandem"] = simple(sc, [(100, 1250), (1190, 2500, 0, d)], B=cat(B0[:bm[1250]], B0[bm[1190]:]))
    c["overlap_b_only"] = simple(sc, [(100, 1250), (1190, 2500, 60, 0)], A=cat(A0[:1250], A0[1190:]))
    c["three_gap_then_overlap"] = simple(sc, [(100, 900), (1000, 1850), (1730, 2800)])
    five = [(50, 600), (650, 1250), (1180, 1700), (1760, 2300), (2210, 2900)]
    c["five_alternating"] = simple(sc, five)
    c["zero_tiles_of_p"] = simple(sc, [(100, 1000), (900, 1040), (1000, 2000)])
    c["nested"] = simple(sc, [(100, 1000), (900, 1050), (950, 2000)], expect=NESTED, fillers=False)
    c["comp"] = simple(sc, five, comp=True)
    c["short_records_200"] = simple(sc, [(14 * i, 14 * i + 10) for i in range(200)])
    # 300 chains of 300 reads against one contig
    b = Builder()
    reads = []
    for i in range(300):
        s = Script(1000 + i, 700, a0=A0)
        reads.append(s.B0)
        cuts = [(20 + i % 7, 300), (340, 650 - i % 5)] if i % 2 == 0 else [(20, 330), (290 - i % 3, 650)]
        b.chain(s, cuts, bread=i)
    c["chains_300"] = b.case([A0[:700]], reads, expect=[OK] * 300, fillers=True)
    # the filler of 100 A bases against 6 000 B bases: in free-shift mode the band lies around the END diagonal, so the
    # global-alignment kernel serves it (the status follows from the band policy on the oracle's score)
    d = 6000 - int(bm[1100] - bm[1000])
    c["filler_100_x_6000"] = simple(sc, [(100, 1000), (1100, 2500, 0, d)], B=cat(B0[:bm[1000]], rnd(6000), B0[bm[1100]:]))
    # two unrelated stretches of 3 000 bases: no band of DH_NW_MAX_BAND diagonals proves their alignment exact
    c["filler_faked"] = simple(sc, [(100, 1000), (1000, 2500, 3000, 3000)], A=cat(A0[:1000], rnd(3000), A0[1000:]),
                               B=cat(B0[:bm[1000]], rnd(3000), B0[bm[1000]:]), expect=FAKED, fillers=False)
    return c


_CASES = None


def cases():
    """name -> case, built once and shared (nobody modifies them)"""
    global _CASES
    if _CASES is None:
        _CASES = build_cases()
    return _CASES


def random_case(seed):
    """a chain of 2 .. 6 records at random cuts and random B shifts (for the plan only: the shifted traces are not alignments)"""
    rng = np.random.default_rng(seed)
    sc = Script(seed, 1500)
    b = Builder()
    n = int(rng.integers(2, 7))
    a0 = int(rng.integers(0, 200))
    cuts = []
    for _ in range(n):
        ln = int(rng.integers(1, 400))
        a1 = min(a0 + ln, 1400)
        cuts.append((a0, a1, 0, int(rng.integers(0, 3)) * int(rng.integers(0, 80))))
        a0 = min(max(a0, a1 + int(rng.integers(-150, 120))), 1399) if rng.random() < 0.8 else a0
    cuts.sort(key=lambda t: t[0])
    b.chain(sc, cuts)
    return b.case([sc.A0], [cat(sc.B0, np.zeros(400, np.uint8))], expect=None, fillers=None)
