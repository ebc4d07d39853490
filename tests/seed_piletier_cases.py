"""Inputs of tests/test_parity_seed_piletiers_gpu.py: the segment-fed 8 192- and 16 384-entry tiers of k_seed (the pile-up
all-vs-all's), built as tests/seed_cases.py builds its cases -- a builder only builds, what it claims is asserted on the
oracle (tests/test_seed_piletier_cases.py for the constructed ranges, the GPU module itself for the simulated pile-ups,
before the device is touched).

Only the pile-up join feeds these tiers as a FIRST tier (DH_SEED_CAP names it), so every case is a grouped DB against itself
with skip_self = 2.  Which read of a pair plays B goes by the parity of a + b (dh_seed.hip, `emit`): an even read r meets
an odd read a exactly when a > r."""
import numpy as np

from dentist_amd import sim
from seed_cases import K, case, differ, rnd
from test_parity_map_gpu import grouped_piles

PILE_KW = dict(k=14, skip_self=2, tcap=400)


# ------------------------------------------------------------------------------------------- runs of a ranged candidate
def ranged_runs():
    """One group: the even reads 0, 2, 4, 6 are copies of stretches of read 7 (12 kb of random bases), the odd reads 1, 3, 5
    are 40 random bases (no k-mer in common with anything).  Every copy is one candidate band pair whose hit range is longer
    than 16 hits, so its seed is picked by the lane groups and not by the serial walk (a hit = an intact 14-mer; hits of one
    diagonal at most k apart form a run; the seed is the first hit of the run that covers most bases, the earliest on ties):
      read 0  c[a : a + 100] with the bases 40..59 changed: two runs of 27 hits that cover 40 bases each -- a tie, the first
              run is the seed (a, 0); score 80
      read 2  c[a : a + 23] + one changed base + c[a + 24 : a + 67]: a run of 10 hits (23 bases) and a run of 30 hits (43
              bases) that begins at hit 10 of the range and ends at hit 39 -- across the 16-hit groups' edges at 16 and 32;
              the seed is its first hit (a + 24, 24); score 66
      read 4, 6  the reverse complements of two more such reads: the same ranges on the other strand (items 9 and 13),
              positions counted on the reverse-complemented read"""
    c = rnd(401, 12000)
    reads, expect = [], {}

    def two_runs(a):
        s = c[a:a + 100].copy()
        s[40:60] = (s[40:60] + 1) % 4
        return s, [(80, 7, a, 0)]

    def straddle(a):
        s = np.concatenate([c[a:a + 23], [differ(c[a + 23])], c[a + 24:a + 67]]).astype(np.uint8)
        return s, [(66, 7, a + 24, 24)]

    def flanked(seed, s):
        l, r = rnd(seed, 30), rnd(seed + 1, 30)
        return np.concatenate([l, s, r]).astype(np.uint8), len(l)
    for idx, (builder, a, rev) in enumerate(((two_runs, 1000, False), (straddle, 3000, False), (two_runs, 5000, True),
                                             (straddle, 7000, True))):
        s, cands = builder(a)
        rd, shift = flanked(410 + 2 * idx, s)
        # (a flank base next to the copy that happens to continue the match would lengthen it: make both differ)
        rd[shift - 1] = differ(c[a - 1])
        rd[shift + len(s)] = differ(c[a + len(s)])
        cands = [(sc, aseq, apos, bpos + shift) for sc, aseq, apos, bpos in cands]
        r = 2 * idx
        if rev:
            rd = sim.revcomp(rd)
            expect[2 * r + 1] = cands
        else:
            expect[2 * r] = cands
        reads.append(rd)
        reads.append(c if idx == 3 else rnd(430 + idx, 40))
    db = sim.SeqDb.from_list(reads)
    db = sim.SeqDb(db.bases, db.off, group=np.zeros(db.n, dtype=np.int32))
    return case("ranged_runs", db, db, dict(PILE_KW, hmin=35), expect=expect)


# ------------------------------------------------------------------------------------------------- simulated pile-ups
def with_shallow_piles(deep):
    """four pile-ups of 1 to 14 reads of 6 kb (groups 0, 1, 3, 4) and `deep` as group 5"""
    return grouped_piles(extra=(deep, 5))


def deep_locus(err=0.13):
    """260 reads of 1 kb over a 1.3 kb locus beside the shallow pile-ups: every read overlaps every other one, a read
    plays B for about 130 partners.  err 0.13 (the reads of test_parity_seedstage_gpu's deep_piles): 3 000 to 6 000 hits per
    read, all inside the 8 192-entry tier; err 0.09: about 10 000, most reads in the 16 384-entry tier, and the band pairs of
    the better partners cover more than 16 k bases -- more than 16 hits, however they lie"""
    g = sim.genome(81, 1300)
    deep, _ = sim.reads(82, g, 260, 1000, 0, min_len=1000, err=err)
    return with_shallow_piles(deep)


def near_capacity(cap):
    """one pile-up whose reads' lengths vary (sd a third of the mean), so that their hit counts spread from a few hundred to
    beyond `cap`: dozens of reads in (3/4 cap, cap], a handful within a few hundred hits of it"""
    if cap == 8192:
        g = sim.genome(97, 3000)
        rd, _ = sim.reads(98, g, 170, 1500, 500, min_len=300, err=0.10)
    else:
        g = sim.genome(97, 4000)
        rd, _ = sim.reads(98, g, 120, 2500, 900, min_len=300, err=0.08)
    return with_shallow_piles(rd)


def covered_deep():
    """50 reads of 700 bases at 3 % error over 1 kb: long runs of hits one base apart, broken every ~16 bases -- the sums
    of covered bases grow fastest per hit (a run of h hits covers k + h - 1 bases)"""
    g = sim.genome(93, 1000)
    rd, _ = sim.reads(94, g, 50, 700, 0, min_len=700, err=0.03)
    return with_shallow_piles(rd)
