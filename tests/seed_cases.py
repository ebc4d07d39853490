"""Inputs of the seed-stage tests (dh_seed_candidates against oz.seed_candidates_all): constructed ties and edges that the
simulated reads never produce.  Everything is seeded and tiny -- a few contigs of at most 20 kb, a handful of reads.  A
builder only builds; what it claims about its case (that the tie exists, that the cut drops something) is asserted by
tests/test_seed_cases.py on the oracle, never on the code under test.

A case is a dict:
  name     id of the case
  A, B     sim.SeqDb; B is A itself (the same object) for the all-vs-all modes
  kw       the alignment options that differ from the defaults (both_opts(**kw))
  none     True: no item of the case has a candidate
  mapping  True: the call has the shape the partitioned mapping join takes (A != B, ungrouped, a, c, g, t only)
  expect   {item: [(score, aseq, apos, bpos), ...]} -- the complete candidate list of some items, worked out by hand from
           the rules of the band filter (docstring of the builder)
  cut      items whose candidate list is cut at max_cand between two candidates of equal score ("some": at least one)
  ties     items that hold at least two candidates of equal score ("some": at least one)

The arithmetic behind `expect` (oracle/align.c, seed_candidates): an exact block of L bases is L - k + 1 hits on one
diagonal and covers L bases; the score of a band b is the coverage of b and b + 1 together; b is a candidate when that
is >= hmin, not below the score of b - 1 and above the score of b + 1; its seed is the first hit of the run of linked
hits (same diagonal, steps <= k) that covers most bases, the first such run on ties.  A sequences start at multiples of
4096 on the diagonal axis, so the band of a hit in contig 0 is (apos - bpos + a multiple of 4096) >> band_shift."""
import functools

import numpy as np

from dentist_amd import sim

K = 14
M64 = (1 << 64) - 1


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 4, n).astype(np.uint8)


def differ(x):
    """a base that differs from x"""
    return np.uint8((int(x) + 1) % 4)


def other(*xs):
    """a base that is none of xs (at most three of them)"""
    return np.uint8(min(set(range(4)) - set(int(x) for x in xs)))


def planted(flank_seed, block, left, right, before=None, after=None):
    """random(left) + block + random(right) with the bases next to the block different from `before` / `after` (the bases
    next to the block where it was copied from): the exact match is the block and not a base more"""
    l, r = rnd(flank_seed, left), rnd(flank_seed + 1, right)
    if left and before is not None:
        l[-1] = differ(before)
    if right and after is not None:
        r[0] = differ(after)
    return np.concatenate([l, np.asarray(block, dtype=np.uint8), r])


def sampled(codes, mod):
    """modimer sampling of the k-mer `codes` (oracle/align.c: kmer_sampled_k, on the canonical k-mer)"""
    km = rc = 0
    for c in codes:
        km = (km << 2) | int(c)
    for c in codes[::-1]:
        rc = (rc << 2) | (3 - int(c))
    c = min(km, rc)
    return (((c * 0x9E3779B97F4A7C15) & M64) >> 32) % mod == 0


def sampled_positions(seq, mod, k=K):
    return [p for p in range(len(seq) - k + 1) if sampled(seq[p:p + k], mod)]


def case(name, A, B, kw, none=False, mapping=None, expect=None, cut=(), ties=()):
    kw = dict(dict(k=K, algo=1, width=64), **kw)
    if mapping is None:
        mapping = (B is not A and A.group is None and B.group is None and kw.get("skip_self", 0) == 0 and
                   not (A.bases > 3).any() and not (B.bases > 3).any() and getattr(A, "mask", None) is None and
                   getattr(B, "mask", None) is None)
    return dict(name=name, A=A, B=B, kw=kw, none=none, mapping=mapping, expect=expect or {},
                cut=cut if cut == "some" else tuple(cut), ties=ties if ties == "some" else tuple(ties))


def with_mask(db, ivs):
    """the DB with the masked intervals ivs = {sequence: [begin, end, begin, end, ...]}"""
    out = sim.SeqDb(db.bases, db.off, db.group)
    ptr = np.zeros(db.n + 1, dtype=np.int64)
    iv = []
    for s in range(db.n):
        iv += ivs.get(s, [])
        ptr[s + 1] = len(iv) // 2
    out.mask = (ptr, np.asarray(iv + [0, 0], dtype=np.int32))
    return out


# ---------------------------------------------------------------------------------------------------------- runs and links
CONTIG = 12000


def runs_and_links(band_shift=6, kmer_mod=1, hmin=35):
    """One contig, reads copied from it (forward, then the same reads reverse-complemented: items 2 r of the first half and
    2 r + 1 of the second half carry the candidates).  w = 2^band_shift diagonals per band; every stretch starts at a
    position a with a known residue mod w, so the bands of its blocks are known:
      two_runs   contig[a : a + 100] with bases 40..60 changed: two runs of 27 linked hits on one diagonal, 80 bases
                 covered, the runs tie and the first one is the seed (a, 0)
      del_in     one base deleted between two 40-base blocks, diagonals a and a + 1 in ONE band: score 80, seed (a, 0)
      del_edge   the same with a = w - 1 mod w: diagonals in bands b and b + 1, one candidate (b) of score 80; the runs of
                 the two bands tie and the one of b -- sorted first -- is the seed
      skip_w     w bases deleted between the blocks: equal coverage 40 in bands b and b + 1, candidate b, score 80
      skip_2w    2 w bases deleted: equal coverage in b and b + 2.  b scores 40, which is not ABOVE the score 40 of b + 1
                 (the empty band and b + 2): dropped.  b + 2 scores 40, not BELOW b + 1: kept, seed = the second block"""
    w = 1 << band_shift
    c = rnd(101, CONTIG)

    def at(base, residue):  # the position >= base with that residue mod w
        return base + (residue - base) % w
    reads, expect = [], {}

    def add(seq, cands):
        if kmer_mod == 1:
            expect[2 * len(reads)] = cands
        reads.append(seq)
    a = at(1000, 8)
    two = c[a:a + 100].copy()
    two[40:60] = (two[40:60] + 1) % 4
    add(two, [(80, 0, a, 0)])

    def two_blocks(a, gap):  # contig[a : a + 40] + contig[a + 40 + gap : a + 80 + gap], neither block a base longer
        c[a + 40] = other(c[a + 39], c[a + 40 + gap]) if gap == 1 else other(c[a + 40 + gap])
        if gap > 1:
            c[a + 39 + gap] = other(c[a + 39])
        return np.concatenate([c[a:a + 40], c[a + 40 + gap:a + 80 + gap]])
    a = at(2000, 8)
    add(two_blocks(a, 1), [(80, 0, a, 0)])
    a = at(3000, w - 1)
    add(two_blocks(a, 1), [(80, 0, a, 0)])
    a = at(4000, 8)
    add(two_blocks(a, w), [(80, 0, a, 0)])
    a = at(6000, 8)
    add(two_blocks(a, 2 * w), [(40, 0, a + 40 + 2 * w, 40)])
    n = len(reads)
    reads += [sim.revcomp(r) for r in reads]
    for it, cands in list(expect.items()):
        expect[2 * (n + it // 2) + 1] = cands
    return case(f"runs_w{band_shift}_mod{kmer_mod}_h{hmin}", sim.SeqDb.from_list([c]), sim.SeqDb.from_list(reads),
                dict(band_shift=band_shift, kmer_mod=kmer_mod, hmin=hmin), expect=expect)


def sampled_links():
    """kmer_mod 4: a read of 1 000 bases copied with one base deleted in the middle, from the first place of the contig where
    consecutive sampled k-mers of the copy lie exactly k and exactly k + 1 bases apart -- a step of k still links two hits
    (and covers k bases), a step of k + 1 starts a new run."""
    c = rnd(102, 20000)
    pos = np.asarray(sampled_positions(c, 4))
    step = np.diff(pos)
    for a in range(0, len(c) - 1001, 10):
        inside = (pos[:-1] >= a + 2) & (pos[1:] < a + 480)  # both steps inside the first block
        if (step[inside] == K).any() and (step[inside] == K + 1).any():
            break
    else:
        raise AssertionError("no stretch with steps of k and k + 1")
    rd = np.concatenate([c[a:a + 500], c[a + 501:a + 1001]])
    out = case("sampled_links_mod4", sim.SeqDb.from_list([c]), sim.SeqDb.from_list([rd, sim.revcomp(rd)]), dict(kmer_mod=4))
    out["steps"] = sorted(set(int(s) for s in step[inside]))
    return out


# --------------------------------------------------------------------------------------------------------------- thresholds
def lone_block(L, hmin, band_shift=6):
    """a single exact block of L bases inside a read of random bases: score L -- kept at hmin = L, dropped at L + 1"""
    c = rnd(103, 8000)
    p = 3000
    rd = planted(201, c[p:p + L], 30, 30, c[p - 1], c[p + L])
    kept = hmin <= L
    return case(f"lone_block_L{L}_h{hmin}_w{band_shift}", sim.SeqDb.from_list([c]), sim.SeqDb.from_list([rd, sim.revcomp(rd)]),
                dict(hmin=hmin, band_shift=band_shift), none=not kept,
                expect={0: [(L, 0, p, 30)], 3: [(L, 0, p, 30)]} if kept else {})


# ------------------------------------------------------------------------------------------------------------------ the cut
def unit_in_contigs(ncontigs, max_cand):
    """A 60-base unit at position 700 + 3 i of contig i, reverse-complemented in every second contig; one read holds the
    unit.  Every copy is a candidate of score 60 -- the even contigs of the forward item, the odd ones of the reverse item
    -- and equal scores are ordered by band, that is by contig: the cut at max_cand keeps the first contigs."""
    unit = rnd(104, 60)
    rd = planted(299, unit, 25, 25)
    seqs = []
    for i in range(ncontigs):  # (the bases next to a copy differ from the read's: the match is the unit and no more)
        if i % 2 == 0:
            seqs.append(planted(300 + 2 * i, unit, 700 + 3 * i, 900, rd[24], rd[85]))
        else:
            seqs.append(planted(300 + 2 * i, sim.revcomp(unit), 700 + 3 * i, 900, 3 - rd[85], 3 - rd[24]))
    per = ncontigs // 2
    expect = {0: [(60, i, 700 + 3 * i, 25) for i in range(0, ncontigs, 2)][:max_cand],
              1: [(60, i, 700 + 3 * i, 25) for i in range(1, ncontigs, 2)][:max_cand]}
    return case(f"unit_in_{ncontigs}_contigs_cut{max_cand}", sim.SeqDb.from_list(seqs), sim.SeqDb.from_list([rd]),
                dict(max_cand=max_cand), expect=expect, cut=(0, 1) if per > max_cand else (), ties=(0, 1))


def symmetric_units(max_cand, algo=1):
    """A == B, skip_self 2: sixteen sequences that share a 60-base unit and a 50-base unit (alternating strands, at positions
    that differ from sequence to sequence).  An item meets about half of the others (the parity rule of the symmetric mode)
    and holds, per partner, a candidate of score 60 and one of score 50: by score the 60s of all partners come first, the
    cut at max_cand falls inside one of the two runs of equal scores, and what is kept is regrouped by partner."""
    u1, u2 = rnd(105, 60), rnd(106, 50)
    seqs = []
    for i in range(16):
        a, b = (u1, u2) if i % 2 == 0 else (sim.revcomp(u2), sim.revcomp(u1))
        s = np.concatenate([planted(400 + 4 * i, a, 500 + 7 * i, 800), planted(402 + 4 * i, b, 300 + 211 * i, 400)])
        seqs.append(s)
    db = sim.SeqDb.from_list(seqs)
    return case(f"symmetric_units_cut{max_cand}_algo{algo}", db, db, dict(max_cand=max_cand, skip_self=2, algo=algo,
                                                                           width=64 if algo == 1 else 30),
                cut="some", ties="some")


# ----------------------------------------------------------------------------------------------------------------- geometry
def page_edges():
    """Contigs of 4095, 4096 and 4097 bases (a sequence's start on the diagonal axis is a multiple of 4096: the second
    contig starts 8192 behind the first whatever a base more or less does, and the page of a hit names its sequence); a
    read for the first and one for the last 40 bases of each, forward and reverse-complemented.  The block stands at the
    start of the one read (bpos 0) and at the end of the other (its last hit is the read's last k-mer)."""
    lens = (4095, 4096, 4097)
    seqs = [rnd(110 + i, n) for i, n in enumerate(lens)]
    reads, expect = [], {}
    for i, s in enumerate(seqs):
        first = planted(500 + 4 * i, s[:40], 0, 33, None, s[40])
        last = planted(502 + 4 * i, s[-40:], 27, 0, s[-41], None)
        for rd, cand in ((first, (40, i, 0, 0)), (last, (40, i, lens[i] - 40, 27))):
            expect[2 * len(reads)] = [cand]
            reads.append(rd)
            expect[2 * len(reads) + 1] = [cand]
            reads.append(sim.revcomp(rd))
    return case("page_edges", sim.SeqDb.from_list(seqs), sim.SeqDb.from_list(reads), dict(hmin=40), expect=expect)


def edge_kmers():
    """hmin = k: one k-mer is a candidate.  Reads that hold one k-mer of the contig as their first k bases (bpos 0) and as
    their last (bpos = length - k), the contig's own first and last k-mer among them, and reads of 0, k - 1 and k bases
    (the read of k bases is the k-mer at 5000; the read of k - 1 bases is its start)."""
    c = rnd(120, 10000)
    n = len(c)
    reads = [planted(600, c[2000:2000 + K], 0, 40, None, c[2000 + K]),
             planted(602, c[3000:3000 + K], 40, 0, c[2999], None),
             planted(604, c[:K], 0, 40, None, c[K]),
             planted(606, c[n - K:], 40, 0, c[n - K - 1], None),
             np.zeros(0, np.uint8), c[5000:5000 + K - 1].copy(), c[5000:5000 + K].copy()]
    expect = {0: [(K, 0, 2000, 0)], 2: [(K, 0, 3000, 40)], 4: [(K, 0, 0, 0)], 6: [(K, 0, n - K, 40)],
              8: [], 9: [], 10: [], 11: [], 12: [(K, 0, 5000, 0)]}
    return case("edge_kmers", sim.SeqDb.from_list([c]), sim.SeqDb.from_list(reads), dict(hmin=K), expect=expect)


def short_reads_only():
    """reads of 0, k - 1 and k bases and nothing else, the read of k bases not from the contig: no hit at all"""
    c = rnd(121, 5000)
    reads = [np.zeros(0, np.uint8), c[100:100 + K - 1].copy(), rnd(122, K)]
    return case("short_reads_only", sim.SeqDb.from_list([c]), sim.SeqDb.from_list(reads), dict(hmin=K), none=True)


# ------------------------------------------------------------------------------------------- degenerate reads and k-mers
def run_of_n():
    """a run of three N inside a block of 100 bases, in the read (read 0) and in the contig (read 1 is a clean copy of a
    stretch of the contig that holds the run): k-mers with an N are neither indexed nor probed; 45 + 52 bases are covered
    on one diagonal in two runs, the second, longer one is the seed.  The tiled band takes a, c, g, t only: algo 0."""
    c = rnd(130, 9000)
    rd0 = planted(700, c[1000:1100], 20, 20, c[999], c[1100])
    rd0[20 + 45:20 + 48] = 4
    c[5045:5048] = 4
    rd1 = planted(702, rnd(130, 9000)[5000:5100], 20, 20, c[4999], c[5100])
    return case("run_of_n", sim.SeqDb.from_list([c]), sim.SeqDb.from_list([rd0, rd1, sim.revcomp(rd0)]), dict(algo=0, width=30),
                expect={0: [(97, 0, 1048, 68)], 2: [(97, 0, 5048, 68)], 5: [(97, 0, 1048, 68)]})


def soft_masks():
    """A block of 40 bases with a masked interval that ends where it begins and one that begins where it ends -- on the
    contig (read 0) and on the read (read 1, forward; read 2 is read 1 reverse-complemented with the mirrored mask): a
    k-mer that only touches a masked interval counts, the score stays 40.  Reads 3 and 4: the intervals reach one base
    into the block, on the contig and on the read: the first and the last k-mer go, 38 bases are covered and the seed
    moves one base in."""
    c = rnd(140, 9000)
    r0 = planted(800, c[1000:1040], 30, 30, c[999], c[1040])
    r1 = planted(802, c[3000:3040], 30, 30, c[2999], c[3040])
    r3 = planted(804, c[5000:5040], 30, 30, c[4999], c[5040])
    r4 = planted(806, c[7000:7040], 30, 30, c[6999], c[7040])
    A = with_mask(sim.SeqDb.from_list([c]), {0: [980, 1000, 1040, 1060, 4980, 5001, 5039, 5060]})
    B = with_mask(sim.SeqDb.from_list([r0, r1, sim.revcomp(r1), r3, r4]),
                  {1: [10, 30, 70, 90], 2: [10, 30, 70, 90], 4: [10, 31, 69, 90]})
    return case("soft_masks", A, B, dict(hmin=35),
                expect={0: [(40, 0, 1000, 30)], 2: [(40, 0, 3000, 30)], 5: [(40, 0, 3000, 30)], 6: [(38, 0, 5001, 31)],
                        8: [(38, 0, 7001, 31)]})


def palindrome(copies, tcap=4):
    """AAAAAAATTTTTTT is its own reverse complement at k = 14: a copy in the read meets every copy in the contig on both
    strands.  `copies` of it in the contig, under the cap -t (3 of 4: every copy a candidate of score k on either strand,
    at bpos 20 in the read of 54 bases either way) or over it (6 of 4: the k-mer is skipped, no hit)."""
    pal = sim.encode("AAAAAAATTTTTTT")
    c = rnd(150, 9000)
    at = [1000 + 1100 * i for i in range(copies)]
    for p in at:
        c[p - 1], c[p + K] = 1, 2  # (the k-mers next to a copy are not the palindrome shifted)
        c[p:p + K] = pal
    rd = np.concatenate([rnd(900, 20), pal, rnd(901, 20)])
    rd[19], rd[20 + K] = 2, 1
    under = copies <= tcap
    cands = [(K, 0, p, 20) for p in at]
    return case(f"palindrome_{copies}_copies_tcap{tcap}", sim.SeqDb.from_list([c]), sim.SeqDb.from_list([rd]),
                dict(hmin=K, tcap=tcap), none=not under, expect={0: cands, 1: cands} if under else {},
                ties=(0, 1) if under else ())


# -------------------------------------------------------------------------------------------------------------------- modes
def overlapping_reads(skip_self, strands=3, algo=1):
    """A == B: eight sequences of 700 bases that start every 150 bases of one stretch (every second one reverse-complemented),
    each with a 90-base unit of its own standing twice in it, 200 bases apart.  skip_self 1: every other sequence but not
    the sequence itself; 2 (no pile-up flags): each pair once; 3 (tandem): the sequence itself below the main diagonal --
    the second copy of its unit against the first."""
    g = rnd(160, 2000)
    seqs = []
    for i in range(8):
        s = g[150 * i:150 * i + 700].copy()
        u = rnd(170 + i, 90)
        s[100:190] = u
        s[300:390] = u
        seqs.append(s if i % 2 == 0 else sim.revcomp(s))
    db = sim.SeqDb.from_list(seqs)
    return case(f"overlapping_reads_self{skip_self}_strands{strands}_algo{algo}", db, db,
                dict(skip_self=skip_self, strands=strands, algo=algo, width=64 if algo == 1 else 30))


def mapping_strands(strands):
    """the reads of runs_and_links (forward and reverse-complemented copies) with one strand left out"""
    c = runs_and_links()
    only = {it: v for it, v in c["expect"].items() if strands & (1 << (it & 1))}
    return case(f"mapping_strands{strands}", c["A"], c["B"], dict(c["kw"], strands=strands), expect=only)


@functools.lru_cache(maxsize=None)
def all_cases():
    cases = [runs_and_links(6), runs_and_links(4), runs_and_links(8),
             runs_and_links(6, kmer_mod=4, hmin=K), runs_and_links(4, kmer_mod=4, hmin=K), sampled_links(),
             lone_block(40, 40), lone_block(40, 41), lone_block(40, 40, 4), lone_block(40, 41, 4), lone_block(40, 40, 8),
             lone_block(40, 41, 8),
             unit_in_contigs(12, 5), unit_in_contigs(12, 12), unit_in_contigs(26, 12),
             symmetric_units(5), symmetric_units(12), symmetric_units(5, algo=0),
             page_edges(), edge_kmers(), short_reads_only(), run_of_n(), soft_masks(), palindrome(3), palindrome(6),
             overlapping_reads(1), overlapping_reads(2), overlapping_reads(2, algo=0), overlapping_reads(3, strands=1),
             overlapping_reads(1, strands=1), overlapping_reads(1, strands=2),
             mapping_strands(1), mapping_strands(2), mapping_strands(3)]
    names = [c["name"] for c in cases]
    assert len(set(names)) == len(names)
    return cases


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)
