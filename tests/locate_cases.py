"""The shapes the exact-match locator is tested on, shared by tests/test_locate_host.py (the lane code on the CPU) and
tests/test_parity_locate_gpu.py (the kernels): one reference of 40 records and the queries that probe every path, with
the oracle's answer (tests/locate_ref.py) computed once per process."""
import functools

import numpy as np

import locate_ref as lr

LENGTHS = [1, 2, 13, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049]  # the wave step boundaries


def rc(seq):
    return (3 - seq[::-1]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def main_case():
    """(refs, queries, notes): base-code arrays; notes names the queries the tests look at by index"""
    rng = np.random.default_rng(20261018)

    def rnd(n):
        return rng.integers(0, 4, n).astype(np.uint8)

    refs = [None] * 40
    refs[0] = rnd(3000)
    refs[1] = rnd(0)                                   # an empty record
    refs[2] = rnd(1)                                   # a 1-base record
    refs[3] = rnd(500)
    refs[4] = refs[3].copy()                           # two identical records
    seven = np.asarray([0, 1, 1, 3, 2, 0, 3], dtype=np.uint8)
    refs[5] = np.concatenate([rnd(100), np.tile(seven, 43)[:300], rnd(100)])  # a 300-base tandem of a 7-mer
    refs[6] = rnd(2500)
    refs[7] = refs[6].copy()
    refs[7][-1] ^= 1                                   # a change at the last position: the masked tail word
    refs[8] = refs[6].copy()
    refs[8][32] ^= 2                                   # a change at base 33, the first base after the anchor
    refs[9] = rnd(1200)
    refs[10] = rc(refs[9])                             # the reverse complement of a third record
    refs[11] = np.zeros(100, dtype=np.uint8)           # a x 100
    refs[12] = rnd(10000)
    pal = np.tile(np.asarray([0, 1, 2, 3], dtype=np.uint8), 12)  # (acgt) x 12 is its own reverse complement
    refs[15] = np.concatenate([rnd(50), pal, rnd(50)])
    for i in range(40):
        if refs[i] is None:
            refs[i] = rnd(int(rng.integers(200, 2100)))
    starts = np.concatenate([[0], np.cumsum([len(r) for r in refs])])
    total = int(starts[-1])
    queries, notes = [], {}

    def add(name, q):
        notes.setdefault(name, []).append(len(queries))
        queries.append(np.ascontiguousarray(q, dtype=np.uint8))

    for k, n in enumerate(LENGTHS):                    # every length, each followed by differing bases in the record
        add("lengths", refs[0][5 + k:5 + k + n])
    for res in range(32):                              # a match at every residue of the text position mod 32
        begin = 100 + (res - (int(starts[12]) + 100)) % 32
        assert (int(starts[12]) + begin) % 32 == res
        add("residues", refs[12][begin:begin + 40])
    add("record ends", refs[13][:50])                  # at the first base of a record
    add("record ends", refs[13][-50:])                 # ending at its last base
    add("record ends", refs[14])                       # a whole record
    add("across", np.concatenate([refs[13][-20:], refs[14][:20]]))  # the tail of record i joined to the head of record i + 1
    add("across", np.concatenate([refs[13][-3:], refs[14][:3]]))
    add("tail mask", refs[0][100:170])                 # 70 bases: a last word of 6 bases, followed by others in the record
    for k in range(20):                                # 20 queries sharing their first 32 bases
        q = refs[0][200:240 + 5 * k].copy()
        if k % 2:
            q[-1] ^= 3
        add("anchor group", q)
    add("poly-a", np.zeros(40, dtype=np.uint8))        # a x 40 against a x 100: 61 hits
    add("palindrome", pal[:40])
    add("longer than a record", rnd(12000))
    add("longer than the reference", rnd(total + 10))
    add("empty", rnd(0))
    add("twins", refs[3][10:200])                      # two hits
    add("triple", refs[6])                             # refs[6] only
    add("triple", refs[6][:-1])                        # refs[6] and refs[7]
    add("triple", refs[6][33:-1])                      # all three
    add("triple", refs[7])                             # refs[7] only: the mismatch against refs[6] is in the tail word
    add("triple", refs[8][:300])                       # refs[8] only: the mismatch is the first base after the anchor
    add("strands", refs[9][100:400])                   # forward in refs[9], complement in refs[10]
    add("tandem", np.tile(seven, 5))
    add("tandem", np.tile(seven, 10))
    return refs, queries, notes


@functools.lru_cache(maxsize=None)
def main_expected(both_strands=True):
    refs, queries, _ = main_case()
    return lr.locate(refs, queries, both_strands)


@functools.lru_cache(maxsize=None)
def segment_case():
    """a 10 000-base query against a 12 000-base record: matching fully, with a mismatch only in the last of its three
    segments of 4 096 bases, and only in the first (behind the bases the scan compares itself)"""
    rng = np.random.default_rng(7)
    refs = [rng.integers(0, 4, 700).astype(np.uint8), rng.integers(0, 4, 12000).astype(np.uint8), rng.integers(0, 4, 300).astype(np.uint8)]
    full = refs[1][1003:11003].copy()
    last, first = full.copy(), full.copy()
    last[9000] ^= 1
    first[300] ^= 2
    return refs, [full, last, first]


def as_tuples(hits):
    """a structured array of EXACT_HIT_DTYPE (or the harness's) as the oracle's tuples"""
    return [(int(h["query"]), int(h["ref"]), int(h["begin"]), int(h["end"]), int(h["complement"])) for h in hits]
