"""The refusal paths of the crop and of the batch entry points of the process stage (dh_crop.cpp, dh_batch.cpp).

Every refusal here is a host-side validation that returns before any kernel of the refused call is launched; each case
pins DhError.code and a distinctive part of the message, so that a reordered or lost guard shows.  The records are made
by hand (the cropper is arithmetic on records and trace values: nothing has to align): two contigs of 3 kb, three reads
of 2.2 kb, pile-up 0 = the gap (contig 0, back) -> (contig 1, front), pile-up 1 = the extension over the back of contig 1.

Two paths have no case, because no input reaches them:
 * "trace does not fit its read" (error 4 of the crop): the slice of a read is clamped to [0, read length) before the
   range check, and the common trace point lies in every entry's region, so some member of its chain covers it; a trace
   whose B sums leave the read ends as a slice shorter than 14 bases, which is dropped (pinned below as what it is).
 * DH_PILE_UNSUPPORTED_JOIN: dh_pileups_create_joins refuses a contig joined with itself (tests/test_abi.py), and no
   other exported constructor makes pile-ups with a join.
"""
import ctypes

import numpy as np
import pytest

import dentist_amd
from dentist_amd import sim

pytestmark = pytest.mark.gpu

DH_EINVAL = -1
PILE_OK, PILE_NO_COMMON_TRACE_POINT = 0, 1
FRONT, BACK = 0, 1
CLEN, RLEN, NREADS = 3000, 2200, 3


def ntp(abpos, aepos, tspace=100):
    return (aepos + tspace - 1) // tspace - abpos // tspace


class Hand:
    """Records 0-2: read r on the back of contig 0; 3-5: on the front of contig 1; 6-8: on the back of contig 1."""

    def __init__(self):
        rng = np.random.default_rng(11)
        self.contigs = sim.SeqDb.from_list([rng.integers(0, 4, CLEN, dtype=np.uint8) for _ in range(2)])
        self.reads = sim.SeqDb.from_list([rng.integers(0, 4, RLEN, dtype=np.uint8) for _ in range(NREADS)])
        self.las = las = np.zeros(3 * NREADS, dtype=dentist_amd.LA_DTYPE)
        toff = 0
        for k, (aread, abpos, aepos, bbpos) in enumerate(((0, 2000, 3000, 0), (1, 0, 1000, 1200), (1, 2200, 3000, 0))):
            for r in range(NREADS):
                i = k * NREADS + r
                las["aread"][i], las["bread"][i], las["abpos"][i], las["aepos"][i] = aread, r, abpos, aepos
                las["bbpos"][i], las["bepos"][i] = bbpos, bbpos + (aepos - abpos)
                las["tlen"][i], las["toff"][i] = 2 * ntp(abpos, aepos), toff
                toff += 2 * ntp(abpos, aepos)
        self.trace = np.zeros(toff, dtype=np.uint16)
        self.trace[1::2] = 100  # no differences, 100 B bases per trace interval
        self.gap = [(r, r, 3 + r) for r in range(NREADS)]
        self.ext = [(r, 6 + r, -1) for r in range(NREADS)]
        self.joins = [(0, BACK, 1, FRONT), (1, BACK, -1, 0)]

    def piles(self, gap=None, ext=None, joins=None):
        return dentist_amd.Pileups.from_joins(joins or self.joins, [gap or self.gap, ext or self.ext])


@pytest.fixture(scope="module")
def hand():
    return Hand()


@pytest.fixture(scope="module")
def dbs(gpu_ctx, hand):
    return gpu_ctx.db(hand.contigs), gpu_ctx.db(hand.reads)


@pytest.fixture(scope="module")
def po():
    return dentist_amd.default_process_opts(algo=1)


def crop(gpu_ctx, dbs, hand, piles, po, las=None, trace=None):
    return dentist_amd.Cropped.crop(gpu_ctx, dbs[0], dbs[1], 0, hand.las if las is None else las,
                                    hand.trace if trace is None else trace, piles, po)


def refused(call, part):
    with pytest.raises(dentist_amd.DhError) as e:
        call()
    assert e.value.code == DH_EINVAL, e.value
    assert part in str(e.value), e.value


def test_the_hand_made_batch_crops(gpu_ctx, dbs, hand, po):
    """The inputs of the cases below are sound: both pile-ups crop, at the trace points the arithmetic gives."""
    rec, pile, entry, read_id, off, bases = crop(gpu_ctx, dbs, hand, hand.piles(), po).arrays()
    assert rec["status"].tolist() == [PILE_OK, PILE_OK] and rec["nreads"].tolist() == [NREADS, NREADS]
    assert (rec[0]["crop_left"], rec[0]["crop_right"]) == (2000, 900) and (rec[1]["crop_left"], rec[1]["crop_right"]) == (2200, -1)
    assert pile.tolist() == [0, 0, 0, 1, 1, 1] and entry.tolist() == [0, 1, 2] * 2 and read_id.tolist() == [0, 1, 2] * 2
    # the gap's reads keep [0, 2100): up to the front anchor's trace point; the extension's keep all of [0, 2200)
    assert np.diff(off).tolist() == [2100] * 3 + [RLEN] * 3
    for i in range(6):
        assert np.array_equal(bases[off[i]:off[i + 1]], hand.reads.seq(read_id[i])[:off[i + 1] - off[i]])


@pytest.mark.parametrize("joins", [[(0, BACK, 5, FRONT), (1, BACK, -1, 0)], [(0, BACK, 1, FRONT), (2, BACK, -1, 0)]])
def test_crop_refuses_a_gap_outside_the_contigs(gpu_ctx, dbs, hand, po, joins):
    refused(lambda: crop(gpu_ctx, dbs, hand, hand.piles(joins=joins), po), "dh_crop_pileups: gap outside the contigs DB")


def test_crop_refuses_a_plain_gap_behind_the_last_contig(gpu_ctx, dbs, hand, po):
    piles = dentist_amd.Pileups.from_triples([1], [hand.gap])   # (contig 1, back) -> (contig 2, front)
    refused(lambda: crop(gpu_ctx, dbs, hand, piles, po), "dh_crop_pileups: gap outside the contigs DB")


@pytest.mark.parametrize("gap, ext", [
    ([(0, 0, 3), (1, 9, 4), (2, 2, 5)], None),      # an LA index >= n
    ([(0, 0, 3), (1, -2, 4), (2, 2, 5)], None),     # ... below -1
    ([(0, 0, 3), (1, -1, -1), (2, 2, 5)], None),    # an entry without any alignment
    (None, [(0, 6, -1), (1, 7, 4), (2, 8, -1)]),    # an extension entry with a second alignment
    ([(0, 0, 3), (1, 4, 1), (2, 2, 5)], None),      # alignments that are not on their flanks' contigs
])
def test_crop_refuses_entries_that_do_not_fit_their_flanks(gpu_ctx, dbs, hand, po, gap, ext):
    refused(lambda: crop(gpu_ctx, dbs, hand, hand.piles(gap=gap, ext=ext), po),
            "dh_crop_pileups: LA index out of range, or an alignment that is not on its flank's contig")


def crop_plain_args(gpu_ctx, dbs, hand, piles, po, trace, out):
    L = dentist_amd.lib()
    L.dh_crop_pileups.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64] + [ctypes.c_void_p] * 4
    L.dh_crop_pileups.restype = ctypes.c_int
    return L.dh_crop_pileups(gpu_ctx._h, dbs[0]._h, dbs[1]._h, 0, hand.las.ctypes.data, len(hand.las), trace,
                             piles._h if piles is not None else None, ctypes.byref(po), ctypes.byref(out))


def test_crop_refuses_a_held_read_without_trace(gpu_ctx, dbs, hand, po):
    """dh_crop_pileups with trace = NULL: fine while no read of the pile-ups is held here, refused otherwise."""
    out = ctypes.c_void_p()
    piles = hand.piles()
    rc = crop_plain_args(gpu_ctx, dbs, hand, piles, po, None, out)
    assert rc == DH_EINVAL and not out.value
    assert dentist_amd.lib().dh_last_error().decode() == "dh_crop_pileups: trace is NULL"
    # the same pile-ups with read ids of another rank's share: nothing to cut, no trace needed
    away = hand.piles(gap=[(r + 10, a, b) for r, a, b in hand.gap], ext=[(r + 10, a, b) for r, a, b in hand.ext])
    assert crop_plain_args(gpu_ctx, dbs, hand, away, po, None, out) == 0 and out.value
    c = dentist_amd.Cropped(out)
    rec = c.arrays()[0]
    assert rec["status"].tolist() == [PILE_OK, PILE_OK] and rec["nreads"].tolist() == [0, 0]
    assert (rec[0]["crop_left"], rec[0]["crop_right"]) == (2000, 900)


def test_crop_and_process_refuse_null_arguments(gpu_ctx, dbs, hand, po):
    out = ctypes.c_void_p()
    assert crop_plain_args(gpu_ctx, dbs, hand, None, po, hand.trace.ctypes.data, out) == DH_EINVAL
    assert dentist_amd.lib().dh_last_error().decode() == "dh_crop_pileups: NULL argument"
    L = dentist_amd.lib()
    L.dh_process_pileups.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_void_p] * 4
    L.dh_process_pileups.restype = ctypes.c_int
    piles = hand.piles()
    rc = L.dh_process_pileups(gpu_ctx._h, dbs[0]._h, dbs[1]._h, hand.las.ctypes.data, len(hand.las), None, piles._h,
                              ctypes.byref(po), ctypes.byref(out))
    assert rc == DH_EINVAL and L.dh_last_error().decode() == "dh_process_pileups: NULL argument"


def test_a_trace_that_leaves_its_read_drops_the_read(gpu_ctx, dbs, hand, po):
    """What a trace whose B sums leave the read comes to today: read 1's slice of the extension pile-up starts behind the
    read's end, is shorter than 14 bases and is dropped; nothing is refused, the other reads are cut as before."""
    las, trace = hand.las.copy(), hand.trace.copy()
    las["bbpos"][7] = 3000   # read 1 on the back of contig 1: its crop point translates to B = 3000 > 2200
    rec, pile, entry, read_id, off, _ = crop(gpu_ctx, dbs, hand, hand.piles(), po, las=las, trace=trace).arrays()
    assert rec["status"].tolist() == [PILE_OK, PILE_OK] and rec["nreads"].tolist() == [3, 2]
    assert pile.tolist() == [0, 0, 0, 1, 1] and entry.tolist() == [0, 1, 2, 0, 2] and read_id.tolist() == [0, 1, 2, 0, 2]
    assert np.diff(off).tolist() == [2100] * 3 + [RLEN] * 2


@pytest.mark.parametrize("broken", [0, 1])
def test_no_common_trace_point_is_a_status_of_its_pile_up_only(gpu_ctx, dbs, hand, po, broken):
    """Alignments of one flank whose A intervals do not intersect: DH_PILE_NO_COMMON_TRACE_POINT for that pile-up, no read
    of it is cut; the other pile-up of the batch is cropped as it is alone."""
    las = hand.las.copy()
    i = 1 if broken == 0 else 7                      # read 1's alignment on flank 0 of the broken pile-up ...
    las["abpos"][i], las["aepos"][i] = (0, 1000) if broken == 0 else (1000, 2000)   # ... away from the other reads'
    las["bepos"][i] = las["bbpos"][i] + 1000
    las["tlen"][i], las["toff"][i] = 2 * ntp(int(las["abpos"][i]), int(las["aepos"][i])), 0
    rec, pile, entry, read_id, off, bases = crop(gpu_ctx, dbs, hand, hand.piles(), po, las=las).arrays()
    other = 1 - broken
    assert rec[broken]["status"] == PILE_NO_COMMON_TRACE_POINT and rec[broken]["nreads"] == 0
    assert rec[broken]["crop_left"] == -1 and (broken == 1 or rec[broken]["crop_right"] == 900)
    assert rec[other]["status"] == PILE_OK and rec[other]["nreads"] == NREADS
    assert pile.tolist() == [other] * 3 and entry.tolist() == [0, 1, 2] and read_id.tolist() == [0, 1, 2]
    ref, rpile, rentry, rread, roff, rbases = crop(gpu_ctx, dbs, hand, hand.piles(), po).arrays()
    mine = rpile == other
    assert rec[other].tobytes() == ref[other].tobytes()
    assert np.array_equal(np.diff(off), np.diff(roff)[mine])
    assert np.array_equal(bases, np.concatenate([rbases[roff[j]:roff[j + 1]] for j in np.flatnonzero(mine)]))


@pytest.fixture(scope="module")
def mapped(gpu_ctx, po):
    """A small mapping whose trace values were left on the device: what dh_process_pileups_set takes."""
    w = sim.Workload(100_000, 1, 300, 7000, seed=77, spacing=20000, gap_max=1500)
    mo = dentist_amd.default_align_opts(kmer_mod=4, k=20, width=64, xdrop=60, algo=1)
    A, B = gpu_ctx.db(w.contigs), gpu_ctx.db(w.reads)
    las, dtrace, _ = gpu_ctx.map_reads(A, B, mo, po, sorted=False, trace_on_device=True)[:3]
    assert dtrace.on_device() and len(las) > 0
    return w, A, B, las, dtrace


def test_process_set_refuses_a_read_outside_the_reads(gpu_ctx, mapped, po):
    w, A, B, las, dtrace = mapped
    for rd in (w.reads.n, -1):
        piles = dentist_amd.Pileups.from_triples([0], [[(int(las[0]["bread"]), 0, 0), (rd, 0, 0)]])
        refused(lambda: dentist_amd.process_pileups(gpu_ctx, A, B, las, dtrace, piles, po),
                "dh_process_pileups_set: read id out of range")
    assert dtrace.on_device()


def test_process_set_refuses_a_record_whose_trace_leaves_the_set(gpu_ctx, mapped, po):
    w, A, B, las, dtrace = mapped
    i = int(np.flatnonzero(las["tlen"] > 0)[0])
    piles = dentist_amd.Pileups.from_triples([0], [[(int(las[i]["bread"]), i, i)]])
    keep = int(las[i]["toff"])
    try:
        for toff in (len(dtrace) - int(las[i]["tlen"]) + 1, -1):
            las["toff"][i] = toff   # (the records are the set's own: the view map_reads returned)
            refused(lambda: dentist_amd.process_pileups(gpu_ctx, A, B, las, dtrace, piles, po),
                    "dh_process_pileups_set: a record's trace lies outside the set's trace")
    finally:
        las["toff"][i] = keep
    assert dtrace.on_device()
