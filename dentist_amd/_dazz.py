"""Files: DAZZ_DB databases, their mask tracks and the extras of a mask track, BED to mask, the read loader, and DENTIST's
pile-ups.db and insertions.db."""
import collections
import ctypes

import numpy as np

from ._abi import CHAIN_LA_DTYPE, INSERTION_REC_DTYPE, SEEDED_DTYPE, _check, lib
from ._align import Db, _take_la_set
from ._marshal import Owner, addr, copy
from ._process import Pileups, _take_insertions


# ---------------------------------------------------------------- DAZZ_DB files (host only)
def dazz_create_dam(path, fasta_text):
    b = fasta_text.encode() if isinstance(fasta_text, str) else fasta_text
    _check(lib().dh_dazz_create_dam(path.encode(), b, len(b)))


def dazz_create_db(path, fasta_text):
    b = fasta_text.encode() if isinstance(fasta_text, str) else fasta_text
    _check(lib().dh_dazz_create_db(path.encode(), b, len(b)))


def dazz_split(path, cutoff=0, all_reads=True, size_mb=200):
    _check(lib().dh_dazz_split(path.encode(), cutoff, int(all_reads), size_mb))


class DazzDb(Owner):
    """Trimmed view of a DAZZ_DB (or of one block, e.g. ``reads.3``) read from disk."""
    _destroy = "dh_dazz_close"

    def __init__(self, path):
        L = lib()
        h = ctypes.c_void_p()
        _check(L.dh_dazz_open(path.encode(), ctypes.byref(h)))
        n = L.dh_dazz_nreads(h)
        self.first_id = L.dh_dazz_first_id(h)
        self.off = copy(L.dh_dazz_offsets(h), n + 1, np.int64)
        self.bases = copy(L.dh_dazz_bases(h), int(self.off[-1]), np.uint8)
        self.origin = copy(L.dh_dazz_origin(h), n, np.int32)
        self.fpulse = copy(L.dh_dazz_fpulse(h), n, np.int32)
        self.headers = [L.dh_dazz_header(h, i).decode() for i in range(n)]
        self.group = None
        self.mask = None
        self._h = h
        self._path = path

    def read_mask(self, name):
        """Intervals of mask track `name` for this (trimmed) view: (ptr int64[n+1], iv int32 pairs)."""
        L = lib()
        ptr = np.zeros(self.n + 1, dtype=np.int64)
        m = L.dh_dazz_read_mask(self._h, self._path.encode(), name.encode(), ptr.ctypes.data, None, 0)
        if m < 0:
            _check(int(m))
        iv = np.zeros(max(2 * m, 2), dtype=np.int32)
        L.dh_dazz_read_mask(self._h, self._path.encode(), name.encode(), ptr.ctypes.data, iv.ctypes.data, m)
        return ptr, iv[:2 * m]

    @property
    def n(self):
        return len(self.off) - 1

    def seq(self, i):
        return self.bases[self.off[i]:self.off[i + 1]]


def dazz_write_mask(db_path, name, ptr, iv):
    p = np.ascontiguousarray(ptr, dtype=np.int64)
    v = np.ascontiguousarray(iv, dtype=np.int32)
    _check(lib().dh_dazz_write_mask(db_path.encode(), name.encode(), len(p) - 1, p.ctypes.data, v.ctypes.data))


ENOTFOUND = -7                    # DH_ENOTFOUND: the mask has no extra of that name
ACCUM_MODES = ("exact", "sum")    # DH_ACCUM_EXACT, DH_ACCUM_SUM
MaskExtra = collections.namedtuple("MaskExtra", "data accum")   # data: int64 or float64 (the vtype), accum: "exact" | "sum"
BedMask = collections.namedtuple("BedMask", "ptr iv contig_ids read_off read_ids")


def read_mask_extra(db_path, mask, name, dtype=None):
    """dh_dazz_read_extra: the first track extra `name` of mask `mask` as MaskExtra(data, accum), None when the mask has none of
    that name.  dtype np.int64 / np.float64 asks for that value type (another one stored is a DhError), None takes either."""
    L = lib()
    want = -1 if dtype is None else {"int64": 0, "float64": 1}[np.dtype(dtype).name]
    vtype, accum = ctypes.c_int32(want), ctypes.c_int32(0)
    args = (db_path.encode(), mask.encode(), name.encode(), ctypes.byref(vtype), ctypes.byref(accum))
    n = L.dh_dazz_read_extra(*args, None, 0)
    if n == ENOTFOUND:
        return None
    if n < 0:
        _check(int(n))
    data = np.zeros(n, dtype=np.float64 if vtype.value == 1 else np.int64)
    m = L.dh_dazz_read_extra(*args, data.ctypes.data, n)
    if m < 0:
        _check(int(m))
    return MaskExtra(data, ACCUM_MODES[accum.value])


def write_mask_extra(db_path, mask, name, data, accum="exact"):
    """dh_dazz_write_extra: `data` (integers as int64, anything else as float64) appended to the mask as the extra `name`."""
    a = np.asarray(data)
    a = np.ascontiguousarray(a, dtype=np.int64 if a.dtype.kind in "iub" else np.float64)
    _check(lib().dh_dazz_write_extra(db_path.encode(), mask.encode(), name.encode(), int(a.dtype == np.float64),
                                     ACCUM_MODES.index(accum), a.ctypes.data, len(a)))


def bed_to_mask(db, bed_text, bed_name="-", data_comments=False):
    """dh_bed_to_mask: the BED text against the opened DazzDb `db` (the whole .dam) as BedMask(ptr, iv, contig_ids, read_off,
    read_ids): the mask as read_mask returns it, contig_ids int64[count, 2], the read ids of interval i at
    read_ids[read_off[i]:read_off[i + 1]]."""
    L = lib()
    b = bed_text.encode() if isinstance(bed_text, str) else bed_text
    h = ctypes.c_void_p()
    _check(L.dh_bed_to_mask(db._h, b, len(b), bed_name.encode(), int(data_comments), ctypes.byref(h)))
    try:
        n = L.dh_bed_mask_count(h)
        read_off = copy(L.dh_bed_mask_read_off(h), n + 1, np.int64)
        return BedMask(copy(L.dh_bed_mask_ptr(h), L.dh_bed_mask_ncontigs(h) + 1, np.int64), copy(L.dh_bed_mask_iv(h), 2 * n, np.int32),
                       copy(L.dh_bed_mask_contig_ids(h), (n, 2), np.int64), read_off,
                       copy(L.dh_bed_mask_read_ids(h), int(read_off[-1]), np.int64))
    finally:
        L.dh_bed_mask_destroy(h)


def load_reads(ctx, path, ids):
    """dh_dazz_load_reads: the reads `ids` (ascending, distinct ids of the trimmed view of `path`, which may name a block) from
    disk to a device Db, without opening the DB on the host.  DH_LOAD_CHUNK_MB sets the packed MiB per chunk."""
    v = np.ascontiguousarray(ids, dtype=np.int32)
    h = ctypes.c_void_p()
    _check(lib().dh_dazz_load_reads(ctx._h, path.encode(), addr(v), len(v), ctypes.byref(h)))
    return Db._from_handle(ctx, h)


def load_stats(ctx):
    """dh_get_load_stats: the context's last load_reads -- ms of file reads, uploads, kernels and the whole call; packed bytes
    read, bases written, runs, chunks."""
    ms, cnt = (ctypes.c_double * 4)(), (ctypes.c_int64 * 4)()
    _check(lib().dh_get_load_stats(ctx._h, ms, cnt))
    return {"ms_file": ms[0], "ms_copy": ms[1], "ms_kernel": ms[2], "ms_total": ms[3], "packed_bytes": cnt[0], "bases": cnt[1],
            "runs": cnt[2], "chunks": cnt[3]}


# ---------------------------------------------------------------- pile-ups.db / insertions.db (host only)
def pileups_from_db(path, first, count, contig_off):
    """dh_pileups_from_db: pile-ups [first, first + count) of a pile-ups.db (count -1: to the end) as (Pileups ordered by node,
    las, trace, tspace, file_index) -- file_index[i] = where pile-up i stood in the file."""
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    hp, hs, fi = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    L = lib()
    _check(L.dh_pileups_from_db(path.encode(), first, count, co.ctypes.data, len(co) - 1, ctypes.byref(hp), ctypes.byref(hs), ctypes.byref(fi)))
    piles = Pileups(None, None, None, _handle=hp)
    file_index = copy(fi, len(piles), np.int32)
    L.dh_shard_free(fi)
    las, trace, ts = _take_la_set(hs)
    return piles, las, trace, ts, file_index


def insertions_from_db(path, contig_off):
    """dh_insertions_from_db: an insertions.db (of process_pileups(insertions_db=...), insertiondb_merge or DENTIST) as
    (rec, bases, (ids, ids_off)) in the dtypes output_assembly takes."""
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    h = ctypes.c_void_p()
    _check(lib().dh_insertions_from_db(path.encode(), co.ctypes.data, len(co) - 1, ctypes.byref(h)))
    return _take_insertions(h, None, True)


def _take_chaindb(h):
    L = lib()
    ins = copy(L.dh_chaindb_insertions(h), L.dh_chaindb_ninsertions(h), INSERTION_REC_DTYPE)
    out = dict(pile_counts=copy(L.dh_chaindb_pile_counts(h), L.dh_chaindb_npiles(h), np.int32),
               ra_counts=copy(L.dh_chaindb_read_alignment_counts(h), L.dh_chaindb_nread_alignments(h), np.int32),
               seeded=copy(L.dh_chaindb_seeded(h), L.dh_chaindb_nseeded(h), SEEDED_DTYPE),
               las=copy(L.dh_chaindb_las(h), L.dh_chaindb_nlas(h), CHAIN_LA_DTYPE),
               trace=copy(L.dh_chaindb_trace(h), L.dh_chaindb_ntrace(h), np.uint16),
               insertions=ins, bases=copy(L.dh_chaindb_bases(h), int(ins["seq_len"].sum()) if len(ins) else 0, np.uint8),
               read_ids=copy(L.dh_chaindb_read_ids(h), int(ins["nread_ids"].sum()) if len(ins) else 0, np.uint32))
    L.dh_chaindb_destroy(h)
    return out


def pileupdb_write(path, pile_counts, ra_counts, seeded, las, trace):
    pc, rc = (np.ascontiguousarray(x, dtype=np.int32) for x in (pile_counts, ra_counts))
    sa, la = np.ascontiguousarray(seeded, dtype=SEEDED_DTYPE), np.ascontiguousarray(las, dtype=CHAIN_LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    _check(lib().dh_pileupdb_write(path.encode(), len(pc), pc.ctypes.data, rc.ctypes.data, sa.ctypes.data, la.ctypes.data,
                                   tr.ctypes.data))


def pileupdb_read(path):
    h = ctypes.c_void_p()
    _check(lib().dh_pileupdb_read(path.encode(), ctypes.byref(h)))
    return _take_chaindb(h)


def insertiondb_write(path, insertions, bases, read_ids, seeded, las, trace):
    ins = np.ascontiguousarray(insertions, dtype=INSERTION_REC_DTYPE)
    b, ids = np.ascontiguousarray(bases, dtype=np.uint8), np.ascontiguousarray(read_ids, dtype=np.uint32)
    sa, la = np.ascontiguousarray(seeded, dtype=SEEDED_DTYPE), np.ascontiguousarray(las, dtype=CHAIN_LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    _check(lib().dh_insertiondb_write(path.encode(), len(ins), ins.ctypes.data, b.ctypes.data, ids.ctypes.data, sa.ctypes.data,
                                      la.ctypes.data, tr.ctypes.data))


def insertiondb_read(path):
    h = ctypes.c_void_p()
    _check(lib().dh_insertiondb_read(path.encode(), ctypes.byref(h)))
    return _take_chaindb(h)


def insertiondb_merge(paths, out_path):
    """`dentist merge-insertions` (commands/mergeInsertions.d:42-164): k-way merge of insertions.db files by
    (start contig, start part, end contig, end part); returns the number of insertions written."""
    arr = (ctypes.c_char_p * max(1, len(paths)))(*[p.encode() for p in paths])
    n = ctypes.c_int64(0)
    _check(lib().dh_insertiondb_merge(arr, len(paths), out_path.encode(), ctypes.byref(n)))
    return n.value
