"""Alignment and mapping: the device DB, dh_align_db and its kin, result sets and .las files, edit paths, transposition,
global alignment, the exact locator and the formatters."""
import ctypes
import os
import re
import weakref

import numpy as np

from ._abi import (_HERE, AlignOpts, AlignStats, CumStats, DhError, EXACT_HIT_DTYPE, LA_DTYPE, SEED_CAND_DTYPE, _check,
                   lib)
from ._marshal import Owner, addr, copy, seq_pairs, view


def join_hit_capacity(bases, reads, skip_self=2, rate=0.0, free_bytes=-1):
    """dh_join_hit_capacity: the hits the first attempt of the pile-up join makes room for.  bases / reads: per group;
    rate <= 0: the figure a fresh context starts with; free_bytes < 0: no memory clamp.  Host arithmetic, no device."""
    b = np.ascontiguousarray(bases, dtype=np.int64)
    r = np.ascontiguousarray(reads, dtype=np.int32)
    if b.shape != r.shape or b.ndim != 1:
        raise ValueError("bases and reads: one entry per group each")
    return int(lib().dh_join_hit_capacity(b.ctypes.data, r.ctypes.data, len(b), int(skip_self), float(rate), int(free_bytes)))


def set_fields(o, kw, hidden=()):
    """Keyword overrides of an options struct; a name it does not have (or a padding field) is an AttributeError."""
    for k, v in kw.items():
        if k in hidden or not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def default_align_opts(**kw):
    o = AlignOpts()
    lib().dh_default_align_opts(ctypes.byref(o))
    return set_fields(o, kw)


class _LaSetOwner(Owner):
    """Keeps a library-owned dh_la_set alive for as long as numpy views of its buffers exist."""
    _destroy = "dh_la_set_destroy"


def _take_la_set(h, trace_on_device=False):
    """Zero-copy numpy views of the (page-locked) buffers of a dh_la_set; the set is destroyed
    when the last view goes away.  trace_on_device: the trace as a DeviceTrace, nothing is downloaded."""
    L = lib()
    n, ts = L.dh_la_set_count(h), L.dh_la_set_tspace(h)
    owner = _LaSetOwner(h)
    las = view(L.dh_la_set_records(h) if n else None, n, LA_DTYPE, owner)
    trace = DeviceTrace(owner, h)
    return las, trace if trace_on_device else trace.numpy(), ts


class DeviceTrace:
    """The trace values of a mapping result left on the device (dh_map_reads, want_sorted & 8).  Keeps the result set
    alive; numpy() is the host copy (downloaded on first use)."""

    def __init__(self, owner, handle):
        self._owner, self._h = owner, handle

    def numpy(self):
        L = lib()
        tn = L.dh_la_set_trace_len(self._h)
        return view(L.dh_la_set_trace(self._h) if tn else None, tn, np.uint16, self._owner)

    def on_device(self):
        return bool(lib().dh_la_set_trace_on_device(self._h))

    def __len__(self):
        return int(lib().dh_la_set_trace_len(self._h))


class Db(Owner):
    """Device-resident sequence DB (HBM); built from a dentist_amd.sim.SeqDb-like object."""
    _destroy = "dh_db_destroy"

    def __init__(self, ctx, seqdb):
        self.ctx = ctx
        bases = np.ascontiguousarray(seqdb.bases, dtype=np.uint8)
        off = np.ascontiguousarray(seqdb.off, dtype=np.int64)
        mask = getattr(seqdb, "mask", None)
        group = None if getattr(seqdb, "group", None) is None else np.ascontiguousarray(seqdb.group, np.int32)
        h = ctypes.c_void_p()
        _check(lib().dh_db_create(ctx._h, bases.ctypes.data, off.ctypes.data, len(off) - 1,
                                  group.ctypes.data if group is not None else None, ctypes.byref(h)))
        self._h = h
        self.off = off  # (host copy of the offsets: Context.output_db reads an insertions.db against them)
        ctx._dbs.append(weakref.ref(self))
        if mask is not None:
            self.set_mask(mask[0], mask[1])

    @classmethod
    def _from_handle(cls, ctx, h):
        """A DB the library made (load_reads): the handle is owned by the new object."""
        self = cls.__new__(cls)
        self.ctx = ctx
        self._h = h
        L = lib()
        n = L.dh_db_nreads(h)
        self.off = np.zeros(n + 1, dtype=np.int64)
        _check(L.dh_db_get_offsets(h, self.off.ctypes.data))
        ctx._dbs.append(weakref.ref(self))
        return self

    def _owned(self):   # a device DB goes before its context; afterwards there is nothing left to destroy
        return bool(self.ctx._h)

    def bases(self, first=0, count=None):
        """dh_db_get_bases: the base codes of sequences [first, first + count) from the device, one uint8 array."""
        n = len(self.off) - 1
        count = n - first if count is None else count
        if first < 0 or count < 0 or first + count > n:
            raise DhError(-1, "Db.bases: sequences outside the DB")
        out = np.zeros(int(self.off[first + count] - self.off[first]), dtype=np.uint8)
        _check(lib().dh_db_get_bases(self._h, first, count, addr(out), len(out)))
        return out

    def drop_cache(self):
        _check(lib().dh_db_drop_cache(self._h))

    def set_mask(self, ptr, iv):
        """Soft mask (union of -m tracks): ptr int64[n+1], iv int32 (begin, end) pairs.  Replaces the tracks
        of an earlier call; the bits of dust() / mask_coverage() are a layer of their own and stay (the
        effective mask is the OR).  None clears everything."""
        if ptr is None:
            _check(lib().dh_db_set_mask(self._h, None, None))
            return
        p = np.ascontiguousarray(ptr, dtype=np.int64)
        v = np.ascontiguousarray(iv, dtype=np.int32)
        _check(lib().dh_db_set_mask(self._h, p.ctypes.data, v.ctypes.data))

    def dust(self):
        """DBdust on the device: low-complexity windows are ORed into the soft mask."""
        _check(lib().dh_db_dust(self._h))

    def mask_coverage(self, las, lower, upper, read_off=None, improper_only=False, allowance=0):
        """dh_db_mask_coverage: regions with alignment coverage outside [lower, upper] join the soft mask
        (maskRepetitiveRegions.d:238-430); improper_only counts improper alignments only."""
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        ro = np.ascontiguousarray(read_off, dtype=np.int64) if read_off is not None else None
        _check(lib().dh_db_mask_coverage(self._h, addr(arr), len(arr),
                                         ro.ctypes.data if ro is not None else None, len(ro) - 1 if ro is not None else 0,
                                         int(lower), int(upper), 1 if improper_only else 0, int(allowance)))

    def get_mask(self):
        """The soft mask as (ptr int64[n+1], iv int32 (begin, end) pairs)."""
        n = lib().dh_db_nreads(self._h)
        ptr = np.zeros(n + 1, dtype=np.int64)
        m = lib().dh_db_get_mask(self._h, ptr.ctypes.data, None, 0)
        if m < 0:
            _check(int(m))
        iv = np.zeros(max(2 * m, 2), dtype=np.int32)
        lib().dh_db_get_mask(self._h, ptr.ctypes.data, iv.ctypes.data, m)
        return ptr, iv[:2 * m]


# ---------------------------------------------------------------- the context's statistics and counters
def align_stats(ctx):
    st = AlignStats()
    _check(lib().dh_get_align_stats(ctx._h, ctypes.byref(st)))
    return st


def cum_stats(ctx, reset=False):
    st = CumStats()
    _check(lib().dh_get_cum_stats(ctx._h, ctypes.byref(st), int(reset)))
    return st


def counts(ctx, which, n, reset):
    """dh_get_<which>_counts: the n int64 counters of that name of the context, as a tuple"""
    out = (ctypes.c_int64 * n)()
    _check(getattr(lib(), "dh_get_%s_counts" % which)(ctx._h, out, int(reset)))
    return tuple(int(x) for x in out)


# ---------------------------------------------------------------- align, map, seed
def align_db(ctx, A, B, opts, select_best=False):
    h = ctypes.c_void_p()
    _check(lib().dh_align_db(ctx._h, A._h, B._h, ctypes.byref(opts), int(select_best), ctypes.byref(h)))
    return _take_la_set(h)[:2]


def align_db_block(ctx, A, B, first, count, opts, select_best=False, raw=False):
    h = ctypes.c_void_p()
    _check(lib().dh_align_db_block(ctx._h, A._h, B._h, first, count, ctypes.byref(opts), int(select_best),
                                   ctypes.byref(h)))
    return h if raw else _take_la_set(h)[:2]


def align_db_transposed(ctx, A, B, opts, select_best=False):
    h, h2 = ctypes.c_void_p(), ctypes.c_void_p()
    _check(lib().dh_align_db_transposed(ctx._h, A._h, B._h, ctypes.byref(opts), int(select_best), ctypes.byref(h),
                                        ctypes.byref(h2)))
    return _take_la_set(h)[:2], _take_la_set(h2)[:2]


def remap_skipping_reads(ctx, contigs, reads, contig_ids, read_ids, opts, allowance):
    ci = np.ascontiguousarray(contig_ids, dtype=np.int32)
    ri = np.ascontiguousarray(read_ids, dtype=np.int32)
    h = ctypes.c_void_p()
    _check(lib().dh_remap_skipping_reads(ctx._h, contigs._h, reads._h, ci.ctypes.data, len(ci), ri.ctypes.data, len(ri),
                                         ctypes.byref(opts), int(allowance), ctypes.byref(h)))
    return _take_la_set(h)[:2]


def seed_candidates(ctx, A, B, opts):
    n = 2 * int(lib().dh_db_nreads(B._h))
    cand = np.zeros((n, int(opts.max_cand)), dtype=SEED_CAND_DTYPE)
    ncand, nhits = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    _check(lib().dh_seed_candidates(ctx._h, A._h, B._h, ctypes.byref(opts), cand.ctypes.data, ncand.ctypes.data,
                                    nhits.ctypes.data))
    return cand, ncand, nhits


def extend_candidates(ctx, A, B, opts, cand, ncand, sort=False, transposed=False):
    n = 2 * int(lib().dh_db_nreads(B._h))
    cand = np.ascontiguousarray(cand, dtype=SEED_CAND_DTYPE)
    ncand = np.ascontiguousarray(ncand, dtype=np.int32)
    if cand.size != n * int(opts.max_cand) or ncand.size != n:
        raise DhError(-1, "extend_candidates: cand is [2 n(B), max_cand], ncand [2 n(B)]")
    h, h2 = ctypes.c_void_p(), ctypes.c_void_p()
    _check(lib().dh_extend_candidates(ctx._h, A._h, B._h, ctypes.byref(opts), cand.ctypes.data, ncand.ctypes.data, int(sort),
                                      ctypes.byref(h), ctypes.byref(h2) if transposed else None))
    if transposed:
        return _take_la_set(h)[:2], _take_la_set(h2)[:2]
    return _take_la_set(h)[:2]


def merge_las(handles):
    """LAmerge of in-memory block results (handles from align_db_block(raw=True), consumed)."""
    arr = (ctypes.c_void_p * len(handles))(*[h.value for h in handles])
    out = ctypes.c_void_p()
    rc = lib().dh_la_set_merge(arr, len(handles), ctypes.byref(out))
    for h in handles:
        lib().dh_la_set_destroy(h)
    _check(rc)
    return _take_la_set(out)[:2]


# ---------------------------------------------------------------- .las files, trace-point arithmetic (host only)
def las_write(path, las, trace, tspace):
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    _check(lib().dh_las_write(path.encode(), arr.ctypes.data, len(arr), tr.ctypes.data, tspace))


def las_read(path):
    h = ctypes.c_void_p()
    _check(lib().dh_las_read(path.encode(), ctypes.byref(h)))
    return _take_la_set(h)


def las_merge(paths, out_path):
    """LAmerge: several .las files (same trace spacing) into one, LAsort order (host only)."""
    arr = (ctypes.c_char_p * len(paths))(*[p.encode() for p in paths])
    _check(lib().dh_las_merge(arr, len(paths), out_path.encode()))


def translate_trace_point(la, trace, tspace, apos, mode="floor"):
    """Trace.translateTracePoint!"contigA" (base.d:185-244) of the product: (a, b) of the trace point
    apos is assigned to; raises DhError when apos is outside the LA.  la: one LA_DTYPE record."""
    rec = np.zeros(1, dtype=LA_DTYPE)
    rec[0] = la
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    a, b = ctypes.c_int32(), ctypes.c_int32()
    _check(lib().dh_translate_trace_point(rec.ctypes.data, tr.ctypes.data, tspace, apos,
                                          {"floor": 0, "ceil": 1}[mode], ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def common_trace_point(las, first, contig_len, tspace, seed_front, mask=None):
    """getCommonTracePoint (cropper.d:446-500) of the product for one flank: first = the first records of the flank's
    alignment chains in las; mask = [(begin, end), ...] of the contig's repeat mask.  -1 when there is none."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    fi = np.ascontiguousarray(first, dtype=np.int32)
    mk = np.ascontiguousarray(mask if mask is not None else [], dtype=np.int32).reshape(-1)
    out = ctypes.c_int32()
    _check(lib().dh_common_trace_point(arr.ctypes.data, len(arr), fi.ctypes.data, len(fi), contig_len, tspace,
                                       int(bool(seed_front)), addr(mk), len(mk) // 2, ctypes.byref(out)))
    return out.value


# ---------------------------------------------------------------- edit paths, chain paths, transposition
class EditPaths(Owner):
    """Result of Context.edit_paths: numpy views of a library-owned dh_edit_paths (alive as long as this object is).
    ops: one byte per op (0 match, 1 deletion, 2 insertion, 3 mismatch), record i at ops[op_off[i]:op_off[i + 1]];
    score: per record; tile_score[tile_off[i]:tile_off[i + 1]]: per trace tile of record i; general_tiles: tiles
    aligned by the full-matrix kernel."""
    _destroy = "dh_edit_paths_destroy"

    def __init__(self, h):
        L = lib()
        self._h = h
        n = L.dh_edit_paths_count(h)
        self.op_off = view(L.dh_edit_paths_op_off(h), n + 1, np.int64, self)
        self.tile_off = view(L.dh_edit_paths_tile_off(h), n + 1, np.int64, self)
        self.score = view(L.dh_edit_paths_score(h), n, np.int32, self)
        self.ops = view(L.dh_edit_paths_ops(h), int(self.op_off[-1]), np.uint8, self)
        self.tile_score = view(L.dh_edit_paths_tile_score(h), int(self.tile_off[-1]), np.uint16, self)
        self.general_tiles = int(L.dh_edit_paths_general_tiles(h))

    def __len__(self):
        return len(self.score)


def la_edit_paths(ctx, A, B, las, trace=None, tspace=None, first=0, count=None):
    h = ctypes.c_void_p()
    L = lib()
    if isinstance(las, ctypes.c_void_p):
        n = L.dh_la_set_count(las)
        count = n - first if count is None else count
        _check(L.dh_la_set_edit_paths(ctx._h, A._h, B._h, las, int(first), int(count), ctypes.byref(h)))
    else:
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16)
        count = len(arr) - first if count is None else count
        _check(L.dh_la_edit_paths(ctx._h, A._h, B._h, arr.ctypes.data, len(arr), tr.ctypes.data, int(tspace), int(first),
                                  int(count), ctypes.byref(h)))
    return EditPaths(h)


CP_OK, CP_FAKED, CP_NESTED = 0, 1, 2  # status of Context.chain_paths


def la_chain_paths(ctx, A, B, las, trace=None, tspace=None, chain_off=None):
    h = ctypes.c_void_p()
    L = lib()
    if isinstance(las, ctypes.c_void_p):
        if chain_off is not None:
            raise ValueError("a set's chains are read from its flags")
        status = np.zeros(max(int(L.dh_la_set_count(las)), 1), dtype=np.int32)
        _check(L.dh_la_set_chain_paths(ctx._h, A._h, B._h, las, ctypes.byref(h), status.ctypes.data))
    else:
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16)
        status = np.zeros(max(len(arr), 1), dtype=np.int32)
        co, nch = None, 0
        if chain_off is not None:
            co = np.ascontiguousarray(chain_off, dtype=np.int64)
            if len(co) < 1:
                raise ValueError("chain_off needs nchains + 1 entries")
            nch = len(co) - 1
            status = np.zeros(max(nch, 1), dtype=np.int32)
        _check(L.dh_la_chain_paths(ctx._h, A._h, B._h, addr(arr), len(arr), addr(tr), int(tspace),
                                   None if co is None else co.ctypes.data, nch, ctypes.byref(h), status.ctypes.data))
    ep = EditPaths(h)
    return ep.op_off.copy(), ep.ops.copy(), ep.score.copy(), status[:len(ep)].copy(), int(L.dh_edit_paths_fillers(ep._h))


def la_transpose(ctx, A, B, las, trace=None, tspace=None, select_best=False):
    h = ctypes.c_void_p()
    L = lib()
    if isinstance(las, ctypes.c_void_p):
        src = np.zeros(L.dh_la_set_count(las), dtype=np.int64)
        _check(L.dh_la_set_transpose(ctx._h, A._h, B._h, las, int(select_best), ctypes.byref(h), src.ctypes.data))
    else:
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16)
        src = np.zeros(len(arr), dtype=np.int64)
        _check(L.dh_la_transpose(ctx._h, A._h, B._h, arr.ctypes.data, len(arr), tr.ctypes.data, int(tspace),
                                 int(select_best), ctypes.byref(h), src.ctypes.data))
    out, otr, _ = _take_la_set(h)
    return out, otr, src


# ---------------------------------------------------------------- global alignment, exact locator
NW_OK, NW_BAND_EXCEEDED = 0, 1
NW_MAX_LEN, NW_MAX_BAND = 65536, 4096
NWA_DEFAULT_SCORING = (5, -4, 16, 4)

# limits the kernels' instantiations decide: read from include/dentist_hip.h, not repeated here -- on first use, so that
# importing the package needs nothing outside it
_HEADER_LIMITS = {"NWA_MAX_LEN": "DH_NWA_MAX_LEN", "NWA_MAX_BAND": "DH_NWA_MAX_BAND"}


def header_limit(name):
    with open(os.path.join(_HERE, "..", "include", "dentist_hip.h")) as f:
        m = re.search(r"^#define\s+" + _HEADER_LIMITS[name] + r"\s+(\d+)\s*$", f.read(), flags=re.M)
    if not m:
        raise RuntimeError(f"{_HEADER_LIMITS[name]} is not defined in include/dentist_hip.h")
    return int(m.group(1))


def _scoring(scoring):
    """dh_nw_scoring as four int32, None for the library's default"""
    if scoring is None:
        return None
    sc = np.asarray(scoring, dtype=np.int64)
    if sc.shape != (4,) or np.any(np.abs(sc) > 2 ** 31 - 1):
        raise ValueError("scoring is (match, mismatch, gap_open, gap_extend), four 32-bit integers")
    return np.ascontiguousarray(sc, dtype=np.int32)


def _seq_bytes(x):
    return np.frombuffer(x.encode(), dtype=np.uint8) if isinstance(x, str) else np.ascontiguousarray(x, dtype=np.uint8)


def _concat_seqs(seqs):
    arrs = [_seq_bytes(x) for x in seqs]
    off = np.zeros(len(arrs) + 1, dtype=np.int64)
    if arrs:
        off[1:] = np.cumsum([len(a) for a in arrs])
    return (np.concatenate(arrs) if arrs else np.zeros(0, np.uint8)), off


def concat_pairs(refs, qrys):
    """refs[i] against qrys[i]: both lists concatenated, as the *_raw calls take them"""
    if len(refs) != len(qrys):
        raise ValueError("refs and qrys differ in length")
    return _concat_seqs(refs) + _concat_seqs(qrys)


def nw_batch_raw(ctx, ref, ref_off, qry, qry_off, free_shift=False):
    r, roff, q, qoff = seq_pairs(ref, ref_off, qry, qry_off)
    n = len(roff) - 1
    status = np.zeros(n, dtype=np.int32)
    h = ctypes.c_void_p()
    _check(lib().dh_nw_batch(ctx._h, r.ctypes.data, roff.ctypes.data, q.ctypes.data, qoff.ctypes.data, n, int(bool(free_shift)),
                             ctypes.byref(h), status.ctypes.data))
    return EditPaths(h), status


def nw_affine_batch_raw(ctx, ref, ref_off, qry, qry_off, scoring=None):
    r, roff, q, qoff = seq_pairs(ref, ref_off, qry, qry_off)
    n = len(roff) - 1
    sc = _scoring(scoring)
    status = np.zeros(n, dtype=np.int32)
    h = ctypes.c_void_p()
    _check(lib().dh_nw_affine_batch(ctx._h, r.ctypes.data, roff.ctypes.data, q.ctypes.data, qoff.ctypes.data, n,
                                    sc.ctypes.data if sc is not None else None, ctypes.byref(h), status.ctypes.data))
    return EditPaths(h), status


def exact_locate_raw(ctx, ref, ref_off, qry, qry_off, both_strands=True):
    r, roff, q, qoff = seq_pairs(ref, ref_off, qry, qry_off, same_count=False)
    h = ctypes.c_void_p()
    L = lib()
    _check(L.dh_exact_locate(ctx._h, r.ctypes.data, roff.ctypes.data, len(roff) - 1, q.ctypes.data, qoff.ctypes.data,
                             len(qoff) - 1, int(bool(both_strands)), ctypes.byref(h)))
    try:
        return copy(L.dh_exact_hits_records(h), L.dh_exact_hits_count(h), EXACT_HIT_DTYPE)
    finally:
        L.dh_exact_hits_destroy(h)


# ---------------------------------------------------------------- formatters (host only)
def _format(fn, *args):
    n = fn(*args, None, 0)
    if n < 0:
        _check(int(n))
    buf = ctypes.create_string_buffer(int(n) + 1)
    assert fn(*args, buf, int(n) + 1) == n
    return buf.value.decode()


def format_cigar(ops, extended=True):
    """dh_format_cigar: runs of = X I D (extended) or M I D of an op array of Context.edit_paths."""
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    return _format(lib().dh_format_cigar, o.ctypes.data, len(o), int(bool(extended)))


def format_alignment(a, b, ops, width=0):
    """dh_format_alignment: the reference's SequenceAlignment.toString(width) of sequences a (A side) and b (B side, in the
    frame of the alignment) under an op array; a / b are strings or base-code arrays."""
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    sa, sb = _seq_bytes(a), _seq_bytes(b)
    if int(np.count_nonzero(o != 2)) > len(sa) or int(np.count_nonzero(o != 1)) > len(sb):
        raise ValueError("the ops consume more bases than the sequences have")
    return _format(lib().dh_format_alignment, sa.ctypes.data, sb.ctypes.data, o.ctypes.data, len(o), int(width))


def format_pair(name_a, a, name_b, b, ops, score, scoring=None, width=0):
    """dh_format_pair: the alignment as EMBOSS `pair` text (what `dentist check-results` reads from stretcher); width 0
    writes one block."""
    o = np.ascontiguousarray(ops, dtype=np.uint8)
    sa, sb = _seq_bytes(a), _seq_bytes(b)
    sc = _scoring(scoring)
    return _format(lib().dh_format_pair, name_a.encode(), sa.ctypes.data, len(sa), name_b.encode(), sb.ctypes.data, len(sb),
                   o.ctypes.data, len(o), int(score), sc.ctypes.data if sc is not None else None, int(width))
