"""Pile-ups and what is done with them: the mapping pass that collects them, crop and process, the stage-level calls and
the scaffold-graph builder."""
import ctypes

import numpy as np

from ._abi import (INSERTION_DTYPE, JOIN_DTYPE, LA_DTYPE, READ_ALIGNMENT_DTYPE, REMAP_FN, ProcessOpts, ScaffoldOpts, _check,
                   lib)
from ._align import DeviceTrace, _take_la_set, set_fields
from ._marshal import Owner, addr, copy, optional_mask


def default_process_opts(**kw):
    o = ProcessOpts()
    lib().dh_default_process_opts(ctypes.byref(o))
    return set_fields(o, kw)


def _triples(triples_per_pile):
    """(count int32[npiles], triples int32[total, 3]) of one (k, 3) array per pile-up"""
    cnt = np.asarray([len(t) for t in triples_per_pile], dtype=np.int32)
    tri = (np.ascontiguousarray(np.concatenate([np.asarray(t, dtype=np.int32).reshape(-1, 3)
                                                for t in triples_per_pile]), dtype=np.int32)
           if len(triples_per_pile) else np.zeros((0, 3), np.int32))
    return cnt, tri


class Pileups(Owner):
    """Spanning-read pile-ups per gap (host only): dh_collect_spanning; ``candidates=True`` skips the
    min/max-reads cut (dh_collect_candidates)."""
    _destroy = "dh_pileups_destroy"

    def __init__(self, las, contig_off, opts, candidates=False, _handle=None, _keep=None):
        self._keep = _keep   # a borrowed handle (owned by _keep, e.g. a ShardPlan): never destroyed here
        if _handle is not None:
            self._h = _handle
            return
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        off = np.ascontiguousarray(contig_off, dtype=np.int64)
        h = ctypes.c_void_p()
        fn = lib().dh_collect_candidates if candidates else lib().dh_collect_spanning
        _check(fn(arr.ctypes.data, len(arr), off.ctypes.data, len(off) - 1, ctypes.byref(opts), ctypes.byref(h)))
        self._h = h

    def _owned(self):
        return getattr(self, "_keep", None) is None

    def close(self):
        super().close()
        self._keep = None

    @classmethod
    def from_triples(cls, contig_left, triples_per_pile):
        """dh_pileups_create: gaps ordered by contig_left, one (k, 3) int32 array of
        (read, left LA index, right LA index) per gap."""
        return cls.from_flat(contig_left, *_triples(triples_per_pile))

    @classmethod
    def from_joins(cls, nodes4, triples_per_pile):
        """dh_pileups_create_joins: pile-ups of any join -- nodes4[i] = (contig0, seed0, contig1, seed1), seed 0 = front,
        1 = back, contig1 = -1 for an extension pile-up; ordered by their nodes."""
        nd = np.ascontiguousarray(nodes4, dtype=np.int32).reshape(-1, 4)
        cnt, tri = _triples(triples_per_pile)
        h = ctypes.c_void_p()
        _check(lib().dh_pileups_create_joins(nd.ctypes.data, cnt.ctypes.data, len(nd), tri.ctypes.data, ctypes.byref(h)))
        return cls(None, None, None, _handle=h)

    def get_join(self, i):
        """(contig0, seed0, contig1, seed1) of pile-up i."""
        nd = np.zeros(4, dtype=np.int32)
        _check(lib().dh_pileups_get_join(self._h, i, nd.ctypes.data))
        return tuple(int(x) for x in nd)

    def write_db(self, path, las, trace, contig_off, read_off, tspace=100):
        """dh_pileups_write_db: DENTIST's pile-ups.db for these pile-ups."""
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16)
        co, ro = np.ascontiguousarray(contig_off, dtype=np.int64), np.ascontiguousarray(read_off, dtype=np.int64)
        _check(lib().dh_pileups_write_db(self._h, arr.ctypes.data, len(arr), tr.ctypes.data, co.ctypes.data, len(co) - 1,
                                         ro.ctypes.data, len(ro) - 1, tspace, path.encode()))

    def flat(self):
        """(contig_left int32[npiles], count int32[npiles], triples int32[total, 3]) in one call."""
        L = lib()
        n = len(self)
        cl, cnt = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        tot = L.dh_pileups_flat(self._h, None, None, None)
        tri = np.zeros((tot, 3), dtype=np.int32)
        L.dh_pileups_flat(self._h, cl.ctypes.data, cnt.ctypes.data, tri.ctypes.data)
        return cl, cnt, tri

    @classmethod
    def from_flat(cls, contig_left, count, triples):
        cl = np.ascontiguousarray(contig_left, dtype=np.int32)
        cnt = np.ascontiguousarray(count, dtype=np.int32)
        tri = np.ascontiguousarray(triples, dtype=np.int32)
        h = ctypes.c_void_p()
        _check(lib().dh_pileups_create(cl.ctypes.data, cnt.ctypes.data, len(cl), tri.ctypes.data, ctypes.byref(h)))
        return cls(None, None, None, _handle=h)

    def select(self, las, opts):
        """dh_pileups_select: the min_reads / max_reads cut."""
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        h = ctypes.c_void_p()
        _check(lib().dh_pileups_select(self._h, arr.ctypes.data, len(arr), ctypes.byref(opts), ctypes.byref(h)))
        return Pileups(None, None, None, _handle=h)

    def __len__(self):
        return lib().dh_pileups_count(self._h)

    def get(self, i):
        g = ctypes.c_int32()
        p = ctypes.c_void_p()
        n = lib().dh_pileups_get(self._h, i, ctypes.byref(g), ctypes.byref(p))
        return g.value, copy(p, (n, 3), np.int32)


def map_reads(ctx, A, B, opts, popts, first=0, count=None, repeat_mask=None, sorted=True, candidates=False,
              trace_on_device=False):
    keep, rp, ri = optional_mask(repeat_mask)
    L = lib()
    n = L.dh_db_nreads(B._h)
    count = n - first if count is None else count
    dropped = np.zeros(6, dtype=np.int64)
    h, ph = ctypes.c_void_p(), ctypes.c_void_p()
    _check(L.dh_map_reads(ctx._h, A._h, B._h, int(first), int(count), ctypes.byref(opts), ctypes.byref(popts), rp, ri,
                          (1 if sorted else 0) | (8 if trace_on_device else 0), dropped.ctypes.data, ctypes.byref(h),
                          ctypes.byref(ph) if candidates else None))
    las, trace, _ = _take_la_set(h, trace_on_device)
    if candidates:
        return las, trace, dropped, Pileups(None, None, None, _handle=ph)
    return las, trace, dropped


# ---------------------------------------------------------------- crop and process
def _take_insertions(h, insertions_db=None, read_ids=False):
    """insertions_db = (path, contig_off, tspace): also write the result as DENTIST's insertions.db.
    read_ids: also return (ids, off): the 0-based read ids of every record's pile-up."""
    L = lib()
    if insertions_db is not None:
        path, contig_off, tspace = insertions_db
        off = np.ascontiguousarray(contig_off, dtype=np.int64)
        rc = L.dh_insertions_write_db(h, off.ctypes.data, len(off) - 1, tspace, path.encode())
        if rc != 0:
            L.dh_insertions_destroy(h)
            _check(rc)
    n = L.dh_insertions_count(h)
    rec = copy(L.dh_insertions_records(h), n, INSERTION_DTYPE)
    bases = copy(L.dh_insertions_bases(h), L.dh_insertions_bases_len(h), np.uint8)
    ids = None
    if read_ids:
        po = L.dh_insertions_read_ids_off(h)
        if po and n:
            off = copy(po, n + 1, np.int32).astype(np.int64)
            ids = (copy(L.dh_insertions_read_ids(h), int(off[-1]), np.int32), off)
        else:
            ids = (np.zeros(0, np.int32), np.zeros(n + 1, np.int64))
    L.dh_insertions_destroy(h)
    return (rec, bases, ids) if read_ids else (rec, bases)


class Cropped(Owner):
    """Cropped pile-ups (dh_cropped): per pile-up record + per cropped read (pile, entry, read id, bases)."""
    _destroy = "dh_cropped_destroy"

    @classmethod
    def crop(cls, ctx, contigs, reads, read_first, las, trace, piles, opts, repeat_mask=None):
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16)
        h = ctypes.c_void_p()
        keep, rp, ri = optional_mask(repeat_mask)
        _check(lib().dh_crop_pileups_masked(ctx._h, contigs._h, reads._h, read_first, arr.ctypes.data, len(arr), addr(tr),
                                            piles._h, rp, ri, ctypes.byref(opts), ctypes.byref(h)))
        return cls(h)

    @classmethod
    def create(cls, rec, pile, entry, read_id, off, bases, kind=None):
        r = np.ascontiguousarray(rec, dtype=INSERTION_DTYPE)
        pi, en, ri = (np.ascontiguousarray(x, dtype=np.int32) for x in (pile, entry, read_id))
        of = np.ascontiguousarray(off, dtype=np.int64)
        ba = np.ascontiguousarray(bases, dtype=np.uint8)
        ki = None if kind is None else np.ascontiguousarray(kind, dtype=np.uint8)
        h = ctypes.c_void_p()
        _check(lib().dh_cropped_create2(r.ctypes.data, len(r), len(pi), pi.ctypes.data, en.ctypes.data, ri.ctypes.data,
                                        addr(ki), of.ctypes.data, addr(ba), ctypes.byref(h)))
        return cls(h)

    def kind(self):
        """Per cropped read: 0 spans the gap, 1 / 2 extension entry of the left / right contig."""
        L, h = lib(), self._h
        return copy(L.dh_cropped_kind(h), L.dh_cropped_nreads(h), np.uint8)

    def arrays(self):
        """(records, pile, entry, read_id, off, bases) as numpy copies (bases come over PCIe)."""
        L, h = lib(), self._h
        npl, nr = L.dh_cropped_npiles(h), L.dh_cropped_nreads(h)
        rec = copy(L.dh_cropped_records(h), npl, INSERTION_DTYPE)
        off = copy(L.dh_cropped_offsets(h), nr + 1, np.int64) if nr else np.zeros(1, np.int64)
        bp = L.dh_cropped_bases(h)
        if not bp:
            _check(-3)
        return (rec, copy(L.dh_cropped_pile(h), nr, np.int32), copy(L.dh_cropped_entry(h), nr, np.int32),
                copy(L.dh_cropped_read_id(h), nr, np.int32), off, copy(bp, int(off[-1]), np.uint8))

    def process(self, ctx, contigs, opts):
        h = ctypes.c_void_p()
        _check(lib().dh_process_cropped(ctx._h, contigs._h, self._h, ctypes.byref(opts), ctypes.byref(h)))
        return _take_insertions(h)


def process_pileups(ctx, contigs, reads, las, trace, piles, opts, insertions_db=None, read_ids=False, repeat_mask=None):
    """dentist `process` for a batch of pile-ups on the GPU. Returns (records, consensus bases);
    insertions_db = (path, contig_off, tspace) also writes DENTIST's insertions.db; read_ids = True adds
    (ids, off): the read ids of every record's pile-up (what `dentist output` lists in its BED / AGP);
    repeat_mask = (ptr, intervals): the contigs' repeat mask for the cropper (dh_process_pileups_masked)."""
    L = lib()
    h = ctypes.c_void_p()
    keep, rp, ri = optional_mask(repeat_mask)
    if isinstance(trace, DeviceTrace):   # (the records are the set's own: `las` is the view of them map_reads returned)
        _check(L.dh_process_pileups_set(ctx._h, contigs._h, reads._h, trace._h, piles._h, rp, ri, ctypes.byref(opts), ctypes.byref(h)))
        return _take_insertions(h, insertions_db, read_ids)
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    _check(L.dh_process_pileups_masked(ctx._h, contigs._h, reads._h, arr.ctypes.data, len(arr), tr.ctypes.data,
                                       piles._h, rp, ri, ctypes.byref(opts), ctypes.byref(h)))
    return _take_insertions(h, insertions_db, read_ids)


def process_pileups_db(ctx, contigs, reads_db_path, pileups_path, opts, first=0, count=-1, repeat_mask=None, insertions_db=None,
                       read_ids=False):
    h = ctypes.c_void_p()
    keep, rp, ri = optional_mask(repeat_mask)
    _check(lib().dh_process_pileups_db(ctx._h if ctx is not None else None, contigs._h, reads_db_path.encode(), pileups_path.encode(),
                                       first, count, rp, ri, ctypes.byref(opts), ctypes.byref(h)))
    return _take_insertions(h, insertions_db, read_ids)


def process_stats(ctx):
    ms = (ctypes.c_float * 7)()
    cnt = (ctypes.c_int64 * 3)()
    _check(lib().dh_get_process_stats(ctx._h, ms, cnt))
    names = ("crop", "pile_align", "tile_qv", "consensus", "realign", "flank_align", "total")
    d = {f"ms_{n}": float(ms[i]) for i, n in enumerate(names)}
    d.update(pile_las=int(cnt[0]), tiles=int(cnt[1]), nw_cells=int(cnt[2]))
    wk = (ctypes.c_int64 * 4)()
    _check(lib().dh_get_process_work(ctx._h, wk))
    d.update(pile_ups=int(wk[0]), entries=int(wk[1]), cropped_bases=int(wk[2]), algorithmic_bytes=int(wk[3]))
    return d


# ---------------------------------------------------------------- stage-level calls
def tile_qv(ctx, db, las, trace, tspace, cov, maxtiles):
    """DAScover + DASqv: intrinsic QV per (read, tile) of a pile-up DB; las grouped by aread."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    qv = np.zeros((lib().dh_db_nreads(db._h), maxtiles), dtype=np.uint8)
    _check(lib().dh_tile_qv(ctx._h, db._h, arr.ctypes.data, len(arr), tr.ctypes.data, tspace, cov, qv.ctypes.data,
                            maxtiles))
    return qv


def consensus(ctx, db, las, trace, tspace, ref_read, rounds=1):
    """computeintrinsicqv + daccord: consensus of read ref_read of the DB from its overlaps."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    cap = 1 << 20
    while True:
        out = np.zeros(cap, dtype=np.uint8)
        n = ctypes.c_int64(0)
        rc = lib().dh_consensus(ctx._h, db._h, arr.ctypes.data, len(arr), tr.ctypes.data, tspace, ref_read, rounds,
                                out.ctypes.data, cap, ctypes.byref(n))
        if rc != 0 and n.value > cap:
            cap = int(n.value)
            continue
        _check(rc)
        return out[:n.value].copy()


# ---------------------------------------------------------------- the scaffold graph (host only)
_SCAFFOLD_INT_OPTS = ("min_spanning_reads", "merge_extensions", "only_joins")
# the callback of dh_scaffold_pileups_cb hands its records over in memory the library frees
_malloc = ctypes.CFUNCTYPE(ctypes.c_void_p, ctypes.c_size_t)(("malloc", ctypes.CDLL(None)))


def scaffold_opts(kw, int_opts=_SCAFFOLD_INT_OPTS):
    """dh_default_scaffold_opts with keyword overrides; an unknown name is a TypeError"""
    o = ScaffoldOpts()
    lib().dh_default_scaffold_opts(ctypes.byref(o))
    for k, v in kw.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown scaffold option {k}")
        setattr(o, k, int(v) if k in int_opts else float(v))
    return o


def input_gaps_array(input_gaps):
    return np.ascontiguousarray(input_gaps if input_gaps is not None else np.zeros((0, 2)), dtype=np.int32).reshape(-1, 2)


def _scaffold(las, contig_off, read_off, input_gaps, kw, resolve=None):
    """The scaffold handle and the LA array it indexes.  resolve = None: dh_scaffold_pileups.  resolve = dict(ctx=, contigs=,
    reads=, map_opts=, trace=, allowance=100): dh_scaffold_pileups_resolved (resolveBubbles, the device re-maps the skipping
    reads); resolve = dict(remap=callable(contig_ids, read_ids) -> LA_DTYPE array): dh_scaffold_pileups_cb.  With resolve the
    result carries (las incl. the added alignments, trace incl. theirs or None, bubbles resolved) in the handle's slot 2."""
    L = lib()
    kw = dict(kw)
    mbs, mit = int(kw.pop("max_bubble_size", 0)), int(kw.pop("max_bubble_iterations", 0))
    o = scaffold_opts(kw, ("min_spanning_reads", "merge_extensions"))   # (only_joins is the sharded plan's)
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    ig = input_gaps_array(input_gaps)
    h = ctypes.c_void_p()
    if resolve is None or "remap" in resolve:
        co, ro = np.ascontiguousarray(contig_off, dtype=np.int64), np.ascontiguousarray(read_off, dtype=np.int64)
        graph = (arr.ctypes.data, len(arr), co.ctypes.data, len(co) - 1, ro.ctypes.data, len(ro) - 1, addr(ig), len(ig), ctypes.byref(o))
    if resolve is None:
        _check(L.dh_scaffold_pileups(*graph, ctypes.byref(h)))
        return h, arr
    ex = ctypes.c_void_p()
    nres = ctypes.c_int32(0)
    if "remap" in resolve:
        fn = resolve["remap"]

        def cb(user, cids, nc, rids, nr, out, nout):
            try:
                got = np.ascontiguousarray(fn([cids[i] for i in range(nc)], [rids[i] for i in range(nr)]), dtype=LA_DTYPE)
                p = _malloc(max(1, got.nbytes))
                if got.nbytes:
                    ctypes.memmove(p, got.ctypes.data, got.nbytes)
                out[0] = p
                nout[0] = len(got)
                return 0
            except Exception:  # noqa: BLE001
                return -1
        _check(L.dh_scaffold_pileups_cb(*graph, mbs, mit, REMAP_FN(cb), None, ctypes.byref(h), ctypes.byref(ex), ctypes.byref(nres)))
        trace = None
    else:
        _check(L.dh_scaffold_pileups_resolved(resolve["ctx"]._h, resolve["contigs"]._h, resolve["reads"]._h, arr.ctypes.data, len(arr),
                                              addr(ig), len(ig), ctypes.byref(o),
                                              ctypes.byref(resolve["map_opts"]), int(resolve.get("allowance", 100)), mbs, mit,
                                              ctypes.byref(h), ctypes.byref(ex), ctypes.byref(nres)))
        trace = np.ascontiguousarray(resolve["trace"], dtype=np.uint16)
    xl, xt, _ = _take_la_set(ex)
    if len(xl):
        xl = xl.copy()
        if trace is not None:
            xl["toff"] += len(trace)
            trace = np.concatenate([trace, xt])
        arr = np.concatenate([arr, xl])
    return h, arr, trace, int(nres.value)


def scaffold_pileups(las, contig_off, read_off, input_gaps=None, resolve=None, **opts):
    """dh_scaffold_pileups: the scaffold-graph pile-up builder of `dentist collect`
    (pileups.d:173-208).  Returns (joins JOIN_DTYPE[npiles], read alignments READ_ALIGNMENT_DTYPE[...]); with
    resolve (see _scaffold: resolveBubbles) also (las incl. the added alignments, trace or None, bubbles resolved)."""
    L = lib()
    sc = _scaffold(las, contig_off, read_off, input_gaps, opts, resolve)
    h = sc[0]
    try:
        joins = copy(L.dh_scaffold_joins(h), L.dh_scaffold_npiles(h), JOIN_DTYPE)
        ent = copy(L.dh_scaffold_entries(h), L.dh_scaffold_nentries(h), READ_ALIGNMENT_DTYPE)
    finally:
        L.dh_scaffold_destroy(h)
    return (joins, ent) + tuple(sc[1:] if resolve is not None else ())


def _scaffold_piles(sc, resolve, fn, *which):
    """The pile-ups fn makes of the scaffold sc (consumed): (Pileups, skipped), with resolve followed by the LA / trace
    arrays the pile-ups index and the bubbles resolved"""
    h, arr = sc[0], sc[1]
    try:
        ph = ctypes.c_void_p()
        skipped = ctypes.c_int32(0)
        _check(fn(h, arr.ctypes.data, len(arr), *which, ctypes.byref(ph), ctypes.byref(skipped)))
    finally:
        lib().dh_scaffold_destroy(h)
    return (Pileups(None, None, None, _handle=ph), int(skipped.value)) + tuple(sc[1:] if resolve is not None else ())


def scaffold_spanning_pileups(las, contig_off, read_off, input_gaps=None, with_extensions=False, resolve=None, **opts):
    """The gap pile-ups of the scaffold graph (collectPileUps/pileups.d:173-208): returns (Pileups, number of
    pile-ups of other kinds).  with_extensions = False: the spanning reads only (dh_scaffold_spanning);
    True: every read alignment of the pile-up, i.e. also the extension entries mergeExtensionsWithGaps moved
    into the gap, as (read, LA, -1) / (read, -1, LA) triples (dh_scaffold_gap_pileups) -- what the reference's
    `dentist process` is handed."""
    sc = _scaffold(las, contig_off, read_off, input_gaps, opts, resolve)
    return _scaffold_piles(sc, resolve, lib().dh_scaffold_gap_pileups if with_extensions else lib().dh_scaffold_spanning)


def scaffold_all_pileups(las, contig_off, read_off, input_gaps=None, only="both", resolve=None, **opts):
    """Every pile-up of the scaffold graph the process stage can take (dh_scaffold_all_pileups): only = "spanning" (gap
    joins of any two contig ends), "extending" (extension joins) or "both".  Returns (Pileups with joins, skipped)."""
    which = {"spanning": 1, "extending": 2, "both": 3}[only]
    sc = _scaffold(las, contig_off, read_off, input_gaps, opts, resolve)
    return _scaffold_piles(sc, resolve, lib().dh_scaffold_all_pileups, which)
