"""The sharded path: the communicator and the host work of one rank between its collectives."""
import ctypes

import numpy as np

from ._abi import INSERTION_DTYPE, LA_DTYPE, _check, lib
from ._marshal import Owner, addr, copy, view
from ._process import Cropped, Pileups, _take_insertions, input_gaps_array, scaffold_opts


def _blobs(blobs):
    """Byte blobs as the library takes them: (the arrays, their addresses, their sizes)"""
    bl = [np.ascontiguousarray(b, dtype=np.uint8) for b in blobs]
    return bl, (ctypes.c_void_p * len(bl))(*[b.ctypes.data for b in bl]), (ctypes.c_int64 * len(bl))(*[len(b) for b in bl])


def _take_blob(out, nbytes):
    """numpy copy of a malloc'd blob of the library, which is released"""
    b = copy(out, nbytes, np.uint8)
    lib().dh_shard_free(out)
    return b


def shard_pack_candidates(cands, las, read_shift=0):
    """dh_shard_pack_candidates: this rank's candidate entries as the blob of the candidate all-gather."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    out, nb = ctypes.c_void_p(), ctypes.c_int64(0)
    _check(lib().dh_shard_pack_candidates(cands._h, arr.ctypes.data, len(arr), read_shift, ctypes.byref(out), ctypes.byref(nb)))
    return _take_blob(out, nb.value)


def shard_read_joins(las, contig_off, read_off, read_first=0):
    """dh_shard_read_joins: the raw scaffold joins of this rank's reads (global read ids in las["bread"], read_off =
    offsets of the rank's reads [read_first, read_first + len(read_off) - 1)) as the blob of the join all-gather."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    co, ro = np.ascontiguousarray(contig_off, dtype=np.int64), np.ascontiguousarray(read_off, dtype=np.int64)
    out, nb = ctypes.c_void_p(), ctypes.c_int64(0)
    _check(lib().dh_shard_read_joins(arr.ctypes.data, len(arr), co.ctypes.data, len(co) - 1, ro.ctypes.data, int(read_first),
                                     len(ro) - 1, ctypes.byref(out), ctypes.byref(nb)))
    return _take_blob(out, nb.value)


class ShardPlan(Owner):
    """dh_shard_plan: the pile-ups every rank derives from the gathered candidates (or, graph = (ncontigs, input_gaps,
    scaffold options): from the gathered scaffold joins), and who processes them."""
    _destroy = "dh_shard_plan_destroy"

    def __init__(self, blobs, opts, graph=None):
        L = lib()
        self._blobs, ptrs, sizes = _blobs(blobs)
        n = len(self._blobs)
        h = ctypes.c_void_p()
        if graph is not None:
            ncontigs, input_gaps, kw = graph
            so = scaffold_opts(kw or {})
            ig = input_gaps_array(input_gaps)
            _check(L.dh_shard_graph_plan_create(ptrs, sizes, n, int(ncontigs), addr(ig), len(ig), ctypes.byref(so), ctypes.byref(opts),
                                                ctypes.byref(h)))
        else:
            _check(L.dh_shard_plan_create(ptrs, sizes, n, ctypes.byref(opts), ctypes.byref(h)))
        self._h = h
        # a view of the plan's records (kept alive by this object)
        self.las = view(L.dh_shard_plan_las(h), L.dh_shard_plan_nlas(h), LA_DTYPE, None)
        self.piles = Pileups(None, None, None, _handle=ctypes.c_void_p(L.dh_shard_plan_pileups(h)), _keep=self)
        self.owner = copy(L.dh_shard_plan_owner(h), len(self.piles), np.int32)

    def close(self):
        if getattr(self, "_h", None):
            self.piles._h = None
            self.las = None
        super().close()


class Comm(Owner):
    """dh_comm: the communicator of the sharded path behind the C ABI -- RCCL between processes (Comm.create) or the
    in-process hub between host threads (Comm.local)."""
    _destroy = "dh_comm_destroy"

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * 128)()
        _check(lib().dh_comm_unique_id(buf))
        return bytes(buf)

    @staticmethod
    def create(ctx, rank, world, uid):
        h = ctypes.c_void_p()
        _check(lib().dh_comm_create(uid, rank, world, ctx._h, ctypes.byref(h)))
        return Comm(h)

    @staticmethod
    def local(world, ctxs=None):
        hs = (ctypes.c_void_p * world)()
        cp = (ctypes.c_void_p * world)(*[c._h for c in ctxs]) if ctxs is not None else None
        _check(lib().dh_comm_create_local(world, cp, hs))
        return [Comm(ctypes.c_void_p(hs[r])) for r in range(world)]

    @property
    def world(self):
        return int(lib().dh_comm_world(self._h))

    def _take(self, out, sizes):
        whole = _take_blob(out, int(sum(sizes)))
        parts, at = [], 0
        for n in sizes:
            parts.append(whole[at:at + int(n)].copy())
            at += int(n)
        return parts

    def all_gather(self, payload):
        p = np.ascontiguousarray(payload, dtype=np.uint8)
        sizes = (ctypes.c_int64 * self.world)()
        out = ctypes.c_void_p()
        _check(lib().dh_comm_all_gather(self._h, addr(p), len(p), ctypes.byref(out), sizes))
        return self._take(out, list(sizes))

    def all_to_all(self, per_dest):
        W = self.world
        bl = [np.ascontiguousarray(x, dtype=np.uint8) for x in per_dest]
        ptrs = (ctypes.c_void_p * W)(*[addr(b) for b in bl])
        ss = (ctypes.c_int64 * W)(*[len(b) for b in bl])
        rs = (ctypes.c_int64 * W)()
        out = ctypes.c_void_p()
        _check(lib().dh_comm_all_to_all(self._h, ptrs, ss, ctypes.byref(out), rs))
        return self._take(out, list(rs))


def shard_run_prepare(comm, contigs_db, reads_db, read_first, contig_off, las, trace, opts, cands=None, graph=None):
    """Everything of shard_run that can fail BEFORE the C call -- array conversion, option names, missing handles -- done
    up front; returns the closure that makes the call.  dentist_amd.parallel lets the ranks agree that all of them got this
    far before any of them enters dh_shard_run's first exchange."""
    L = lib()
    for what, h in (("communicator", comm), ("contigs DB", contigs_db), ("reads DB", reads_db)):
        if h is None or not getattr(h, "_h", None):
            raise ValueError(f"shard_run: no {what}")
    if cands is None and graph is None:
        raise ValueError("shard_run: neither candidates nor graph options")
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    if co.ndim != 1 or len(co) < 1:
        raise ValueError("shard_run: contig_off must hold at least one offset")
    ro = ig = so = None
    if cands is None:
        g = dict(graph or {})
        ro = np.ascontiguousarray(g.pop("read_off"), dtype=np.int64)
        ig = input_gaps_array(g.pop("input_gaps", None))
        g.setdefault("min_spanning_reads", opts.min_reads)
        so = scaffold_opts(g)
    elif not getattr(cands, "_h", None):
        raise ValueError("shard_run: the candidates have no handle")

    def call():
        h = ctypes.c_void_p()
        info = (ctypes.c_int64 * 4)()
        _check(L.dh_shard_run(comm._h, contigs_db._h, reads_db._h, read_first, co.ctypes.data, len(co) - 1, arr.ctypes.data, len(arr),
                              tr.ctypes.data, ctypes.byref(opts), cands._h if cands is not None else None,
                              ro.ctypes.data if ro is not None else None, addr(ig), len(ig) if ig is not None else 0,
                              ctypes.byref(so) if so is not None else None, ctypes.byref(h), info))
        rec, bases = _take_insertions(h, None, False)
        return rec, bases, {"piles": int(info[0]), "owned": int(info[1]), "entries": int(info[2]), "cropped_bytes_sent": int(info[3])}
    return call


def shard_run(comm, contigs_db, reads_db, read_first, contig_off, las, trace, opts, cands=None, graph=None):
    """dh_shard_run: `collect` + `process` of one rank's share with its three exchanges behind the C ABI.  graph =
    dict(read_off=..., input_gaps=..., scaffold options) selects the scaffold-graph collector, cands the spanning-read
    one.  Returns (records of all ranks by gap, consensus bases, info)."""
    return shard_run_prepare(comm, contigs_db, reads_db, read_first, contig_off, las, trace, opts, cands=cands, graph=graph)()


class _Block(Owner):
    """The one malloc'd block behind all the blobs of shard_pack_cropped: released with the last view"""
    _destroy = "dh_shard_free"


def shard_pack_cropped(crop, owner, world):
    """dh_shard_pack_cropped: the reads this rank cropped, one blob per owner rank."""
    ow = np.ascontiguousarray(owner, dtype=np.int32)
    ptrs = (ctypes.c_void_p * world)()
    sizes = (ctypes.c_int64 * world)()
    _check(lib().dh_shard_pack_cropped(crop._h, ow.ctypes.data, world, ptrs, sizes))
    total = sum(int(sizes[r]) for r in range(world))
    whole = view(ptrs[0], max(total, 1), np.uint8, _Block(ptrs[0]))
    out, at = [], 0
    for r in range(world):   # views, no copy: the collective (or torch.from_numpy) reads them in place
        out.append(whole[at:at + int(sizes[r])])
        at += int(sizes[r])
    return out


def shard_unpack_cropped(blobs, rec, owner, rank):
    """dh_shard_unpack_cropped: what an owner received -> Cropped for dh_process_cropped."""
    bl, ptrs, sizes = _blobs(blobs)
    r = np.ascontiguousarray(rec, dtype=INSERTION_DTYPE)
    ow = np.ascontiguousarray(owner, dtype=np.int32)
    h = ctypes.c_void_p()
    _check(lib().dh_shard_unpack_cropped(ptrs, sizes, len(bl), r.ctypes.data, len(r), ow.ctypes.data, rank, ctypes.byref(h)))
    return Cropped(h)
