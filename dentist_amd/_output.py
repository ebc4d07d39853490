"""`dentist output`: the gap-closed assembly as FASTA, AGP and BED, on the host and with the text formatted on the device."""
import ctypes

import numpy as np

from ._abi import INSERTION_DTYPE, OutputFilter, OutputOpts, _check, lib
from ._marshal import addr, copy

JOIN_POLICIES = {"scaffoldGaps": 0, "scaffolds": 1, "contigs": 2}


def _output_opts(line_width, highlight, join_policy, agp_dazzler, agp_skip_read_ids, only, min_extension_length, tool, input_assembly):
    o = OutputOpts()
    lib().dh_default_output_opts(ctypes.byref(o))
    o.line_width, o.highlight, o.join_policy = line_width, int(bool(highlight)), JOIN_POLICIES[join_policy]
    o.agp_dazzler, o.agp_skip_read_ids = int(bool(agp_dazzler)), int(bool(agp_skip_read_ids))
    o.only, o.min_extension_length = {"spanning": 1, "extending": 2, "both": 3}[only], int(min_extension_length)
    if tool is not None:
        o.tool = tool.encode()
    if input_assembly is not None:
        o.input_assembly = input_assembly.encode()
    return o


def _strings(names):
    """A list of str as the char ** the library reads; None stays None"""
    return (ctypes.c_char_p * len(names))(*[x.encode() for x in names]) if names is not None else None


def _scaffolding(scaffold_of, gap_len):
    return np.ascontiguousarray(scaffold_of, dtype=np.int32), np.ascontiguousarray(gap_len, dtype=np.int32) if gap_len is not None else None


def output_db(ctx, fasta_path, contigs, scaffold_of, headers, gap_len, insertions_db, bed_path=None, agp_path=None,
              join_policy="scaffoldGaps", agp_dazzler=False, agp_skip_read_ids=False, read_names=None, line_width=50,
              highlight=True, tool=None, input_assembly=None, only="spanning", min_extension_length=100,
              max_insertion_error=None, skip_gaps=None):
    L = lib()
    vp = ctypes.c_void_p
    co = np.ascontiguousarray(contigs.off, dtype=np.int64)
    h = vp()
    _check(L.dh_insertions_from_db(insertions_db.encode(), co.ctypes.data, len(co) - 1, ctypes.byref(h)))
    try:
        o = _output_opts(line_width, highlight, join_policy, agp_dazzler, agp_skip_read_ids, only, min_extension_length, tool, input_assembly)
        so, gl = _scaffolding(scaffold_of, gap_len)
        hs, rn = _strings(headers), _strings(read_names)
        flt = None
        if max_insertion_error is not None or skip_gaps:
            sg = np.ascontiguousarray(skip_gaps if skip_gaps else np.zeros((0, 2)), dtype=np.int32).reshape(-1, 2)
            flt = OutputFilter(int(round(max_insertion_error * 1e6)) if max_insertion_error is not None else 0, len(sg), addr(sg))
        dropped = ctypes.c_int32(0)
        _check(L.dh_output_db(ctx._h, contigs._h, fasta_path.encode() if fasta_path else None, bed_path.encode() if bed_path else None,
                              agp_path.encode() if agp_path else None, so.ctypes.data, ctypes.cast(hs, vp),
                              gl.ctypes.data if gl is not None else None, h, len(read_names) if read_names is not None else -1,
                              ctypes.cast(rn, vp) if rn is not None else None, ctypes.byref(o),
                              ctypes.byref(flt) if flt is not None else None, ctypes.byref(dropped)))
    finally:
        L.dh_insertions_destroy(h)
    return int(dropped.value)


def output_stats(ctx):
    ms = (ctypes.c_double * 4)()
    _check(lib().dh_get_output_stats(ctx._h, ms))
    return dict(kernel=ms[0], copy=ms[1], fwrite=ms[2], total=ms[3])


def output_plan(contig_off, scaffold_of, headers, gap_len, rec, bases_len, join_policy="scaffoldGaps", line_width=50, highlight=True,
                only="spanning", min_extension_length=100):
    """dh_output_plan: the plan dh_output_db formats on the device, as a dict of arrays (rec_off, hdr_off, seg_first, seg_base,
    seg_src, seg_flags, hdr) plus width (host only; the layout is stated in csrc/dh_outfmt.h)."""
    L = lib()
    vp = ctypes.c_void_p
    o = _output_opts(line_width, highlight, join_policy, False, False, only, min_extension_length, None, None)
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    so, gl = _scaffolding(scaffold_of, gap_len)
    r = np.ascontiguousarray(rec, dtype=INSERTION_DTYPE)
    hs = _strings(headers)
    h = vp()
    _check(L.dh_output_plan(co.ctypes.data, len(co) - 1, so.ctypes.data, ctypes.cast(hs, vp), gl.ctypes.data if gl is not None else None,
                            addr(r), len(r), int(bases_len), ctypes.byref(o), ctypes.byref(h)))
    out = {"width": int(line_width)}
    for which, (name, dt) in enumerate((("rec_off", np.int64), ("hdr_off", np.int64), ("seg_first", np.int64), ("seg_base", np.int64),
                                        ("seg_src", np.int64), ("seg_flags", np.uint32), ("hdr", np.uint8))):
        n = ctypes.c_int64(0)
        p = L.dh_out_plan_array(h, which, ctypes.byref(n))
        out[name] = copy(p, n.value, dt)
    L.dh_out_plan_destroy(h)
    return out


def output_assembly(fasta_path, contigs, scaffold_of, headers, gap_len, rec, bases, read_ids=None, bed_path=None,
                    agp_path=None, join_policy="scaffoldGaps", agp_dazzler=False, agp_skip_read_ids=False, read_names=None,
                    line_width=50, highlight=True, tool=None, input_assembly=None, only="spanning", min_extension_length=100):
    """`dentist output` (host only): assembly graph with the join policy, fixCropping, FASTA, AGP and closed-gaps
    BED (dh_output_assembly).  read_ids = (ids, off) from process_pileups(read_ids=True).  Returns the number of
    insertions the join policy dropped."""
    o = _output_opts(line_width, highlight, join_policy, agp_dazzler, agp_skip_read_ids, only, min_extension_length, tool, input_assembly)
    cb = np.ascontiguousarray(contigs.bases, dtype=np.uint8)
    co = np.ascontiguousarray(contigs.off, dtype=np.int64)
    so, gl = _scaffolding(scaffold_of, gap_len)
    r = np.ascontiguousarray(rec, dtype=INSERTION_DTYPE)
    b = np.ascontiguousarray(bases, dtype=np.uint8)
    hs, rn = _strings(headers), _strings(read_names)
    ids = off = None
    if read_ids is not None:
        ids = np.ascontiguousarray(read_ids[0], dtype=np.int32)
        off = np.ascontiguousarray(read_ids[1], dtype=np.int32)
    dropped = ctypes.c_int32(0)
    vp = ctypes.c_void_p
    _check(lib().dh_output_assembly(fasta_path.encode(), bed_path.encode() if bed_path else None,
                                    agp_path.encode() if agp_path else None, cb.ctypes.data, co.ctypes.data, len(co) - 1,
                                    so.ctypes.data, ctypes.cast(hs, vp), gl.ctypes.data if gl is not None else None,
                                    r.ctypes.data, len(r), addr(b), ids.ctypes.data if ids is not None else None,
                                    off.ctypes.data if off is not None else None, len(read_names) if read_names is not None else -1,
                                    ctypes.cast(rn, vp) if rn is not None else None,
                                    ctypes.byref(o), ctypes.byref(dropped)))
    return int(dropped.value)


def output_fasta(fasta_path, contigs, scaffold_of, headers, gap_len, rec, bases, bed_path=None, line_width=50,
                 highlight=True):
    """`dentist output` for linear scaffolds (host only): contigs = SeqDb-like (.bases, .off),
    scaffold_of[c] = input scaffold of contig c, headers[s] = its FASTA header without '>',
    gap_len[c] = gap after contig c; rec / bases = result of process_pileups."""
    cb = np.ascontiguousarray(contigs.bases, dtype=np.uint8)
    co = np.ascontiguousarray(contigs.off, dtype=np.int64)
    so, gl = _scaffolding(scaffold_of, gap_len)
    r = np.ascontiguousarray(rec, dtype=INSERTION_DTYPE)
    b = np.ascontiguousarray(bases, dtype=np.uint8)
    _check(lib().dh_output_fasta(fasta_path.encode(), bed_path.encode() if bed_path else None, cb.ctypes.data,
                                 co.ctypes.data, len(co) - 1, so.ctypes.data, _strings(headers),
                                 gl.ctypes.data if gl is not None else None, r.ctypes.data, len(r),
                                 addr(b), line_width, int(bool(highlight))))
