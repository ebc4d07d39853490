"""The batched commands over local alignments -- chain, propagate-mask, validate-regions, the collect filters,
mask-repetitive-regions, the mask algebra, the gap analysis of check-results -- their host forms and their result classes."""
import ctypes

import numpy as np

from ._abi import (CONTIG_MAPPING_DTYPE, EXACT_HIT_DTYPE, GAP_SUMMARY_DTYPE, LA_DTYPE, REGION_DTYPE, REGION_REPORT_DTYPE,
                   ChainOpts, MaskOpts, RepeatOpts, _check, lib)
from ._align import DeviceTrace, _scoring, _take_la_set, set_fields
from ._marshal import Owner, addr, copy, mask_pair, optional_mask, view


# ---------------------------------------------------------------- chain
def default_chain_opts(tspace, **kw):
    o = ChainOpts()
    lib().dh_default_chain_opts(ctypes.byref(o), tspace)
    return set_fields(o, kw, hidden=("pad_",))


class Chains(Owner):
    """Result of Context.chain: numpy views of a library-owned dh_la_chains (alive as long as this object is).  Chain i is
    the output records off[i]:off[i + 1]; score: per chain; src_index / flags: per output record, the index of the record
    in the input and the flags it is written with; big_pairs: pairs that took the global-memory tier."""
    _destroy = "dh_la_chains_destroy"

    def __init__(self, h):
        L = lib()
        self._h = h
        n, nrec = L.dh_la_chains_count(h), L.dh_la_chains_records(h)
        self.off = view(L.dh_la_chains_off(h), n + 1, np.int64, self)
        self.score = view(L.dh_la_chains_score(h), n, np.int32, self)
        self.src_index = view(L.dh_la_chains_src_index(h), nrec, np.int64, self)
        self.flags = view(L.dh_la_chains_flags(h), nrec, np.uint32, self)
        self.big_pairs = int(L.dh_la_chains_big_pairs(h))

    def __len__(self):
        return len(self.score)

    def to_set(self, las, trace, tspace):
        """dh_la_chains_to_set: (records, trace) of the chained set in output order; las / trace: what was chained"""
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16) if trace is not None else None
        if tr is not None and len(arr) and int((arr["toff"] + arr["tlen"]).max()) > len(tr):
            raise ValueError("a record's trace lies behind the end of the trace array")
        h = ctypes.c_void_p()
        _check(lib().dh_la_chains_to_set(self._h, arr.ctypes.data, len(arr), tr.ctypes.data if tr is not None else None, tspace,
                                         ctypes.byref(h)))
        return _take_la_set(h)[:2]


def la_chain(ctx, las, tspace=None, **opts):
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    o = default_chain_opts(100 if tspace is None else tspace, **opts)
    h = ctypes.c_void_p()
    _check(lib().dh_la_chain(ctx._h, arr.ctypes.data, len(arr), ctypes.byref(o), ctypes.byref(h)))
    return Chains(h)


# ---------------------------------------------------------------- propagate-mask
def propagate_mask(las, trace, tspace, mask, ncontigs, read_off):
    """dh_propagate_mask: the contig mask (ptr, iv) carried to the reads (propagateMask.d:136-305).
    Returns (ptr int64[nreads + 1], iv int32[m, 2])."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    tr = np.ascontiguousarray(trace, dtype=np.uint16)
    mp, mi = mask_pair(mask)
    ro = np.ascontiguousarray(read_off, dtype=np.int64)
    L = lib()
    ptr = np.zeros(len(ro), dtype=np.int64)
    args = (addr(arr), len(arr), addr(tr), int(tspace), mp.ctypes.data, mi.ctypes.data, int(ncontigs), ro.ctypes.data,
            len(ro) - 1, ptr.ctypes.data)
    m = L.dh_propagate_mask(*args, None, 0)
    if m < 0:
        _check(int(m))
    iv = np.zeros((max(int(m), 1), 2), dtype=np.int32)
    L.dh_propagate_mask(*args, iv.ctypes.data, int(m))
    return ptr, iv[:int(m)]


class PropagatedMask:
    """Result of Context.propagate_mask: ptr int64[nreads + 1] and iv int32[m, 2], laid out as the module-level
    propagate_mask returns them (copies); raw: non-empty intervals before the union, hit: records with an intersecting mask
    interval, passes: destination ranges the call took."""

    def __init__(self, h, nreads):
        L = lib()
        try:
            self.ptr = copy(L.dh_mask_result_ptr(h), nreads + 1, np.int64)
            self.iv = copy(L.dh_mask_result_iv(h), (int(L.dh_mask_result_count(h)), 2), np.int32)
            self.raw, self.hit, self.passes = int(L.dh_mask_result_raw(h)), int(L.dh_mask_result_hit(h)), int(L.dh_mask_result_passes(h))
        finally:
            L.dh_mask_result_destroy(h)

    def __len__(self):
        return len(self.iv)


def la_propagate_mask(ctx, las, trace, tspace, mask, ncontigs, read_off):
    ro = np.ascontiguousarray(read_off, dtype=np.int64)
    short = "mask[0] needs ncontigs + 1 entries, read_off nreads + 1"
    if len(ro) < 1:
        raise ValueError(short)
    mp, mi = mask_pair(mask, int(ncontigs), short)
    h = ctypes.c_void_p()
    L = lib()
    if isinstance(trace, DeviceTrace):
        _check(L.dh_la_set_propagate_mask(ctx._h, trace._h, mp.ctypes.data, mi.ctypes.data, int(ncontigs), ro.ctypes.data, len(ro) - 1,
                                          ctypes.byref(h)))
    else:
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        tr = np.ascontiguousarray(trace, dtype=np.uint16)
        _check(L.dh_la_propagate_mask(ctx._h, addr(arr), len(arr), addr(tr), len(tr), int(tspace), mp.ctypes.data, mi.ctypes.data,
                                      int(ncontigs), ro.ctypes.data, len(ro) - 1, ctypes.byref(h)))
    return PropagatedMask(h, len(ro) - 1)


# ---------------------------------------------------------------- validate-regions
def _regions(regions):
    rg = np.zeros(len(regions), dtype=REGION_DTYPE)
    r = np.asarray(regions, dtype=np.int32).reshape(-1, 3)
    rg["contig"], rg["begin"], rg["end"] = r[:, 0], r[:, 1], r[:, 2]
    return rg


def validate_regions(las, contig_off, regions, min_coverage_reads, min_spanning_reads=3, region_context=1000,
                     weak_coverage_window=500):
    """dh_validate_regions (`dentist validate-regions`, validateRegions.d:325-512).  regions: (contig,
    begin, end) rows.  Returns (reports REGION_REPORT_DTYPE[nregions], weak (contig, begin, end) int32[m, 3])."""
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    rg = _regions(regions)
    rep = np.zeros(len(rg), dtype=REGION_REPORT_DTYPE)
    L = lib()
    args = (addr(arr), len(arr), co.ctypes.data, len(co) - 1, addr(rg), len(rg), int(region_context), int(weak_coverage_window),
            int(min_coverage_reads), int(min_spanning_reads), addr(rep))
    m = L.dh_validate_regions(*args, None, 0)
    if m < 0:
        _check(int(m))
    weak = np.zeros((max(int(m), 1), 3), dtype=np.int32)
    L.dh_validate_regions(*args, weak.ctypes.data, int(m))
    return rep, weak[:int(m)]


class ValidatedRegions:
    """Result of Context.validate_regions (copies): reports REGION_REPORT_DTYPE[nregions] and weak int32[m, 3] as the
    module-level validate_regions returns them; span_off int64[nregions + 1] and span_ids int32: the bread of the records that
    span a region, in ascending record index; mask = (ptr int64[ncontigs + 1], iv int32[k, 2]): the weak intervals of all
    regions merged per contig; pairs: (record, region) pairs that intersect, big_regions: regions that took the global-memory
    tier, groups: launch groups."""

    def __init__(self, h, ncontigs):
        L = lib()
        try:
            n = int(L.dh_region_result_count(h))
            self.reports = copy(L.dh_region_result_reports(h), n, REGION_REPORT_DTYPE)
            self.weak = copy(L.dh_region_result_weak(h), (int(L.dh_region_result_weak_count(h)), 3), np.int32)
            self.span_off = copy(L.dh_region_result_span_off(h), n + 1, np.int64)
            self.span_ids = copy(L.dh_region_result_span_ids(h), int(self.span_off[n]), np.int32)
            self.mask = (copy(L.dh_region_result_mask_ptr(h), ncontigs + 1, np.int64),
                         copy(L.dh_region_result_mask_iv(h), (int(L.dh_region_result_mask_count(h)), 2), np.int32))
            self.pairs, self.big_regions, self.groups = (int(L.dh_region_result_pairs(h)), int(L.dh_region_result_big_regions(h)),
                                                         int(L.dh_region_result_groups(h)))
        finally:
            L.dh_region_result_destroy(h)

    def __len__(self):
        return len(self.reports)


def la_validate_regions(ctx, las, contig_off, regions, min_coverage_reads, min_spanning_reads=3, region_context=1000,
                        weak_coverage_window=500):
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    if len(co) < 1:
        raise ValueError("contig_off needs ncontigs + 1 entries")
    rg = _regions(regions)
    h = ctypes.c_void_p()
    tail = (co.ctypes.data, len(co) - 1, addr(rg), len(rg), int(region_context), int(weak_coverage_window),
            int(min_coverage_reads), int(min_spanning_reads), ctypes.byref(h))
    if isinstance(las, ctypes.c_void_p):
        _check(lib().dh_la_set_validate_regions(ctx._h, las, *tail))
    else:
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        _check(lib().dh_la_validate_regions(ctx._h, addr(arr), len(arr), *tail))
    return ValidatedRegions(h, len(co) - 1)


# ---------------------------------------------------------------- the collect filters
def _filter_args(contig_off, read_off, opts, repeat_mask, checked):
    """The arguments dh_collect_filter and its device forms share, behind the records: (tail, dropped, used, keep-alive).
    checked: the device forms refuse empty offsets here, the host form leaves them to the library."""
    co, ro = np.ascontiguousarray(contig_off, dtype=np.int64), np.ascontiguousarray(read_off, dtype=np.int64)
    if checked and (len(co) < 1 or len(ro) < 1):
        raise ValueError("contig_off and read_off need n + 1 entries")
    dropped = np.zeros(6, dtype=np.int64)
    used = np.ones(len(ro) - 1, dtype=np.uint8)
    keep, rp, ri = optional_mask(repeat_mask)
    tail = (co.ctypes.data, len(co) - 1, ro.ctypes.data, len(ro) - 1, rp, ri, ctypes.byref(opts), dropped.ctypes.data,
            used.ctypes.data)
    return tail, dropped, used, (co, ro, keep)


def _own_records(las, inplace):
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    if not inplace or arr is not las or not arr.flags.writeable:
        arr = arr.copy()
    return arr


def collect_filter(las, contig_off, read_off, opts, repeat_mask=None, inplace=False):
    """The six filters of `dentist collect` (filter.d:122-356). Returns (las with DISABLED flags -- a
    copy unless inplace, dropped-per-stage int64[6], read_used uint8[nreads])."""
    arr = _own_records(las, inplace)
    tail, dropped, used, keep = _filter_args(contig_off, read_off, opts, repeat_mask, False)
    _check(lib().dh_collect_filter(arr.ctypes.data, len(arr), *tail))
    return arr, dropped, used


def la_collect_filter(ctx, las, contig_off, read_off, opts, repeat_mask=None, inplace=False):
    tail, dropped, used, keep = _filter_args(contig_off, read_off, opts, repeat_mask, True)
    L = lib()
    if isinstance(las, ctypes.c_void_p):
        _check(L.dh_la_set_collect_filter(ctx._h, las, *tail))
        return copy(L.dh_la_set_records(las), L.dh_la_set_count(las), LA_DTYPE), dropped, used
    arr = _own_records(las, inplace)
    _check(L.dh_la_collect_filter(ctx._h, addr(arr), len(arr), *tail))
    return arr, dropped, used


# ---------------------------------------------------------------- mask-repetitive-regions, mask algebra
def max_coverage_reads(read_coverage):
    """--max-coverage-reads derived from --read-coverage (commandline.d:1876-1889)."""
    return int(lib().dh_max_coverage_reads(float(read_coverage)))


def max_improper_coverage_reads(read_coverage):
    """--max-improper-coverage-reads derived from --read-coverage (commandline.d:1957-1970)."""
    return int(lib().dh_max_improper_coverage_reads(float(read_coverage)))


class RepeatMask:
    """Result of Context.repeat_mask (copies): mask, all, improper as (ptr int64[ncontigs + 1], iv int32[m, 2]); units and
    improper_units: the chains counted; tier_contigs[t]: contigs without events, of the wavefront, the LDS and the global
    tier; groups: launch groups."""

    def __init__(self, h, ncontigs):
        L = lib()
        try:
            for which in ("mask", "all", "improper"):
                m = int(getattr(L, "dh_repeat_result_%s_count" % which)(h))
                setattr(self, which, (copy(getattr(L, "dh_repeat_result_%s_ptr" % which)(h), ncontigs + 1, np.int64),
                                      copy(getattr(L, "dh_repeat_result_%s_iv" % which)(h), (m, 2), np.int32)))
            self.units, self.improper_units = int(L.dh_repeat_result_units(h)), int(L.dh_repeat_result_improper_units(h))
            self.tier_contigs = [int(L.dh_repeat_result_tier_contigs(h, t)) for t in range(4)]
            self.groups = int(L.dh_repeat_result_groups(h))
        finally:
            L.dh_repeat_result_destroy(h)


def la_repeat_mask(ctx, las, contig_off, read_off=None, lower=0, upper=4, improper=None, allowance=100):
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    ro = None if read_off is None else np.ascontiguousarray(read_off, dtype=np.int64)
    if len(co) < 1 or (ro is not None and len(ro) < 1):
        raise ValueError("contig_off and read_off need n + 1 entries")
    o = RepeatOpts(int(lower), int(upper), 0, 0, int(allowance), 0)
    if improper is not None:
        o.improper_lower, o.improper_upper, o.with_improper = int(improper[0]), int(improper[1]), 1
    h = ctypes.c_void_p()
    tail = (co.ctypes.data, len(co) - 1, ro.ctypes.data if ro is not None else None, len(ro) - 1 if ro is not None else 0,
            ctypes.byref(o), ctypes.byref(h))
    if isinstance(las, ctypes.c_void_p):
        _check(lib().dh_la_set_repeat_mask(ctx._h, las, *tail))
    else:
        arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
        _check(lib().dh_la_repeat_mask(ctx._h, addr(arr), len(arr), *tail))
    return RepeatMask(h, len(co) - 1)


class MaskSet:
    """Result of Context.combine_masks / tandem_mask (copies): ptr int64[ncontigs + 1], iv int32[m, 2]; events: keys written
    (twice the non-empty intervals given); sort_passes: radix passes run; groups: launch groups."""

    def __init__(self, h, ncontigs):
        L = lib()
        try:
            self.ptr = copy(L.dh_mask_set_ptr(h), ncontigs + 1, np.int64)
            self.iv = copy(L.dh_mask_set_iv(h), (int(L.dh_mask_set_count(h)), 2), np.int32)
            self.events, self.sort_passes, self.groups = (int(L.dh_mask_set_events(h)), int(L.dh_mask_set_sort_passes(h)),
                                                          int(L.dh_mask_set_groups(h)))
        finally:
            L.dh_mask_set_destroy(h)


def mask_combine(ctx, masks, contig_off, min_count=1, subtract=None, min_gap=0, min_interval=0):
    co = np.ascontiguousarray(contig_off, dtype=np.int64)
    if len(co) < 1:
        raise ValueError("contig_off needs n + 1 entries")

    def pair(m):
        ptr = np.ascontiguousarray(m[0], dtype=np.int64)
        if len(ptr) != len(co):
            raise ValueError("a mask's ptr needs ncontigs + 1 entries")
        iv = np.ascontiguousarray(m[1], dtype=np.int32).reshape(-1)
        return ptr, iv if len(iv) else np.zeros(2, dtype=np.int32)   # (never an empty array)
    keep = [pair(m) for m in masks]
    sub = pair(subtract) if subtract is not None else None
    ptrs = (ctypes.c_void_p * max(len(keep), 1))(*[k[0].ctypes.data for k in keep])
    ivs = (ctypes.c_void_p * max(len(keep), 1))(*[k[1].ctypes.data for k in keep])
    o = MaskOpts(int(min_count), int(min_gap), int(min_interval), 0)
    h = ctypes.c_void_p()
    _check(lib().dh_mask_combine(ctx._h, ptrs, ivs, len(keep), sub[0].ctypes.data if sub else None, sub[1].ctypes.data if sub else None,
                                 co.ctypes.data, len(co) - 1, ctypes.byref(o), ctypes.byref(h)))
    return MaskSet(h, len(co) - 1)


def la_tandem_mask(ctx, las, read_off, first_read=0, min_len=500):
    ro = np.ascontiguousarray(read_off, dtype=np.int64)
    if len(ro) < 1:
        raise ValueError("read_off needs n + 1 entries")
    arr = np.ascontiguousarray(las, dtype=LA_DTYPE)
    h = ctypes.c_void_p()
    _check(lib().dh_la_tandem_mask(ctx._h, addr(arr), len(arr), ro.ctypes.data, len(ro) - 1, int(first_read), int(min_len),
                                   ctypes.byref(h)))
    return MaskSet(h, len(ro) - 1)


# ---------------------------------------------------------------- check-results
class GapReport:
    """Result of Context.check_gaps, copied out of the library: summaries (GAP_SUMMARY_DTYPE, one per gap), identity (float64: matches
    over kept columns, NaN at zero columns), the uncropped ops of gap i at ops[op_off[i]:op_off[i + 1]] (empty unless align_status is
    1), score per gap, and the counters aligned (pairs handed to the aligner) and groups (its launch groups)."""

    def __init__(self, h):
        L = lib()
        try:
            n = int(L.dh_gap_report_count(h))
            self.summaries = copy(L.dh_gap_report_summaries(h), n, GAP_SUMMARY_DTYPE)
            p = L.dh_gap_report_paths(h)
            self.op_off = copy(L.dh_edit_paths_op_off(p), n + 1, np.int64)
            self.ops = copy(L.dh_edit_paths_ops(p), int(self.op_off[-1]), np.uint8)
            self.score = copy(L.dh_edit_paths_score(p), n, np.int32)
            self.aligned, self.groups = int(L.dh_gap_report_aligned(h)), int(L.dh_gap_report_groups(h))
        finally:
            L.dh_gap_report_destroy(h)
        cols = (self.summaries["col_end"] - self.summaries["col_begin"]).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.identity = np.where(cols > 0, self.summaries["matches"] / cols, np.nan)

    def __len__(self):
        return len(self.summaries)

    def ops_of(self, i):
        return self.ops[self.op_off[i]:self.op_off[i + 1]]


def check_gaps(ctx, true_db, result_db, mapped, maps, result_gap, dust=None, crop=0, scoring=None, first_contig=1, count=None):
    mp = np.ascontiguousarray(mapped, dtype=np.int32).reshape(-1, 3)
    ma = np.ascontiguousarray(maps, dtype=CONTIG_MAPPING_DTYPE)
    rg = np.ascontiguousarray(np.concatenate([np.asarray(result_gap, dtype=np.int32).reshape(-1), [0]]), dtype=np.int32)
    n_res = lib().dh_db_nreads(result_db._h)
    if len(rg) - 1 != n_res:
        raise ValueError("result_gap needs one entry per result contig")
    dp = di = None
    if dust is not None:
        dp, di = mask_pair(dust, lib().dh_db_nreads(true_db._h), "dust[0] needs one entry per true contig and one more", "dust mask")
    sc = _scoring(scoring)
    if count is None:
        count = max(len(mp) - int(first_contig) + 1, 0)
    h = ctypes.c_void_p()
    _check(lib().dh_check_gaps(ctx._h, true_db._h, result_db._h, addr(mp), len(mp), addr(ma), len(ma), rg.ctypes.data,
                               dp.ctypes.data if dp is not None else None, di.ctypes.data if di is not None else None, int(crop),
                               sc.ctypes.data if sc is not None else None, int(first_contig), int(count), ctypes.byref(h)))
    return GapReport(h)


def contig_mappings(ctx, ref_seqs, result_seqs, crop_alignment=0, crop_ambiguous=0):
    """findReferenceContigs / findPerfectAlignmentsChunk of `dentist check-results` (commands/checkResults.d:399-565) over
    Context.exact_locate: the input contigs ref_seqs cropped by crop_alignment on both sides are searched in result_seqs on both
    strands, every hit is a mapping; an input contig is a duplicate when, cropped by crop_ambiguous, it occurs in another input
    contig.  A contig that the crop leaves empty is not searched.  Returns CONTIG_MAPPING_DTYPE records sorted by input contig."""
    def cropped(crop):
        ids = [i for i, s in enumerate(ref_seqs) if len(s) > 2 * crop]
        return ids, [np.asarray(ref_seqs[i], dtype=np.uint8)[crop:len(ref_seqs[i]) - crop] for i in ids]
    ids, qs = cropped(int(crop_ambiguous))
    dup = set()
    if qs:
        for h in ctx.exact_locate(ref_seqs, qs, True):
            if int(h["ref"]) != ids[int(h["query"])]:
                dup.add(ids[int(h["query"])])
    ids, qs = cropped(int(crop_alignment))
    hits = ctx.exact_locate(result_seqs, qs, True) if qs else np.zeros(0, EXACT_HIT_DTYPE)
    out = np.zeros(len(hits), dtype=CONTIG_MAPPING_DTYPE)
    for k, h in enumerate(hits):
        q = ids[int(h["query"])]
        out[k] = (int(h["ref"]) + 1, int(h["begin"]), int(h["end"]), len(result_seqs[int(h["ref"])]), q + 1, int(q in dup), int(h["complement"]), 0.0)
    return out[np.argsort(out["query_contig"], kind="stable")]
