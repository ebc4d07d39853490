"""Context: one class with a method per device command; each method is its documentation and a call into the module of its role."""
import ctypes

from . import _align, _lacmd, _output, _process
from ._abi import _check, lib
from ._marshal import Owner


class Context(Owner):
    """One per process / GPU. ``stream``: a raw hipStream_t (e.g. torch.cuda.current_stream().cuda_stream)."""
    _destroy = "dh_ctx_destroy"

    def __init__(self, device=0, stream=None):
        h = ctypes.c_void_p()
        _check(lib().dh_ctx_create(device, ctypes.c_void_p(stream) if stream else None, ctypes.byref(h)))
        self._h = h
        self._dbs = []

    def close(self):
        if getattr(self, "_h", None):
            for ref in self._dbs:  # device DBs must go before their context
                d = ref()
                if d is not None:
                    d.close()
            self._dbs = []
        super().close()

    def sync(self):
        _check(lib().dh_ctx_sync(self._h))

    def db(self, seqdb):
        return _align.Db(self, seqdb)

    def align_stats(self):
        return _align.align_stats(self)

    def release_scratch(self):
        """dh_ctx_release_scratch: hand the context's grow-only device scratch back (the next call allocates again)."""
        _check(lib().dh_ctx_release_scratch(self._h))

    def mjoin_counts(self, reset=False):
        """(chunks seeded by the partitioned k-mer join, chunks redone by the directory lookups) of this context's mapping calls."""
        return _align.counts(self, "mjoin", 2, reset)

    def join_counts(self, reset=False):
        """(k_join launches, reruns among them, hits of the last join, capacity of its first attempt) of this context's
        pile-up joins; after process_pileups the last two are sums over the concurrent parts of that call."""
        return _align.counts(self, "join", 4, reset)

    def tjoin_counts(self, reset=False):
        """(calls seeded by the per-group k-mer table on chip, grouped calls A != B that kept the directory, hits of the last
        call, reruns of the hit buffer) of this context; after process_pileups the sums over the concurrent parts."""
        return _align.counts(self, "tjoin", 4, reset)

    def seed_tier_counts(self, reset=False):
        """(chunks whose first seed tier was the 256-thread middle tier, reads redone behind it by the 512-thread tiers) of
        this context; after process_pileups the sums over the concurrent parts."""
        return _align.counts(self, "seed_tier", 2, reset)

    def seed_band_counts(self, reset=False):
        """(reads whose band heads went to the table in LDS, reads that kept the slab of global scratch) of the segment-fed
        8192- and 16384-entry seed tiers on this context's device since the last reset."""
        return _align.counts(self, "seed_band", 2, reset)

    def cum_stats(self, reset=False):
        return _align.cum_stats(self, reset)

    def remap_skipping_reads(self, contigs, reads, contig_ids, read_ids, opts, allowance):
        """dh_remap_skipping_reads: the re-mapping call of `resolveBubbles` (pileups.d:1316-1385)."""
        return _align.remap_skipping_reads(self, contigs, reads, contig_ids, read_ids, opts, allowance)

    def align_db_transposed(self, A, B, opts, select_best=False):
        """dh_align_db_transposed (`damapper -C`): ((records, trace), (transposed records, trace)), LAsort order."""
        return _align.align_db_transposed(self, A, B, opts, select_best)

    def align_db(self, A, B, opts, select_best=False):
        """Every read of B against A on the GPU. Returns (records, trace u16) in LAsort order."""
        return _align.align_db(self, A, B, opts, select_best)

    def seed_candidates(self, A, B, opts):
        """dh_seed_candidates: the seed stage of align_db alone.  Returns (cand[nitems, max_cand] SEED_CAND_DTYPE, ncand[nitems],
        nhits[nitems]), item = 2 * read + strand; row i holds the ncand[i] candidates of item i in the order the extension
        takes them (what lies behind them is not defined)."""
        return _align.seed_candidates(self, A, B, opts)

    def extend_candidates(self, A, B, opts, cand, ncand, sort=False, transposed=False):
        """dh_extend_candidates: the extension stage of align_db alone on the caller's candidates (cand[nitems, max_cand]
        SEED_CAND_DTYPE, ncand[nitems], item = 2 * read + strand), taken as they stand.  Returns (records, trace u16) in item
        and slot order (sort=True: LAsort order); transposed=True: ((records, trace), (transposed records, trace))."""
        return _align.extend_candidates(self, A, B, opts, cand, ncand, sort, transposed)

    def map_reads(self, A, B, opts, popts, first=0, count=None, repeat_mask=None, sorted=True, candidates=False,
                  trace_on_device=False):
        """dh_map_reads: the mapping pass (chain flags as with select_best) with the six `collect` filters
        applied chunk by chunk on the host while the device maps on.  Returns (las, trace, dropped[6]);
        with sorted=False, candidates=True also the spanning-read candidates (Pileups, not yet cut).
        trace_on_device=True: `trace` is a DeviceTrace -- the values stay in HBM (process_pileups takes it as it is and
        fetches what the cropper reads; .numpy() downloads everything)."""
        return _process.map_reads(self, A, B, opts, popts, first, count, repeat_mask, sorted, candidates, trace_on_device)

    def edit_paths(self, A, B, las, trace=None, tspace=None, first=0, count=None):
        """dh_la_edit_paths: the base-level alignment of records [first, first + count) from their trace points, as an
        EditPaths.  `las` may be a raw handle of align_db_block(..., raw=True) (dh_la_set_edit_paths; trace and tspace are
        the set's own)."""
        return _align.la_edit_paths(self, A, B, las, trace, tspace, first, count)

    def chain_paths(self, A, B, las, trace=None, tspace=None, chain_off=None):
        """dh_la_chain_paths: the base-level alignment of whole chains (the chain padder).  chain_off: nchains + 1 record
        offsets (what Chains gives together with chains_to_set), None = chains by flags (a record without NEXT starts one).
        `las` may be a raw handle of align_db_block(..., raw=True) (dh_la_set_chain_paths, by flags).  Returns (op_off, ops,
        score, status, fillers): status[i] is CP_OK, CP_FAKED or CP_NESTED (no ops, score -1), fillers the number of
        fillers the global-alignment kernel aligned."""
        return _align.la_chain_paths(self, A, B, las, trace, tspace, chain_off)

    def nw_batch(self, refs, qrys, free_shift=False):
        """dh_nw_batch: the global alignment (findAlignment, indel penalty 1) of refs[i] against qrys[i] for every i; the
        sequences are strings or base-code arrays, compared byte by byte.  Returns (EditPaths, status): ops and score
        per pair as for Context.edit_paths (no tiles); status[i] is NW_OK or NW_BAND_EXCEEDED (score -1, no ops)."""
        return self.nw_batch_raw(*_align.concat_pairs(refs, qrys), free_shift)

    def nw_batch_raw(self, ref, ref_off, qry, qry_off, free_shift=False):
        """nw_batch on concatenated sequences: pair i is ref[ref_off[i]:ref_off[i + 1]] against qry[qry_off[i]:qry_off[i + 1]]."""
        return _align.nw_batch_raw(self, ref, ref_off, qry, qry_off, free_shift)

    def nw_affine_batch(self, refs, qrys, scoring=None):
        """dh_nw_affine_batch: the global alignment of refs[i] against qrys[i] with affine gap costs (what EMBOSS stretcher
        computes).  scoring: (match, mismatch, gap_open, gap_extend), None = (5, -4, 16, 4); a gap of k bases scores
        -(gap_open + k * gap_extend).  Returns (EditPaths, status) as nw_batch does; score[i] is the alignment score."""
        return self.nw_affine_batch_raw(*_align.concat_pairs(refs, qrys), scoring)

    def nw_affine_batch_raw(self, ref, ref_off, qry, qry_off, scoring=None):
        """nw_affine_batch on concatenated sequences, laid out as for nw_batch_raw."""
        return _align.nw_affine_batch_raw(self, ref, ref_off, qry, qry_off, scoring)

    def exact_locate(self, refs, queries, both_strands=True):
        """dh_exact_locate: every exact occurrence of queries[j] (and, with both_strands, of its reverse complement) in the
        records refs[i]; sequences are base-code arrays (0..3).  Returns a structured array of EXACT_HIT_DTYPE ordered by
        query, then strand (forward first), then (ref, begin); begin / end are 0-based, right-open, relative to the record."""
        return self.exact_locate_raw(*_align._concat_seqs(refs), *_align._concat_seqs(queries), both_strands)

    def exact_locate_raw(self, ref, ref_off, qry, qry_off, both_strands=True):
        """exact_locate on concatenated sequences: record i is ref[ref_off[i]:ref_off[i + 1]], query j likewise."""
        return _align.exact_locate_raw(self, ref, ref_off, qry, qry_off, both_strands)

    def chain(self, las, tspace=None, **opts):
        """dh_la_chain: chainLocalAlignments on records sorted by (aread, bread).  tspace: the trace spacing, the default of
        min_score (100 when omitted); opts: fields of ChainOpts.  Returns a Chains object."""
        return _lacmd.la_chain(self, las, tspace, **opts)

    def propagate_mask(self, las, trace, tspace, mask, ncontigs, read_off):
        """dh_la_propagate_mask: the contig mask (ptr, iv) carried to the reads on the device (propagateMask.d:136-305); the
        arguments of the module-level propagate_mask.  Returns a PropagatedMask.  A DeviceTrace as `trace` (map_reads with
        trace_on_device=True) takes the records, trace values and tspace of its result set (dh_la_set_propagate_mask): the
        values are used where they are."""
        return _lacmd.la_propagate_mask(self, las, trace, tspace, mask, ncontigs, read_off)

    def validate_regions(self, las, contig_off, regions, min_coverage_reads, min_spanning_reads=3, region_context=1000,
                         weak_coverage_window=500):
        """dh_la_validate_regions: `dentist validate-regions` (validateRegions.d:141-512) on the device; the arguments of the
        module-level validate_regions.  Returns a ValidatedRegions.  `las` may be a raw handle of align_db_block(..., raw=True)
        (dh_la_set_validate_regions): the records of the set are taken, the handle stays the caller's."""
        return _lacmd.la_validate_regions(self, las, contig_off, regions, min_coverage_reads, min_spanning_reads, region_context,
                                          weak_coverage_window)

    def collect_filter(self, las, contig_off, read_off, opts, repeat_mask=None, inplace=False):
        """dh_la_collect_filter: the six filters of `dentist collect` (filter.d:122-356) on the device; arguments and result of
        the module-level collect_filter (the mask's intervals sorted and disjoint per contig).  `las` may be a raw handle of
        align_db_block(..., raw=True) (dh_la_set_collect_filter): the flags are written into the set's records, a copy of which
        is returned; the handle stays the caller's."""
        return _lacmd.la_collect_filter(self, las, contig_off, read_off, opts, repeat_mask, inplace)

    def repeat_mask(self, las, contig_off, read_off=None, lower=0, upper=4, improper=None, allowance=100):
        """dh_la_repeat_mask: `dentist mask-repetitive-regions` (maskRepetitiveRegions.d:129-430) on the device, from records
        sorted by aread and the lengths to intervals.  (lower, upper): the bounds of the assessor over all chains; improper:
        None, or the (lower, upper) of the assessor over the improper chains (needs read_off).  Returns a RepeatMask.  `las`
        may be a raw handle of align_db_block(..., raw=True) (dh_la_set_repeat_mask): the handle stays the caller's."""
        return _lacmd.la_repeat_mask(self, las, contig_off, read_off, lower, upper, improper, allowance)

    def combine_masks(self, masks, contig_off, min_count=1, subtract=None, min_gap=0, min_interval=0):
        """dh_mask_combine: `dentist merge-masks` / `filter-mask` and the ReferenceRegion operators on the device.  masks: a list
        of (ptr int64[ncontigs + 1], iv (begin, end) pairs), intervals in any order; a base is kept iff at least min_count masks
        have it (1: union, len(masks): intersection) and `subtract` (one such pair, or None) does not; then gaps up to min_gap
        are closed, then runs shorter than min_interval dropped.  Returns a MaskSet."""
        return _lacmd.mask_combine(self, masks, contig_off, min_count, subtract, min_gap, min_interval)

    def check_gaps(self, true_db, result_db, mapped, maps, result_gap, dust=None, crop=0, scoring=None, first_contig=1, count=None):
        """dh_check_gaps: the gap analysis of `dentist check-results`.  true_db / result_db: Db objects; mapped: (n_input, 3) rows of
        (true contig 1-based, begin, end); maps: CONTIG_MAPPING_DTYPE records in any order; result_gap: the N-run behind every result
        contig; dust: (ptr, iv) in the layout of read_mask, or None; gap i lies behind input contig first_contig + i (1-based); count
        None: every gap from first_contig on.  Returns a GapReport."""
        return _lacmd.check_gaps(self, true_db, result_db, mapped, maps, result_gap, dust, crop, scoring, first_contig, count)

    def output_db(self, fasta_path, contigs, scaffold_of, headers, gap_len, insertions_db, bed_path=None, agp_path=None,
                  join_policy="scaffoldGaps", agp_dazzler=False, agp_skip_read_ids=False, read_names=None, line_width=50,
                  highlight=True, tool=None, input_assembly=None, only="spanning", min_extension_length=100,
                  max_insertion_error=None, skip_gaps=None):
        """dh_output_db: `dentist output` with the FASTA text formatted on the device.  contigs: a Db of this context;
        insertions_db: the path of an insertions.db (read with dh_insertions_from_db against the Db's contig offsets);
        fasta_path None: stdout.  The other keywords as for output_assembly; max_insertion_error (a fraction, None: no cut)
        and skip_gaps (pairs of 0-based contig ids) are the filter.  Returns the number of insertions the join policy dropped."""
        return _output.output_db(self, fasta_path, contigs, scaffold_of, headers, gap_len, insertions_db, bed_path, agp_path,
                                 join_policy, agp_dazzler, agp_skip_read_ids, read_names, line_width, highlight, tool, input_assembly,
                                 only, min_extension_length, max_insertion_error, skip_gaps)

    def process_pileups_db(self, contigs, reads_db_path, pileups_path, opts, first=0, count=-1, repeat_mask=None, insertions_db=None,
                           read_ids=False):
        """dh_process_pileups_db: `dentist process --batch` on files -- pile-ups [first, first + count) of pile-ups.db (count -1:
        to the end), only the reads they name loaded from the reads DB.  Returns what process_pileups returns (records in node
        order, read ids of the whole DB)."""
        return _process.process_pileups_db(self, contigs, reads_db_path, pileups_path, opts, first, count, repeat_mask, insertions_db,
                                           read_ids)

    def output_stats(self):
        """The last output_db of this context in ms: kernels, copies back, fwrite, the whole formatting."""
        return _output.output_stats(self)

    def tandem_mask(self, las, read_off, first_read=0, min_len=500):
        """dh_la_tandem_mask: TANmask's rule on the device -- the union of [min(abpos, bbpos), max(aepos, bepos)) over the
        records with aread == bread on the same strand that are at least min_len long, per read aread - first_read.  Returns
        a MaskSet indexed by read."""
        return _lacmd.la_tandem_mask(self, las, read_off, first_read, min_len)

    def transpose(self, A, B, las, trace=None, tspace=None, select_best=False):
        """dh_la_transpose: the same alignments with the roles of the sequences exchanged (aread = B read, trace points on
        the B read's grid), from their edit paths.  Returns (las', trace', src_index), LAsort order; src_index[i] is the
        source record of las'[i].  `las` may be a raw handle of align_db_block(..., raw=True) (dh_la_set_transpose)."""
        return _align.la_transpose(self, A, B, las, trace, tspace, select_best)

    def align_db_block(self, A, B, first, count, opts, select_best=False, raw=False):
        """`damapper ref reads.<block>`: reads [first, first + count) of B against A.  raw=True
        returns the library handle (for merge_las) instead of numpy views."""
        return _align.align_db_block(self, A, B, first, count, opts, select_best, raw)
