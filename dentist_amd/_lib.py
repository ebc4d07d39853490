"""ctypes binding of include/dentist_hip.h (libdentist_hip.so). No compute, no fallback.

The facade over the modules the binding is made of, one per role:
  _abi      loading, DhError, struct layouts, record dtypes, the table of prototypes
  _marshal  array pointers, the mask pair, offsets checks, views and copies of library memory, the owner of a handle
  _align    Db, align / seed, result sets and .las files, edit paths, transposition, nw, nwa, locate, the formatters
  _lacmd    chain, propagate-mask, validate-regions, the collect filters, repeat mask, mask algebra, check-gaps
  _process  Pileups, map_reads, Cropped, the process calls, the scaffold graph
  _shard    Comm, ShardPlan, shard_*
  _output   the output calls
  _dazz     DazzDb, mask track extras, bed_to_mask, load_reads, pile-ups.db and insertions.db
  _context  Context: a docstring and a one-line call per command
"""
from ._abi import (AlignOpts, AlignStats, ChainOpts, CumStats, DhError, MaskOpts, OutputFilter, OutputOpts,  # noqa: F401
                   ProcessOpts, RepeatOpts, ScaffoldOpts, REMAP_FN, SYMBOLS, CHAIN_LA_DTYPE, CONTIG_MAPPING_DTYPE,
                   EXACT_HIT_DTYPE, GAP_STATES, GAP_SUMMARY_DTYPE, INSERTION_DTYPE, INSERTION_REC_DTYPE, JOIN_DTYPE,
                   LA_DTYPE, READ_ALIGNMENT_DTYPE, REGION_DTYPE, REGION_REPORT_DTYPE, SEED_CAND_DTYPE, SEEDED_DTYPE,
                   _check, lib, lib_path)
from ._align import (CP_FAKED, CP_NESTED, CP_OK, NW_BAND_EXCEEDED, NW_MAX_BAND, NW_MAX_LEN, NW_OK,  # noqa: F401
                     NWA_DEFAULT_SCORING, Db, DeviceTrace, EditPaths, _HEADER_LIMITS, _take_la_set, common_trace_point,
                     default_align_opts, format_alignment, format_cigar, format_pair, header_limit, join_hit_capacity,
                     las_merge, las_read, las_write, merge_las, translate_trace_point)
from ._lacmd import (Chains, GapReport, MaskSet, PropagatedMask, RepeatMask, ValidatedRegions, collect_filter,  # noqa: F401
                     contig_mappings, default_chain_opts, max_coverage_reads, max_improper_coverage_reads,
                     propagate_mask, validate_regions)
from ._process import (Cropped, Pileups, _take_insertions, consensus, default_process_opts, process_pileups,  # noqa: F401
                       process_stats, scaffold_all_pileups, scaffold_pileups, scaffold_spanning_pileups, tile_qv)
from ._shard import (Comm, ShardPlan, shard_pack_candidates, shard_pack_cropped, shard_read_joins, shard_run,  # noqa: F401
                     shard_run_prepare, shard_unpack_cropped)
from ._output import JOIN_POLICIES, output_assembly, output_fasta, output_plan  # noqa: F401
from ._dazz import (BedMask, DazzDb, MaskExtra, bed_to_mask, dazz_create_dam, dazz_create_db, dazz_split,  # noqa: F401
                    dazz_write_mask, insertiondb_merge, insertiondb_read, insertiondb_write, insertions_from_db, load_reads,
                    load_stats, pileupdb_read, pileupdb_write, pileups_from_db, read_mask_extra, write_mask_extra)
from ._context import Context  # noqa: F401


def __getattr__(name):   # NWA_MAX_LEN, NWA_MAX_BAND: read from the header on first use
    if name not in _HEADER_LIMITS:
        raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
    globals()[name] = header_limit(name)
    return globals()[name]
