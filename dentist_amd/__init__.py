"""dentist_amd -- MI355X (gfx950) implementation of DENTIST's alignment + consensus hot path.

The product is ``libdentist_hip.so`` (hand-written HIP kernels behind the C ABI declared in
``include/dentist_hip.h``).  This package is the thin ctypes binding tests and ``bench.py`` use to
call that ABI; it contains no compute of its own and no CPU fallback -- loading fails loudly when
the library is missing, and every compute call fails with ``DhError`` when no HIP device is
usable.
"""
from ._lib import (AlignOpts, AlignStats, Context, DazzDb, Db, DhError, dazz_create_dam, dazz_create_db, dazz_split, dazz_write_mask, INSERTION_DTYPE, LA_DTYPE, SEED_CAND_DTYPE, EXACT_HIT_DTYPE, ChainOpts, Chains, default_chain_opts, PropagatedMask, RepeatMask, RepeatOpts, MaskOpts, MaskSet, GapReport, contig_mappings, CONTIG_MAPPING_DTYPE, GAP_SUMMARY_DTYPE, GAP_STATES, Pileups, DeviceTrace,  # noqa: F401
                   ProcessOpts, default_align_opts, default_process_opts, join_hit_capacity, las_read, las_write, lib, lib_path,
                   process_pileups, process_stats, output_fasta, output_assembly, tile_qv, consensus, las_merge, merge_las, Cropped, translate_trace_point, common_trace_point, pileupdb_write, pileupdb_read,
                   insertiondb_write, insertiondb_read, insertiondb_merge, insertions_from_db, output_plan, collect_filter, scaffold_pileups, scaffold_spanning_pileups, scaffold_all_pileups, max_coverage_reads, max_improper_coverage_reads, propagate_mask, validate_regions, ValidatedRegions, REGION_DTYPE, REGION_REPORT_DTYPE, EditPaths, NW_OK, NW_BAND_EXCEEDED, CP_OK, CP_FAKED, CP_NESTED, NW_MAX_LEN, NW_MAX_BAND, NWA_DEFAULT_SCORING, format_cigar, format_alignment, format_pair, JOIN_DTYPE, READ_ALIGNMENT_DTYPE, SEEDED_DTYPE, CHAIN_LA_DTYPE, INSERTION_REC_DTYPE, Comm, shard_run, load_reads, load_stats, pileups_from_db, bed_to_mask, read_mask_extra, write_mask_extra, BedMask, MaskExtra)
from . import _lib


def __getattr__(name):  # NWA_MAX_LEN, NWA_MAX_BAND: read from the header on first use (_lib.__getattr__)
    if name in _lib._HEADER_LIMITS:
        return getattr(_lib, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
