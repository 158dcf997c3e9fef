"""One call from the input files to the output tables: the hot path with the rows either side of it.

What `pymasc sample.bam -m track.bw -d MAX_SHIFT -q MAPQ -r READ_LEN -o OUTDIR` does between argument parsing and the
statistics / plots (PyMaSC/pymasc.py:90-160, handler/calc.py:100-161): open the BAM, open the mappability track,
load or compute the mappable-length cache, run the calculator over the reads, write the `_cc` / `_mscc` / `_nreads`
tables and, with ``stats=True``, the `_stats.tab` of the fragment-length estimate and the quality scores (pymasc_amd.stats).
Without READ_LEN the read length is estimated from the BAM file first (pymasc.py:187-227, handler/calc.py:74-98;
pymasc_amd.readlen).  No CLI and no figures.
Under `torch.distributed` (one process per GPU) the chromosomes are sharded over the ranks and rank 0 writes.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import List, Optional, Sequence

from . import readlen, tables
from .inputs import default_device_ingest, open_alignments, open_track
from .mappability import MappabilityStats
from .sharding import _collective_device_setup, on_rank0, rank_and_world, run_sharded


def run(bam_path, outdir, max_shift: int, read_len: Optional[int] = None, mapq_criteria: int = 1, mappability_path=None,
        mappability_stats_path=None, skip_ncc: bool = False, references: Optional[Sequence[str]] = None,
        device: Optional[int] = None, save_mappability_stats: bool = True, group=None, context=None,
        device_ingest: Optional[bool] = None, readlen_estimator: str = "MEDIAN", chromfilter=None, stats: bool = False,
        library_length: Optional[int] = None, smooth_window: int = 15, mask_size: int = 5, bg_avr_width: int = 50,
        chi2_pval: float = 0.05):
    """Returns (genome-wide result, [paths written]).  ``outdir/<bam stem>_{cc,mscc,nreads}.tab`` are written by
    rank 0 (every rank holds the result).  ``context``: an existing pymasc_amd.ffi.Context to run on (default: one per
    call on ``device``).  ``device_ingest``: see sharding.run_sharded (default: the BAM file is inflated and decoded on the GPU
    when there is one rank on a real GPU).  ``read_len`` None: estimated from the BAM file with ``readlen_estimator``
    (MEAN / MEDIAN / MODE / MIN / MAX) at ``mapq_criteria``, as ``pymasc`` does without -r; longer than ``max_shift`` is a
    ValueError (handler/calc.py:93-98).  The estimate is taken over the whole file, as PyMaSC takes it, and on one rank it
    reuses the device reader that then feeds the run: with ``read_len`` None the whole file is opened even when
    ``references`` or ``chromfilter`` choose some chromosomes; with ``read_len`` given and a .bai present, the device reader
    reads only the chosen chromosomes' BGZF members (sharding.run_sharded).  ``chromfilter``: PyMaSC's -i / -e filter as
    ``[(include, [patterns]), ...]`` (pymasc_amd.chromfilter), not together with ``references``.  ``bam_path`` may be a SAM
    file, plain or BGZF (pymasc_amd.sam); the tables are named after ``Path(bam_path).stem`` as PyMaSC names them.
    ``stats``: rank 0 also writes ``<stem>_stats.tab`` (pymasc_amd.stats.genome_wide_stats / write_stats) with PyMaSC's
    options -l ``library_length``, -w ``smooth_window``, --mask-size ``mask_size``, --bg-avr-width ``bg_avr_width`` and
    --chi2-pval ``chi2_pval``.  A ``library_length`` longer than ``max_shift`` or below 1, or a ``smooth_window`` below 1, is
    a ValueError before any GPU work (PyMaSC logs a too long ``library_length`` and ignores it)."""
    if references is not None and chromfilter is not None:
        raise ValueError("give references or chromfilter, not both")
    from .stats import check_params
    check_params(None, library_length, smooth_window, max_shift)
    stat_opts = None
    if stats:
        stat_opts = dict(library_length=library_length, smooth_window=smooth_window, mask_size=mask_size,
                         bg_avr_width=bg_avr_width, chi2_pval=chi2_pval)
    on, rank, world = rank_and_world(group)
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if on else 0
    _collective_device_setup(device, group)
    bam = None                      # a reader opened here for the estimate and handed on: the file is inflated once per run
    try:
        if read_len is None:
            read_len, bam = _estimate_read_len(bam_path, max_shift, mapq_criteria, readlen_estimator, device, group,
                                               context, device_ingest, world)
        return _run(bam_path, outdir, max_shift, read_len, mapq_criteria, mappability_path, mappability_stats_path,
                    skip_ncc, references, device, save_mappability_stats, group, context, device_ingest, bam, rank,
                    chromfilter, stat_opts)
    finally:
        if bam is not None:
            bam.close()


def _estimate_read_len(bam_path, max_shift, mapq_criteria, esttype, device, group, context, device_ingest, world):
    """(read length, the device reader it was estimated on or None).  One rank: on the device reader that the run then
    feeds from when the BAM file goes through the GPU, on the host reader otherwise.  Several ranks: rank 0 estimates on the
    host reader and broadcasts the value or its error (sharding.on_rank0); every rank raises on an error, none waits."""
    readlen._check_esttype(esttype)                     # (every rank: a wrong name fails before any collective)
    if world == 1 and (default_device_ingest(world, context) if device_ingest is None else device_ingest):
        bam = open_alignments(bam_path, True, device=(context.device if context is not None else device))
        try:
            return readlen.estimate_from_reader(bam, esttype, mapq_criteria, max_shift), bam
        except BaseException:
            bam.close()
            raise

    def estimate():                 # the whole file: the host reader without its index
        with open_alignments(bam_path, False, index=False) as b:
            return readlen.estimate_from_reader(b, esttype, mapq_criteria, max_shift)
    return int(on_rank0(estimate, group, "read length estimation")), None


def _run(bam_path, outdir, max_shift, read_len, mapq_criteria, mappability_path, mappability_stats_path, skip_ncc,
         references, device, save_mappability_stats, group, context, device_ingest, bam, rank, chromfilter=None,
         stat_opts=None):
    # The mappable-length cache (handler/mappability.py:239-309): loaded when valid; otherwise computed ONCE, on rank 0,
    # written atomically, and broadcast -- the other ranks neither recompute it per chromosome nor read a file that is
    # being rewritten.
    def mappable_lengths():
        with open_track(mappability_path, False) as bw:
            stats = MappabilityStats(bw, max_shift, read_len, map_path=mappability_stats_path, track_path=mappability_path,
                                     device=device, context=context)
            try:
                if stats.is_called:                          # a valid cache: the autocorrelation pass is skipped
                    return stats.chrom2mappable_len
                if save_mappability_stats:
                    stats.calc_mappability()
                    stats.save_mappability_stats()
                    return stats.chrom2mappable_len
                return None
            finally:
                stats.close()
    known = None if mappability_path is None else on_rank0(mappable_lengths, group, "mappability statistics")
    result = run_sharded(bam_path, max_shift, read_len, mapq_criteria, bigwig_path=mappability_path,
                         references=references, skip_ncc=skip_ncc, device=device, chrom2mappable_len=known,
                         group=group, context=context, device_ingest=device_ingest, bam=bam, chromfilter=chromfilter)
    written: List[Path] = []
    if rank == 0:
        out = Path(outdir)
        out.mkdir(parents=True, exist_ok=True)
        written = tables.write_tables(out / Path(bam_path).name, result)
        if stat_opts is not None:   # every rank holds the same result: the statistics are rank 0's alone
            from . import stats
            written.append(stats.write_stats(out / Path(bam_path).stem,
                                             stats.genome_wide_stats(result, read_len, **stat_opts)))
    return result, written
