"""One call from the input files to the output tables: the hot path with the rows either side of it.

What `pymasc sample.bam -m track.bw -d MAX_SHIFT -q MAPQ -r READ_LEN -o OUTDIR` does between argument parsing and the
statistics / plots (PyMaSC/pymasc.py:90-160, handler/calc.py:100-161): open the BAM, open the mappability track,
load or compute the mappable-length cache, run the calculator over the reads, write the `_cc` / `_mscc` / `_nreads`
tables and, with ``stats=True``, the `_stats.tab` of the fragment-length estimate and the quality scores (pymasc_amd.stats).
Without READ_LEN the read length is estimated from the BAM file first (pymasc.py:187-227, handler/calc.py:74-98;
pymasc_amd.readlen).  No CLI and no figures.
Under `torch.distributed` (one process per GPU) the chromosomes are sharded over the ranks and rank 0 writes.
`run_files` is the same for several files in one call, as `pymasc a.bam b.bam -n A B` runs them (pymasc.py:90-160):
one read length, one mappable-length cache, one track reader and one context for all of them.
"""
from __future__ import annotations

import logging
import os
import pickle
from collections import namedtuple
from itertools import zip_longest
from pathlib import Path
from typing import List, Optional, Sequence

from . import ffi, readlen, tables
from .chromfilter import NoTargetChromosomesError, filter_references
from .exceptions import InputUnseekable, ReadUnsortedError
from .inputs import default_device_ingest, is_stream, open_alignments, open_header, open_track, track_on_device
from .mappability import MappabilityStats
from .sharding import _collective_device_setup, on_rank0, rank_and_world, run_sharded

logger = logging.getLogger(__name__)


def run(bam_path, outdir, max_shift: int, read_len: Optional[int] = None, mapq_criteria: int = 1, mappability_path=None,
        mappability_stats_path=None, skip_ncc: bool = False, references: Optional[Sequence[str]] = None,
        device: Optional[int] = None, save_mappability_stats: bool = True, group=None, context=None,
        device_ingest: Optional[bool] = None, readlen_estimator: str = "MEDIAN", chromfilter=None, stats: bool = False,
        library_length: Optional[int] = None, smooth_window: int = 15, mask_size: int = 5, bg_avr_width: int = 50,
        chi2_pval: float = 0.05, chrom_sizes=None, complexity: bool = False):
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
    a ValueError before any GPU work (PyMaSC logs a too long ``library_length`` and ignores it).
    ``bam_path`` may also be a BED read file (tagAlign, ``pymasc_amd.bed_reads``); its references are ``chrom_sizes`` (a path or
    an ordered ``{name: length}``), without which it is a ValueError; other inputs keep their header's.
    ``complexity``: rank 0 also writes ``<stem>_complexity.tab`` (pymasc_amd.complexity: NRF, PBC1, PBC2 of the reads at
    ``mapq_criteria`` on the chosen chromosomes, flagged duplicates kept).  One rank: counted on the reader
    the run feeds from, so the file is inflated once (a stream is counted window by window while it is fed).  Several ranks:
    rank 0 alone counts the chosen chromosomes on one more read of the file through ``inputs.open_alignments``, after the
    run; no collective is added.  A run that raises (unsorted reads) writes no table."""
    if references is not None and chromfilter is not None:
        raise ValueError("give references or chromfilter, not both")
    _check_bed_sizes(bam_path, chrom_sizes)
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
                                               context, device_ingest, world, chrom_sizes)
        return _run(bam_path, outdir, max_shift, read_len, mapq_criteria, mappability_path, mappability_stats_path,
                    skip_ncc, references, device, save_mappability_stats, group, context, device_ingest, bam, rank,
                    chromfilter, stat_opts, chrom_sizes, complexity)
    finally:
        if bam is not None:
            bam.close()


def _check_bed_sizes(path, chrom_sizes) -> None:
    """A BED read file needs ``chrom_sizes``: ValueError before any work."""
    from .bed_reads import is_bed_reads
    if chrom_sizes is None and is_bed_reads(path):
        raise ValueError("'{}' is a BED read file: give the chromosome sizes (chrom_sizes=, --chrom-sizes)".format(path))


def _estimate_read_len(bam_path, max_shift, mapq_criteria, esttype, device, group, context, device_ingest, world,
                       chrom_sizes=None):
    """(read length, the device reader it was estimated on or None).  One rank: on the device reader that the run then
    feeds from when the BAM file goes through the GPU, on the host reader otherwise.  Several ranks: rank 0 estimates on the
    host reader and broadcasts the value or its error (sharding.on_rank0); every rank raises on an error, none waits."""
    readlen._check_esttype(esttype)                     # (every rank: a wrong name fails before any collective)
    if world == 1 and (default_device_ingest(world, context) if device_ingest is None else device_ingest):
        bam = open_alignments(bam_path, True, device=(context.device if context is not None else device),
                              chrom_sizes=chrom_sizes)
        try:
            return readlen.estimate_from_reader(bam, esttype, mapq_criteria, max_shift), bam
        except BaseException:
            bam.close()
            raise

    def estimate():                 # the whole file: the host reader without its index
        with open_alignments(bam_path, False, index=False, chrom_sizes=chrom_sizes) as b:
            return readlen.estimate_from_reader(b, esttype, mapq_criteria, max_shift)
    return int(on_rank0(estimate, group, "read length estimation")), None


def _run(bam_path, outdir, max_shift, read_len, mapq_criteria, mappability_path, mappability_stats_path, skip_ncc,
         references, device, save_mappability_stats, group, context, device_ingest, bam, rank, chromfilter=None,
         stat_opts=None, chrom_sizes=None, complexity=False):
    # The mappable-length cache (handler/mappability.py:239-309): loaded when valid; otherwise computed ONCE, on rank 0,
    # written atomically, and broadcast -- the other ranks neither recompute it per chromosome nor read a file that is
    # being rewritten.
    # A genome FASTA's track is generated once per rank (on its GPU when it has one, inputs.track_on_device) and that one
    # reader serves the mappable lengths and the feed.
    track = None
    if mappability_path is not None and _is_fasta(mappability_path):
        track = open_track(mappability_path, track_on_device(mappability_path, False, context),
                           context.device if context is not None else device, k=read_len)

    def mappable_lengths():
        bw = track if track is not None else open_track(mappability_path, False)
        try:
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
        finally:
            if bw is not track:
                bw.close()
    counted = _ComplexityCount(mapq_criteria) if complexity else None
    try:
        known = None if mappability_path is None else on_rank0(mappable_lengths, group, "mappability statistics")
        result = run_sharded(bam_path, max_shift, read_len, mapq_criteria, bigwig_path=mappability_path,
                             references=references, skip_ncc=skip_ncc, device=device, chrom2mappable_len=known,
                             group=group, context=context, device_ingest=device_ingest, bam=bam, chromfilter=chromfilter,
                             chrom_sizes=chrom_sizes, track=track,
                             reader_hook=counted.hook if counted is not None and rank_and_world(group)[2] == 1 else None)
    finally:
        if track is not None:
            track.close()
    written: List[Path] = []
    if rank == 0:
        written = _write_outputs(outdir, Path(bam_path).stem, result, read_len, stat_opts)
        if counted is not None:
            written.append(counted.write(outdir, Path(bam_path).stem, bam_path, references, chromfilter,
                                         rank_and_world(group)[2], device_ingest, context, device, chrom_sizes))
    return result, written


class _ComplexityCount:
    """The library complexity of one file's run (pymasc_amd.complexity).  ``hook`` is run_sharded's ``reader_hook`` on one
    rank: the count is taken on the reader that feeds the run (a stream: armed before the feed, summed window by window).
    ``write`` writes the table; without a count so far (several ranks) it first counts the chosen chromosomes on one more
    read of the file, through the reader ``inputs.open_alignments`` gives a run of that many ranks."""

    def __init__(self, mapq_criteria: int):
        self.mapq_criteria = int(mapq_criteria)
        self.value = None

    def hook(self, reader, names):
        from . import complexity
        if hasattr(reader, "arm_complexity"):
            acc = reader.arm_complexity(self.mapq_criteria, names)

            def after():
                reader.disarm_complexity()
                self.value = acc.result()
            return after

        def after():
            self.value = complexity.from_reader(reader, self.mapq_criteria, names)
        return after

    def write(self, outdir, basename: str, path, references, chromfilter, world, device_ingest, context, device,
              chrom_sizes) -> Path:
        from . import complexity
        if self.value is None:
            ingest = bool(default_device_ingest(world, context) if device_ingest is None else device_ingest)
            dev = context.device if (context is not None and ingest) else (device or 0)
            with open_alignments(path, ingest, dev, chrom_sizes=chrom_sizes) as r:
                if chromfilter is not None:
                    names = filter_references(r.references, chromfilter)
                else:
                    names = [n for n in r.references if references is None or n in set(references)]
                self.value = complexity.from_reader(r, self.mapq_criteria, names)
        return complexity.write_complexity(Path(outdir) / basename, basename, self.value)


def _write_outputs(outdir, basename: str, result, read_len, stat_opts) -> List[Path]:
    """``outdir/<basename>_{cc,mscc,nreads}.tab`` and, with ``stat_opts``, ``<basename>_stats.tab`` whose Name row is
    ``basename``; the paths written."""
    out = Path(outdir)
    out.mkdir(parents=True, exist_ok=True)
    # write_tables names the tables after the stem of its path (table.py:185-188): a suffix keeps a dotted base name whole
    written = tables.write_tables(out / (basename + ".bam"), result)
    if stat_opts is not None:       # every rank holds the same result: the statistics are rank 0's alone
        from . import stats
        written.append(stats.write_stats(out / basename, stats.genome_wide_stats(result, read_len, **stat_opts)))
    return written



# ---------------------------------------------------------------------------------------------------------------------
# Several files in one call: `pymasc a.bam b.bam -n A B` (pymasc.py:90-160)
# ---------------------------------------------------------------------------------------------------------------------

FileResult = namedtuple("FileResult", "path basename result written error")
FileResult.__doc__ = """One input of run_files: ``basename`` names its outputs; a skipped file has ``result`` None, ``written``
[] and in ``error`` the exception that skipped it."""


def run_files(paths, outdir, max_shift: int, read_len: Optional[int] = None, mapq_criteria: int = 1, mappability_path=None,
              mappability_stats_path=None, skip_ncc: bool = False, references: Optional[Sequence[str]] = None,
              device: Optional[int] = None, save_mappability_stats: bool = True, group=None, context=None,
              device_ingest: Optional[bool] = None, readlen_estimator: str = "MEDIAN", chromfilter=None, stats: bool = False,
              library_length: Optional[int] = None, smooth_window: int = 15, mask_size: int = 5, bg_avr_width: int = 50,
              chi2_pval: float = 0.05, names: Optional[Sequence[Optional[str]]] = None, chrom_sizes=None,
              complexity: bool = False) -> List[FileResult]:
    """``run`` over several alignment files in one call, as ``pymasc a.bam b.bam -n A B`` runs them; returns one FileResult per
    file, in input order.  Every keyword means what it means for ``run`` (``complexity``: ``<name>_complexity.tab`` for every
    file that runs, counted as ``run`` counts it; a file that is skipped gets no table).

    ``names``: PyMaSC's -n, paired with the files by position (a missing or None name: ``Path(file).stem``, so that a file
    without a name gets exactly what ``run`` writes for it); a name ``N`` gives ``N_cc.tab`` ... ``N_stats.tab``, whole even
    when it holds a dot.  ``chrom_sizes``: the references of every BED read file among ``paths`` (``run``); a BED read file
    without them is skipped in step 1 with run's ValueError, and BAM / SAM files keep their header's lengths (logged once when
    ``chrom_sizes`` is given beside them).  More names than files, an empty name or one with a path separator, and two files with the same base
    name are a ValueError before any work, as bad options are.  Outputs that exist already are warned about first
    (pymasc.py:178-182).

    The steps, in the reference's order (pymasc.py:99-160, 187-250):

    1. Every file's header is read on the host (``inputs.open_header``: no record is read) and the chromosome filter
       applied; a file that fails -- missing, not BAM / SAM, a bad or empty header, no chromosome left by ``chromfilter`` --
       is logged and skipped.
    2. The read length: ``read_len``, or the estimate of every file left (on the device reader when the run ingests on the
       device); a file whose estimate raises ValueError (no reads, longer than ``max_shift``) is logged and skipped, and the
       others run with the LONGEST estimate, with PyMaSC's warning when they differ.  No file left: ValueError.  Only one device
       reader is open at a time, so with several files and no ``read_len`` each file is inflated twice: once for its estimate,
       once for its run; a single file is inflated once, as ``run`` does it.
    3. The mappable-length cache, once: loaded, or computed with the common read length (and saved with
       ``save_mappability_stats``); every file's calculator takes its lag tables from it.
    4. The files one after the other, each sharded over the ranks as ``run`` shards it.  A file whose reads are not sorted
       (ReadUnsortedError) is logged and skipped; any other error propagates.

    One context (``context``, else one made here and closed at the end) serves every file and the cache: each file's
    calculator gives its bit-vectors back to the context's pool and frees its result arena before the next file.  The track is
    opened once per rank.  Several ranks: rank 0 alone takes steps 1 and 2 and broadcasts which files are left and the read
    length; every rank then walks the same files, the skip of an unsorted file is decided from every rank's outcome, and
    rank 0 writes (``written`` is [] on the other ranks)."""
    paths = list(paths)
    if not paths:
        raise ValueError("no input files")
    if references is not None and chromfilter is not None:
        raise ValueError("give references or chromfilter, not both")
    from .stats import check_params
    check_params(None, library_length, smooth_window, max_shift)
    if read_len is None:
        readlen._check_esttype(readlen_estimator)
    bases = _basenames(paths, names)
    stat_opts = None
    if stats:
        stat_opts = dict(library_length=library_length, smooth_window=smooth_window, mask_size=mask_size,
                         bg_avr_width=bg_avr_width, chi2_pval=chi2_pval)
    on, rank, world = rank_and_world(group)
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if on else 0
    _collective_device_setup(device, group)
    if rank == 0:
        _warn_existing(outdir, bases, mappability_path is not None, skip_ncc, stats, complexity)
        if chrom_sizes is not None and not all(_is_bed(p) for p in paths):
            logger.info("The chromosome sizes are used for BED read files only: BAM and SAM files keep their header's lengths.")
    ingest = bool(default_device_ingest(world, context) if device_ingest is None else device_ingest)
    dev = context.device if (context is not None and ingest) else device         # the device readers' GPU

    errors: List[Optional[BaseException]] = [None] * len(paths)
    kept = {}                       # index -> device reader opened in _choose that feeds that file's run too
    ctx, own_ctx, track = context, False, None
    try:
        if world == 1:
            read_len, kept = _choose(paths, errors, read_len, chromfilter, readlen_estimator, mapq_criteria, max_shift,
                                     dev if ingest else None, chrom_sizes)
        else:                       # rank 0 decides, every rank learns the same (none waits for a value that never comes)
            def choose():
                errs: List[Optional[BaseException]] = [None] * len(paths)
                rl, _k = _choose(paths, errs, read_len, chromfilter, readlen_estimator, mapq_criteria, max_shift, None,
                                 chrom_sizes)
                return rl, [None if e is None else _portable(e) for e in errs]
            read_len, errors = on_rank0(choose, group, "choosing the input files")
        if read_len is None:
            raise ValueError("no input file is left to run")
        live = [i for i, e in enumerate(errors) if e is None]
        if ctx is None:
            ctx, own_ctx = ffi.Context(device), True
        known = None
        if mappability_path is not None:        # (a genome FASTA: its k-mer track with k = the read length)
            fasta = _is_fasta(mappability_path)
            track = open_track(mappability_path, track_on_device(mappability_path, ingest, ctx),
                               getattr(ctx, "device", dev) if fasta else dev, k=read_len)

            def mappable_lengths():
                ms = MappabilityStats(track, max_shift, read_len, map_path=mappability_stats_path,
                                      track_path=mappability_path, device=device, context=ctx)
                try:
                    if not ms.is_called:                    # no valid cache: the lag tables of every file, computed once
                        ms.calc_mappability()
                        if save_mappability_stats:
                            ms.save_mappability_stats()
                    return ms.chrom2mappable_len
                finally:
                    ms.close()
            known = on_rank0(mappable_lengths, group, "mappability statistics")
        logger.info("Calculate cross-correlation between 0 to {} base shift with reads MAPQ >= {}"
                    "".format(max_shift, mapq_criteria))
        results = {}
        for i in live:
            logger.info("Process {}".format(paths[i]))
            bam = None
            bam = kept.pop(i, None)
            counted = _ComplexityCount(mapq_criteria) if complexity else None
            try:
                result = run_sharded(paths[i], max_shift, read_len, mapq_criteria, bigwig_path=mappability_path,
                                     references=references, skip_ncc=skip_ncc, device=device, chrom2mappable_len=known,
                                     group=group, context=ctx, device_ingest=ingest, bam=bam, chromfilter=chromfilter,
                                     track=track, chrom_sizes=chrom_sizes,
                                     reader_hook=counted.hook if counted is not None and world == 1 else None)
            except Exception as e:
                skip = _unsorted_on_every_rank(e, world)
                if skip is None:
                    raise
                logger.error("Reads of '{}' are not sorted by position: the file is skipped ({})".format(paths[i], skip))
                errors[i] = skip
                continue
            finally:
                if bam is not None:
                    bam.close()
            def write_all():
                out = _write_outputs(outdir, bases[i], result, read_len, stat_opts)
                if counted is not None:
                    out.append(counted.write(outdir, bases[i], paths[i], references, chromfilter, world, ingest, ctx, device,
                                             chrom_sizes))
                return out
            written = on_rank0(write_all, group, "writing the outputs of '{}'".format(paths[i]))
            results[i] = (result, list(written) if rank == 0 else [])
    finally:
        for r in kept.values():
            r.close()
        if track is not None:
            track.close()
        if own_ctx:
            ctx.close()
    return [FileResult(p, b, *results[i], None) if i in results else FileResult(p, b, None, [], errors[i])
            for i, (p, b) in enumerate(zip(paths, bases))]


def _basenames(paths, names) -> List[str]:
    """The base name of every file's outputs (pymasc.py:172-177), checked."""
    names = list(names or [])
    if len(names) > len(paths):
        raise ValueError("{} names for {} input files".format(len(names), len(paths)))
    out = []
    for f, n in zip_longest(paths, names):
        if n is None:
            n = Path(f).stem
        elif not n or os.sep in n or (os.altsep and os.altsep in n) or n in (".", ".."):
            raise ValueError("an output name is a file name: {!r}".format(n))
        out.append(str(n))
    seen = {}
    for f, n in zip(paths, out):
        if n in seen:
            raise ValueError("'{}' and '{}' would both write '{}_*': give them different names".format(seen[n], f, n))
        seen[n] = f
    return out


def _warn_existing(outdir, bases, has_track, skip_ncc, stats, complexity=False):
    """prepare_output's warning (pymasc.py:178-182) for every output about to be replaced."""
    suffixes = [s for s, on in (("_cc.tab", not (has_track and skip_ncc)), ("_mscc.tab", has_track), ("_nreads.tab", True),
                                ("_stats.tab", stats), ("_complexity.tab", complexity)) if on]
    for b in bases:
        for suffix in suffixes:
            path = Path(outdir) / (b + suffix)
            if path.exists():
                logger.warning("Existing file '{}' will be overwritten.".format(path))


def _is_fasta(path) -> bool:
    from .kmer_track import is_fasta
    return is_fasta(path)


def _is_bed(path) -> bool:
    from .bed_reads import is_bed_reads
    return is_bed_reads(path)


def _choose(paths, errors, read_len, chromfilter, esttype, mapq_criteria, max_shift, device, chrom_sizes=None):
    """Steps 1 and 2 of run_files: the files that open and keep a chromosome, then the common read length.  Fills ``errors``
    with the exception of every file skipped; returns (read length or None when no file is left, {index: device reader} of
    the readers opened here that feed their file's run).  ``device``: the GPU of the device reader the estimates are made on,
    None for the host reader.  A stream (inputs.is_stream: ``-``, a FIFO) is opened once, here, by the stream reader, which
    then feeds its run; without ``read_len`` it is skipped before a byte of it is read (PyMaSC: handler/calc.py:81,
    pymasc.py:199-201), and without the device reader (``device`` None) too.  A BED read file takes its references from
    ``chrom_sizes`` (inputs.open_header); without them it is skipped here."""
    kept = {}
    for i, p in enumerate(paths):
        stream = is_stream(p)
        if stream and read_len is None:
            logger.error("Cannot execute read length checking for unseekable input.")
            logger.error("If your input can't reread, specify read length using `-r` option.")
            errors[i] = InputUnseekable("'{}' is not seekable: give the read length".format(p))
            continue
        if stream and device is None:
            logger.error("Failed to open file '{}'".format(p))
            logger.error("A stream input is read by the device reader only: one process on a GPU.")
            errors[i] = ValueError("'{}' is a stream: it needs the device reader".format(p))
            continue
        try:
            r = open_alignments(p, True, device=device) if stream else open_header(p, chrom_sizes)
            try:
                if not r.references:
                    raise ValueError("File has no sequences defined.")
                filter_references(r.references, chromfilter)
                if stream:
                    kept[i], r = r, None
            finally:
                if r is not None:
                    r.close()
        except NoTargetChromosomesError as e:
            logger.error("Check your -i/--include-chrom and/or -e/--exclude-chrom options.")
            errors[i] = e
        except (OSError, ValueError) as e:
            logger.error("Failed to open file '{}'".format(p))
            logger.error(str(e))
            errors[i] = e
    live = [i for i, e in enumerate(errors) if e is None]
    if not live:
        return None, kept
    if read_len is not None:
        return int(read_len), kept
    logger.info("Check read length: Get {} from read length distribution".format(str(esttype).lower()))
    lengths = []
    for i in live:
        logger.info("Check read length... : {}".format(paths[i]))
        if device is None:
            r = open_alignments(paths[i], False, index=False, chrom_sizes=chrom_sizes)   # the whole file, without its index
        else:
            r = open_alignments(paths[i], True, device=device, chrom_sizes=chrom_sizes)
        estimated = False
        try:
            lengths.append(readlen.estimate_from_reader(r, esttype, mapq_criteria, max_shift))
            estimated = True
        except ValueError as e:
            logger.error(str(e))
            errors[i] = e
        finally:
            if estimated and device is not None and len(live) == 1:
                kept[i] = r
            else:
                r.close()
    if not lengths:
        return None, kept
    if len(set(lengths)) != 1:
        logger.warning("There are multiple read length candidates. Use max length "
                       "({}) for MSCC calculation.".format(max(lengths)))
    return max(lengths), kept


def _portable(error: BaseException) -> BaseException:
    """``error`` when it survives a pickle round trip (the ranks' broadcast), else a RuntimeError that says what it was."""
    try:
        back = pickle.loads(pickle.dumps(error))
        if type(back) is type(error) and str(back) == str(error):
            return error
    except Exception:
        pass
    return RuntimeError("{}: {}".format(type(error).__name__, error))


def _unsorted_on_every_rank(error: BaseException, world: int) -> Optional[ReadUnsortedError]:
    """The ReadUnsortedError that skips a file on every rank, or None when ``error`` propagates on every rank.  Several ranks:
    the decision is taken from ``failed_ranks``, which sharding.gather_chromosome_results attaches to what it raises on every
    rank (the failing rank's own exception, a RuntimeError on the others) and which is the same list on every rank -- skip when
    every failing rank's reads were unsorted.  An exception that did not come through that gather propagates."""
    if world == 1:
        return error if isinstance(error, ReadUnsortedError) else None
    failed = getattr(error, "failed_ranks", None)
    if not failed or any(kind != ReadUnsortedError.__name__ for _rank, kind, _msg in failed):
        return None
    return error if isinstance(error, ReadUnsortedError) else ReadUnsortedError(failed[0][2])
