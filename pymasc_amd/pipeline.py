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
from dataclasses import dataclass, fields, replace
from itertools import zip_longest
from pathlib import Path
from typing import List, Optional, Sequence

from . import complexity, coverage, ffi, fingerprint, fragments, gcbias, peaks, readlen, tables, tss
from .chromfilter import NoTargetChromosomesError, filter_references, kept_references
from .exceptions import InputUnseekable, ReadUnsortedError
from .inputs import (check_bed_sizes, default_device_ingest, is_stream, open_alignments, open_header, open_track,
                     reader_device, track_on_device)
from .mappability import MappabilityStats
from .sharding import _collective_device_setup, on_rank0, rank_and_world, run_sharded

logger = logging.getLogger(__name__)


def run(bam_path, outdir, max_shift: int, read_len: Optional[int] = None, mapq_criteria: int = 1, mappability_path=None,
        mappability_stats_path=None, skip_ncc: bool = False, references: Optional[Sequence[str]] = None,
        device: Optional[int] = None, save_mappability_stats: bool = True, group=None, context=None,
        device_ingest: Optional[bool] = None, readlen_estimator: str = "MEDIAN", chromfilter=None, stats: bool = False,
        library_length: Optional[int] = None, smooth_window: int = 15, mask_size: int = 5, bg_avr_width: int = 50,
        chi2_pval: float = 0.05, chrom_sizes=None, complexity: bool = False, exclude_regions=None,
        fingerprint: bool = False, fingerprint_bin: int = 500, fingerprint_extend: int = 0, fingerprint_control=None,
        peaks=None, peaks_extend: int = 0, coverage: bool = False, coverage_extend="auto", gc_bias=None, gc_window: int = 100,
        fragments: bool = False, fragments_max: int = 2000, tss=None, tss_flank: int = 2000, tss_extend: int = 0,
        coverage_format: str = "bedgraph", coverage_compress=False, coverage_bin: int = 1, coverage_normalize: str = "none",
        coverage_scale: float = 1.0, coverage_genome_size: Optional[int] = None, coverage_control=None,
        coverage_compare: str = "log2", coverage_pseudocount: float = 1.0, coverage_call=None, coverage_call_gap: int = 30,
        coverage_call_length: int = 200, coverage_poisson: bool = False, coverage_lambda=(1000, 10000),
        coverage_qvalue: bool = False, coverage_call_q=None):
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
    run; no collective is added.  A run that raises (unsorted reads) writes no table.
    ``exclude_regions``: a BED file (plain, gzip or bgzip) or an ordered ``{name: [(start, end), ...]}`` of regions to leave out,
    as ENCODE leaves out its blacklist (pymasc_amd.region_mask): reads whose extent
    ``[pos1, pos1 + read_len - 1]`` overlaps a merged region are removed before the feeders (on the GPU with device ingest), the
    track is cleared where a read of the run's length would touch a region, ``complexity`` counts the reads that are left, and the
    mappable-length cache is ``<track stem>_<mask file stem>_mappability.json`` (a dict: none) unless ``mappability_stats_path``
    names it.  The read length is still estimated over the whole file.  No region's chromosome among the references: ValueError
    before any table is written.
    ``fingerprint``: rank 0 also writes ``<stem>_fingerprint.tab`` (pymasc_amd.fingerprint): the reads the
    correlation sees -- ``mapq_criteria``, flagged duplicates dropped, the chosen chromosomes, less the excluded regions -- counted
    per genome bin of ``fingerprint_bin`` bases, each read covering ``fingerprint_extend`` bases from its 5' end (0: its own
    length); the table holds the fingerprint's AUC, X-intercept and elbow, the Jensen-Shannon distance to a Poisson model and the
    number of bins at every count.  Counted where ``complexity`` is counted.  ``fingerprint_control``: an alignment file counted
    the same way (once per call, never correlated), with the Jensen-Shannon distance to it in the table; it turns
    ``fingerprint`` on.  Its chosen references must have the sample's names and lengths: ValueError before the run.
    ``peaks``: a peak file (narrowPeak, broadPeak, gappedPeak or any BED3+ file; plain, gzip or bgzip) or an ordered
    ``{name: [(start, end), ...]}``: rank 0 also writes ``<stem>_peaks.tab`` (pymasc_amd.peaks): the reads the
    fingerprint counts, each covering ``peaks_extend`` bases from its 5' end (0: its own length), counted per line of the file
    and in at least one line -- FRiP, its enrichment over the share of the genome the lines cover, a row per chromosome and a
    BED table of the reads per line.  Counted where ``complexity`` is counted.  No line's chromosome among the references:
    ValueError before any table is written.
    ``coverage``: rank 0 also writes ``<stem>_coverage.bedGraph`` (pymasc_amd.coverage): the reads the
    fingerprint counts, each covering ``coverage_extend`` bases from its 5' end (0: its own length), piled up base by base and
    written as runs of constant depth above 0.  An integer ``coverage_extend`` is counted where ``complexity`` is counted.
    ``"auto"`` (the default) extends to the run's own fragment-length estimate, ``stats.genome_wide_stats(...).est_lib_len``
    with the run's statistics options, whether or not ``stats`` writes them; it exists only after the correlation, so rank 0
    counts on one more read of the file, and a stream (``-``, a FIFO) with ``"auto"`` is a ValueError before anything runs.  The
    device table is 4 bytes per chosen base (12.4 GB for hg38).  ``coverage_format="bigwig"`` writes ``<stem>_coverage.bw`` instead
    (DESIGN.md 7.18.1): the same runs as a bigWig file with zoom levels, its sections and zoom records made on the GPU with device
    ingest; a depth is a float32 there, exact up to 2^24 and rounded to nearest above.  ``coverage_compress``: every section of
    that file through zlib on the host (True), or (``"device"``) through the GPU's own DEFLATE encoder before it
    leaves the device, which needs device ingest (a host reader is a ValueError, not zlib); the decoded file is the same, the
    compressed bytes are not zlib's.  With ``"bedgraph"`` either is a ValueError.
    ``coverage_bin`` (1 .. 65536), ``coverage_normalize`` (``"none"``, ``"cpm"``, ``"rpgc"``), ``coverage_scale`` and
    ``coverage_genome_size`` (a positive integer, with ``"rpgc"`` only): when any is not its default, the file holds the signal
    track made of the pileup -- the mean depth per bin times ``coverage.scale_of(...)``, float32, equal
    neighbours merged, made on the GPU with device ingest -- in either format; with the defaults the file is the depth track, byte
    for byte.
    ``coverage_control``: an alignment file (a regular file, not a stream; it implies ``coverage``): the file holds the treatment
    against the control instead -- ``coverage_compare`` ``"log2"``, ``"ratio"`` or ``"subtract"`` of the two scaled
    mean depths per bin, with ``coverage_pseudocount`` added to both for the first two; the factors are ``coverage.factors_of``.
    The control is piled up with the run's ``mapq_criteria``, chromosome filter, excluded regions and ``chrom_sizes`` and the
    treatment's extend (``"pair"``: its own pairs), once for every file; its chosen references must be the treatment's
    (ValueError).  A compare setting without a control is a ValueError.
    ``coverage_call``: a cutoff (any finite number; it implies ``coverage``): rank 0 also writes
    ``<stem>_coverage_peaks.narrowPeak``, the peaks of exactly the track the coverage file holds -- the compared
    track, the signal track or the depth --: runs of at least the cutoff, linked over gaps of at most ``coverage_call_gap`` bases
    and kept from ``coverage_call_length`` bases, called on the GPU with device ingest (``coverage.DeviceCount.call``) and in numpy
    otherwise (``coverage.Signal.call``).  The caller itself computes no p-value; ``peaks=`` reads the file in a second run.
    ``coverage_poisson``: with ``coverage_control``, which it needs (ValueError): the file holds -log10 of the Poisson upper tail
    ``P(X >= k | lambda)`` per bin instead of a compare operation -- ``k`` the treatment's mean depth per bin as
    an integer, ``lambda`` the largest of the control's mean over the genome, at the bin and over the two windows
    ``coverage_lambda = (small, large)`` in bases (each 0 .. 2^31 - 1, 0: off), the control scaled to the treatment's library size
    (``coverage.factors_of("none", ...)[1]``) --, made on the GPU with device ingest (``coverage.DeviceCount.poisson``) and in numpy
    otherwise (``coverage.Coverage.poisson``); with ``coverage_call`` the narrowPeak holds the score in column 8 as well.  It
    excludes a given ``coverage_compare`` or ``coverage_pseudocount`` and a ``coverage_normalize`` / ``coverage_scale`` other than
    ``"none"`` / 1 (ValueError: the treatment is not scaled, the score counts reads); ``coverage_lambda`` without it is a ValueError.
    ``coverage_qvalue``: with ``coverage_poisson`` and one of ``coverage_call`` / ``coverage_call_q``, which it needs (ValueError):
    the Benjamini-Hochberg q-scores of the p-score track over every base of the chosen references, made on the
    GPU with device ingest (``coverage.DeviceCount.qvalue``) and in numpy otherwise (``coverage.Signal.qvalues``); column 9 of the
    narrowPeak holds the q-score of every peak.  ``coverage_call_q``: a finite number ``X``: the peaks are called at ``pcut(X)``,
    the smallest p-score whose q-score reaches ``X`` (``X = 2``: q <= 0.01); it needs ``coverage_poisson``, excludes
    ``coverage_call`` and implies ``coverage_qvalue`` (ValueError otherwise); ``coverage_call_gap`` / ``coverage_call_length``
    apply as with ``coverage_call``.  The coverage file itself stays the p-score track.
    ``gc_bias``: a genome FASTA (plain, gzip or bgzip): rank 0 also writes ``<stem>_gcbias.tab`` (pymasc_amd.gcbias, DESIGN.md
    7.19): the reads the fingerprint counts, each placed on the genome window of ``gc_window`` bases (1 .. 1024) that begins at
    its 5' end, counted per G + C content of the window beside the number of genome windows of that content; windows with a base
    that is not A C G T or inside ``exclude_regions`` are left out.  Counted where ``complexity`` is counted.  The genome is
    parsed once per call (on the GPU with device ingest).  A chosen reference without a record of its name and length:
    ValueError before the run; a FASTA that cannot be parsed: ``GenomeError``.
    ``fragments``: rank 0 also writes ``<stem>_fragments.tab`` (pymasc_amd.fragments): the paired-end fragment
    sizes of the reads the fingerprint counts, each pair counted at its read1 record from that record's own mate fields, with
    median and spread per orientation (FR, RF, TANDEM) and the histogram up to ``fragments_max`` bases (1 .. 65536); an excluded
    region drops a pair whose fragment touches it.  Counted where ``complexity`` is counted.  ``coverage_extend="pair"`` piles the
    FR pairs of at most ``fragments_max`` bases at their own extent instead of extended reads; it is known before the feed, so a
    stream takes it.  A BED read file has no mate fields: ValueError before anything is read, with either.
    ``tss``: anchor sites (transcription start sites, motif hits) as a BED6 file (plain, gzip or bgzip) or an ordered
    ``{name: [(a, "+" | "-"), ...]}``: rank 0 also writes ``<stem>_tss.tab`` (pymasc_amd.tss): the reads the
    fingerprint counts, each covering ``tss_extend`` bases from its 5' end (0: its own length; 1: the 5' base only), piled up by
    their offset from every anchor within ``tss_flank`` bases (1 .. 4095) and by their strand relative to the anchor's, with the
    TSS enrichment over the mean of the table's outer edges.  Counted where ``complexity`` is counted.  The anchors are read once
    per call, against the alignment's own references: a line on a chromosome the alignment lacks, a strand of ``.`` or an anchor
    beyond its chromosome's end is a ValueError before any table is written."""
    check_bed_sizes(bam_path, chrom_sizes)
    s = _settings(locals())
    _check_coverage_input(s, bam_path)
    _check_pairs_input(s, bam_path)
    from .kmer_track import is_fasta
    bam = track = None              # a reader opened here for the estimate and handed on: the file is inflated once per run
    try:
        if read_len is None:        # (one rank: on_rank0 is the call itself, and the reader comes back with the length)
            read_len, bam = on_rank0(lambda: _estimate(s, bam_path, True), group, "read length estimation")
        # A genome FASTA's track is generated once per rank (on its GPU when it has one, inputs.track_on_device) and that one
        # reader serves the mappable lengths and the feed; any other track is opened where it is read.
        if mappability_path is not None and is_fasta(mappability_path):
            track = open_track(mappability_path, track_on_device(mappability_path, False, context),
                               reader_device(context, s.device), k=read_len)
        # (no name in common: ValueError before the cache pass and any table)
        mask, bam = _resolve_regions(s, s.exclude_regions, bam_path, bam)
        _lines, bam = _resolve_regions(s, s.peaks, bam_path, bam)
        if ((s.fingerprint_control is not None or s.coverage_control is not None) and bam is None and is_stream(bam_path)
                and s.estimate_gpu is not None):
            bam = open_alignments(bam_path, True, device=s.estimate_gpu)                # (no header to read apart, as above)
        _check_inputs(s, bam_path, bam)
        known = _mappable_lengths(s, read_len, track, False, mask)
        result, counted = _run_file(s, bam_path, read_len, known, bam, track, mask)
    finally:
        if s.gc_bias is not None:
            s.gc_bias.close()
        if track is not None:
            track.close()
        if bam is not None:
            bam.close()
    written = _write_file(s, bam_path, Path(bam_path).stem, result, read_len, counted) if s.rank == 0 else []
    return result, written


_STAT_OPTS = ("library_length", "smooth_window", "mask_size", "bg_avr_width", "chi2_pval")


@dataclass(frozen=True)
class _Settings:
    """What is constant over one call of run / run_files: its keywords under their own names, checked, with the defaults
    resolved -- ``device`` (this rank's GPU), ``ingest`` (``device_ingest``), ``stat_opts`` (the keywords
    of stats.genome_wide_stats with ``stats``, else None), ``rank`` and ``world``."""
    outdir: object
    max_shift: int
    mapq_criteria: int
    mappability_path: object
    mappability_stats_path: object
    skip_ncc: bool
    references: Optional[Sequence[str]]
    chromfilter: object
    group: object
    context: object
    readlen_estimator: str
    chrom_sizes: object
    complexity: bool
    exclude_regions: object         # None, or the region_mask.ExcludeMask read once for the call
    fingerprint: bool
    fingerprint_bin: int
    fingerprint_extend: int
    fingerprint_control: object     # None, or the _FingerprintControl counted once for the call
    peaks: object                   # None, or the lines of the peak file, read once for the call (peaks.open_peaks)
    peaks_extend: int
    coverage: bool
    coverage_extend: object         # an int (0: every read's own length), or "auto": the run's fragment-length estimate
    coverage_format: str            # "bedgraph" or "bigwig"
    coverage_compress: object       # the sections of a bigWig file through zlib: False, True (on the host) or "device" (on the GPU)
    coverage_bin: int               # the signal track: its bin, the normalisation's word, the caller's factor and
    coverage_normalize: str         # the genome size of "rpgc" (None: the chosen references' lengths); all at their defaults: the
    coverage_scale: float           # depth track
    coverage_genome_size: object
    coverage_control: object        # None, or the _CoverageControl of the call: the track is the treatment against it
    coverage_compare: str           # "log2", "ratio" or "subtract"
    coverage_pseudocount: float
    coverage_call: object           # None, or the cutoff: the peaks of the file's track are written beside it
    coverage_call_gap: int          # the largest gap inside a peak, and the smallest peak
    coverage_call_length: int
    coverage_poisson: bool          # the track is the Poisson -log10 p of the treatment against coverage_control
    coverage_lambda: tuple          # its small and its large window in bases (0: off)
    coverage_qvalue: bool           # the narrowPeak holds the Benjamini-Hochberg q-score of every peak in column 9
    coverage_call_q: object         # None, or X: the peaks are called at pcut(X), the smallest p-score whose q-score reaches X
    gc_bias: object                 # None, or the _GcGenome parsed once for the call
    gc_window: int
    fragments: bool
    fragments_max: int              # the largest fragment size counted, and piled by a "pair" pileup
    tss: object                     # None, or the tss.AnchorSource of the call: read once for every distinct header
    tss_flank: int
    tss_extend: int
    save_mappability_stats: bool
    device: int
    ingest: bool
    stat_opts: Optional[dict]
    stat_kw: dict                   # the keywords of stats.genome_wide_stats, with ``stats`` or without
    rank: int
    world: int

    @property
    def estimate_gpu(self) -> Optional[int]:
        """The GPU of the device reader that one rank estimates the read length on and then feeds the run from; None when the
        host reader estimates (no device ingest, or several ranks: rank 0 estimates for all)."""
        return reader_device(self.context, self.device) if self.world == 1 and self.ingest else None


def _settings(kw: dict) -> _Settings:
    """The settings of one call from the keywords of run / run_files (their ``locals()``).  Bad options raise ValueError
    before any file, context or collective is touched."""
    if kw["references"] is not None and kw["chromfilter"] is not None:
        raise ValueError("give references or chromfilter, not both")
    from .stats import check_params
    check_params(None, kw["library_length"], kw["smooth_window"], kw["max_shift"])
    if kw["read_len"] is None:
        readlen._check_esttype(kw["readlen_estimator"])
    on, rank, world = rank_and_world(kw["group"])
    device = kw["device"]
    if device is None:
        device = int(os.environ.get("LOCAL_RANK", "0")) if on else 0
    _collective_device_setup(device, kw["group"])
    ingest = default_device_ingest(world, kw["context"]) if kw["device_ingest"] is None else kw["device_ingest"]
    given = {f.name: kw[f.name] for f in fields(_Settings) if f.name in kw}
    if kw.get("exclude_regions") is not None:      # read once (on the GPU with device ingest); each file resolves the names
        from .region_mask import open_mask
        given["exclude_regions"] = open_mask(kw["exclude_regions"], bool(ingest), reader_device(kw["context"], device, bool(ingest)))
    if int(kw["peaks_extend"]) < 0:
        raise ValueError("peaks_extend is at least 0")
    if kw["peaks"] is None and int(kw["peaks_extend"]):
        raise ValueError("peaks_extend needs peaks")
    if kw["peaks"] is not None:
        from .peaks import open_peaks
        given["peaks"] = open_peaks(kw["peaks"], bool(ingest), reader_device(kw["context"], device, bool(ingest)))
    given["peaks_extend"] = int(kw["peaks_extend"])
    extend = kw["coverage_extend"]
    if extend not in ("auto", coverage.PAIR) and (isinstance(extend, (str, bool)) or int(extend) != extend or int(extend) < 0):
        raise ValueError("coverage_extend is \"auto\", \"pair\" or an integer of at least 0")
    cutoff, gap, length = kw["coverage_call"], kw["coverage_call_gap"], kw["coverage_call_length"]
    if cutoff is not None:
        cutoff, gap, length = coverage.check_call(cutoff, gap, length)
    call_q = kw["coverage_call_q"]
    if call_q is not None:
        if cutoff is not None:
            raise ValueError("coverage_call_q excludes coverage_call: the cutoff is pcut(coverage_call_q)")
        if not kw["coverage_poisson"]:
            raise ValueError("coverage_call_q needs coverage_poisson: q-scores are made of a p-score track")
        call_q = coverage.check_q(call_q)
        _c, gap, length = coverage.check_call(0.0, gap, length)
    elif cutoff is None and (gap != coverage.CALL_GAP or length != coverage.CALL_LENGTH):
        raise ValueError("coverage_call_gap and coverage_call_length need coverage_call")
    if kw["coverage_qvalue"]:
        if not kw["coverage_poisson"]:
            raise ValueError("coverage_qvalue needs coverage_poisson: q-scores are made of a p-score track")
        if cutoff is None and call_q is None:
            raise ValueError("coverage_qvalue needs coverage_call or coverage_call_q: the q-scores are written with the peaks")
    given.update(coverage_call=cutoff, coverage_call_gap=gap, coverage_call_length=length, coverage_call_q=call_q,
                 coverage_qvalue=bool(kw["coverage_qvalue"]) or call_q is not None)
    given.update(coverage=bool(kw["coverage"]) or kw["coverage_control"] is not None or cutoff is not None or call_q is not None,
                 coverage_extend=extend if extend in ("auto", coverage.PAIR) else int(extend),
                 coverage_format=coverage.check_format(kw["coverage_format"], kw["coverage_compress"]),
                 coverage_compress=coverage.check_compress(kw["coverage_compress"]))
    if given["coverage"] and given["coverage_compress"] == coverage.DEVICE and not ingest:     # (no silent fall-back to zlib)
        raise ValueError("coverage_compress=\"device\" needs device ingest (device_ingest=False reads on the host); "
                         "use coverage_compress=True for zlib on the host")
    normalize = coverage.check_normalize(kw["coverage_normalize"])
    given.update(coverage_bin=coverage.check_bin(kw["coverage_bin"]), coverage_normalize=normalize,
                 coverage_scale=coverage.check_factor(kw["coverage_scale"]),
                 coverage_genome_size=coverage.check_genome_size(kw["coverage_genome_size"], normalize))
    control, op = kw["coverage_control"], coverage.check_compare(kw["coverage_compare"])
    if control is None and (op != "log2" or kw["coverage_pseudocount"] != 1.0):
        raise ValueError("coverage_compare and coverage_pseudocount need coverage_control")
    if control is not None:
        if is_stream(control):
            raise ValueError("coverage_control '{}' is a stream: the control is a regular file, read once per input file".format(control))
        given.update(coverage_control=_CoverageControl(control))
    given.update(coverage_compare=op, coverage_pseudocount=coverage.check_pseudocount(kw["coverage_pseudocount"], op))
    windows = coverage.check_lambda_windows(kw["coverage_lambda"])
    if not kw["coverage_poisson"] and windows != coverage.LAMBDA_WINDOWS:
        raise ValueError("coverage_lambda needs coverage_poisson")
    if kw["coverage_poisson"]:
        if control is None:
            raise ValueError("coverage_poisson needs coverage_control")
        if op != "log2" or kw["coverage_pseudocount"] != 1.0:
            raise ValueError("coverage_poisson excludes coverage_compare and coverage_pseudocount: the score is not a compare operation")
        if normalize != "none" or given["coverage_scale"] != 1.0:
            raise ValueError("coverage_poisson excludes coverage_normalize and coverage_scale: the treatment is not scaled (the score "
                             "counts reads), the control is scaled to the treatment's library size")
    given.update(coverage_poisson=bool(kw["coverage_poisson"]), coverage_lambda=windows)
    given.update(fragments=bool(kw["fragments"]), fragments_max=fragments.check_max_size(kw["fragments_max"]))
    if kw["tss"] is None and (int(kw["tss_flank"]) != tss.DEFAULT_FLANK or int(kw["tss_extend"])):
        raise ValueError("tss_flank and tss_extend need tss")
    given.update(tss_flank=tss.check_flank(kw["tss_flank"]), tss_extend=tss.check_extend(kw["tss_extend"]))
    if kw["tss"] is not None:
        given["tss"] = tss.AnchorSource(kw["tss"], bool(ingest), reader_device(kw["context"], device, bool(ingest)))
    if int(kw["fingerprint_bin"]) < 1 or int(kw["fingerprint_extend"]) < 0:
        raise ValueError("fingerprint_bin is at least 1 and fingerprint_extend at least 0")
    control = kw["fingerprint_control"]
    given.update(fingerprint=bool(kw["fingerprint"]) or control is not None, fingerprint_bin=int(kw["fingerprint_bin"]),
                 fingerprint_extend=int(kw["fingerprint_extend"]),
                 fingerprint_control=None if control is None else _FingerprintControl(control))
    if kw["gc_bias"] is not None or int(kw["gc_window"]) != 100:
        from .gcbias import check_window
        if kw["gc_bias"] is None:
            raise ValueError("gc_window needs gc_bias")
        given.update(gc_bias=_GcGenome(kw["gc_bias"], bool(ingest), reader_device(kw["context"], device, bool(ingest))),
                     gc_window=check_window(kw["gc_window"]))
    stat_kw = {k: kw[k] for k in _STAT_OPTS}
    given.update(device=device, ingest=bool(ingest), rank=rank, world=world, stat_opts=stat_kw if kw["stats"] else None,
                 stat_kw=stat_kw)
    return _Settings(**given)


def _check_coverage_input(s: _Settings, path) -> None:
    """ValueError for a stream whose pileup would need the run's own estimate: it cannot be read a second time."""
    if s.coverage and s.coverage_extend == "auto" and is_stream(path):
        raise ValueError("'{}' is a stream and cannot be read twice: give coverage_extend an integer".format(path))


def _check_pairs_input(s: _Settings, path) -> None:
    """ValueError for a BED read file when the call counts pairs: it has no mate fields."""
    from .bed_reads import is_bed_reads
    if (s.fragments or (s.coverage and s.coverage_extend == coverage.PAIR)) and not is_stream(path) and is_bed_reads(path):
        raise ValueError("'{}' is a BED read file: {}".format(path, fragments.NO_MATES))


def _check_inputs(s: _Settings, path, bam) -> None:
    """ValueError unless the chosen references of ``path`` (``bam``: its open reader, or None: its header is read) are those of
    the fingerprint control and have their records in the genome of ``gc_bias``, and the anchors of ``tss`` can be bound to its
    references, where the call has any of them."""
    if s.fingerprint_control is not None:
        s.fingerprint_control.check(s, path, bam)
    if s.coverage_control is not None:
        s.coverage_control.check(s, path, bam)
    if s.gc_bias is not None:
        s.gc_bias.check(s, path, bam)
    if s.tss is not None:
        _bind_anchors(s, path, bam)


def _bind_anchors(s: _Settings, path, bam) -> None:
    """The anchors of ``tss`` bound to the references of ``path`` before its run (once per distinct header; the count finds them
    bound).  What the BED read readers refuse -- a chromosome the alignment lacks, a strand of ``.`` -- is the file's ValueError, as
    an anchor beyond its chromosome's end is."""
    from .native import PmxIOError
    if bam is not None:
        refs, lengths = bam.references, bam.lengths
    elif is_stream(path):           # (no header to read apart: the count binds them when the stream is armed)
        return
    else:
        with open_header(path, s.chrom_sizes) as h:
            refs, lengths = h.references, h.lengths
    try:
        s.tss.resolve(refs, lengths)
    except PmxIOError as e:
        raise ValueError("anchor file '{}': {}".format(s.tss.source, e.msg)) from e


def _estimate(s: _Settings, path, keep: bool):
    """(read length of ``path``, the reader it was estimated on or None): on the device reader on ``s.estimate_gpu``, handed
    back open with ``keep`` to feed the run too, else on the host reader over the whole file, without its index.  A reader
    that is not handed back is closed, after an error too."""
    gpu = s.estimate_gpu
    if gpu is None:
        r = open_alignments(path, False, index=False, chrom_sizes=s.chrom_sizes)
    else:
        r = open_alignments(path, True, device=gpu, chrom_sizes=s.chrom_sizes)
    back = None
    try:
        length = readlen.estimate_from_reader(r, s.readlen_estimator, s.mapq_criteria, s.max_shift)
        back = r if keep and gpu is not None else None
        return length, back
    finally:
        if back is None:
            r.close()


def _resolve_regions(s: _Settings, regions, path, bam):
    """(``regions`` -- the run's excluded regions or its peak file, a ``region_mask.ExcludeMask`` or None -- bound to the
    references of ``path``: a ``region_mask.ResolvedMask`` or None, the open reader of ``path``).  The references come from
    ``bam`` when the file is open already, else from its header alone (``inputs.open_header``); a stream has no header to read
    apart, so its device reader is opened here and handed back to feed the run.  ValueError when no name of ``regions`` is a
    reference."""
    if regions is None:
        return None, bam
    if bam is None and is_stream(path) and s.estimate_gpu is not None:
        bam = open_alignments(path, True, device=s.estimate_gpu)
    if bam is not None:
        try:
            return regions.resolve(bam.references, bam.lengths), bam
        except BaseException:
            bam.close()
            raise
    if is_stream(path):             # (no device reader: run_sharded says so)
        return regions, bam
    with open_header(path, s.chrom_sizes) as h:
        return regions.resolve(h.references, h.lengths), bam


def _mappable_lengths(s: _Settings, read_len: int, track, unsaved: bool, mask=None):
    """The mappable-length cache (handler/mappability.py:239-309) on every rank, None without a track: loaded when valid;
    otherwise computed ONCE, on rank 0, written atomically with ``save_mappability_stats``, and broadcast -- the other ranks
    neither recompute it per chromosome nor read a file that is being rewritten.  Not valid and not to be saved: computed all
    the same with ``unsaved``, else None (each calculator computes its own in the fused pass).  ``track``: the track's open
    reader, or None for rank 0 to open one on the host.  ``mask``: the excluded regions whose positions are cut out of the
    track first (``_resolve_regions`` of ``exclude_regions``), with a cache of their own."""
    if s.mappability_path is None:
        return None

    def lengths():
        bw = track if track is not None else open_track(s.mappability_path, False)
        try:
            feeder, map_path, masked = bw, s.mappability_stats_path, None
            if mask is not None:    # the track less the regions, with a cache of its own
                from .region_mask import MaskedTrack, stats_path
                feeder, masked = MaskedTrack(bw, mask, read_len), read_len
                if map_path is None:
                    map_path = stats_path(s.mappability_path, s.exclude_regions, getattr(bw, "k", None))
            save = s.save_mappability_stats and (masked is None or map_path is not None)
            ms = MappabilityStats(feeder, s.max_shift, read_len, map_path=map_path,
                                  track_path=s.mappability_path, device=s.device, context=s.context, masked_read_len=masked)
            try:
                if not ms.is_called:                        # no valid cache: the autocorrelation pass
                    if not (save or unsaved):
                        return None
                    ms.calc_mappability()
                    if save:
                        ms.save_mappability_stats()
                return ms.chrom2mappable_len
            finally:
                ms.close()
        finally:
            if bw is not track:
                bw.close()
    return on_rank0(lengths, s.group, "mappability statistics")


def _run_file(s: _Settings, path, read_len: int, known, bam, track, mask=None):
    """One file sharded over the ranks: (its genome-wide result, the counts taken beside it: the _SideCount of every row of
    ``_SIDES`` that is asked for, in that order).  ``known``: the lag tables of _mappable_lengths; ``bam`` / ``track``: the file's
    and the track's open readers, or None for run_sharded to open its own.  One rank: run_sharded's one ``reader_hook`` serves
    every count (``_hooks``)."""
    counted = [row.count(s, row) for row in _SIDES if row.enabled(s)]
    hooks = [c.hook for c in counted if c.hooked]
    result = run_sharded(path, s.max_shift, read_len, s.mapq_criteria, bigwig_path=s.mappability_path,
                         references=s.references, skip_ncc=s.skip_ncc, device=s.device, chrom2mappable_len=known,
                         group=s.group, context=s.context, device_ingest=s.ingest, bam=bam, chromfilter=s.chromfilter,
                         track=track, chrom_sizes=s.chrom_sizes, exclude_regions=mask if mask is not None else s.exclude_regions,
                         reader_hook=_hooks(hooks) if hooks and s.world == 1 else None)
    return result, counted


def _hooks(hooks):
    """One ``reader_hook`` of run_sharded out of several: each is called before the feed, and what they return after it, in order."""
    def hook(reader, names):
        after = [h(reader, names) for h in hooks]

        def after_feed():
            for a in after:
                if a is not None:
                    a()
        return after_feed
    return hook


def _write_file(s: _Settings, path, basename: str, result, read_len: int, counted) -> List[Path]:
    """Rank 0's part after _run_file: ``outdir/<basename>_{cc,mscc,nreads}.tab``, with ``stat_opts`` ``<basename>_stats.tab``
    whose Name row is ``basename``, and the output of every count in ``counted`` (``<basename><suffix>`` of its row of
    ``_SIDES``); the paths written.  The statistics are computed once, for ``_stats.tab`` and for a pileup that extends to their
    estimate."""
    out = Path(s.outdir)
    out.mkdir(parents=True, exist_ok=True)
    # write_tables names the tables after the stem of its path (table.py:185-188): a suffix keeps a dotted base name whole
    written = tables.write_tables(out / (basename + ".bam"), result)
    from . import stats
    memo = []

    def statistics():
        if not memo:
            memo.append(stats.genome_wide_stats(result, read_len, **s.stat_kw))
        return memo[0]
    if s.stat_opts is not None:     # every rank holds the same result: the statistics are rank 0's alone
        written.append(stats.write_stats(out / basename, statistics()))
    for c in counted:
        paths = c.write(path, basename, statistics)     # (the coverage side may write two files)
        written.extend(paths if isinstance(paths, list) else [paths])
    return written


class _SideCount:
    """One count taken beside one file's run, by its row of ``_SIDES``.  ``hook`` is run_sharded's ``reader_hook`` on one rank: the
    count is taken on the reader that feeds the run -- a stream reader (it has the row's ``arm`` method) is armed before the feed
    and counted window by window, any other reader is counted after the feed through the module's ``from_reader``.  ``write``
    writes the table; without a count so far (several ranks) it first counts the chosen chromosomes on one more read of the file,
    through the reader ``inputs.open_alignments`` gives a run of that many ranks (``_count_again``).  ``hooked``: whether the
    count is taken in ``hook``; ``statistics``: the run's statistics, computed when called (``_write_file``)."""
    hooked = True

    def __init__(self, s: _Settings, row):
        self.s, self.row = s, row
        self.value = None

    def _take(self, reader, names, acc=None):
        """The count of ``reader``: what ``acc``, armed before the feed, has summed, else counted now."""
        if acc is not None:
            return acc.result(reader)
        return self.row.module.from_reader(reader, *self.row.args(self.s, names))

    def hook(self, reader, names):
        arm = getattr(reader, self.row.arm, None)       # (a whole-file device reader has none: counted after the feed)
        acc = None if arm is None else arm(*self.row.args(self.s, names))

        def after():
            try:
                self.value = self._take(reader, names, acc)
            finally:
                if acc is not None:
                    reader._disarm(self.row.kind)
        return after

    def write(self, path, basename: str, statistics=None) -> Path:
        s = self.s
        if self.value is None:
            self.value = _count_again(s, path, self._take)
        return self.row.write(s, Path(s.outdir) / basename, basename, self.value)


def _count_again(s: _Settings, path, count):
    """``count(reader, names)`` on one more read of ``path`` through the reader ``inputs.open_alignments`` gives this run, with
    the run's chosen chromosomes and excluded regions (several ranks: rank 0 counts alone and no collective is added)."""
    with open_alignments(path, s.ingest, reader_device(s.context, s.device, s.ingest), chrom_sizes=s.chrom_sizes) as r:
        names = kept_references(r.references, s.references, s.chromfilter)
        if s.exclude_regions is not None:
            r.set_exclude(s.exclude_regions.resolve(r.references, r.lengths))
        return count(r, names)


class _CoverageCount(_SideCount):
    """The fragment pileup of one file's run (pymasc_amd.coverage); its value is (extend, reads, chunks of lines), or the chunks of
    the whole file for a bigWig.  An integer ``coverage_extend`` is counted where every _SideCount is: a host reader's
    ``Coverage`` is kept for ``write``; a device reader's lines are formatted on the GPU while the reader is open and kept in an
    unnamed temporary file in the output directory until ``write`` names them -- for a bigWig the sections, their tables and the
    zoom records are pulled and the file is assembled there.  ``"auto"`` needs the run's statistics, so it is not hooked: ``write``
    counts with ``statistics().est_lib_len`` on one more read of the file (``_count_again``), as several ranks do for an integer,
    and writes while that reader is open.  With ``coverage_call`` the peaks of the track the file holds are called where the pileup
    is taken (``called``: the chunks of their lines; a device reader's are spooled like the track's) and ``write`` returns two
    paths, the coverage file's and ``<basename>_coverage_peaks.narrowPeak``'s."""
    called = None
    hooked = property(lambda self: self.s.coverage_extend != "auto")

    @property
    def signal(self) -> bool:
        """Whether the file holds the signal track: any of its four settings is not the default."""
        s = self.s
        return (s.coverage_bin, s.coverage_normalize, s.coverage_scale, s.coverage_genome_size) != (1, "none", 1.0, None)

    def _scale(self, totals, refs) -> float:
        """The final scale factor from a pileup's totals (by name) and its chosen references."""
        s = self.s
        return coverage.scale_of(s.coverage_normalize, totals["reads"], totals["fragment_bases"], [l for _n, l in refs], s.coverage_scale,
                                 s.coverage_genome_size)

    def _take(self, reader, names, acc=None, extend=None):
        """``extend`` None: the run's integer, and the reader closes before the lines are written: they are spooled."""
        from .bam_device import DeviceBamReader
        spool, mapq = extend is None, int(self.s.mapq_criteria)
        bigwig = self.s.coverage_format == "bigwig"
        if spool:
            extend = self.s.coverage_extend     # (an integer or "pair")
        if not isinstance(reader, DeviceBamReader):
            if bigwig and self.s.coverage_compress == coverage.DEVICE:      # (no silent fall-back to zlib)
                raise ValueError("coverage_compress=\"device\" needs a device reader: this input is read on the host "
                                 "(device_ingest=False or a host reader); use coverage_compress=True for zlib on the host")
            c = coverage.from_reader(reader, mapq, names, extend, self.s.fragments_max)
            tail = ()
            if self.s.coverage_control is not None:
                c = self._against(lambda r, chosen: self._compare_host(c, coverage.from_reader(r, mapq, chosen, extend, self.s.fragments_max)))
                tail = (c.tail,)
            elif self.signal:
                c = c.signal(self.s.coverage_bin, self._scale(dict(zip(coverage.TOTALS, c.totals)), c.refs), self.s.coverage_normalize)
                tail = (c.tail,)
            if self.calls:                          # (of the depth track: through its signal at bin 1 and scale 1.0)
                if self.s.coverage_qvalue:          # (a p-score track: the table, and with coverage_call_q the cutoff from it)
                    qtable = c.qvalues()
                    cutoff = self.s.coverage_call if self.s.coverage_call_q is None else qtable.cutoff(self.s.coverage_call_q)
                    self.called = _Later(c.call(cutoff, *self._call[1:], qtable).text_chunks)
                else:
                    self.called = _Later(c.call(*self._call).text_chunks)
            return self._bigwig(coverage.bigwig_source(c), False) if bigwig else (extend, c.reads, c.text_chunks()) + tail
        if acc is None:             # (an armed count is not built again: its ``begin`` would zero the table)
            acc = coverage.device_count_of(reader, mapq, names, extend, self.s.fragments_max)
        totals = acc.finish(reader)
        reads, signal, tail = totals["reads"], self.signal, ()
        if self.s.coverage_control is not None:     # the control is piled up on a handle of its own; the track stays on this one
            self._against(lambda r, chosen: self._compare_device(acc, reader, r, coverage.device_count_of(
                r, mapq, chosen, extend, self.s.fragments_max)))
            signal, tail = True, (coverage.signal_tail(acc.sig["bin"], acc.sig["normalize"], acc.sig["scale"]) + acc.sig["more"],)
        elif signal:                # the signal runs are made on the handle, beside the depth runs
            acc.signal(reader, self.s.coverage_bin, self._scale(totals, acc.refs), self.s.coverage_normalize)
            tail = (coverage.signal_tail(acc.sig["bin"], acc.sig["normalize"], acc.sig["scale"]),)
        if self.calls:                              # on the track the file holds; the depth track through signal(1, 1.0), and the
            cutoff = self.s.coverage_call           # file is still written from the depth runs.  The lines are few: always spooled
            if self.s.coverage_qvalue:              # (the table beside the p-score runs; with coverage_call_q the cutoff from it)
                acc.qvalue(reader)
                if self.s.coverage_call_q is not None:
                    cutoff = acc.qvalue_cutoff(reader, self.s.coverage_call_q)
            acc.call(reader, cutoff, *self._call[1:])
            fp = self._temporary()
            for chunk in acc.call_text_chunks(reader):
                fp.write(chunk)
            self.called = _spooled(fp)
        if bigwig:
            return self._bigwig(coverage.bigwig_source(acc, reader, signal), True)
        if not spool:
            return (extend, reads, acc.text_chunks(reader, signal=signal)) + tail
        fp = self._temporary()
        for chunk in acc.text_chunks(reader, signal=signal):
            fp.write(chunk)
        return (extend, reads, _spooled(fp)) + tail

    def _against(self, make):
        """``make(reader, names)`` on the control, opened as ``_count_again`` opens a file of this run and closed behind it."""
        return _count_again(self.s, self.s.coverage_control.path, make)

    def _factors(self, totals_t, totals_c, refs):
        s = self.s
        return coverage.factors_of(s.coverage_normalize, totals_t, totals_c, [l for _n, l in refs], s.coverage_scale, s.coverage_genome_size)

    def _compare_host(self, c, control):
        s = self.s
        a_t, a_c = self._factors(dict(zip(coverage.TOTALS, c.totals)), dict(zip(coverage.TOTALS, control.totals)), c.refs)
        if s.coverage_poisson:
            return c.poisson(control, s.coverage_bin, a_c, *s.coverage_lambda, s.coverage_control.path)
        return c.compare(control, s.coverage_bin, s.coverage_compare, a_t, a_c, s.coverage_pseudocount, s.coverage_normalize,
                         s.coverage_control.path)

    def _compare_device(self, acc, reader, control_reader, control_acc):
        from .bam_device import DeviceBamReader
        s = self.s
        if not isinstance(control_reader, DeviceBamReader):
            raise ValueError("the coverage control '{}' is read on the host and the input on the device".format(s.coverage_control.path))
        a_t, a_c = self._factors(acc.finish(reader), control_acc.finish(control_reader), acc.refs)
        if s.coverage_poisson:
            acc.poisson(reader, control_acc, control_reader, s.coverage_bin, a_c, *s.coverage_lambda, s.coverage_control.path)
            return
        acc.compare(reader, control_acc, control_reader, s.coverage_bin, s.coverage_compare, a_t, a_c, s.coverage_pseudocount,
                    s.coverage_normalize, s.coverage_control.path)

    def _temporary(self):
        import tempfile
        Path(self.s.outdir).mkdir(parents=True, exist_ok=True)
        return tempfile.TemporaryFile(dir=str(self.s.outdir))

    def _bigwig(self, source, now: bool):
        """The chunks of the bigWig file of ``source``; ``now``: assembled at once (the source's reader is open only now)."""
        def chunks():
            fp = self._temporary()
            try:
                coverage.assemble_bigwig(fp, source, self.s.coverage_compress)
            except BaseException:
                fp.close()
                raise
            return _spooled(fp)
        if not now:
            return _Later(chunks)
        done = chunks()
        return _Later(lambda: done)

    _call = property(lambda self: (self.s.coverage_call, self.s.coverage_call_gap, self.s.coverage_call_length))
    calls = property(lambda self: self.s.coverage_call is not None or self.s.coverage_call_q is not None)

    def _write(self, base, basename: str, value):
        """The coverage file; with ``coverage_call`` [it, ``<basename>_coverage_peaks.narrowPeak``] (the lines ``_take`` left)."""
        track = self.row.write(self.s, base, basename, value)
        if not self.calls:
            return track
        return [track, coverage.write_called(base, self.called)]

    def write(self, path, basename: str, statistics=None):
        s = self.s
        base = Path(s.outdir) / basename
        if self.value is not None:
            return self._write(base, basename, self.value)
        extend = int(statistics().est_lib_len) if s.coverage_extend == "auto" else s.coverage_extend
        return _count_again(s, path, lambda r, names: self._write(base, basename, self._take(r, names, None, extend)))


class _Later:
    """Chunks of bytes that are made when they are first asked for."""

    def __init__(self, make):
        self.make = make

    def __iter__(self):
        return iter(self.make())


def _write_coverage(s: _Settings, base, basename: str, value) -> Path:
    if s.coverage_format == "bigwig":
        return coverage.write_file(str(base) + coverage.BIGWIG_SUFFIX, value)
    return coverage.write_track(base, basename, *value)


def _spooled(fp, size: int = 1 << 22):
    """The bytes of the temporary file ``fp`` from its beginning, ``size`` at a time; closes (and so removes) it at the end."""
    try:
        fp.seek(0)
        while True:
            chunk = fp.read(size)
            if not chunk:
                return
            yield chunk
    finally:
        fp.close()


def _write_fingerprint(s: _Settings, base, basename: str, value) -> Path:
    control = s.fingerprint_control
    return fingerprint.write_fingerprint(base, basename, value, None if control is None else control.counts(s),
                                         "" if control is None else control.path)


_Side = namedtuple("_Side", "kind enabled suffix module args arm write count", defaults=(_SideCount,))
_Side.__doc__ = """One count taken beside the correlation: ``kind`` (its name in ``native.SIDE_KINDS``), ``enabled(s)``, the
``suffix`` of its output (or a function of the settings that gives it), its ``module`` (``from_reader``), ``args(s, names)`` -- what ``from_reader`` takes after the reader, and
the stream reader's ``arm`` method (named here) takes --, ``write(s, base, basename, value)`` and the class that takes it."""

#: every side count, in the order the outputs are written and listed (that of ``native.SIDE_KINDS``)
_SIDES = (
    _Side("complexity", lambda s: s.complexity, complexity.COMPLEXITY_SUFFIX, complexity,
          lambda s, names: (int(s.mapq_criteria), names), "arm_complexity",
          lambda s, base, basename, value: complexity.write_complexity(base, basename, value)),
    _Side("fingerprint", lambda s: s.fingerprint, fingerprint.FINGERPRINT_SUFFIX, fingerprint,
          lambda s, names: (int(s.mapq_criteria), names, s.fingerprint_bin, s.fingerprint_extend), "arm_fingerprint",
          _write_fingerprint),
    _Side("peaks", lambda s: s.peaks is not None, peaks.PEAKS_SUFFIX, peaks,
          lambda s, names: (s.peaks, int(s.mapq_criteria), names, s.peaks_extend), "arm_peaks",
          lambda s, base, basename, value: peaks.write_peaks(base, basename, value, s.peaks.source or "")),
    _Side("coverage", lambda s: s.coverage, lambda s: coverage.SUFFIXES[s.coverage_format], coverage,
          lambda s, names: (int(s.mapq_criteria), names, s.coverage_extend, s.fragments_max), "arm_coverage",
          _write_coverage, _CoverageCount),
    _Side("gcbias", lambda s: s.gc_bias is not None, gcbias.GCBIAS_SUFFIX, gcbias,      # (the genome is parsed when first needed)
          lambda s, names: (s.gc_bias.open(), int(s.mapq_criteria), names, s.gc_window), "arm_gcbias",
          lambda s, base, basename, value: gcbias.write_gcbias(base, basename, value)),
    _Side("fragments", lambda s: s.fragments, fragments.FRAGMENTS_SUFFIX, fragments,
          lambda s, names: (int(s.mapq_criteria), names, s.fragments_max), "arm_fragments",
          lambda s, base, basename, value: fragments.write_fragments(base, basename, value)),
    _Side("tss", lambda s: s.tss is not None, tss.TSS_SUFFIX, tss,
          lambda s, names: (s.tss, int(s.mapq_criteria), names, s.tss_flank, s.tss_extend), "arm_tss",
          lambda s, base, basename, value: tss.write_tss(base, basename, value, s.tss.source)),
)


class GenomeError(RuntimeError):
    """``gc_bias`` names a FASTA file that cannot be read or parsed: the call fails, as it does for a bad track."""


class _GcGenome:
    """``gc_bias``: the genome of a call's GC tables, parsed once, when the first file needs it (``open``: a
    ``gcbias.DeviceGenome`` with device ingest, else a ``gcbias.HostGenome``) and closed with the call.  ``check`` compares a
    file's chosen references with its records before the run: ValueError in ``pmx_dbam_gcbias_begin``'s words."""

    def __init__(self, path, ingest: bool, device: int):
        self.path, self.ingest, self.device = os.fspath(path), ingest, device
        self._genome = None

    def open(self):
        if self._genome is None:
            from . import gcbias
            from .native import PmxIOError
            try:
                self._genome = gcbias.open_genome(self.path, self.ingest, self.device)
            except (PmxIOError, OSError, ValueError) as e:
                logger.error("Failed to read the genome '{}'".format(self.path))
                logger.error(str(e))
                raise GenomeError(str(e)) from e
        return self._genome

    def close(self) -> None:
        if self._genome is not None and hasattr(self._genome, "close"):
            self._genome.close()
        self._genome = None

    def check(self, s: _Settings, path, bam) -> None:
        from .gcbias import match_references
        # the genome is opened before anything here can raise ValueError: run_files takes a ValueError of this check as the
        # file's (skipped) and relies on a FASTA that cannot be parsed raising GenomeError, the call's, whichever file is first
        genome = self.open()
        if bam is not None:
            refs, lengths = bam.references, bam.lengths
        elif is_stream(path):       # (no header to read apart: pmx_dbam_gcbias_begin says the same when the stream is armed)
            return
        else:
            with open_header(path, s.chrom_sizes) as h:
                refs, lengths = h.references, h.lengths
        chosen = set(kept_references(refs, s.references, s.chromfilter))
        match_references(refs, lengths, [n in chosen for n in refs], dict(zip(genome.names, genome.lengths)))


class _FingerprintControl:
    """``fingerprint_control``: the control file of a call's fingerprints.  ``check`` compares its chosen references with a
    sample's from the headers alone; ``counts`` is its table, counted once per call (by rank 0, when the first table is written)
    with the run's ``mapq_criteria``, chromosome filter, excluded regions and ``chrom_sizes``.  It is never correlated."""
    label = "fingerprint control"       # what ``check`` calls the file

    def __init__(self, path):
        self.path = os.fspath(path)
        self._chosen = None
        self._counts = None

    def _chosen_of(self, s: _Settings, header):
        names = set(kept_references(header.references, s.references, s.chromfilter))
        return [(n, int(l)) for n, l in zip(header.references, header.lengths) if n in names]

    def check(self, s: _Settings, path, reader=None) -> None:
        """ValueError unless the chosen references of ``path`` (``reader``: its open reader, else its header is read) have the
        names and lengths of the control's."""
        if self._chosen is None:
            with open_header(self.path, s.chrom_sizes) as h:
                self._chosen = self._chosen_of(s, h)
        if reader is not None:
            mine = self._chosen_of(s, reader)
        elif is_stream(path):       # (no device reader to read it: run_sharded says so)
            return
        else:
            with open_header(path, s.chrom_sizes) as h:
                mine = self._chosen_of(s, h)
        if mine != self._chosen:
            raise ValueError("the chosen references of the {} '{}' differ from those of '{}' in name or length"
                             "".format(self.label, self.path, path))

    def counts(self, s: _Settings):
        from . import fingerprint
        if self._counts is None:
            self._counts = _count_again(s, self.path, lambda r, names: fingerprint.from_reader(
                r, int(s.mapq_criteria), names, s.fingerprint_bin, s.fingerprint_extend))
        return self._counts


class _CoverageControl(_FingerprintControl):
    """``coverage_control``: the control file of a call's compared tracks, checked from the headers as the
    fingerprint's is.  It is piled up again for every file (``_CoverageCount._against``): nothing of it is kept between files."""
    label = "coverage control"


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
              complexity: bool = False, exclude_regions=None, fingerprint: bool = False, fingerprint_bin: int = 500,
              fingerprint_extend: int = 0, fingerprint_control=None, peaks=None, peaks_extend: int = 0, coverage: bool = False,
              coverage_extend="auto", gc_bias=None, gc_window: int = 100, fragments: bool = False,
              fragments_max: int = 2000, tss=None, tss_flank: int = 2000, tss_extend: int = 0,
              coverage_format: str = "bedgraph", coverage_compress=False, coverage_bin: int = 1, coverage_normalize: str = "none",
              coverage_scale: float = 1.0, coverage_genome_size: Optional[int] = None, coverage_control=None,
              coverage_compare: str = "log2", coverage_pseudocount: float = 1.0, coverage_call=None, coverage_call_gap: int = 30,
              coverage_call_length: int = 200, coverage_poisson: bool = False, coverage_lambda=(1000, 10000),
              coverage_qvalue: bool = False, coverage_call_q=None) -> List[FileResult]:
    """``run`` over several alignment files in one call, as ``pymasc a.bam b.bam -n A B`` runs them; returns one FileResult per
    file, in input order.  Every keyword means what it means for ``run``; a file that is skipped gets no table.

    ``names``: PyMaSC's -n, paired with the files by position (a missing or None name: ``Path(file).stem``, so that a file
    without a name gets exactly what ``run`` writes for it); a name ``N`` gives ``N_cc.tab`` ... ``N_stats.tab``, whole even
    when it holds a dot.  A BED read file without ``chrom_sizes`` is skipped in step 1 with run's ValueError, and BAM / SAM
    files keep their header's lengths (logged once when ``chrom_sizes`` is given beside them).  More names than files, an
    empty name or one with a path separator, and two files with the same base name are a ValueError before any work, as bad
    options are.  Outputs that exist already are warned about first (pymasc.py:178-182).

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
    rank 0 writes inside ``sharding.on_rank0``, so that a write error reaches every rank (``written`` is [] on the others).

    ``gc_bias``: the genome is parsed once, before the first file runs, and serves every file; a file whose chosen references
    have no record of their name and length in it is logged and skipped; a FASTA that cannot be parsed raises ``GenomeError``.
    ``fragments`` / ``coverage_extend="pair"``: a BED read file has no mate fields and is skipped in step 1 with run's ValueError.
    ``tss``: the anchors are bound to every file's references before its run; a file whose references they do not match is logged
    and skipped with its ValueError, and the other files go on."""
    paths = list(paths)
    if not paths:
        raise ValueError("no input files")
    bases = _basenames(paths, names)
    s = _settings(locals())
    from .bed_reads import is_bed_reads
    from .kmer_track import is_fasta
    if s.rank == 0:
        _warn_existing(s, bases)
        if chrom_sizes is not None and not all(is_bed_reads(p) for p in paths):
            logger.info("The chromosome sizes are used for BED read files only: BAM and SAM files keep their header's lengths.")
    dev = reader_device(context, s.device, s.ingest)

    errors: List[Optional[BaseException]] = [None] * len(paths)
    kept = {}                       # index -> device reader opened in _choose that feeds that file's run too
    own_ctx, track = False, None
    try:
        if s.world == 1:
            read_len, kept = _choose(s, paths, errors, read_len)
        else:                       # rank 0 decides, every rank learns the same (none waits for a value that never comes)
            def choose():
                errs: List[Optional[BaseException]] = [None] * len(paths)
                rl, _k = _choose(s, paths, errs, read_len)
                return rl, [None if e is None else _portable(e) for e in errs]
            read_len, errors = on_rank0(choose, group, "choosing the input files")
        if read_len is None:
            raise ValueError("no input file is left to run")
        live = [i for i, e in enumerate(errors) if e is None]
        if context is None:
            s, own_ctx = replace(s, context=ffi.Context(s.device)), True
        if mappability_path is not None:        # (a genome FASTA: its k-mer track with k = the read length)
            track = open_track(mappability_path, track_on_device(mappability_path, s.ingest, s.context),
                               getattr(s.context, "device", dev) if is_fasta(mappability_path) else dev, k=read_len)

        def skip(i, e, bam=None):
            """A file that fails a check before its run is logged and left out like one that cannot be opened."""
            if bam is not None:
                bam.close()
            logger.error("Failed to open file '{}'".format(paths[i]))
            logger.error(str(e))
            errors[i] = _portable(e)
        # the excluded regions are bound to every file's references before the cache pass: a file none of whose references the
        # mask names is skipped like a file that cannot be opened; the cache is cut with the first file's clipped intervals.
        # The peak file is bound the same way: a file none of whose references it names is skipped too.
        masks = {}
        for i in list(live):
            try:
                masks[i], kept_i = _resolve_regions(s, s.exclude_regions, paths[i], kept.get(i))
                if kept_i is not None:
                    kept[i] = kept_i
                _lines, kept_i = _resolve_regions(s, s.peaks, paths[i], kept.get(i))
                if kept_i is not None:
                    kept[i] = kept_i
            except ValueError as e:
                kept.pop(i, None)
                skip(i, e)
                live.remove(i)
        if not live:
            raise ValueError("no input file is left to run")
        known = _mappable_lengths(s, read_len, track, True, masks[live[0]])     # the lag tables of every file, computed once
        logger.info("Calculate cross-correlation between 0 to {} base shift with reads MAPQ >= {}"
                    "".format(max_shift, mapq_criteria))
        results = {}
        for i in live:
            logger.info("Process {}".format(paths[i]))
            bam = kept.pop(i, None)
            # from the headers, the same on every rank: a control or a genome of another assembly skips the file like one that
            # does not open (ValueError); a FASTA that cannot be parsed is the call's error (GenomeError is none: it propagates)
            try:
                _check_inputs(s, paths[i], bam)
            except ValueError as e:
                skip(i, e, bam)
                continue
            try:
                result, counted = _run_file(s, paths[i], read_len, known, bam, track, masks[i])
            except Exception as e:
                unsorted = _unsorted_on_every_rank(e, s.world)
                if unsorted is None:
                    raise
                logger.error("Reads of '{}' are not sorted by position: the file is skipped ({})".format(paths[i], unsorted))
                errors[i] = unsorted
                continue
            finally:
                if bam is not None:
                    bam.close()
            written = on_rank0(lambda: _write_file(s, paths[i], bases[i], result, read_len, counted), group,
                               "writing the outputs of '{}'".format(paths[i]))
            results[i] = (result, list(written) if s.rank == 0 else [])
    finally:
        for r in kept.values():
            r.close()
        if s.gc_bias is not None:
            s.gc_bias.close()
        if track is not None:
            track.close()
        if own_ctx:
            s.context.close()
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


def _warn_existing(s: _Settings, bases):
    """prepare_output's warning (pymasc.py:178-182) for every output about to be replaced."""
    has_track = s.mappability_path is not None
    suffixes = [x for x, on in (("_cc.tab", not (has_track and s.skip_ncc)), ("_mscc.tab", has_track), ("_nreads.tab", True),
                                ("_stats.tab", s.stat_opts is not None)) if on]
    suffixes += [row.suffix(s) if callable(row.suffix) else row.suffix for row in _SIDES if row.enabled(s)]
    if s.coverage_call is not None or s.coverage_call_q is not None:
        suffixes.append(coverage.CALL_SUFFIX)
    for b in bases:
        for suffix in suffixes:
            path = Path(s.outdir) / (b + suffix)
            if path.exists():
                logger.warning("Existing file '{}' will be overwritten.".format(path))


def _choose(s: _Settings, paths, errors, read_len):
    """Steps 1 and 2 of run_files: the files that open and keep a chromosome, then the common read length.  Fills ``errors``
    with the exception of every file skipped; returns (read length or None when no file is left, {index: device reader} of
    the readers opened here that feed their file's run).  A stream (inputs.is_stream: ``-``, a FIFO) is opened once, here, by
    the stream reader, which then feeds its run; without ``read_len`` it is skipped before a byte of it is read (PyMaSC:
    handler/calc.py:81, pymasc.py:199-201), and without the device reader (``s.estimate_gpu`` None) too.  A BED read file
    takes its references from ``chrom_sizes`` (inputs.open_header); without them it is skipped here."""
    device = s.estimate_gpu
    kept = {}
    for i, p in enumerate(paths):
        stream = is_stream(p)
        if stream and read_len is None:
            logger.error("Cannot execute read length checking for unseekable input.")
            logger.error("If your input can't reread, specify read length using `-r` option.")
            errors[i] = InputUnseekable("'{}' is not seekable: give the read length".format(p))
            continue
        if stream and s.coverage and s.coverage_extend == "auto":
            logger.error("Failed to open file '{}'".format(p))
            logger.error("A stream cannot be read twice: give --coverage-extend a number or 'read'.")
            try:
                _check_coverage_input(s, p)
            except ValueError as e:
                errors[i] = e
            continue
        try:
            _check_pairs_input(s, p)
        except ValueError as e:
            logger.error("Failed to open file '{}'".format(p))
            logger.error(str(e))
            errors[i] = e
            continue
        if stream and device is None:
            logger.error("Failed to open file '{}'".format(p))
            logger.error("A stream input is read by the device reader only: one process on a GPU.")
            errors[i] = ValueError("'{}' is a stream: it needs the device reader".format(p))
            continue
        try:
            r = open_alignments(p, True, device=device) if stream else open_header(p, s.chrom_sizes)
            try:
                if not r.references:
                    raise ValueError("File has no sequences defined.")
                filter_references(r.references, s.chromfilter)
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
    logger.info("Check read length: Get {} from read length distribution".format(str(s.readlen_estimator).lower()))
    lengths = []
    for i in live:
        logger.info("Check read length... : {}".format(paths[i]))
        try:                        # (one live file: its device reader feeds its run too)
            length, r = _estimate(s, paths[i], len(live) == 1)
        except ValueError as e:
            logger.error(str(e))
            errors[i] = e
            continue
        lengths.append(length)
        if r is not None:
            kept[i] = r
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
