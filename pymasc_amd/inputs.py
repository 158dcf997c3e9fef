"""Which reader a run reads its input through: the one place that chooses between the host readers (libpymasc_io.so) and
the device readers (libpymasc_ingest.so) of an alignment file -- BAM, SAM (pymasc_amd.sam) or BED reads (pymasc_amd.bed_reads) -- and
of a mappability track: BigWig or bigBed, or text (pymasc_amd.text_track).

The reader modules import ``find_index`` from here, so they are imported inside the openers, and the device classes are
looked up through their module each time (a test may replace ``bam_device.DeviceBamReader``).
"""
from __future__ import annotations

import os


def find_index(path):
    """``<path>.bai`` or ``<stem>.bai``, as pysam looks for it; None when neither exists."""
    path = os.fspath(path)
    for cand in (path + ".bai", os.path.splitext(path)[0] + ".bai"):
        if os.path.exists(cand):
            return cand
    return None


def default_device_ingest(world: int, context=None) -> bool:
    """The default of ``device_ingest``: the input is inflated and decoded on the GPU when this is the only rank and it runs
    on a real GPU (``context`` None or a pymasc_amd.ffi.Context).  False when the device count cannot be read."""
    from . import ffi
    if world != 1 or not (context is None or isinstance(context, ffi.Context)):
        return False
    try:
        return ffi.device_count() > 0
    except Exception:
        return False


def is_stream(path) -> bool:
    """An input read as a stream: ``-`` (standard input) or a path that is not a regular file -- a FIFO,
    ``/dev/fd/N`` of a pipe, a character device."""
    from .stream_device import is_stream_path
    return is_stream_path(path)


#: free device bytes kept back when the whole-file device reader is chosen (the calculator's pool and the track live there too)
DEVICE_INGEST_MARGIN = 4 << 30


def device_ingest_budget(device: int = 0) -> int:
    """Free bytes of ``device`` (hipMemGetInfo through torch) that the whole-file device reader may use; a test replaces it."""
    import torch
    free, _total = torch.cuda.mem_get_info(device)
    return int(free) - DEVICE_INGEST_MARGIN


def whole_file_footprint(path) -> int:
    """Device bytes the whole-file reader needs for a BAM file of this size: the compressed copy, the inflated stream at the
    bound its output buffer is allocated for (6x), and the kept-record arrays (13 bytes per record of >= 36 bytes)."""
    fsize = os.path.getsize(path)
    inflated = 6 * fsize
    return fsize + inflated + 13 * (inflated // 36)


def reader_device(context, device, device_ingest: bool = True) -> int:
    """The GPU of a run's device readers: the one of ``context`` when the run has one and ingests on the device (a genome
    FASTA's track goes there whatever the ingest: its callers leave ``device_ingest`` True), else ``device`` (None: 0)."""
    if context is not None and device_ingest:
        return context.device
    return device or 0


def check_bed_sizes(path, chrom_sizes) -> None:
    """A BED read file (``bed_reads.is_bed_reads``) needs ``chrom_sizes``: ValueError without them, before any work."""
    from .bed_reads import is_bed_reads
    if chrom_sizes is None and is_bed_reads(path):
        raise ValueError("'{}' is a BED read file: give the chromosome sizes (chrom_sizes=, --chrom-sizes)".format(os.fspath(path)))


def bed_sizes(path, chrom_sizes):
    """(references, lengths) of a BED read file (``bed_reads.is_bed_reads``) from ``chrom_sizes``; ValueError without them."""
    from .bed_reads import chrom_sizes_of
    check_bed_sizes(path, chrom_sizes)
    return chrom_sizes_of(chrom_sizes)


def open_alignments(path, device_ingest: bool, device: int = 0, references=None, index=None, chrom_sizes=None):
    """The reader of an alignment file: ``DeviceSamReader`` / ``DeviceBamReader`` on ``device`` with ``device_ingest``, else
    ``SamReader`` / ``BamReader``.  ``references`` and ``index`` as ``DeviceBamReader`` takes them (the host readers read the
    whole file and leave the choice of chromosomes to ``feed``); ``index=False`` also opens the host BAM reader without its
    .bai, as a read-length estimate over the whole file wants it.  A stream (``is_stream``) is read by
    ``DeviceStreamReader`` and needs ``device_ingest``; so is a whole BAM file whose footprint (``whole_file_footprint``)
    exceeds ``device_ingest_budget``, where the whole-file reader would fail to allocate.  A BED read file
    (``bed_reads.is_bed_reads``: named .tagAlign / .bed) is read by ``DeviceBedReadsReader`` / ``BedReadsReader`` with the
    references of ``chrom_sizes`` (a path or an ordered ``{name: length}``; ValueError without them), never as a stream
    (DESIGN.md 7.11); other files do not use ``chrom_sizes``."""
    from . import bam, bam_device, bed_reads, sam, stream_device
    if bed_reads.is_bed_reads(path):
        names, lengths = bed_sizes(path, chrom_sizes)
        if is_stream(path):
            raise ValueError("'{}' is a BED read file: it is sorted whole, so it cannot be read as a stream".format(os.fspath(path)))
        if device_ingest:
            return bed_reads.DeviceBedReadsReader(path, names, lengths, device=device, select=references)
        return bed_reads.BedReadsReader(path, names, lengths)
    if is_stream(path):
        if not device_ingest:
            raise ValueError("'{}' is a stream: it is read by the device reader only (one rank, a GPU)".format(os.fspath(path)))
        return stream_device.DeviceStreamReader(path, device=device, references=references)
    is_sam = sam.is_sam(path)
    if device_ingest:
        if not is_sam and (references is None or index is False or find_index(path) is None) \
                and whole_file_footprint(path) > device_ingest_budget(device):
            return stream_device.DeviceStreamReader(path, device=device, references=references)
        cls = sam.DeviceSamReader if is_sam else bam_device.DeviceBamReader
        return cls(path, device=device, references=references, index=index)
    return sam.SamReader(path) if is_sam else bam.BamReader(path, index=index)


def open_header(path, chrom_sizes=None):
    """The host reader of an alignment file with its header read and no record: ``references`` / ``lengths``.  A BAM file's
    open reads the header only (its records are read by ``feed``); a SAM file is opened with ``header_only``; a BED read file
    gives the references of ``chrom_sizes`` once it is found readable (``bed_reads.SizesHeader``; none of it is read)."""
    from . import bam, bed_reads, sam
    if bed_reads.is_bed_reads(path):
        return bed_reads.SizesHeader(path, *bed_sizes(path, chrom_sizes))
    return sam.SamReader(path, header_only=True) if sam.is_sam(path) else bam.BamReader(path, index=False)


def track_on_device(path, device_ingest: bool, context=None) -> bool:
    """Where a run's track is read: a genome FASTA (``kmer_track.is_fasta``) on the GPU whenever this rank has a GPU context
    (``context`` None or a pymasc_amd.ffi.Context, and a device visible) -- uniqueness is genome-wide, so every rank generates
    the whole track on its own device, never on the host; any other track where ``device_ingest`` says."""
    from . import ffi, kmer_track
    if not kmer_track.is_fasta(path):
        return bool(device_ingest)
    if not (context is None or isinstance(context, ffi.Context)):
        return False
    try:
        return ffi.device_count() > 0
    except Exception:
        return False


def open_track(path, device_ingest: bool, device: int = 0, k=None):
    """The reader of a mappability track: a BigWig file (``text_track.is_bigwig``: the bbi magic or a .bw / .bigwig name) or a
    bigBed file (``text_track.is_bigbed``: the bigBed magic or a .bb / .bigbed name) is read by
    ``DeviceBigWigReader`` on ``device`` with ``device_ingest``, else ``BigWigReader``; a genome FASTA (``kmer_track.is_fasta``:
    .fa / .fasta / .fna / .fas, optionally .gz / .bgz) becomes its k-mer uniqueness track with ``k`` = the read length
    (``DeviceKmerTrackReader`` / ``KmerTrackReader``; ValueError without ``k``); any other file is a text track
    (bedGraph, BED, WIG; plain, BGZF or gzip) read by ``DeviceTextTrackReader`` / ``TextTrackReader``.  Tracks
    other than FASTA ignore ``k``."""
    from . import bigwig, bigwig_device, kmer_track, text_track
    if kmer_track.is_fasta(path):
        if k is None:
            raise ValueError("'{}' is a genome FASTA: its track needs the k-mer length (the read length)".format(os.fspath(path)))
        return kmer_track.open_kmer_track(path, k, device_ingest, device)
    if text_track.is_bigwig(path) or text_track.is_bigbed(path):
        if device_ingest:
            return bigwig_device.DeviceBigWigReader(path, device=device)
        return bigwig.BigWigReader(path)
    if device_ingest:
        return text_track.DeviceTextTrackReader(path, device=device)
    return text_track.TextTrackReader(path)
