"""SAM input (SAM spec v1 section 1), plain or BGZF-compressed (``bgzip``): what PyMaSC accepts besides BAM.

* ``detect_format(path)`` tells BAM from SAM text without reading more than the first BGZF member (or 64 KB);
* ``SamReader`` (host, libpymasc_io.so ``pmx_sam_*``) has ``BamReader``'s surface: the whole text is indexed and parsed at open
  on the reader's threads; it is the checker of the device reader, the path without a GPU and the path of a rank of several;
* ``DeviceSamReader`` (libpymasc_ingest.so ``pmx_dsam_open``) is a ``DeviceBamReader`` whose stream is the text: the line index,
  the parse, the filter and the read-length histogram are HIP kernels over the text in HBM.

Both give for a SAM file exactly what the BAM readers give for its BAM twin: the same records, runs, read-length histogram and
counters; only the first-occurrence keys differ (byte offsets of lines in the text instead of records in the BAM stream).
"""
from __future__ import annotations

import os
import zlib
from typing import Iterator, Tuple

import numpy as np

from .bam import feed_bam
from .bam_device import DeviceBamReader
from .native import PMX_BAM_DEFAULT_EXCLUDE, AlignmentReader, PmxIOError, load_ingest_library, load_io_library

_PROBE = 65536


def _is_bgzf(head: bytes) -> bool:
    """The gzip member at the front of ``head`` has the BGZF 'BC' subfield in its extra field (SAM spec 4.1)."""
    if len(head) < 18 or not head[3] & 4:
        return False
    x, end = 12, min(12 + (head[10] | head[11] << 8), len(head))
    while x + 4 <= end:
        if head[x:x + 2] == b"BC":
            return True
        x += 4 + (head[x + 2] | head[x + 3] << 8)
    return False


def detect_format(path) -> str:
    """``"bam"``, ``"sam"`` (plain text) or ``"sam.bgzf"`` (bgzip'd text).  Text whose first byte is '@' is SAM; a BGZF file whose
    first member inflates to text starting with '@' is BGZF SAM; everything else is ``"bam"`` and goes to the BAM readers, which
    report what is wrong with it as before.  A plain-gzip SAM file raises ``PmxIOError``: htslib reads it, this project asks
    for ``bgzip``."""
    try:
        with open(os.fspath(path), "rb") as fh:
            head = fh.read(_PROBE)
    except OSError:
        return "bam"                # (the BAM reader reports it, as before)
    if head[:1] == b"@":
        return "sam"
    if head[:3] != b"\x1f\x8b\x08":
        return "bam"
    try:                            # the first byte of the first member (a BGZF member is a gzip member)
        text = zlib.decompressobj(16 + 15).decompress(head, 1)
    except zlib.error:
        return "bam"
    if text[:1] != b"@":
        return "bam"
    if not _is_bgzf(head):
        raise PmxIOError(-2, "{}: gzip-compressed SAM that is not BGZF: recompress it with bgzip".format(os.fspath(path)))
    return "sam.bgzf"


def is_sam(path) -> bool:
    return detect_format(path) != "bam"


class SamReader(AlignmentReader):
    """A SAM file (plain or BGZF) as batches of filtered read arrays, like ``pymasc_amd.bam.BamReader``; no index."""
    _P = "pmx_sam"
    _WHAT = "SAM reader"
    _COUNTERS = ("records", "kept", "bytes_out", "bytes_in", "members")

    def __init__(self, path, threads: int = 0, header_only: bool = False):
        """``header_only``: read the header and no record (pmx_sam_open_header) -- ``references``, ``lengths`` and
        ``header_text`` only; a plain file is read to its first record line, a BGZF one inflated until it."""
        self._L = load_io_library()
        self.path = os.fspath(path)
        if header_only:
            self._h = self._open_handle("pmx_sam_open_header", self.path.encode())
        else:
            self._h = self._open_handle("pmx_sam_open", self.path.encode(), int(threads))
        self._load_references()

    def has_index(self) -> bool:
        return False

    def counters(self) -> dict:
        """records (alignment lines), kept (last decode), bytes_out (text), bytes_in (file), members (BGZF), rewalked (0):
        the keys of ``DeviceBamReader.counters``."""
        out = super().counters()
        out["rewalked"] = 0
        return out

    def feed(self, calculator, mapq_criteria: int, references=None, finish: bool = True) -> int:
        """``pymasc_amd.bam.feed_bam`` over this reader."""
        return feed_bam(calculator, self, mapq_criteria, references, finish)

    def batches(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE,
                batch: int = 1 << 22) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        """Yields (ref_id, pos_1based, read_len, is_reverse) of the reads that pass the reference's filter, in file order."""
        total = self.decode(mapq_criteria, flag_exclude)
        self._dropped = 0
        for first in range(0, total, batch):
            yield self._drop_excluded(*self._fetch(first, min(batch, total - first)))

    def mate_batches(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, batch: int = 1 << 22):
        """``BamReader.mate_batches`` for the text: (ref_id, pos_1based, read_len, is_reverse, flag, mate_ref_id, mate_pos_1based,
        tlen) by ``pmx_sam_fetch_mates``; a PNEXT or TLEN that is no decimal integer raises ``PmxIOError`` with ``line N: ...``."""
        total = self.decode(mapq_criteria, flag_exclude)
        for first in range(0, total, batch):
            n = min(batch, total - first)
            flag, mref, mpos, tlen = (np.empty(n, dtype=t) for t in (np.uint16, np.int32, np.int32, np.int32))
            rc = self._L.pmx_sam_fetch_mates(self._h, first, n, flag.ctypes.data, mref.ctypes.data, mpos.ctypes.data, tlen.ctypes.data)
            if rc:
                self._raise(rc)
            yield self._fetch(first, n) + (flag, mref, mpos, tlen)

    def fetch(self, reference: str, *args, **kwargs):
        raise ValueError("fetch() needs an index: {} is a SAM file".format(self.path))


class DeviceSamReader(DeviceBamReader):
    """A SAM file (plain or BGZF) copied to HBM and parsed there; the surface of ``DeviceBamReader`` (its stream is the text).
    ``references`` selects records as for a BAM file without an index; ``select`` works the same way."""

    def __init__(self, path, device: int = 0, threads: int = 0, references=None, index=None):
        self._L = load_ingest_library()
        self.path = os.fspath(path)
        self.indexed = False
        self._attach(self._open_handle("pmx_dsam_open", self.path.encode(), int(device), int(threads)), references)
