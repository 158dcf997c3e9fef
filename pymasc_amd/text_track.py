"""Text mappability tracks -- bedGraph, BED and WIG, plain, BGZF or gzip -- read as BigWig tracks are.

``TextTrackReader`` (libpymasc_io.so, pmx_ttrack_open) and ``DeviceTextTrackReader`` (libpymasc_ingest.so, pmx_dtt_open) have the
surface of ``BigWigReader`` / ``DeviceBigWigReader``: ``chromsizes``, ``fetch(valfilter, chrom)``, ``fetch_arrays`` (and, on the
device, ``fetch_device``), ``close``.  A text track has no chromosome sizes: ``chromsizes`` holds the largest end of each
chromosome's lines, and ``chromsizes_are_extents`` says so.  ``sorted``: the intervals of the last fetch are ascending and
disjoint.  ``is_bigwig`` and ``is_bigbed`` are the rules that send a file to the bbi (BigWig) readers instead.
"""
from __future__ import annotations

import os

from .bigwig_device import DeviceBigWigReader
from .native import (HostTrackReader, PmxIOError, existing_path, load_ingest_library,  # noqa: F401  (PmxIOError re-exported)
                     load_io_library)

BBI_MAGIC = (0x888FFC26).to_bytes(4, "little")
BIGBED_MAGIC = (0x8789F2EB).to_bytes(4, "little")


def is_bigwig(path) -> bool:
    """A BigWig file: its first four bytes are the bbi magic, or its name ends in .bw / .bigwig (any case) -- such a file goes
    to the BigWig readers, whose errors (a bad "magic") stay as they are.  Every other file is a text track."""
    p = os.fspath(path)
    if p.lower().endswith((".bw", ".bigwig")):
        return True
    try:
        with open(p, "rb") as fh:
            return fh.read(4) == BBI_MAGIC
    except OSError:
        return False


def is_bigbed(path) -> bool:
    """A bigBed file: its first four bytes are the bigBed magic, or its name ends in .bb / .bigbed (any case) -- read by the
    BigWig readers, which take both kinds of bbi file."""
    p = os.fspath(path)
    if p.lower().endswith((".bb", ".bigbed")):
        return True
    try:
        with open(p, "rb") as fh:
            return fh.read(4) == BIGBED_MAGIC
    except OSError:
        return False


class TextTrackReader(HostTrackReader):
    chromsizes_are_extents = True

    def __init__(self, path, threads: int = 0):
        self.path = existing_path(path)
        self._L = load_io_library()
        self._attach(self._open_handle("pmx_ttrack_open", self.path.encode(), int(threads)))


class DeviceTextTrackReader(DeviceBigWigReader):
    """The text is copied (or inflated) to HBM and parsed there; the handle is a pmx_dbw, so ``fetch_device``,
    ``fetch_arrays`` and ``fetch`` are DeviceBigWigReader's.  No host fallback: without a GPU the constructor raises."""
    chromsizes_are_extents = True

    def __init__(self, path, device: int = 0, threads: int = 0):
        self.path = existing_path(path)
        self._L = load_ingest_library()
        self._attach(self._open_handle("pmx_dtt_open", self.path.encode(), int(device), int(threads)))
