"""Text mappability tracks -- bedGraph, BED and WIG, plain, BGZF or gzip -- read as BigWig tracks are.

``TextTrackReader`` (libpymasc_io.so, pmx_ttrack_*) and ``DeviceTextTrackReader`` (libpymasc_ingest.so, pmx_dtt_open) have the
surface of ``BigWigReader`` / ``DeviceBigWigReader``: ``chromsizes``, ``fetch(valfilter, chrom)``, ``fetch_arrays`` (and, on the
device, ``fetch_device``), ``close``.  A text track has no chromosome sizes: ``chromsizes`` holds the largest end of each
chromosome's lines, and ``chromsizes_are_extents`` says so.  ``sorted``: the intervals of the last fetch are ascending and
disjoint.  ``is_bigwig`` and ``is_bigbed`` are the rules that send a file to the bbi (BigWig) readers instead.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Iterator, Tuple

import numpy as np

from .bam import NativeReader, PmxIOError, _raise, load_io_library  # noqa: F401  (PmxIOError re-exported)
from .bam_device import load_ingest_library
from .bigwig_device import DeviceBigWigReader
from .bigwig_device import _raise as _raise_device

PMX_IO_ERR_NOTFOUND = -4
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


class TextTrackReader(NativeReader):
    _CLOSE = "pmx_ttrack_close"
    chromsizes_are_extents = True

    def __init__(self, path, threads: int = 0):
        path_str = os.fspath(path)
        if not os.path.exists(path_str):
            raise IOError("input file '{0}' dose not exist.".format(path_str))
        self._L = load_io_library()
        self.path = path_str
        h = ctypes.c_void_p()
        rc = self._L.pmx_ttrack_open(path_str.encode(), int(threads), ctypes.byref(h))
        if rc:
            _raise(rc)
        self._h = h
        n = self._L.pmx_ttrack_nchrom(h)
        self.chromsizes: Dict[str, int] = {
            self._L.pmx_ttrack_chrom_name(h, i).decode(): int(self._L.pmx_ttrack_chrom_len(h, i)) for i in range(n)}

    @property
    def sorted(self) -> bool:
        return bool(self._L.pmx_ttrack_sorted(self._h))

    def fetch_arrays(self, valfilter: float, chrom: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(begin, end, value) arrays of the chromosome's lines with value >= valfilter, in file order."""
        if self.closed:
            raise ValueError("I/O operation on closed track reader")
        if chrom not in self.chromsizes:
            raise KeyError(chrom)
        name = chrom.encode()
        n = self._L.pmx_ttrack_fetch(self._h, name, float(valfilter), 0, None, None, None)
        if n == PMX_IO_ERR_NOTFOUND:
            raise KeyError(chrom)
        if n < 0:
            _raise(n)
        begin = np.empty(n, dtype=np.uint32)
        end = np.empty(n, dtype=np.uint32)
        value = np.empty(n, dtype=np.float32)
        if n:
            m = self._L.pmx_ttrack_fetch(self._h, name, float(valfilter), n, begin.ctypes.data, end.ctypes.data,
                                         value.ctypes.data)
            if m < 0:
                _raise(m)
            assert m == n
        return begin, end, value

    def fetch(self, valfilter: float, chrom: str) -> Iterator[Tuple[int, int, float]]:
        begin, end, value = self.fetch_arrays(valfilter, chrom)
        return iter(zip(begin.tolist(), end.tolist(), value.tolist()))

    def disable_progress_bar(self) -> None:
        pass


class DeviceTextTrackReader(DeviceBigWigReader):
    """The text is copied (or inflated) to HBM and parsed there; the handle is a pmx_dbw, so ``fetch_device``,
    ``fetch_arrays`` and ``fetch`` are DeviceBigWigReader's.  No host fallback: without a GPU the constructor raises."""
    chromsizes_are_extents = True

    def __init__(self, path, device: int = 0, threads: int = 0):
        path_str = os.fspath(path)
        if not os.path.exists(path_str):
            raise IOError("input file '{0}' dose not exist.".format(path_str))
        self._L = load_ingest_library()
        self.path = path_str
        h = ctypes.c_void_p()
        rc = self._L.pmx_dtt_open(path_str.encode(), int(device), int(threads), ctypes.byref(h))
        if rc:
            _raise_device(rc)
        self._h = h
        n = self._L.pmx_dbw_nchrom(h)
        self.chromsizes: Dict[str, int] = {self._L.pmx_dbw_chrom_name(h, i).decode(): int(self._L.pmx_dbw_chrom_len(h, i))
                                           for i in range(n)}

    @property
    def sorted(self) -> bool:
        return bool(self._L.pmx_dbw_sorted(self._h))
