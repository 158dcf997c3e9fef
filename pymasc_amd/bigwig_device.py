"""BigWig (bbi) ingest ON THE DEVICE: binding of the pmx_dbw_* entry points of libpymasc_ingest.so.

``DeviceBigWigReader`` has the surface of ``pymasc_amd.bigwig.BigWigReader`` -- the part of the reference's
PyMaSC/reader/bigwig.pyx the calculation touches: ``chromsizes``, ``fetch(valfilter, chrom)``, ``fetch_arrays``, ``close`` -- plus
``fetch_device``, which leaves a chromosome's intervals in HBM for ``CCHipCalculator`` to build its mappability vector from
(pmx_bits_set_regions_dev_ex).  The file is copied to the GPU once; data blocks are inflated (the BGZF kernel), Adler-32-checked and
decoded by HIP kernels.  No host fallback: without a GPU the constructor raises.  A bigBed file is read by the same reader
(``kind == "bigbed"``; k_bb_records decodes its records).
"""
from __future__ import annotations

import ctypes
from typing import Tuple

import numpy as np

from .native import PMX_IO_ERR_NOTFOUND, TrackReader, existing_path, load_ingest_library


class DeviceBigWigReader(TrackReader):
    _P = "pmx_dbw"
    _WHAT = "BigWig reader"

    def __init__(self, path, device: int = 0, threads: int = 0):
        self.path = existing_path(path)
        self._L = load_ingest_library()
        self._attach(self._open_handle("pmx_dbw_open", self.path.encode(), int(device), int(threads)))

    def fetch_device(self, valfilter: float, chrom: str) -> Tuple[int, int, int, bool]:
        """The chromosome's intervals with value >= valfilter, left in device memory: (address of uint32 begin[], address of
        uint32 end[], count, sorted and disjoint?) -- valid until the next fetch on this reader."""
        self._check_chrom(chrom)
        n = self._L.pmx_dbw_fetch(self._h, chrom.encode(), float(valfilter))
        if n == PMX_IO_ERR_NOTFOUND:
            raise KeyError(chrom)
        if n < 0:
            self._raise(n)
        b, e, v = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
        rc = self._L.pmx_dbw_device_arrays(self._h, ctypes.byref(b), ctypes.byref(e), ctypes.byref(v))
        if rc:
            self._raise(rc)
        return int(b.value or 0), int(e.value or 0), int(n), self.sorted

    def fetch_arrays(self, valfilter: float, chrom: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(begin, end, value) host arrays, as BigWigReader.fetch_arrays."""
        _b, _e, n, _s = self.fetch_device(valfilter, chrom)
        begin = np.empty(n, dtype=np.uint32)
        end = np.empty(n, dtype=np.uint32)
        value = np.empty(n, dtype=np.float32)
        if n:
            rc = self._L.pmx_dbw_copy(self._h, 0, n, begin.ctypes.data, end.ctypes.data, value.ctypes.data)
            if rc:
                self._raise(rc)
        return begin, end, value
