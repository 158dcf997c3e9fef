"""BigWig mappability track reader over libpymasc_io.so.

Same surface as the reference's BigWigReader (PyMaSC/reader/bigwig.pyx:100-200): ``chromsizes``,
``fetch(valfilter, chrom)`` -> iterator of ``(begin, end, value)`` (KeyError for an unknown chromosome, intervals
with value >= valfilter only when valfilter > 0), ``disable_progress_bar``, ``close`` -- so it drops into
``CCHipCalculator(bwfeeder=...)`` and ``MappabilityStats(feeder=...)`` where the reference passes its own reader.
``fetch_arrays`` is the bulk form the calculator prefers: numpy arrays straight into ``pmx_bits_set_regions``.
A bigBed file (the same bbi container) is read by the same reader: its records are intervals of value 1;
``kind`` tells the two apart.
"""
from __future__ import annotations

from .native import HostTrackReader, PmxIOError, existing_path, load_io_library  # noqa: F401  (PmxIOError re-exported)


class BigWigReader(HostTrackReader):
    _WHAT = "BigWig reader"

    def __init__(self, path):
        self.path = existing_path(path)
        self._L = load_io_library()
        self._attach(self._open_handle("pmx_bigwig_open", self.path.encode()))
