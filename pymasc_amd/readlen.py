"""Read-length estimation from the BAM file (PyMaSC core/readlen.pyx:estimate_readlen, handler/calc.py:74-98).

What ``pymasc`` does when ``-r/--read-length`` is left out: a histogram of the query lengths of the file's records under the
ESTIMATOR's filter (not the calculation's: read2, secondary, supplementary and QC-fail records count here), reduced to one
integer by ``--readlen-estimator`` (MEAN / MEDIAN / MODE / MIN / MAX).  The histogram is built natively -- on the GPU by one
more walk over the record chain the device reader keeps in HBM (include/pymasc_amd_ingest.h, pmx_dbam_readlen_hist), on host
threads by the host reader (include/pymasc_amd_io.h, pmx_bam_readlen_hist) -- and reduced here with Python's own arithmetic,
so the result is the reference's bit for bit.  One deliberate divergence: a record without a query length
(no CIGAR, or only H/D/N/P operations) is not counted but reported in ``nnoqlen``; the reference puts None in its counter and
fails on it.
"""
from __future__ import annotations

import ctypes
import logging
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

logger = logging.getLogger(__name__)

#: the reference's ESTFUNCTIONS (readlen.pyx:84-86), in the order its --readlen-estimator help lists them
ESTIMATORS = ("MEAN", "MEDIAN", "MODE", "MIN", "MAX")
COUNTER_NAMES = ("nreads", "nunmapped", "ncounted", "npaired", "nread2", "nnoqlen")


def _check_esttype(esttype) -> str:
    name = str(esttype).upper()                     # case-insensitive, as the reference's _make_upper
    if name not in ESTIMATORS:
        raise ValueError("unknown read length estimator {!r}: one of {}".format(esttype, ", ".join(ESTIMATORS)))
    return name


@dataclass
class ReadLengthHistogram:
    """Distinct counted lengths in ascending order, their counts, and the file-order key of each length's first counted
    record (the reference's counter is a dict in first-insertion order; MODE breaks ties by it)."""
    lengths: np.ndarray                 # int64 [k], ascending
    counts: np.ndarray                  # int64 [k]
    first: np.ndarray                   # uint64 [k]: offset of the first counted record of that length
    counters: Dict[str, int] = field(default_factory=dict)
    mapq_criteria: int = 0

    @property
    def ncounted(self) -> int:
        return int(self.counts.sum()) if self.counts.size else 0

    def as_counter(self) -> Dict[int, int]:
        """{length: count} in the reference's dict order (first counted occurrence in the file)."""
        order = np.argsort(self.first, kind="stable")
        return {int(self.lengths[i]): int(self.counts[i]) for i in order}

    def estimate(self, esttype="MEDIAN") -> int:
        """The reference's reduction (readlen.pyx:27-86) with Python's rules: float64 division and round-half-to-even."""
        name = _check_esttype(esttype)
        if self.counts.size == 0:
            raise ValueError("no reads to estimate the read length from")
        lens = [int(x) for x in self.lengths]
        cnts = [int(x) for x in self.counts]
        if name == "MIN":
            return lens[0]
        if name == "MAX":
            return lens[-1]
        if name == "MEAN":                          # _mean: int(round(sum(l * c) / float(sum(c))))
            return int(round(sum(l * c for l, c in zip(lens, cnts)) / float(sum(cnts))))
        if name == "MODE":                          # _mode: stable sort by count of the first-insertion-ordered items, last one
            items = sorted(zip((int(x) for x in self.first), lens, cnts))
            return sorted(((l, c) for _f, l, c in items), key=lambda x: x[1])[-1][0]
        num = sum(cnts)                             # _median
        target = num / 2
        run = 0
        for i, (l, c) in enumerate(zip(lens, cnts)):
            run += c
            if num % 2:
                if target <= run:
                    return l
            elif target < run:
                return l
            elif target == run:
                return int(round((l + float(lens[i + 1])) / 2))
        raise AssertionError("unreachable: the running sum reaches the total")


def histogram_from_library(fn_hist, fn_counters, handle, mapq_criteria: int, raise_error) -> ReadLengthHistogram:
    """Two-call protocol of pmx_bam_readlen_hist / pmx_dbam_readlen_hist (same signature) + the counters."""
    n = fn_hist(handle, int(mapq_criteria), 0, None, None, None)
    if n < 0:
        raise_error(n)
    lengths = np.empty(max(n, 1), dtype=np.int32)
    counts = np.empty(max(n, 1), dtype=np.uint64)
    first = np.empty(max(n, 1), dtype=np.uint64)
    m = fn_hist(handle, int(mapq_criteria), n, lengths.ctypes.data, counts.ctypes.data, first.ctypes.data)
    if m < 0:
        raise_error(m)
    c = (ctypes.c_uint64 * 6)()
    rc = fn_counters(handle, c)
    if rc:
        raise_error(rc)
    return ReadLengthHistogram(lengths[:m].astype(np.int64), counts[:m].astype(np.int64), first[:m].copy(),
                               dict(zip(COUNTER_NAMES, (int(x) for x in c))), int(mapq_criteria))


def estimate_from_reader(reader, esttype="MEDIAN", mapq_criteria: int = 0, max_shift: Optional[int] = None) -> int:
    """The estimate on an open alignment reader (pymasc_amd.inputs.open_alignments), with the reference's log lines
    (readlen.pyx:167-175) and its check against the shift size (handler/calc.py:93-98)."""
    name = _check_esttype(esttype)
    hist = reader.read_length_histogram(mapq_criteria)
    length = hist.estimate(name)
    c = hist.counters
    logger.info("Scan {:,} reads, {:,} reads were unmapped and {:,} reads >= MAPQ {}."
                "".format(c["nreads"], c["nunmapped"], c["ncounted"], mapq_criteria))
    if c["nnoqlen"]:
        logger.info("{:,} reads >= MAPQ {} had no query length and were not counted.".format(c["nnoqlen"], mapq_criteria))
    if c["npaired"] > 0:
        logger.info("{:,} reads were paired: {:,} reads were 1st and {:,} reads were last segment."
                    "".format(c["npaired"], c["npaired"] - c["nread2"], c["nread2"]))
        logger.info("Note that only 1st reads in the templates will be used for calculation.")
    else:
        logger.info("All reads were single-ended.")
    logger.info("Estimated read length = {:,}".format(length))
    if max_shift is not None and length > max_shift:
        raise ValueError("Read length ({}) seems to be longer than shift size ({}).".format(length, max_shift))
    return length


def estimate_readlen(path, esttype, mapq_criteria, max_shift: Optional[int] = None, device: Optional[int] = None) -> int:
    """Drop-in for PyMaSC.core.readlen.estimate_readlen(path, esttype, mapq_criteria) (handler/calc.py:87): the file is read
    by the device reader when there is a GPU, by the host reader otherwise; a SAM file (pymasc_amd.sam) by the SAM readers.  ``max_shift``: also the check of
    handler/calc.py:93-98 (ValueError when the estimate is longer).  ``device``: the GPU (default 0); None with no GPU."""
    from .inputs import default_device_ingest, open_alignments
    name = _check_esttype(esttype)
    logger.info("Check read length... : {}".format(path))
    with open_alignments(path, default_device_ingest(1), device=device or 0, index=False) as reader:
        return estimate_from_reader(reader, name, int(mapq_criteria), max_shift)
