"""BAM ingest for the calculator: native reader binding + the feeding loop.

Host mirror of what the reference does between the file and the calculator:

* ``BamReader`` has the surface of the reference's BAMFileProcessor that the calculation touches
  (PyMaSC/reader/bam.py:84-165: ``references``, ``lengths``, ``close``, context manager) over
  libpymasc_io.so's BGZF/BAM reader (include/pymasc_amd_io.h) instead of pysam.
* ``feed_bam`` is the single-process loop of PyMaSC/handler/calc.py:131-161 with the read filter and field
  extraction of handler/read.py:62-155 done natively and in bulk: records arrive as arrays in file order, are cut
  into runs of one chromosome and handed to ``CCHipCalculator.feed_reads`` (which applies the sortedness and
  duplicate rules of mscc.pyx:351-418), then ``finishup_calculation``.
"""
from __future__ import annotations

import os
from typing import Iterator, Optional, Sequence, Tuple

import numpy as np

from .inputs import find_index
from .native import (IO_PROTOTYPES, PMX_BAM_DEFAULT_EXCLUDE, PMX_BAM_FLAG_DUPLICATE, PMX_BAM_FLAG_READ2,  # noqa: F401
                     PMX_BAM_FLAG_REVERSE, PMX_BAM_FLAG_UNMAPPED, AlignmentReader, NativeReader, PmxIOError, load_io_library)

#: every symbol include/pymasc_amd_io.h declares (tests/test_abi.py checks the built library against this list)
IO_EXPORTS = list(IO_PROTOTYPES)


class BamReader(AlignmentReader):
    """A coordinate-sorted BAM file as batches of filtered read arrays."""
    _P = "pmx_bam"
    _COUNTERS = ("records", "kept", "bytes_out", "bytes_in")

    def __init__(self, path, threads: int = 0, index=None):
        """``index``: path of the .bai; None: ``<path>.bai`` or ``<stem>.bai`` when present (like pysam); False: none."""
        self._L = load_io_library()
        self.path = os.fspath(path)
        self._h = h = self._open_handle("pmx_bam_open", self.path.encode(), int(threads))
        self._load_references()
        if index is None:
            index = find_index(self.path)
        if index:
            rc = self._L.pmx_bam_index_load(h, os.fspath(index).encode())
            if rc:
                self.close()
                self._raise(rc)

    def has_index(self) -> bool:
        """reader/bam.py:128-135."""
        return bool(self._L.pmx_bam_has_index(self._h))

    def fetch(self, reference: str, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE,
              batch: int = 1 << 22) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        """The reads of ONE reference through the .bai index, as ``batches`` yields them -- what a worker of the
        reference's multi-process mode gets from ``AlignmentFile.fetch(chrom)`` (handler/worker.py:106-132)."""
        self._check_open()
        if reference not in self.references:
            raise KeyError(reference)
        if not self.has_index():
            raise ValueError("fetch() needs an index: {}.bai not found".format(self.path))
        rc = self._L.pmx_bam_fetch_ref(self._h, self.references.index(reference))
        if rc:
            self._raise(rc)
        return self.batches(mapq_criteria, flag_exclude, batch, _region=True)

    def feed(self, calculator, mapq_criteria: int, references: Optional[Sequence[str]] = None, finish: bool = True) -> int:
        """``feed_bam`` over this reader, as ``DeviceBamReader.feed`` is over the device reader."""
        return feed_bam(calculator, self, mapq_criteria, references, finish)

    def batches(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, batch: int = 1 << 22,
                _region: bool = False) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        """Yields (ref_id, pos_1based, read_len, is_reverse) of the reads that pass the reference's filter
        (handler/read.py:62-90,131-141), in file order, at most ``batch`` per round."""
        self._check_open()
        if not _region:      # a plain pass always starts at the first record, whatever was fetched before
            self._dropped = 0
            rc = self._L.pmx_bam_fetch_ref(self._h, -1)
            if rc:
                self._raise(rc)
        ref = np.empty(batch, dtype=np.int32)
        pos = np.empty(batch, dtype=np.int32)
        rlen = np.empty(batch, dtype=np.int32)
        rev = np.empty(batch, dtype=np.uint8)
        while True:
            n = self._L.pmx_bam_next_batch(self._h, int(mapq_criteria), int(flag_exclude), batch, ref.ctypes.data,
                                           pos.ctypes.data, rlen.ctypes.data, rev.ctypes.data)
            if n < 0:
                self._raise(n)
            if n == 0:
                return
            yield self._drop_excluded(ref[:n].copy(), pos[:n].copy(), rlen[:n].copy(), rev[:n].astype(bool))

    def mate_batches(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, batch: int = 1 << 22):
        """``batches`` with four raw columns more (``pmx_bam_next_mates``): yields (ref_id, pos_1based, read_len, is_reverse, flag,
        mate_ref_id, mate_pos_1based, tlen) of the reads that pass the filter, in file order.  The reader's mask is not applied:
        a pair is masked by its fragment's extent (``fragments.rows_host``)."""
        self._check_open()
        rc = self._L.pmx_bam_fetch_ref(self._h, -1)
        if rc:
            self._raise(rc)
        cols = [np.empty(batch, dtype=t) for t in (np.int32, np.int32, np.int32, np.uint8, np.uint16, np.int32, np.int32, np.int32)]
        while True:
            n = self._L.pmx_bam_next_mates(self._h, int(mapq_criteria), int(flag_exclude), batch, *[c.ctypes.data for c in cols])
            if n < 0:
                self._raise(n)
            if n == 0:
                return
            out = [c[:n].copy() for c in cols]
            out[3] = out[3].astype(bool)
            yield tuple(out)


def feed_bam(calculator, reader: BamReader, mapq_criteria: int, references: Optional[Sequence[str]] = None,
             finish: bool = True, use_index: Optional[bool] = None) -> int:
    """Stream every usable read of ``reader`` into ``calculator`` (handler/calc.py:131-161).

    ``references``: the chromosomes taken into account (config.references, calc.py:143-144); default: the
    calculator's.  ``use_index``: read only those chromosomes through the .bai (default: when an index is loaded
    and fewer than all references are wanted -- a rank of a multi-GPU run); otherwise one pass over the file.
    Returns the number of reads fed.  Raises what the calculator raises (ReadUnsortedError for unsorted input,
    mscc.pyx:351-364)."""
    names = reader.references
    wanted = set(calculator.references if references is None else references)
    use = np.array([n in wanted for n in names], dtype=bool)
    if use_index is None:
        use_index = reader.has_index() and not use.all()
    fed = 0
    dropped = 0                                             # (a pass through the index restarts the reader's count per chromosome)

    def feed(ref, pos, rlen, rev):
        cuts = np.flatnonzero(np.diff(ref)) + 1           # runs of one chromosome, in file order
        starts = np.concatenate(([0], cuts))
        ends = np.concatenate((cuts, [ref.size]))
        for s, e in zip(starts.tolist(), ends.tolist()):
            calculator.feed_reads(names[int(ref[s])], pos[s:e], rlen[s:e], rev[s:e])
        return int(ref.size)

    if use_index:
        for name in (n for n in names if n in wanted):    # file order = header order for a sorted BAM
            reader._dropped = 0
            for ref, pos, rlen, rev in reader.fetch(name, mapq_criteria):
                if ref.size:
                    fed += feed(ref, pos, rlen, rev)
            dropped += reader.excluded()
        reader._dropped = dropped
    else:
        for ref, pos, rlen, rev in reader.batches(mapq_criteria):
            if not use.all():
                m = use[ref]
                ref, pos, rlen, rev = ref[m], pos[m], rlen[m], rev[m]
            if ref.size:
                fed += feed(ref, pos, rlen, rev)
    if finish:
        calculator.finishup_calculation()
    return fed
