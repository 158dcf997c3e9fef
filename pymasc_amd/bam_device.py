"""BAM ingest ON THE DEVICE: binding of libpymasc_ingest.so (include/pymasc_amd_ingest.h).

``DeviceBamReader`` has the surface of ``pymasc_amd.bam.BamReader`` (itself the part of the reference's
BAMFileProcessor the calculation touches, PyMaSC/reader/bam.py:84-165) -- ``references``, ``lengths``, ``batches``,
``fetch``, ``close`` -- so ``pymasc_amd.bam.feed_bam`` takes either; the difference is where the work happens: the whole
file is copied to HBM compressed, and BGZF inflate, CRC32, the record chain and the reference's read filter
(handler/read.py:62-155) run as HIP kernels.  There is no host fallback: without a GPU ``DeviceBamReader`` raises.
With ``references`` and a .bai, only the BGZF members of those references are read, copied and inflated.
"""
from __future__ import annotations

import ctypes
import os
from typing import Iterator, Tuple

import numpy as np

from .inputs import find_index
from .native import INGEST_PROTOTYPES, PMX_BAM_DEFAULT_EXCLUDE, AlignmentReader, load_ingest_library

#: every symbol include/pymasc_amd_ingest.h declares (tests/test_abi.py checks the built library against this list)
INGEST_EXPORTS = list(INGEST_PROTOTYPES)


class UnknownReferenceError(ValueError, KeyError):
    """A reference name the BAM header does not hold (a ValueError; a KeyError too, as ``fetch`` raised before)."""


class DeviceBamReader(AlignmentReader):
    """A BAM file inflated and decoded on the GPU; batches of filtered read arrays like ``BamReader``.

    ``references``: None reads the whole file (every reference selected).  A list of names with an index present (``index``:
    its path; None: ``<path>.bai`` / ``<stem>.bai``; False: none) reads only the BGZF members of those references
    (``pmx_dbam_open_indexed`` + ``pmx_dbam_select``); without an index the whole file is read and the selection is applied to
    the records.  ``select(names)`` replaces the selection (the two-step use: open with ``references=[]``, read the header,
    choose).  ``references`` / ``lengths`` always list the whole header; ``selected`` the chosen names in header order."""
    _P = "pmx_dbam"
    _COUNTERS = ("records", "kept", "bytes_out", "bytes_in", "members", "rewalked")

    def __init__(self, path, device: int = 0, threads: int = 0, references=None, index=None):
        self._L = load_ingest_library()
        self.path = os.fspath(path)
        if references is not None and index is not False:
            index = find_index(self.path) if index is None else os.fspath(index)
        else:
            index = None
        self.indexed = index is not None
        if self.indexed:
            h = self._open_handle("pmx_dbam_open_indexed", self.path.encode(), index.encode(), int(device), int(threads))
        else:
            h = self._open_handle("pmx_dbam_open", self.path.encode(), int(device), int(threads))
        self._attach(h, references)

    def _attach(self, h, references) -> None:
        """The handle of an open: the header's references, then the selection."""
        self._h = h
        self._load_references()
        self._selected = frozenset(range(len(self.references)))
        if references is not None:
            references = [references] if isinstance(references, str) else list(references)
            try:
                if self.indexed and not references:
                    self._selected = frozenset()     # (the open read the header only: nothing to select yet)
                else:
                    self.select(references)
            except BaseException:
                self.close()
                raise

    def _ids(self, names):
        if isinstance(names, str):
            names = [names]
        ids = []
        for name in names:
            if name not in self.references:
                raise UnknownReferenceError(name)
            ids.append(self.references.index(name))
        return ids

    def select(self, names) -> None:
        """Only the records of ``names`` from now on.  An indexed reader reads, copies and inflates just their BGZF members
        (the stream is replaced; ``counters()`` counts what was read); an unknown name raises ValueError."""
        self._check_open()
        ids = sorted(set(self._ids(names)))
        if self.indexed:
            arr = (ctypes.c_int32 * max(len(ids), 1))(*ids)
            rc = self._L.pmx_dbam_select(self._h, arr, len(ids))
            if rc:
                self._selected = frozenset()
                self._raise(rc)
        self._selected = frozenset(ids)

    @property
    def selected(self) -> Tuple[str, ...]:
        return tuple(n for i, n in enumerate(self.references) if i in self._selected)

    def _check_selected(self, names):
        for i, name in zip(self._ids(names), names):
            if i not in self._selected:
                raise ValueError("reference {} was not selected".format(name))

    def set_exclude(self, mask) -> None:
        """``AlignmentReader.set_exclude`` on the device: the mask's lines go to ``pmx_dbam_set_exclude``, which clips, sorts and
        merges them in HBM; every later ``decode`` (``feed``, ``batches``, each window of a stream) and ``library_complexity``
        leaves the overlapping reads out on the GPU."""
        self._check_open()
        if mask is None:
            rc = self._L.pmx_dbam_set_exclude(self._h, 0, None, None, None)
        else:
            offsets, begin, end = mask.csr()
            rc = self._L.pmx_dbam_set_exclude(self._h, len(mask.references), offsets.ctypes.data, begin.ctypes.data if begin.size else None,
                                              end.ctypes.data if end.size else None)
        if rc:
            self._raise(rc)
        self._exclude = mask
        self._dropped = 0

    def exclude_intervals(self):
        """(ref_id int32, begin uint32, end uint32) of the merged intervals the library holds, in (reference, begin) order."""
        self._check_open()
        n = self._L.pmx_dbam_exclude_intervals(self._h, 0, None, None, None)
        if n < 0:
            self._raise(n)
        ref, begin, end = np.empty(max(n, 1), np.int32), np.empty(max(n, 1), np.uint32), np.empty(max(n, 1), np.uint32)
        m = self._L.pmx_dbam_exclude_intervals(self._h, n, ref.ctypes.data, begin.ctypes.data, end.ctypes.data)
        if m < 0:
            self._raise(m)
        return ref[:m], begin[:m], end[:m]

    def decode(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, reference: int = -1) -> int:
        n = super().decode(mapq_criteria, flag_exclude, reference)
        if self._exclude is not None:       # (the count of this decode: pmx_dbam_excluded; a stream's windows add up)
            d = ctypes.c_uint64()
            rc = self._L.pmx_dbam_excluded(self._h, ctypes.byref(d), None)
            if rc:
                self._raise(rc)
            self._dropped += int(d.value)
        return n

    def has_index(self) -> bool:
        """Every selected reference can be fetched on its own (its records are resident): no .bai needed for that."""
        return True

    def timings(self) -> dict:
        t = (ctypes.c_double * 6)()
        rc = self._L.pmx_dbam_timings(self._h, t)
        if rc:
            self._raise(rc)
        return dict(zip(("upload_s", "inflate_s", "crc_s", "header_s", "chain_s", "write_s"), (float(x) for x in t)))

    def inflated(self, first: int = 0, n: int = None) -> bytes:
        """(test hook) bytes of the inflated stream."""
        if n is None:
            n = self.counters()["bytes_out"] - first
        buf = np.empty(max(n, 1), dtype=np.uint8)
        rc = self._L.pmx_dbam_inflated(self._h, int(first), int(n), buf.ctypes.data)
        if rc:
            self._raise(rc)
        return buf[:n].tobytes()

    def device_arrays(self) -> Tuple[int, int, int, int]:
        """Device addresses of (ref_id int32, pos1 int32, read_len int32, reverse uint8) of the last decode."""
        v = [ctypes.c_void_p() for _ in range(4)]
        rc = self._L.pmx_dbam_device_arrays(self._h, *[ctypes.byref(x) for x in v])
        if rc:
            self._raise(rc)
        return tuple(int(x.value or 0) for x in v)

    def device_runs(self):
        """The kept records of the last decode as runs of one reference, in file order: a list of
        (ref_id, start index, count, first pos, last pos) -- None when the file has more than 65536 runs (unsorted)."""
        n = self._L.pmx_dbam_runs(self._h, 0, None, None, None, None)
        if n == -3:
            return None
        if n < 0:
            self._raise(n)
        start = np.empty(max(n, 1), dtype=np.int64)
        ref = np.empty(max(n, 1), dtype=np.int32)
        first = np.empty(max(n, 1), dtype=np.int32)
        last = np.empty(max(n, 1), dtype=np.int32)
        m = self._L.pmx_dbam_runs(self._h, n, start.ctypes.data, ref.ctypes.data, first.ctypes.data, last.ctypes.data)
        if m < 0:
            self._raise(m)
        total = self.counters()["kept"]
        ends = list(start[1:m]) + [total]
        return [(int(ref[r]), int(start[r]), int(ends[r] - start[r]), int(first[r]), int(last[r])) for r in range(m)]

    def feed(self, calculator, mapq_criteria: int, references=None, finish: bool = True) -> int:
        """handler/calc.py:131-161 with nothing on the host: decode + filter on the device, then every run of one chromosome is
        handed to ``calculator.feed_reads_device`` as three device addresses (the same duplicate / order rules, mscc.pyx:351-418,
        applied by the device feeders).  Falls back to ``pymasc_amd.bam.feed_bam`` (host arrays) for an unsorted file or a
        calculator without the device entry point.  Returns the number of reads fed."""
        from .bam import feed_bam
        wanted = list(calculator.references if references is None else references)
        self._check_selected(wanted)
        wanted = set(wanted)
        self._dropped = 0
        if not hasattr(calculator, "feed_reads_device"):
            return feed_bam(calculator, self, mapq_criteria, references, finish, use_index=False)
        self.decode(mapq_criteria)
        runs = self.device_runs()
        if runs is None:
            return feed_bam(calculator, self, mapq_criteria, references, finish, use_index=False)
        d_ref, d_pos, d_len, d_rev = self.device_arrays()
        fed = 0
        for ref, start, count, first, last in runs:
            name = self.references[ref]
            if name not in wanted:
                continue
            calculator.feed_reads_device(name, d_pos + 4 * start, d_len + 4 * start, d_rev + start, count, first, last)
            fed += count
        if finish:
            calculator.finishup_calculation()
        else:
            calculator._ctx.sync()      # the feeders read this reader's arrays: they must be done before it may be closed
        return fed

    def batches(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, batch: int = 1 << 22,
                _reference: int = -1) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        """Yields (ref_id, pos_1based, read_len, is_reverse) of the reads that pass the reference's filter
        (handler/read.py:62-90,131-141), in file order, at most ``batch`` per round -- as ``BamReader.batches``."""
        self._dropped = 0
        total = self.decode(mapq_criteria, flag_exclude, _reference)
        keep = None
        if not self.indexed and len(self._selected) < len(self.references):
            keep = np.zeros(max(len(self.references), 1), dtype=bool)
            keep[list(self._selected)] = True
        for first in range(0, total, batch):
            ref, pos, rlen, rev = self._fetch(first, min(batch, total - first))
            if keep is not None:
                m = keep[ref]
                ref, pos, rlen, rev = ref[m], pos[m], rlen[m], rev[m]
            yield ref, pos, rlen, rev

    def fetch(self, reference: str, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE,
              batch: int = 1 << 22):
        """The reads of ONE reference (handler/worker.py:106-132: what a worker gets from ``AlignmentFile.fetch(chrom)``)."""
        self._check_selected([reference])
        return self.batches(mapq_criteria, flag_exclude, batch, _reference=self.references.index(reference))
