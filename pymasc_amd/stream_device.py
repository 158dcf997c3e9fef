"""Alignments read from a STREAM on the device, in bounded windows: binding of pmx_dbam_open_stream /
pmx_dbam_stream_next (include/pymasc_amd_ingest.h).

``DeviceStreamReader`` has the surface of ``pymasc_amd.bam_device.DeviceBamReader`` for a source that cannot be read twice
or is too large to hold in HBM: ``-`` (standard input), a pipe, a FIFO, ``/dev/fd/N``, or a regular file.  BAM, BGZF SAM and
plain SAM are told apart from the first bytes.  The input is read window by window; every window is inflated, CRC-checked,
walked and filtered by the kernels of the whole-file reader, and ``feed`` hands each window's runs to the calculator's device
feeders before the next window overwrites them.  PyMaSC refuses to estimate a read length on an unseekable input
(handler/calc.py:81, ``InputUnseekable``); so does ``read_length_histogram`` here.
"""
from __future__ import annotations

import ctypes
import os
import stat
from typing import Iterator, Tuple

import numpy as np

from .bam_device import DeviceBamReader
from .exceptions import InputUnseekable
from .native import PMX_BAM_DEFAULT_EXCLUDE, SIDE_KINDS, load_ingest_library

STREAM_INFO_NAMES = ("windows", "bytes_in", "max_tail", "peak_device_bytes", "window_bytes", "inflated_budget")


def is_stream_path(path) -> bool:
    """True for an input that is read as a stream: ``-`` (standard input) or a path that is not a regular file (a FIFO,
    ``/dev/fd/N``, a character device).  A path that does not exist is not a stream (its open reports it)."""
    p = os.fspath(path)
    if p == "-":
        return True
    try:
        return not stat.S_ISREG(os.stat(p).st_mode)
    except OSError:
        return False


class DeviceStreamReader(DeviceBamReader):
    """An alignment stream read through the GPU one window at a time.

    ``source``: ``"-"`` (fd 0), an int fd, an object with ``fileno()`` (the caller keeps these open), or a path (opened here,
    closed by ``close``).  ``window_bytes``: compressed bytes per window (None: the library's 64 MiB).  ``references`` /
    ``select`` choose records as for a BAM file without an index.  A source that is not a regular file is read once:
    ``read_length_histogram`` raises ``InputUnseekable`` and a second ``feed`` / ``batches`` raises too."""

    def __init__(self, source, device: int = 0, threads: int = 0, window_bytes=None, references=None):
        self._L = load_ingest_library()
        self._own_fd = False
        self._armed = dict.fromkeys(SIDE_KINDS)     # kind -> the armed accumulator (native.SideAccumulator) or None
        if isinstance(source, int):
            fd, self.path = source, "/dev/fd/{}".format(source)
        elif isinstance(source, (str, bytes, os.PathLike)) and os.fspath(source) in ("-", b"-"):
            fd, self.path = 0, "-"
        elif hasattr(source, "fileno"):
            fd, self.path = source.fileno(), getattr(source, "name", "<stream>")
        else:
            self.path = os.fspath(source)
            fd = os.open(self.path, os.O_RDONLY)
            self._own_fd = True
        self._fd = fd
        self.indexed = False
        self._device, self._threads = int(device), int(threads)
        self._window = 0 if window_bytes is None else int(window_bytes)
        try:
            self.seekable = stat.S_ISREG(os.fstat(fd).st_mode)
            self._start = os.lseek(fd, 0, os.SEEK_CUR) if self.seekable else 0
            self._consumed = False
            self._attach(self._open(), references)
        except BaseException:
            self._close_fd()
            raise

    def _open(self):
        return self._open_handle("pmx_dbam_open_stream", self._fd, self._device, self._threads, self._window)

    def _close_fd(self):
        if self._own_fd and self._fd is not None:
            os.close(self._fd)
        self._fd = None

    def close(self) -> None:
        super().close()
        if getattr(self, "_own_fd", False):
            self._close_fd()

    def stream_info(self) -> dict:
        """pmx_dbam_stream_info: windows read, compressed bytes read, largest carried tail, peak device bytes, the budgets."""
        v = (ctypes.c_uint64 * 6)()
        rc = self._L.pmx_dbam_stream_info(self._h, v)
        if rc:
            self._raise(rc)
        return dict(zip(STREAM_INFO_NAMES, (int(x) for x in v)))

    def _windows(self) -> Iterator[int]:
        """Makes every window current in turn (the first pass reads the windows the open has begun; a regular file is opened
        again for a later pass, any other source raises)."""
        self._check_open()
        if self._consumed:
            if not self.seekable:
                raise InputUnseekable("'{}' cannot be read twice: it is not a regular file".format(self.path))
            os.lseek(self._fd, self._start, os.SEEK_SET)
            selected = self._selected
            self._L.pmx_dbam_close(self._h)
            self._h = None
            self._h = self._open()
            self._selected = selected
            if self._exclude is not None:       # (the mask belongs to the handle: attached again)
                self.set_exclude(self._exclude)
            for acc in self._each_armed():      # (so do the tables of the side counts: zeroed on the new handle)
                acc.begin(self)
        self._consumed = True
        while True:
            n = self._L.pmx_dbam_stream_next(self._h)
            if n < 0:
                self._raise(n)
            if n == 0:
                for acc in self._each_armed():
                    acc.flush(self)                 # (what the library held back of the last window)
                return
            yield int(n)
            for acc in self._each_armed():          # the caller is done with the window: its arrays stay as they are
                acc.add(self)

    def _each_armed(self):
        """The armed accumulators in the order of ``SIDE_KINDS``, whatever the order they were armed in."""
        return [acc for acc in self._armed.values() if acc is not None]

    def _arm(self, kind: str, acc):
        self._armed[kind] = acc
        return acc

    def _disarm(self, kind: str) -> None:
        self._armed[kind] = None

    def arm_complexity(self, mapq_criteria: int = 0, references=None):
        """From now on every window a pass makes current (``feed``, ``batches``) is also counted for the library complexity
        (``pmx_dbam_complexity``: the window's last position waits for the next window); returns the
        ``pymasc_amd.complexity.WindowedCount`` whose ``result()`` is the whole stream's once the pass has ended.  A stream
        that cannot be read twice is counted this way, in the pass that feeds it."""
        from .complexity import WindowedCount
        return self._arm("complexity", WindowedCount(self, mapq_criteria, references))

    def disarm_complexity(self) -> None:
        self._disarm("complexity")

    def arm_fingerprint(self, mapq_criteria: int = 0, references=None, bin_size: int = 500, extend: int = 0):
        """From now on every window a pass makes current is also counted per genome bin (``pmx_dbam_bincount_add``, into the
        table ``pmx_dbam_bincount_begin`` allocates here); returns the ``pymasc_amd.fingerprint.DeviceCount`` whose
        ``result(reader)`` is the whole stream's once the pass has ended.  A read is counted in the window that decodes it, so
        nothing is held back and the stream need not be sorted."""
        from .fingerprint import DeviceCount
        return self._arm("fingerprint", DeviceCount(self, mapq_criteria, references, bin_size, extend))

    def disarm_fingerprint(self) -> None:
        self._disarm("fingerprint")

    def arm_peaks(self, peaks, mapq_criteria: int = 0, references=None, extend: int = 0):
        """From now on every window a pass makes current is also counted per line of ``peaks`` (``pmx_dbam_peakcount_add``, into
        the table ``pmx_dbam_peakcount_begin`` builds here); returns the ``pymasc_amd.peaks.DeviceCount`` whose ``result(reader)``
        is the whole stream's once the pass has ended.  A read is counted in the window that decodes it, as for
        ``arm_fingerprint``."""
        from .peaks import DeviceCount
        return self._arm("peaks", DeviceCount(self, peaks, mapq_criteria, references, extend))

    def disarm_peaks(self) -> None:
        self._disarm("peaks")

    def arm_coverage(self, mapq_criteria: int = 0, references=None, extend=0, max_size: int = 2000):
        """From now on every window a pass makes current is also piled up base by base (``pmx_dbam_coverage_add``, into the table
        ``pmx_dbam_coverage_begin`` allocates here); returns the ``pymasc_amd.coverage.DeviceCount`` whose ``finish(reader)`` /
        ``result(reader)`` is the whole stream's once the pass has ended.  A read is marked in the window that decodes it, as
        for ``arm_fingerprint``.  ``extend`` ``"pair"``: the FR pairs of at most ``max_size`` bases at their own extent."""
        from .coverage import DeviceCount
        return self._arm("coverage", DeviceCount(self, mapq_criteria, references, extend, max_size))

    def disarm_coverage(self) -> None:
        self._disarm("coverage")

    def arm_gcbias(self, genome, mapq_criteria: int = 0, references=None, window: int = 100):
        """From now on every window a pass makes current is also placed on the windows of ``genome`` (a FASTA path or an open
        ``gcbias.DeviceGenome``) per G + C content (``pmx_dbam_gcbias_add``, into the table ``pmx_dbam_gcbias_begin`` builds
        here); returns the ``pymasc_amd.gcbias.DeviceCount`` whose ``result(reader)`` is the whole stream's once the pass has
        ended.  A read is counted in the window that decodes it, as for ``arm_fingerprint``."""
        from .gcbias import DeviceCount
        return self._arm("gcbias", DeviceCount(self, genome, mapq_criteria, references, window))

    def disarm_gcbias(self) -> None:
        self._disarm("gcbias")

    def arm_fragments(self, mapq_criteria: int = 0, references=None, max_size: int = 2000):
        """From now on the pairs of every window a pass makes current are also counted by fragment size
        (``pmx_dbam_fragments_add``, into the table ``pmx_dbam_fragments_begin`` allocates here); returns the
        ``pymasc_amd.fragments.DeviceCount`` whose ``result(reader)`` is the whole stream's once the pass has ended.  A pair is
        counted at its read1 record, in the window that decodes it: nothing is held back."""
        from .fragments import DeviceCount
        return self._arm("fragments", DeviceCount(self, mapq_criteria, references, max_size))

    def disarm_fragments(self) -> None:
        self._disarm("fragments")

    def arm_tss(self, anchors, mapq_criteria: int = 0, references=None, flank: int = 2000, extend: int = 0):
        """From now on every window a pass makes current is also piled up around ``anchors`` (``pmx_dbam_tss_add``, into the table
        ``pmx_dbam_tss_begin`` builds here); returns the ``pymasc_amd.tss.DeviceCount`` whose ``result(reader)`` is the whole
        stream's once the pass has ended.  A read is counted in the window that decodes it, as for ``arm_fingerprint``."""
        from .tss import DeviceCount
        return self._arm("tss", DeviceCount(self, anchors, mapq_criteria, references, flank, extend))

    def disarm_tss(self) -> None:
        self._disarm("tss")

    def _keep_mask(self):
        if len(self._selected) == len(self.references):
            return None
        keep = np.zeros(max(len(self.references), 1), dtype=bool)
        keep[list(self._selected)] = True
        return keep

    def read_length_histogram(self, mapq_criteria: int = 0):
        """The histogram of ``DeviceBamReader.read_length_histogram`` summed over one pass of the windows (the first-occurrence
        keys are offsets in the whole inflated stream); the next ``feed`` reads the file again.  A stream raises
        ``InputUnseekable`` before reading anything, as PyMaSC refuses it (handler/calc.py:81)."""
        from .readlen import COUNTER_NAMES, ReadLengthHistogram, histogram_from_library
        if not self.seekable:
            raise InputUnseekable("Cannot execute read length checking for unseekable input.")
        acc, counters = {}, dict.fromkeys(COUNTER_NAMES, 0)
        for _ in self._windows():
            h = histogram_from_library(self._L.pmx_dbam_readlen_hist, self._L.pmx_dbam_readlen_counters, self._h, mapq_criteria,
                                       self._raise)
            for ln, c, f in zip(h.lengths.tolist(), h.counts.tolist(), h.first.tolist()):
                c0, f0 = acc.get(ln, (0, f))
                acc[ln] = (c0 + c, min(f0, f))
            for k, v in h.counters.items():
                counters[k] += v
        lens = sorted(acc)
        return ReadLengthHistogram(np.array(lens, dtype=np.int64), np.array([acc[x][0] for x in lens], dtype=np.int64),
                                   np.array([acc[x][1] for x in lens], dtype=np.uint64), counters, int(mapq_criteria))

    def feed(self, calculator, mapq_criteria: int, references=None, finish: bool = True) -> int:
        """``DeviceBamReader.feed`` window by window: every window's runs of one chromosome go to
        ``calculator.feed_reads_device`` (a chromosome that spans windows arrives as several runs: the feeders' duplicate and
        order rules, mscc.pyx:351-418, carry over from one call to the next), and the calculator's context is synchronised
        before the next window overwrites the arrays.  A window with too many runs (unsorted input) goes through host arrays
        and ``feed_reads``, which raises ``ReadUnsortedError`` as for the file.  Returns the number of reads fed."""
        wanted = list(calculator.references if references is None else references)
        self._check_selected(wanted)
        wanted = set(wanted)
        use = np.array([n in wanted for n in self.references] or [False], dtype=bool)
        on_device = hasattr(calculator, "feed_reads_device")
        ctx = getattr(calculator, "_ctx", None)
        fed = 0
        self._dropped = 0
        for _ in self._windows():
            total = self.decode(mapq_criteria)
            if total == 0:
                continue
            runs = self.device_runs() if on_device else None
            if runs is None:
                ref, pos, rlen, rev = self._fetch(0, total)
                m = use[ref]
                ref, pos, rlen, rev = ref[m], pos[m], rlen[m], rev[m]
                cuts = np.flatnonzero(np.diff(ref)) + 1
                for s, e in zip(np.concatenate(([0], cuts)).tolist(), np.concatenate((cuts, [ref.size])).tolist()):
                    if e > s:
                        calculator.feed_reads(self.references[int(ref[s])], pos[s:e], rlen[s:e], rev[s:e])
                fed += int(ref.size)
                continue
            d_ref, d_pos, d_len, d_rev = self.device_arrays()
            for ref, start, count, first, last in runs:
                if self.references[ref] not in wanted:
                    continue
                calculator.feed_reads_device(self.references[ref], d_pos + 4 * start, d_len + 4 * start, d_rev + start, count,
                                             first, last)
                fed += count
            if ctx is not None:
                ctx.sync()              # the feeders read this window's arrays: done before the next window replaces them
        if finish:
            calculator.finishup_calculation()
        return fed

    def batches(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, batch: int = 1 << 22,
                _reference: int = -1) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
        """``DeviceBamReader.batches`` per window: (ref_id, pos_1based, read_len, is_reverse) of the reads that pass the
        reference's filter, in stream order, at most ``batch`` per round."""
        keep = self._keep_mask()
        self._dropped = 0
        for _ in self._windows():
            total = self.decode(mapq_criteria, flag_exclude, _reference)
            for first in range(0, total, batch):
                ref, pos, rlen, rev = self._fetch(first, min(batch, total - first))
                if keep is not None:
                    m = keep[ref]
                    ref, pos, rlen, rev = ref[m], pos[m], rlen[m], rev[m]
                yield ref, pos, rlen, rev
