"""The fragment pileup as a bedGraph track: ``--coverage`` / ``coverage=``, what a ChIP-seq user builds next from
the estimated fragment length, taken from the reads that are in device memory already.

The definitions, which the device code (csrc/ingest/coverage_device.inc), the host checker here and the tests state the same way.
They are this project's own: nothing here was compared with ``bedtools genomecov``, deepTools or MACS2.

* The reads are the ones the correlation sees: the run's filter, the chosen references, less the reads an exclude mask drops.
* The extent is the fingerprint's (7.16) with ``extend``: ``L = extend``, or the read's own length at 0; a forward read covers
  ``[pos1, pos1 + L - 1]``, a reverse read ``[pos1 + read_len - L, pos1 + read_len - 1]``; both clipped to ``[1, len]`` of the
  reference.  A read with nothing left after the clip adds nothing and is not in ``reads``.
* With ``extend = "pair"`` (``PAIR``) the reads are replaced by the FR rows of ``pymasc_amd.fragments`` (pairs
  counted at read1, ``size <= max_size``, masked by the fragment's extent): a row covers ``[start1, start1 + size - 1]``, clipped
  the same way, and ``reads`` is the number of rows piled.
* ``depth[r][p]`` is the number of kept reads whose clipped extent holds position ``p`` of reference ``r``, a 32-bit count.
* Per chosen reference, in header order, the maximal intervals of constant depth greater than 0 are the runs
  ``(start0, end0, depth)``, 0-based and half-open as in bedGraph.  Two reads that abut at equal depth form one run; depth 0 is not
  written; a reference without reads has no run.
* Totals: ``reads`` (the reads that added something), ``runs``, ``covered_bases = sum (end0 - start0)``,
  ``fragment_bases = sum depth * (end0 - start0)`` (the sum of the clipped extents' lengths), ``max_depth``.

The file is ``<name>_coverage.bedGraph``: a ``track`` line, then ``chrom<TAB>start0<TAB>end0<TAB>depth`` per run, plain text.

A device reader counts on the GPU and formats the lines there (``pmx_dbam_coverage_*``, include/pymasc_amd_ingest.h); a host reader
goes through its ``batches`` and ``HostCount`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import ctypes
import os
import re
from pathlib import Path
from typing import Dict, Iterator, Tuple

import numpy as np

from .complexity import _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, SideAccumulator, count_over

COVERAGE_SUFFIX = "_coverage.bedGraph"
TILE = 4096                 # slots per scan tile of the device code (PMX_COVERAGE_TILE of include/pymasc_amd_ingest.h)
TEXT_CHUNK = 1 << 18        # runs per call of pmx_dbam_coverage_text when a file is written
MAX_READS = 1 << 31
TOTALS = ("reads", "runs", "covered_bases", "fragment_bases", "max_depth")
PAIR = "pair"               # ``extend``: the FR pairs at their own extent
_TRACK = re.compile(r'^track type=bedGraph name="(.*)" description="pymasc_amd fragment pileup extend=(\d+|read|pair) reads=(\d+)"$')


def check_extend(extend):
    """``extend`` as the pileup takes it: ``"pair"`` or an integer of at least 0."""
    if extend == PAIR:
        return PAIR
    if isinstance(extend, (str, bool)) or int(extend) != extend or int(extend) < 0:
        raise ValueError("extend is \"pair\" or an integer that is not negative")
    return int(extend)


class Coverage:
    """``runs``: ``{name: (start0, end0, depth)}``, uint32, of the chosen references that have a run, in header order;
    ``reads``: the reads that added; ``extend`` (0: every read's own length; ``"pair"``: the FR pairs at their own extent)."""

    def __init__(self, runs, reads: int, extend: int):
        self.runs = {str(k): tuple(np.asarray(x, dtype=np.uint32).ravel() for x in v) for k, v in runs.items()}
        self.reads, self.extend = int(reads), check_extend(extend)
        if any(len(v) != 3 or not (v[0].size == v[1].size == v[2].size > 0) for v in self.runs.values()):
            raise ValueError("every reference has as many starts as ends and depths, and at least one run")

    n_runs = property(lambda self: sum(int(v[0].size) for v in self.runs.values()))
    covered_bases = property(lambda self: sum(int((e.astype(np.int64) - s.astype(np.int64)).sum()) for s, e, _d in self.runs.values()))
    fragment_bases = property(lambda self: sum(int(((e.astype(np.int64) - s.astype(np.int64)) * d.astype(np.int64)).sum())
                                               for s, e, d in self.runs.values()))
    max_depth = property(lambda self: max((int(d.max()) for _s, _e, d in self.runs.values()), default=0))

    @property
    def totals(self) -> Tuple[int, int, int, int, int]:
        """(reads, runs, covered_bases, fragment_bases, max_depth), the order of ``pmx_dbam_coverage_finish``."""
        return self.reads, self.n_runs, self.covered_bases, self.fragment_bases, self.max_depth

    def rows(self):
        """Every run as a plain tuple (name, start0, end0, depth), in file order."""
        return [(n, *r) for n, v in self.runs.items() for r in zip(*(x.tolist() for x in v))]

    def text_chunks(self, chunk: int = 1 << 16) -> Iterator[bytes]:
        """The bedGraph lines, formatted with numpy, ``chunk`` runs at a time."""
        for name, (s, e, d) in self.runs.items():
            head = name + "\t"
            for a in range(0, s.size, chunk):
                cols = [x[a:a + chunk].astype("U10") for x in (s, e, d)]
                lines = np.char.add(np.char.add(np.char.add(np.char.add(np.char.add(head, cols[0]), "\t"), cols[1]), "\t"), cols[2])
                yield ("\n".join(lines.tolist()) + "\n").encode()

    def __eq__(self, other) -> bool:
        return (isinstance(other, Coverage) and (self.reads, self.extend) == (other.reads, other.extend)
                and list(self.runs) == list(other.runs)
                and all(np.array_equal(a, b) for k in self.runs for a, b in zip(self.runs[k], other.runs[k])))

    __hash__ = None

    def __repr__(self) -> str:
        return "Coverage(extend={}, reads={}, runs={}, covered_bases={}, fragment_bases={}, max_depth={})".format(self.extend, *self.totals)


class HostCount:
    """The host checker, plain numpy, and the path of host readers: a difference array per chosen reference that has a read (one
    slot per base and a closing one); ``add`` marks a batch of reads given as four columns with ``np.add.at``, ``result`` takes the running sum and
    cuts it into runs where a slot is not 0."""

    def __init__(self, names, lengths, use, extend=0):
        """``extend`` ``"pair"``: ``add`` is given the FR rows of ``fragments.rows_host`` as forward reads of ``size`` bases."""
        self.label = check_extend(extend)
        extend = 0 if self.label == PAIR else self.label
        self.names, self.lengths = tuple(names), tuple(max(int(x), 0) for x in lengths)
        self.use = np.asarray(use, dtype=bool)
        if not self.use.any():
            raise ValueError("no chosen reference")
        self.extend, self.reads = int(extend), 0
        self.steps = {r: None for r in range(len(self.names)) if self.use[r]}      # (allocated with the reference's first read)

    def add(self, ref_id, pos1, read_len, reverse) -> int:
        ref = np.asarray(ref_id, dtype=np.int64).ravel()
        pos = np.asarray(pos1, dtype=np.int64).ravel()
        rl = np.asarray(read_len, dtype=np.int64).ravel()
        rev = np.asarray(reverse).ravel().astype(bool)
        span = np.full(ref.size, self.extend, dtype=np.int64) if self.extend else rl
        lo_all = np.maximum(np.where(rev, pos + rl - span, pos), 1)
        hi_all = np.where(rev, pos + rl - 1, pos + span - 1)
        added = 0
        for r in np.unique(ref).tolist():
            if r not in self.steps:
                continue
            sel = ref == r
            lo, hi = lo_all[sel], np.minimum(hi_all[sel], self.lengths[r])
            on = lo <= hi
            if self.steps[r] is None:
                self.steps[r] = np.zeros(self.lengths[r] + 1, dtype=np.int32)
            steps = self.steps[r]
            np.add.at(steps, lo[on] - 1, 1)
            np.add.at(steps, hi[on], -1)
            added += int(on.sum())
        self.reads += added
        if self.reads >= MAX_READS:
            raise ValueError("2^31 reads or more: the depth is a 32-bit count")
        return added

    def result(self) -> Coverage:
        runs = {}
        for r, steps in self.steps.items():
            at = np.flatnonzero(steps) if steps is not None else np.zeros(0, dtype=np.int64)
            if at.size:
                depth = np.cumsum(steps[at], dtype=np.int64)
                keep = depth[:-1] > 0
                runs[self.names[r]] = (at[:-1][keep], at[1:][keep], depth[:-1][keep])
        return Coverage(runs, self.reads, self.label)


def count_host(ref_id, pos1, read_len, reverse, names, lengths, use, extend: int = 0) -> Coverage:
    """The pileup of the reads given as four columns over the references ``names`` / ``lengths`` chosen by ``use``."""
    acc = HostCount(names, lengths, use, extend)
    acc.add(ref_id, pos1, read_len, reverse)
    return acc.result()


class DeviceCount(SideAccumulator):
    """The pileup a device reader's handle holds between ``pmx_dbam_coverage_begin`` and the next one: ``add`` marks what the handle
    holds now (a stream reader calls it for every window), ``finish`` turns the table into runs, ``runs`` / ``text`` read them
    back, ``result`` is all of it as a ``Coverage``."""

    def __init__(self, reader, mapq_criteria: int, references=None, extend=0, max_size: int = 2000):
        """``extend`` ``"pair"``: ``add`` marks the FR rows of at most ``max_size`` bases (``pmx_dbam_coverage_add_fragments``)."""
        reader._check_open()
        self.mapq_criteria, self.extend, self.max_size = int(mapq_criteria), check_extend(extend), int(max_size)
        self.names = tuple(reader.references)
        self.use = _selected_mask(reader, references)
        self.totals = None
        self.begin(reader)

    def begin(self, reader) -> None:
        """A zeroed table on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        mask = np.ascontiguousarray(self.use, dtype=np.uint8) if self.names else np.zeros(1, dtype=np.uint8)
        self.totals = None
        rc = reader._L.pmx_dbam_coverage_begin(reader._h, 0 if self.extend == PAIR else self.extend, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> int:
        added = ctypes.c_uint64()
        if self.extend == PAIR:
            rc = reader._L.pmx_dbam_coverage_add_fragments(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, self.max_size,
                                                           ctypes.byref(added))
        else:
            rc = reader._L.pmx_dbam_coverage_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(added))
        if rc:
            reader._raise(rc)
        return int(added.value)

    def finish(self, reader) -> Dict[str, int]:
        """The totals of ``pmx_dbam_coverage_finish`` by name (``TOTALS``); a second call gives the first one's."""
        if self.totals is None:
            out = np.zeros(5, dtype=np.uint64)
            rc = reader._L.pmx_dbam_coverage_finish(reader._h, out.ctypes.data)
            if rc:
                reader._raise(rc)
            self.totals = dict(zip(TOTALS, (int(x) for x in out)))
        return self.totals

    def runs(self, reader, first: int = 0, n=None):
        """(reference int32, start0, end0, depth uint32) of the runs ``[first, first + n)`` (``pmx_dbam_coverage_runs``)."""
        n = self.finish(reader)["runs"] - int(first) if n is None else int(n)
        out = [np.zeros(max(n, 1), dtype=t) for t in (np.int32, np.uint32, np.uint32, np.uint32)]
        rc = reader._L.pmx_dbam_coverage_runs(reader._h, int(first), n, *(x.ctypes.data for x in out))
        if rc:
            reader._raise(rc)
        return tuple(x[:n] for x in out)

    def text(self, reader, first: int = 0, n=None) -> bytes:
        """The bedGraph lines of the runs ``[first, first + n)``, formatted on the device (``pmx_dbam_coverage_text``: the size,
        then the bytes)."""
        n = self.finish(reader)["runs"] - int(first) if n is None else int(n)
        size = reader._L.pmx_dbam_coverage_text(reader._h, int(first), n, None, 0)
        if size < 0:
            reader._raise(size)
        buf = np.zeros(max(int(size), 1), dtype=np.uint8)
        got = reader._L.pmx_dbam_coverage_text(reader._h, int(first), n, buf.ctypes.data, int(size))
        if got < 0:
            reader._raise(got)
        assert got == size
        return buf[:int(size)].tobytes()

    def text_chunks(self, reader, chunk: int = TEXT_CHUNK) -> Iterator[bytes]:
        total = self.finish(reader)["runs"]
        for first in range(0, total, int(chunk)):
            yield self.text(reader, first, min(int(chunk), total - first))

    def result(self, reader) -> Coverage:
        totals = self.finish(reader)
        ref, start, end, depth = self.runs(reader)
        cut = np.flatnonzero(np.diff(ref)) + 1 if ref.size else np.zeros(0, dtype=np.int64)
        edges = np.concatenate(([0], cut, [ref.size])).astype(np.int64) if ref.size else np.zeros(1, dtype=np.int64)
        c = Coverage({self.names[int(ref[a])]: (start[a:z], end[a:z], depth[a:z]) for a, z in zip(edges[:-1], edges[1:])},
                     totals["reads"], self.extend)
        if c.totals != tuple(totals[k] for k in TOTALS):
            raise RuntimeError("pmx_dbam_coverage_finish: the runs do not add up to the totals")
        return c


def count_device(reader, mapq_criteria: int, references=None, extend=0, max_size: int = 2000) -> Coverage:
    """``begin`` + ``add`` + ``finish`` + ``runs`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, mapq_criteria, references, extend, max_size)
    acc.add(reader)
    return acc.result(reader)


def device_count_of(reader, mapq_criteria: int = 0, references=None, extend=0, max_size: int = 2000) -> DeviceCount:
    """The finished ``DeviceCount`` of everything a device reader reads: one ``add`` for a whole-file reader, every window of a
    stream reader (read once more when it is a regular file, ``InputUnseekable`` otherwise)."""
    acc = count_over(reader, "coverage", lambda: DeviceCount(reader, mapq_criteria, references, extend, max_size))
    acc.finish(reader)
    return acc


def from_reader(reader, mapq_criteria: int = 0, references=None, extend=0, max_size: int = 2000) -> Coverage:
    """The pileup of the reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the reader has
    selected).  A device reader counts on the GPU (``device_count_of``); a host reader through ``batches`` and ``HostCount``.
    ``extend`` ``"pair"``: the FR pairs of at most ``max_size`` bases at their own extent; a host reader through
    ``fragments.rows_host``."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        return device_count_of(reader, mapq_criteria, references, extend, max_size).result(reader)
    acc = HostCount(reader.references, reader.lengths, _selected_mask(reader, references), extend)
    if acc.label == PAIR:
        from .fragments import FR, rows_host
        for ref, start1, size, orient, _c in rows_host(reader, mapq_criteria, references, max_size):
            fr = orient == FR
            if fr.any():
                acc.add(ref[fr], start1[fr], size[fr], np.zeros(int(fr.sum()), dtype=bool))
        return acc.result()
    for batch in reader.batches(mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE):
        if len(batch[0]):
            acc.add(*batch)
    return acc.result()


def track_line(name: str, extend, reads: int) -> bytes:
    return 'track type=bedGraph name="{}" description="pymasc_amd fragment pileup extend={} reads={}"\n'.format(
        name, PAIR if extend == PAIR else int(extend) if int(extend) else "read", int(reads)).encode()


def write_track(path_base, name: str, extend, reads: int, chunks) -> Path:
    """Writes ``<path_base>_coverage.bedGraph`` (to a temporary file beside it, renamed into place) and returns its path: the
    track line, then the bytes of ``chunks`` (the lines of the runs)."""
    path = Path(str(path_base) + COVERAGE_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "wb") as fp:
            fp.write(track_line(name, extend, reads))
            for chunk in chunks:
                fp.write(chunk)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def write_coverage(path_base, name: str, c, reader=None) -> Path:
    """``write_track`` of a ``Coverage`` (the lines formatted with numpy) or, with ``reader``, of a finished ``DeviceCount`` on that
    reader's handle: the lines are formatted on the device and pulled ``TEXT_CHUNK`` runs at a time."""
    if reader is None:
        return write_track(path_base, name, c.extend, c.reads, c.text_chunks())
    return write_track(path_base, name, c.extend, c.finish(reader)["reads"], c.text_chunks(reader))


def read_coverage(path) -> Tuple[str, Coverage]:
    """(name, Coverage) of a ``_coverage.bedGraph`` as ``write_coverage`` writes it."""
    with open(path) as fp:
        head = _TRACK.match(fp.readline().rstrip("\n"))
        if head is None:
            raise ValueError("'{}' does not begin with the track line of a fragment pileup".format(path))
        cols: Dict[str, list] = {}
        for ln in fp:
            chrom, s, e, d = ln.rstrip("\n").split("\t")
            cols.setdefault(chrom, []).append((int(s), int(e), int(d)))
    runs = {k: tuple(zip(*v)) for k, v in cols.items()}
    extend = head.group(2)
    return head.group(1), Coverage(runs, int(head.group(3)), 0 if extend == "read" else PAIR if extend == PAIR else int(extend))
