"""GC bias of an alignment file: how the number of reads placed on a genome window depends on the window's G + C
content, beside NSC / RSC, NRF / PBC and the fingerprint.

``W`` is the window length (1 .. 1024).  A chosen reference of length ``len`` has a window at every 1-based start ``s`` with
``s + W - 1 <= len``; it is *blocked* when any of its positions is not ``A C G T`` (either case) or lies inside a region of the
reader's mask.  ``g(s)`` is the number of ``G`` / ``C`` among the bases of an unblocked window; ``N[g]`` the number of unblocked
windows with that ``g``.  The reads are the ones the correlation sees (``-q``, ``PMX_BAM_DEFAULT_EXCLUDE``, the chosen
chromosomes, the region mask).  A forward read is placed at ``s = pos1``, a reverse read at ``s = pos1 + read_len - W`` (its
window ends on its 5' base; not clipped): a window past either end counts in ``off_end``, a blocked one in ``blocked``, any other
adds 1 to ``F[g(s)]``.  Everything reported is a function of the integer tables ``N`` and ``F``.  The definitions are this
project's own, modelled on Picard's CollectGcBiasMetrics: nothing here was compared with Picard's or deepTools' output.

A device reader counts on the GPU (``pmx_dgc_*``, ``pmx_dbam_gcbias_*``, include/pymasc_amd_ingest.h); a host reader goes through
its ``batches`` and ``count_host`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import ctypes
import gzip
import os
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from .complexity import _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, NativeReader, SideAccumulator, count_over, load_ingest_library

GCBIAS_SUFFIX = "_gcbias.tab"
DEFAULT_WINDOW = 100
MAX_WINDOW = 1024
BAD_WINDOW = "the window is {}: it must lie in [1, 1024]"
NO_REFERENCE = "no chosen reference"
NO_RECORD = "reference '{}' has no record in the genome"
OTHER_LENGTH = "reference '{}' is {} long in the alignment header and {} in the genome"
_REF_HEADER = ("chrom", "windows")
_GC_HEADER = ("gc", "windows", "reads", "normalized")
_NAN = float("nan")


def check_window(window) -> int:
    if isinstance(window, bool) or int(window) != window or not 1 <= int(window) <= MAX_WINDOW:
        raise ValueError(BAD_WINDOW.format(window))
    return int(window)


class GcBias:
    """``N`` (``windows_by_gc``) and ``F`` (``reads_by_gc``), uint64 arrays of ``window + 1``; ``per_reference``: ``{name: windows
    of any kind}`` = ``max(0, len - window + 1)`` of the chosen references in header order; ``off_end`` / ``blocked``: the reads that
    were not placed.  The metrics are float64, computed here and nowhere else."""

    def __init__(self, window: int, per_reference: Dict[str, int], windows_by_gc, reads_by_gc, off_end: int, blocked: int,
                 genome: str = ""):
        self.window, self.off_end, self.blocked, self.genome = int(window), int(off_end), int(blocked), str(genome)
        self.per_reference = {str(k): int(v) for k, v in per_reference.items()}
        self.N = np.asarray(windows_by_gc, dtype=np.uint64).ravel().copy()
        self.F = np.asarray(reads_by_gc, dtype=np.uint64).ravel().copy()
        if self.N.size != self.window + 1 or self.F.size != self.window + 1:
            raise ValueError("N and F hold window + 1 counts")

    windows = property(lambda self: int(self.N.sum(dtype=np.uint64)))
    reads = property(lambda self: int(self.F.sum(dtype=np.uint64)))

    def _shares(self) -> Optional[Tuple[np.ndarray, np.ndarray]]:
        if not self.windows or not self.reads:
            return None
        return self.N.astype(np.float64) / float(self.windows), self.F.astype(np.float64) / float(self.reads)

    @property
    def normalized(self) -> np.ndarray:
        """``f[g] / n[g]``; nan where ``N[g]`` is 0, and everywhere without reads or windows."""
        out = np.full(self.window + 1, _NAN)
        nf = self._shares()
        if nf is not None:
            on = self.N > 0
            out[on] = nf[1][on] / nf[0][on]
        return out

    def _dropout(self, upper: bool) -> float:
        nf = self._shares()
        if nf is None:
            return _NAN
        side = (2 * np.arange(self.window + 1) > self.window) == upper
        return float(100.0 * np.sum(np.maximum(0.0, nf[0][side] - nf[1][side])))

    at_dropout = property(lambda self: self._dropout(False))
    gc_dropout = property(lambda self: self._dropout(True))

    def _mean_gc(self, t: np.ndarray) -> float:
        if not self.windows or not self.reads:
            return _NAN
        return float(np.sum(np.arange(self.window + 1, dtype=np.float64) * t.astype(np.float64)) / (self.window * float(t.sum(dtype=np.uint64))))

    window_gc = property(lambda self: self._mean_gc(self.N))
    read_gc = property(lambda self: self._mean_gc(self.F))

    @property
    def distance(self) -> float:
        nf = self._shares()
        return _NAN if nf is None else float(0.5 * np.sum(np.abs(nf[0] - nf[1])))

    def __eq__(self, other) -> bool:
        return (isinstance(other, GcBias) and (self.window, self.off_end, self.blocked) == (other.window, other.off_end, other.blocked)
                and list(self.per_reference.items()) == list(other.per_reference.items())
                and np.array_equal(self.N, other.N) and np.array_equal(self.F, other.F))

    __hash__ = None

    def __repr__(self) -> str:
        return "GcBias(window={}, windows={}, reads={}, off_end={}, blocked={})".format(self.window, self.windows, self.reads,
                                                                                      self.off_end, self.blocked)


def _per_reference(names, lengths, use, window: int) -> Dict[str, int]:
    return {n: max(0, int(l) - window + 1) for n, l, u in zip(names, lengths, use) if u}


class DeviceGenome(NativeReader):
    """A genome FASTA (plain, BGZF or gzip) parsed and packed in HBM (``pmx_dgc_open``): ``names`` and ``lengths`` of its records
    in file order.  A context manager; ``pmx_dbam_gcbias_begin`` does not refer to it once it has returned."""
    _P = "pmx_dgc"
    _WHAT = "genome"

    def __init__(self, path, device: int = 0, nthreads: int = 0):
        self._L = load_ingest_library()
        self.path, self.device = os.fspath(path), int(device)
        self._h = self._open_handle("pmx_dgc_open", self.path.encode(), self.device, int(nthreads))
        n = self._L.pmx_dgc_nrec(self._h)
        self.names = tuple(self._L.pmx_dgc_rec_name(self._h, i).decode() for i in range(n))
        self.lengths = tuple(int(self._L.pmx_dgc_rec_len(self._h, i)) for i in range(n))


class DeviceCount(SideAccumulator):
    """The table a device reader's handle holds between ``pmx_dbam_gcbias_begin`` and the next one: ``add`` counts what the handle
    holds now (a stream reader calls it for every window), ``result`` reads ``N`` and ``F`` back.  ``genome``: an open
    ``DeviceGenome`` or a FASTA path (opened for the length of each ``begin``)."""

    def __init__(self, reader, genome, mapq_criteria: int, references=None, window: int = DEFAULT_WINDOW):
        reader._check_open()
        self.mapq_criteria, self.window, self.genome = int(mapq_criteria), int(window), genome
        self.names, self.lengths = tuple(reader.references), tuple(reader.lengths)
        self.use = _selected_mask(reader, references)
        self.genome_path = genome.path if isinstance(genome, DeviceGenome) else os.fspath(genome)
        self.begin(reader)

    def begin(self, reader) -> None:
        """``N`` computed and ``F`` zeroed on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        if not isinstance(self.genome, DeviceGenome):
            with DeviceGenome(self.genome, getattr(reader, "_device", 0)) as g:
                return self._begin(reader, g)
        self.genome._check_open()
        self._begin(reader, self.genome)

    def _begin(self, reader, genome: DeviceGenome) -> None:
        mask = np.ascontiguousarray(self.use, dtype=np.uint8) if self.names else np.zeros(1, dtype=np.uint8)
        if self.window < 0:
            raise ValueError(BAD_WINDOW.format(self.window))
        rc = reader._L.pmx_dbam_gcbias_begin(reader._h, genome._h, self.window, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> Tuple[int, int, int]:
        """(reads placed, off_end, blocked) of what the handle holds now."""
        out = (ctypes.c_uint64 * 3)()
        rc = reader._L.pmx_dbam_gcbias_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, out)
        if rc:
            reader._raise(rc)
        return int(out[0]), int(out[1]), int(out[2])

    def tables(self, reader) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(N uint64 [window + 1], F likewise, totals uint64 [4] = windows, reads, off_end, blocked)."""
        totals = np.zeros(4, dtype=np.uint64)
        n = reader._L.pmx_dbam_gcbias_tables(reader._h, None, None, 0, totals.ctypes.data)
        if n < 0:
            reader._raise(n)
        windows, reads = np.zeros(int(n), dtype=np.uint64), np.zeros(int(n), dtype=np.uint64)
        m = reader._L.pmx_dbam_gcbias_tables(reader._h, windows.ctypes.data, reads.ctypes.data, int(n), totals.ctypes.data)
        if m < 0:
            reader._raise(m)
        assert m == n == self.window + 1
        return windows, reads, totals

    def result(self, reader) -> GcBias:
        windows, reads, totals = self.tables(reader)
        c = GcBias(self.window, _per_reference(self.names, self.lengths, self.use, self.window), windows, reads, int(totals[2]),
                   int(totals[3]), self.genome_path)
        if (c.windows, c.reads) != (int(totals[0]), int(totals[1])):
            raise RuntimeError("pmx_dbam_gcbias_tables: the tables do not add up to their totals")
        return c


def count_device(reader, genome, mapq_criteria: int, references=None, window: int = DEFAULT_WINDOW) -> GcBias:
    """``begin`` + ``add`` + ``tables`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, genome, mapq_criteria, references, window)
    acc.add(reader)
    return acc.result(reader)


# ---- the host path: the checker, and what a run without device ingest uses ----

_LINE_ERRORS = {"before": "sequence before the first header", "noname": "empty sequence name", "dup": "duplicate sequence name",
                "empty": "record with no bases", "byte": "sequence byte that is not a letter"}


def read_fasta(path) -> Dict[str, np.ndarray]:
    """``{name: the record's bases as uppercased bytes (uint8)}`` of a FASTA file, plain, gzip or bgzip, in file order, by the
    rules of the device parser: the name runs to the first space or tab, blank lines are ignored, a trailing ``\\r`` is dropped;
    ValueError ``line N: <reason>`` for the first malformed line."""
    with open(path, "rb") as fp:
        blob = fp.read()
    if blob[:2] == b"\x1f\x8b":
        blob = gzip.decompress(blob)
    records: Dict[str, List[bytes]] = {}
    errors: List[Tuple[int, str]] = []
    current, header_line = None, 0
    letters = bytes(range(ord("A"), ord("Z") + 1))

    def close_record():
        if current is not None and not any(records[current]):
            errors.append((header_line, "empty"))
    lines = blob.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    for i, line in enumerate(lines):
        if line.endswith(b"\r"):
            line = line[:-1]
        if not line:
            continue
        if line[:1] == b">":
            close_record()
            name = line[1:].replace(b"\t", b" ").split(b" ", 1)[0].decode("latin-1")
            if not name:
                errors.append((i, "noname"))
            elif name in records:
                errors.append((i, "dup"))
            current, header_line = name, i
            records.setdefault(name, [])
            if errors and errors[-1][0] == i:
                records[name] = [b"x"]          # (the record is reported once)
            continue
        if current is None:
            errors.append((i, "before"))
            continue
        up = line.upper()
        if up.translate(None, letters):
            errors.append((i, "byte"))
        records[current].append(up)
    close_record()
    if errors:
        line, what = min(errors)
        raise ValueError("{}: line {}: {}".format(path, line + 1, _LINE_ERRORS[what]))
    if not records:
        raise ValueError("{}: no FASTA record".format(path))
    return {n: np.frombuffer(b"".join(parts), dtype=np.uint8) for n, parts in records.items()}


def match_references(names, lengths, use, record_lengths: Dict[str, int]) -> None:
    """ValueError, in ``pmx_dbam_gcbias_begin``'s words, for the first chosen reference without a record of its name and length."""
    if not any(use):
        raise ValueError(NO_REFERENCE)
    for n, l, u in zip(names, lengths, use):
        if u and n not in record_lengths:
            raise ValueError(NO_RECORD.format(n))
        if u and int(record_lengths[n]) != int(l):
            raise ValueError(OTHER_LENGTH.format(n, int(l), int(record_lengths[n])))


class HostGenome:
    """What ``count_host`` needs of a FASTA file, kept between the files of a run: per record the cumulative sums of its G / C
    and of its bases that are not A C G T."""

    def __init__(self, path):
        self.path = os.fspath(path)
        self._records = read_fasta(self.path)
        self.names = tuple(self._records)
        self.lengths = tuple(int(v.size) for v in self._records.values())

    def sums(self, name: str, masked=None) -> Tuple[np.ndarray, np.ndarray]:
        """(cumulative G / C, cumulative blocked) of the record, each of len + 1 int64 with a leading 0; ``masked``: (begin, end)
        arrays of 0-based half-open intervals that count as blocked."""
        seq = self._records[name]
        gc = (seq == ord("G")) | (seq == ord("C"))
        bad = ~(gc | (seq == ord("A")) | (seq == ord("T")))
        if masked is not None:
            for b, e in zip(np.asarray(masked[0]).tolist(), np.asarray(masked[1]).tolist()):
                bad[int(b):int(e)] = True
        zero = np.zeros(1, dtype=np.int64)
        return np.concatenate((zero, np.cumsum(gc, dtype=np.int64))), np.concatenate((zero, np.cumsum(bad, dtype=np.int64)))


def count_host(reader, fasta_path, mapq_criteria: int = 0, references=None, window: int = DEFAULT_WINDOW) -> GcBias:
    """The host checker, plain numpy: the GC bias of the reads of a host reader (through its ``batches``, its mask applied) against
    the FASTA file ``fasta_path`` (or an open ``HostGenome``), with a cumulative sum of GC and of blocked over each record."""
    window = check_window(window)
    genome = fasta_path if isinstance(fasta_path, HostGenome) else HostGenome(fasta_path)
    use = _selected_mask(reader, references)
    names, lengths = tuple(reader.references), tuple(int(l) for l in reader.lengths)
    match_references(names, lengths, use, dict(zip(genome.names, genome.lengths)))
    mask = getattr(reader, "_exclude", None)
    N, F = np.zeros(window + 1, dtype=np.int64), np.zeros(window + 1, dtype=np.int64)
    sums = {}
    for r, (n, l, u) in enumerate(zip(names, lengths, use)):
        if not u:
            continue
        gc, bad = genome.sums(n, None if mask is None else mask.merged(r))
        sums[r] = (gc, bad)
        if l >= window:
            open_ = (bad[window:] - bad[:l - window + 1]) == 0
            N += np.bincount((gc[window:] - gc[:l - window + 1])[open_], minlength=window + 1)
    off_end = blocked = 0
    for ref, pos, rlen, rev in reader.batches(int(mapq_criteria), PMX_BAM_DEFAULT_EXCLUDE):
        ref, pos, rlen = np.asarray(ref, dtype=np.int64), np.asarray(pos, dtype=np.int64), np.asarray(rlen, dtype=np.int64)
        rev = np.asarray(rev).astype(bool)
        for r in np.unique(ref).tolist():
            if r not in sums:
                continue
            sel = ref == r
            s = np.where(rev[sel], pos[sel] + rlen[sel] - window, pos[sel])
            inside = (s >= 1) & (s + window - 1 <= lengths[r])
            off_end += int((~inside).sum())
            s = s[inside]
            gc, bad = sums[r]
            open_ = (bad[s - 1 + window] - bad[s - 1]) == 0
            blocked += int((~open_).sum())
            s = s[open_]
            F += np.bincount(gc[s - 1 + window] - gc[s - 1], minlength=window + 1)
    return GcBias(window, _per_reference(names, lengths, use, window), N, F, off_end, blocked, genome.path)


def from_reader(reader, genome, mapq_criteria: int = 0, references=None, window: int = DEFAULT_WINDOW) -> GcBias:
    """The GC bias of the reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the reader has
    selected) against ``genome``.  A device reader counts on the GPU (``genome``: a FASTA path or an open ``DeviceGenome``) --
    window by window for a stream reader, which is read once more when it is a regular file and raises ``InputUnseekable``
    otherwise; a host reader through ``count_host`` (``genome``: a FASTA path or a ``HostGenome``)."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        window = check_window(window)       # (the host branch checks inside count_host)
        return count_over(reader, "gcbias",
                          lambda: DeviceCount(reader, genome, mapq_criteria, references, window)).result(reader)
    return count_host(reader, genome, mapq_criteria, references, window)


def open_genome(path, device_ingest: bool, device: int = 0):
    """The genome of a run, parsed once: a ``DeviceGenome`` on ``device`` with device ingest, else a ``HostGenome``.  A file that
    cannot be parsed raises ValueError (host) or ``PmxIOError`` (device) with ``line N: <reason>``."""
    return DeviceGenome(path, device) if device_ingest else HostGenome(path)


# ---- the table ----

_FLOAT_ROWS = ("Window GC", "Read GC", "AT dropout", "GC dropout", "Distance")


def gcbias_rows(name: str, c: GcBias):
    """The first block of ``_gcbias.tab``: (label, value) pairs; the floats with ``repr`` (they read back exactly)."""
    return [("Name", name), ("Genome", c.genome), ("Window", c.window), ("Windows", c.windows), ("Reads", c.reads),
            ("Off end", c.off_end), ("Blocked", c.blocked), ("Window GC", repr(float(c.window_gc))), ("Read GC", repr(float(c.read_gc))),
            ("AT dropout", repr(float(c.at_dropout))), ("GC dropout", repr(float(c.gc_dropout))), ("Distance", repr(float(c.distance)))]


def write_gcbias(path_base, name: str, c: GcBias) -> Path:
    """Writes ``<path_base>_gcbias.tab`` (to a temporary file beside it, renamed into place) and returns its path: the label /
    value block, one row per chosen reference, and one row per ``g`` in ``0 .. window``."""
    path = Path(str(path_base) + GCBIAS_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w") as fp:
            for label, value in gcbias_rows(name, c):
                fp.write("{}\t{}\n".format(label, value))
            fp.write("\t".join(_REF_HEADER) + "\n")
            for chrom, n in c.per_reference.items():
                fp.write("{}\t{}\n".format(chrom, n))
            fp.write("\t".join(_GC_HEADER) + "\n")
            for g, (n, f, x) in enumerate(zip(c.N.tolist(), c.F.tolist(), c.normalized.tolist())):
                fp.write("{}\t{}\t{}\t{}\n".format(g, n, f, repr(float(x))))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def read_gcbias(path) -> Tuple[str, GcBias, Dict[str, object]]:
    """(name, GcBias, the label / value block as written with the floats as float) of a ``_gcbias.tab``."""
    with open(path) as fp:
        lines = [ln.rstrip("\n").split("\t") for ln in fp if ln.strip()]
    at_ref = lines.index(list(_REF_HEADER))
    at_gc = lines.index(list(_GC_HEADER))
    head = {row[0]: row[1] if len(row) > 1 else "" for row in lines[:at_ref]}
    per = {row[0]: int(row[1]) for row in lines[at_ref + 1:at_gc]}
    rows = lines[at_gc + 1:]
    c = GcBias(int(head["Window"]), per, [int(r[1]) for r in rows], [int(r[2]) for r in rows], int(head["Off end"]),
               int(head["Blocked"]), head["Genome"])
    block = {k: (float(v) if k in _FLOAT_ROWS else v) for k, v in head.items()}
    block["normalized"] = [float(r[3]) for r in rows]
    return head["Name"], c, block
