"""The fraction of reads in peaks (FRiP) and the reads per peak line: ``--peaks FILE`` / ``peaks=``, beside
NSC / RSC, NRF / PBC and the fingerprint.

The definitions, which the device code (csrc/ingest/peakcount_device.inc), the host checker here and the tests state the same way.
They are this project's own: nothing here was compared with ``bedtools`` or with ENCODE's pipeline.

* The peak file is narrowPeak, broadPeak, gappedPeak or any BED3+ file, plain, gzip or bgzip, read through the text-track readers
  as the mask file is (``region_mask.open_mask``), or an ordered ``{name: [(start, end), ...]}``.  Only the first three columns are
  used: names, scores and summits are not carried through.  Intervals are 0-based, half-open: ``(b, e)`` covers the 1-based
  positions ``b + 1 .. e``.  Lines may be unsorted, overlap, nest, abut and repeat, and each line has a count of its own (two
  summits of one narrowPeak interval are two identical lines).  A line is clipped to its reference's length; one that is empty
  then stays in the table with the count 0 and adds nothing to the union.  A name that is not among the alignment's references is
  skipped, with one warning that counts them; no name matching at all is a ValueError (``ExcludeMask.resolve``).  Lines on
  references that the chromosome filter leaves out are not in the table.
* The reads are the ones the correlation sees: the run's filter, the chosen references, less the reads an exclude mask drops.
  ``N`` is their number: every kept read on a chosen reference, whether or not it touches a peak.
* The extent is the fingerprint's (7.16) with ``peaks_extend``: ``L = peaks_extend``, or the read's own length at 0; a forward read
  covers ``[pos1, pos1 + L - 1]``, a reverse read ``[pos1 + read_len - L, pos1 + read_len - 1]``; both clipped to ``[1, len]``.
* A read with the clipped extent ``[lo, hi]`` is *in* the line ``(b, e)`` when ``b + 1 <= hi and lo <= e``.  ``count[line]`` is the
  number of reads in it; a read in three overlapping lines adds 1 to each.  ``n_in`` is the number of reads in at least one line,
  once per read.  ``union_bases`` is the total length of the clipped, merged lines on chosen references, ``genome_bases`` the sum
  of the chosen references' lengths.  ``FRiP = n_in / N``, ``enrichment = FRiP / (union_bases / genome_bases)``; ``N = 0``: nan.

A device reader counts on the GPU (``pmx_dbam_peakcount_*``, include/pymasc_amd_ingest.h); a host reader goes through its
``batches`` and ``count_host`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, Tuple

import numpy as np

from .complexity import _ratio, _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, SideAccumulator, count_over
from .region_mask import ExcludeMask, merge, open_mask, resolve_lines

PEAKS_SUFFIX = "_peaks.tab"
WHAT = "peak file"
_REF_HEADER = ("chrom", "lines", "reads", "reads_in_peaks")
_LINE_HEADER = ("#chrom", "start", "end", "reads")
_NAN = float("nan")


def open_peaks(source, device_ingest: bool = False, device: int = 0) -> ExcludeMask:
    """The lines of a peak file (a path, an ordered ``{name: [(start, end), ...]}``, or what this returned) by chromosome name,
    in file order: ``region_mask.open_mask``, whose messages then speak of a peak file."""
    return open_mask(source, device_ingest, device, what=WHAT)


class PeakCounts:
    """``lines``: ``{name: (begin, end)}`` of the chosen references in header order, uint32, the lines as they were read (file
    order, unclipped); ``counts``: ``{name: reads of every line}``, int64; ``per_reference``: ``{name: (reads, reads in at least one
    line)}``; ``N`` / ``n_in``: their sums; ``union_bases``, ``genome_bases``, ``extend``."""

    def __init__(self, lines, counts, per_reference, union_bases: int, genome_bases: int, extend: int):
        self.lines = {str(k): (np.asarray(b, dtype=np.uint32).ravel(), np.asarray(e, dtype=np.uint32).ravel()) for k, (b, e) in lines.items()}
        self.counts = {str(k): np.asarray(v, dtype=np.int64).ravel() for k, v in counts.items()}
        self.per_reference = {str(k): (int(v[0]), int(v[1])) for k, v in per_reference.items()}
        self.union_bases, self.genome_bases, self.extend = int(union_bases), int(genome_bases), int(extend)
        if not (list(self.lines) == list(self.counts) == list(self.per_reference)) \
                or any(self.lines[k][0].size != self.counts[k].size or self.lines[k][0].size != self.lines[k][1].size for k in self.lines):
            raise ValueError("lines, counts and per_reference name the same references, with one count per line")

    N = property(lambda self: sum(v[0] for v in self.per_reference.values()))
    n_in = property(lambda self: sum(v[1] for v in self.per_reference.values()))
    n_lines = property(lambda self: sum(int(c.size) for c in self.counts.values()))
    frip = property(lambda self: _ratio(self.n_in, self.N))

    @property
    def enrichment(self) -> float:
        """FRiP over the share of the genome the merged lines cover."""
        return _ratio(self.frip, _ratio(self.union_bases, self.genome_bases)) if self.N else _NAN

    def __eq__(self, other) -> bool:
        return (isinstance(other, PeakCounts)
                and (self.union_bases, self.genome_bases, self.extend) == (other.union_bases, other.genome_bases, other.extend)
                and list(self.per_reference.items()) == list(other.per_reference.items()) and list(self.lines) == list(other.lines)
                and all(np.array_equal(self.lines[k][0], other.lines[k][0]) and np.array_equal(self.lines[k][1], other.lines[k][1])
                        and np.array_equal(self.counts[k], other.counts[k]) for k in self.lines))

    __hash__ = None

    def __repr__(self) -> str:
        return "PeakCounts(lines={}, N={}, n_in={}, union_bases={}, genome_bases={}, extend={})".format(
            self.n_lines, self.N, self.n_in, self.union_bases, self.genome_bases, self.extend)


class _Layout:
    """A peak file bound to a reader's references and its chosen ones: the rows of the table and the union."""

    def __init__(self, reader, peaks: ExcludeMask, references):
        self.names, self.lengths = tuple(reader.references), tuple(int(x) for x in reader.lengths)
        self.use = np.asarray(_selected_mask(reader, references), dtype=np.uint8)
        self.resolved, (self.offsets, self.begin, self.end) = resolve_lines(peaks, self.names, self.lengths, self.use)
        self.chosen = [r for r in range(len(self.names)) if self.use[r]]

    def union_bases(self) -> int:
        total = 0
        for r in self.chosen:
            mb, me = merge(*self.resolved.lines(r), self.lengths[r])
            total += int(me.astype(np.int64).sum() - mb.astype(np.int64).sum())
        return total

    def result(self, counts, per_ref, union_bases: int, extend: int) -> PeakCounts:
        """``counts``: one per row of ``csr`` order; ``per_ref``: [nref, 2]."""
        o = self.offsets
        return PeakCounts({self.names[r]: (self.begin[o[r]:o[r + 1]], self.end[o[r]:o[r + 1]]) for r in self.chosen},
                          {self.names[r]: counts[o[r]:o[r + 1]] for r in self.chosen},
                          {self.names[r]: per_ref[r] for r in self.chosen}, union_bases,
                          sum(max(self.lengths[r], 0) for r in self.chosen), extend)


def count_host(ref_id, pos1, read_len, reverse, resolved, use, extend: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The host checker, plain numpy: (the count of every line in ``resolved.csr(use)`` order, int64; per_ref int64 [nref, 2] =
    reads, reads in at least one line) of the reads given as four columns.  Per reference, a line ``(b, e)`` holds every read
    but those that begin behind it (``lo > e``) and those that end in front of it (``hi < b + 1``) -- two searches over the sorted
    extents' ends; a read is in at least one line when it overlaps the merged lines (``region_mask.merge``)."""
    nref = len(resolved.references)
    offsets, _b, _e = resolved.csr(use)
    counts = np.zeros(int(offsets[-1]), dtype=np.int64)
    per_ref = np.zeros((nref, 2), dtype=np.int64)
    ref = np.asarray(ref_id, dtype=np.int64).ravel()
    pos = np.asarray(pos1, dtype=np.int64).ravel()
    rl = np.asarray(read_len, dtype=np.int64).ravel()
    rev = np.asarray(reverse).ravel().astype(bool)
    span = np.full(ref.size, int(extend), dtype=np.int64) if extend else rl
    lo_all = np.maximum(np.where(rev, pos + rl - span, pos), 1)
    hi_all = np.where(rev, pos + rl - 1, pos + span - 1)
    for r in range(nref):
        if not use[r]:
            continue
        sel = ref == r
        per_ref[r, 0] = int(sel.sum())
        lo, hi = lo_all[sel], np.minimum(hi_all[sel], resolved.lengths[r])
        ok = lo <= hi
        lo, hi = lo[ok], hi[ok]
        b, e = (x.astype(np.int64) for x in resolved.lines(r, clip=True))
        behind = lo.size - np.searchsorted(np.sort(lo), e, side="right")
        in_front = np.searchsorted(np.sort(hi), b + 1, side="left")
        counts[offsets[r]:offsets[r + 1]] = np.where(b < e, lo.size - behind - in_front, 0)
        mb, me = (x.astype(np.int64) for x in merge(b, e))
        if mb.size and lo.size:
            k = np.searchsorted(mb, hi - 1, side="right") - 1
            per_ref[r, 1] = int(((k >= 0) & (me[np.maximum(k, 0)] >= lo)).sum())
    return counts, per_ref


class DeviceCount(SideAccumulator):
    """The table a device reader's handle holds between ``pmx_dbam_peakcount_begin`` and the next one: ``add`` counts what the
    handle holds now (a stream reader calls it for every window), ``result`` reads the counts back."""

    def __init__(self, reader, peaks, mapq_criteria: int, references=None, extend: int = 0):
        reader._check_open()
        if int(extend) < 0:
            raise ValueError("extend is not negative")
        self.mapq_criteria, self.extend = int(mapq_criteria), int(extend)
        self.layout = _Layout(reader, open_peaks(peaks), references)
        self.begin(reader)

    def begin(self, reader) -> None:
        """A zeroed table on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        lay = self.layout
        mask = np.ascontiguousarray(lay.use, dtype=np.uint8) if lay.names else np.zeros(1, dtype=np.uint8)
        rc = reader._L.pmx_dbam_peakcount_begin(reader._h, len(lay.names), lay.offsets.ctypes.data, lay.begin.ctypes.data,
                                                lay.end.ctypes.data, self.extend, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> Tuple[int, int]:
        out = np.zeros(2, dtype=np.uint64)
        rc = reader._L.pmx_dbam_peakcount_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, out.ctypes.data)
        if rc:
            reader._raise(rc)
        return int(out[0]), int(out[1])

    def counts(self, reader) -> np.ndarray:
        """Every line's count in input order (``pmx_dbam_peakcount_copy``), uint32."""
        out = np.zeros(max(int(self.layout.offsets[-1]), 1), dtype=np.uint32)
        rc = reader._L.pmx_dbam_peakcount_copy(reader._h, 0, int(self.layout.offsets[-1]), out.ctypes.data)
        if rc:
            reader._raise(rc)
        return out[:int(self.layout.offsets[-1])]

    def totals(self, reader) -> Tuple[np.ndarray, np.ndarray]:
        """(totals uint64 [4] = N, n_in, union_bases, lines; per_ref uint64 [nref, 2]) of ``pmx_dbam_peakcount_totals``."""
        totals = np.zeros(4, dtype=np.uint64)
        per_ref = np.zeros((max(len(self.layout.names), 1), 2), dtype=np.uint64)
        rc = reader._L.pmx_dbam_peakcount_totals(reader._h, totals.ctypes.data, per_ref.ctypes.data)
        if rc:
            reader._raise(rc)
        return totals, per_ref[:len(self.layout.names)]

    def result(self, reader) -> PeakCounts:
        totals, per_ref = self.totals(reader)
        c = self.layout.result(self.counts(reader).astype(np.int64), per_ref.astype(np.int64), int(totals[2]), self.extend)
        if (c.N, c.n_in, c.n_lines) != (int(totals[0]), int(totals[1]), int(totals[3])):
            raise RuntimeError("pmx_dbam_peakcount_totals: the references do not add up to the totals")
        return c


def count_device(reader, peaks, mapq_criteria: int, references=None, extend: int = 0) -> PeakCounts:
    """``begin`` + ``add`` + ``copy`` / ``totals`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, peaks, mapq_criteria, references, extend)
    acc.add(reader)
    return acc.result(reader)


def from_reader(reader, peaks, mapq_criteria: int = 0, references=None, extend: int = 0) -> PeakCounts:
    """The reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the reader has selected)
    counted per line of ``peaks`` (``open_peaks``).  A device reader counts on the GPU -- window by window for a stream reader,
    which is read once more when it is a regular file and raises ``InputUnseekable`` otherwise; a host reader through ``batches``
    and ``count_host``."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        return count_over(reader, "peaks", lambda: DeviceCount(reader, peaks, mapq_criteria, references, extend)).result(reader)
    if int(extend) < 0:
        raise ValueError("extend is not negative")
    lay = _Layout(reader, open_peaks(peaks), references)
    counts = np.zeros(int(lay.offsets[-1]), dtype=np.int64)
    per_ref = np.zeros((len(lay.names), 2), dtype=np.int64)
    for batch in reader.batches(mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE):
        if len(batch[0]):
            c, p = count_host(*batch, lay.resolved, lay.use, extend)
            counts += c
            per_ref += p
    return lay.result(counts, per_ref, lay.union_bases(), int(extend))


def peaks_rows(name: str, c: PeakCounts, peak_file: str = ""):
    """The first block of ``_peaks.tab``: (label, value) pairs; the floats with ``repr`` (they read back exactly)."""
    return [("Name", name), ("Peak file", peak_file), ("Extend", c.extend), ("Lines", c.n_lines), ("Peak bases", c.union_bases),
            ("Genome bases", c.genome_bases), ("Reads", c.N), ("Reads in peaks", c.n_in), ("FRiP", repr(float(c.frip))),
            ("Enrichment", repr(float(c.enrichment)))]


def write_peaks(path_base, name: str, c: PeakCounts, peak_file: str = "") -> Path:
    """Writes ``<path_base>_peaks.tab`` (to a temporary file beside it, renamed into place) and returns its path: the label /
    value block, one row per chosen reference, and ``#chrom start end reads`` for every line -- in file order per reference, the
    references in header order, the intervals as they were read: BED from that header line down."""
    path = Path(str(path_base) + PEAKS_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w") as fp:
            for label, value in peaks_rows(name, c, peak_file):
                fp.write("{}\t{}\n".format(label, value))
            fp.write("\t".join(_REF_HEADER) + "\n")
            for chrom, (reads, inside) in c.per_reference.items():
                fp.write("{}\t{}\t{}\t{}\n".format(chrom, c.counts[chrom].size, reads, inside))
            fp.write("\t".join(_LINE_HEADER) + "\n")
            for chrom, (b, e) in c.lines.items():
                for row in zip(b.tolist(), e.tolist(), c.counts[chrom].tolist()):
                    fp.write("{}\t{}\t{}\t{}\n".format(chrom, *row))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def read_peaks(path) -> Tuple[str, PeakCounts, Dict[str, object]]:
    """(name, PeakCounts, the label / value block as written: ``FRiP`` and ``Enrichment`` as float) of a ``_peaks.tab``."""
    with open(path) as fp:
        rows = [ln.rstrip("\n").split("\t") for ln in fp if ln.strip()]
    at_ref = rows.index(list(_REF_HEADER))
    at_line = rows.index(list(_LINE_HEADER))
    head = {row[0]: row[1] if len(row) > 1 else "" for row in rows[:at_ref]}
    per = {row[0]: (int(row[2]), int(row[3])) for row in rows[at_ref + 1:at_line]}
    cols = {k: ([], [], []) for k in per}
    for chrom, b, e, n in rows[at_line + 1:]:
        for col, x in zip(cols[chrom], (b, e, n)):
            col.append(int(x))
    c = PeakCounts({k: (v[0], v[1]) for k, v in cols.items()}, {k: v[2] for k, v in cols.items()}, per, int(head["Peak bases"]),
                   int(head["Genome bases"]), int(head["Extend"]))
    block = {k: (float(v) if k in ("FRiP", "Enrichment") else v) for k, v in head.items()}
    return head["Name"], c, block
