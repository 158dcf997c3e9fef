"""The fingerprint of an alignment file and its Jensen-Shannon distance: how unevenly the reads are spread over
the genome, beside NSC / RSC and NRF / PBC.

The reads are the ones the correlation sees (``-q``, ``PMX_BAM_DEFAULT_EXCLUDE``, the chosen chromosomes, the region mask).  A
chosen reference of length ``len`` has ``len // bin_size`` bins, bin ``j`` covering the 1-based positions ``j * bin_size + 1 ..
(j + 1) * bin_size``; the tail shorter than a bin has none, and the chosen references' bins lie end to end in header order.  A
read covers ``[pos1, pos1 + L - 1]`` when forward and ``[pos1 + read_len - L, pos1 + read_len - 1]`` when reverse, with ``L =
extend`` or, with ``extend`` 0, its own length; the extent is clipped to ``[1, len]`` and the read adds 1 to every bin it
overlaps.  Everything reported is a function of one integer table, ``H[k]`` = the number of bins that hold exactly ``k`` reads.
The definitions are this project's own: they were not compared with deepTools' plotFingerprint.

A device reader counts on the GPU (``pmx_dbam_bincount_*``, include/pymasc_amd_ingest.h); a host reader goes through its
``batches`` and ``count_host`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import math
import os
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from .complexity import _ratio, _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, PMX_BINCOUNT_HIST, SideAccumulator, count_over

FINGERPRINT_SUFFIX = "_fingerprint.tab"
DEFAULT_BIN = 500
NO_BINS = "no chosen reference is as long as one bin"
TOO_MANY_BINS = "2^31 bins or more: choose a larger bin size"
ZERO_BIN = "the bin size is 0"
_REF_HEADER = ("chrom", "bins")
_HIST_HEADER = ("count", "bins")
_NAN = float("nan")


def jsd(k_p, p, k_q, q) -> float:
    """The Jensen-Shannon distance (base 2, in [0, 1]) of two distributions given as (values, probabilities), over the union of
    their values: ``sqrt(1/2 sum p log2(p / m) + 1/2 sum q log2(q / m))`` with ``m = (p + q) / 2`` and ``0 log 0 = 0``."""
    keys = np.union1d(np.asarray(k_p, dtype=np.int64), np.asarray(k_q, dtype=np.int64))
    a, b = np.zeros(keys.size), np.zeros(keys.size)
    a[np.searchsorted(keys, k_p)] = p
    b[np.searchsorted(keys, k_q)] = q
    m = (a + b) / 2

    def half(x):
        on = (x > 0) & (m > 0)                 # (a share so small that m underflows adds nothing)
        return float(np.sum(x[on] * np.log2(x[on] / m[on])))
    return math.sqrt(max(0.5 * half(a) + 0.5 * half(b), 0.0))


def _curve(k, w) -> Tuple[np.ndarray, np.ndarray]:
    """(X, Y) at the breakpoints of the fingerprint: bins sorted ascending by count, ``w`` the share of the bins at count ``k``;
    X the cumulative share of bins, Y the cumulative share of reads."""
    k, w = np.asarray(k, dtype=np.float64), np.asarray(w, dtype=np.float64)
    kw = k * w
    return np.cumsum(w), np.cumsum(kw) / kw.sum()


def _auc(k, w) -> float:
    """The area under the fingerprint, trapezoids over the breakpoints: perfectly even counts give 0.5."""
    _x, y = _curve(k, w)
    return float(np.sum(np.asarray(w, dtype=np.float64) * (np.concatenate(([0.0], y[:-1])) + y) / 2))


class BinCounts:
    """``H`` as ``values`` (the counts that occur, ascending) and ``bins`` (how many bins hold each), int64; ``per_reference``:
    ``{name: bins}`` of the chosen references in header order; ``reads``: the reads that added to at least one bin."""

    def __init__(self, bin_size: int, extend: int, per_reference: Dict[str, int], values, bins, reads: int):
        self.bin_size, self.extend, self.reads = int(bin_size), int(extend), int(reads)
        self.per_reference = {str(k): int(v) for k, v in per_reference.items()}
        values, bins = np.asarray(values, dtype=np.int64).ravel(), np.asarray(bins, dtype=np.int64).ravel()
        order = np.argsort(values, kind="stable")
        self.values, self.bins = values[order].copy(), bins[order].copy()
        if self.values.size != self.bins.size or np.any(np.diff(self.values) <= 0) or np.any(self.bins <= 0):
            raise ValueError("H needs distinct counts and a positive number of bins for each")

    @classmethod
    def from_counts(cls, bin_size, extend, per_reference, counts, reads) -> "BinCounts":
        values, bins = np.unique(np.asarray(counts), return_counts=True)
        return cls(bin_size, extend, per_reference, values, bins, reads)

    B = property(lambda self: int(self.bins.sum()))
    T = property(lambda self: int(np.sum(self.values * self.bins)))
    mean = property(lambda self: _ratio(self.T, self.B))
    kmax = property(lambda self: int(self.values[-1]) if self.values.size else 0)

    def _p(self) -> np.ndarray:
        return self.bins / float(self.B)

    @property
    def x_intercept(self) -> float:
        """The share of the bins without a read."""
        return float(self.bins[0]) / self.B if self.values.size and self.values[0] == 0 else 0.0

    @property
    def auc(self) -> float:
        return _auc(self.values, self._p()) if self.T else _NAN

    @property
    def elbow(self) -> float:
        """X where the fingerprint lies farthest below the diagonal (the first such breakpoint)."""
        if not self.T:
            return _NAN
        x, y = _curve(self.values, self._p())
        return float(x[int(np.argmax(x - y))])

    def poisson(self) -> Tuple[np.ndarray, np.ndarray]:
        """(k, q): the Poisson model with the mean of the bins over ``0 .. max(kmax, ceil(mean + 10 sqrt(mean) + 20))``,
        renormalised to sum to 1."""
        lam = self.mean
        top = max(self.kmax, int(math.ceil(lam + 10 * math.sqrt(lam) + 20)))
        k = np.arange(top + 1, dtype=np.float64)
        logq = k * math.log(lam) - lam - np.frompyfunc(math.lgamma, 1, 1)(k + 1).astype(np.float64)
        q = np.exp(logq - logq.max())
        return np.arange(top + 1, dtype=np.int64), q / q.sum()

    @property
    def synthetic_auc(self) -> float:
        return _auc(*self.poisson()) if self.T else _NAN

    @property
    def synthetic_jsd(self) -> float:
        return jsd(self.values, self._p(), *self.poisson()) if self.T else _NAN

    def jsd_to(self, other: "BinCounts") -> float:
        """The Jensen-Shannon distance between the two tables' shares of bins per count; no depth scaling."""
        if not self.T or not other.T:
            return _NAN
        return jsd(self.values, self._p(), other.values, other._p())

    def __eq__(self, other) -> bool:
        return (isinstance(other, BinCounts) and (self.bin_size, self.extend, self.reads) == (other.bin_size, other.extend, other.reads)
                and list(self.per_reference.items()) == list(other.per_reference.items())
                and np.array_equal(self.values, other.values) and np.array_equal(self.bins, other.bins))

    __hash__ = None

    def __repr__(self) -> str:
        return "BinCounts(bin_size={}, extend={}, B={}, T={}, reads={}, kmax={})".format(self.bin_size, self.extend, self.B, self.T,
                                                                                        self.reads, self.kmax)


def layout(lengths: Sequence[int], use, bin_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """(first bin, number of bins) of every reference, int64; a reference that is not in ``use`` has no bins.  ValueError for
    a bin size of 0, no bin at all, or 2^31 bins or more (the messages of ``pmx_dbam_bincount_begin``)."""
    if int(bin_size) < 1:
        raise ValueError(ZERO_BIN)
    nb = np.array([max(int(l), 0) // int(bin_size) if u else 0 for l, u in zip(lengths, use)], dtype=np.int64)
    total = int(nb.sum())
    if total == 0:
        raise ValueError(NO_BINS)
    if total >= 1 << 31:
        raise ValueError(TOO_MANY_BINS)
    return np.concatenate(([0], np.cumsum(nb)[:-1])).astype(np.int64), nb


def count_host(ref_id, pos1, read_len, reverse, lengths, use, bin_size: int, extend: int = 0) -> Tuple[np.ndarray, int]:
    """The host checker, plain numpy: (the count of every bin, int64; the reads that added to a bin) of the reads given as four
    columns.  Each read marks its first bin +1 and the bin behind its last -1; a running sum gives the counts."""
    first, nb = layout(lengths, use, bin_size)
    total = int(nb.sum())
    ref = np.asarray(ref_id, dtype=np.int64).ravel()
    pos = np.asarray(pos1, dtype=np.int64).ravel()
    rl = np.asarray(read_len, dtype=np.int64).ravel()
    rev = np.asarray(reverse).ravel().astype(bool)
    inside = (ref >= 0) & (ref < len(nb))
    ref, pos, rl, rev = ref[inside], pos[inside], rl[inside], rev[inside]
    span = np.full(ref.size, int(extend), dtype=np.int64) if extend else rl
    lo = np.maximum(np.where(rev, pos + rl - span, pos), 1)
    hi = np.minimum(np.where(rev, pos + rl - 1, pos + span - 1), nb[ref] * int(bin_size))
    on = (lo <= hi) & np.asarray(use, dtype=bool)[ref]
    steps = np.zeros(total + 1, dtype=np.int64)
    np.add.at(steps, first[ref[on]] + (lo[on] - 1) // int(bin_size), 1)
    np.add.at(steps, first[ref[on]] + (hi[on] - 1) // int(bin_size) + 1, -1)
    return np.cumsum(steps)[:total], int(on.sum())


def _per_reference(names, use, nb) -> Dict[str, int]:
    return {n: int(nb[i]) for i, n in enumerate(names) if use[i]}


class DeviceCount(SideAccumulator):
    """The table a device reader's handle holds between ``pmx_dbam_bincount_begin`` and the next one: ``add`` counts what the
    handle holds now (a stream reader calls it for every window), ``result`` reads ``H`` back."""

    def __init__(self, reader, mapq_criteria: int, references=None, bin_size: int = DEFAULT_BIN, extend: int = 0):
        reader._check_open()
        if int(bin_size) < 0 or int(extend) < 0:
            raise ValueError("bin_size and extend are not negative")
        self.mapq_criteria, self.bin_size, self.extend = int(mapq_criteria), int(bin_size), int(extend)
        self.names = tuple(reader.references)
        self.use = _selected_mask(reader, references)
        self.begin(reader)
        self.nb = np.array([int(l) // self.bin_size if u else 0 for l, u in zip(reader.lengths, self.use)], dtype=np.int64)

    def begin(self, reader) -> None:
        """A zeroed table on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        mask = np.ascontiguousarray(self.use, dtype=np.uint8) if self.names else np.zeros(1, dtype=np.uint8)
        rc = reader._L.pmx_dbam_bincount_begin(reader._h, self.bin_size, self.extend, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> int:
        import ctypes
        added = ctypes.c_uint64()
        rc = reader._L.pmx_dbam_bincount_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(added))
        if rc:
            reader._raise(rc)
        return int(added.value)

    def tables(self, reader) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(hist uint64 [PMX_BINCOUNT_HIST], totals uint64 [3] = B, T, reads, the values of the bins at or above the table)."""
        hist = np.zeros(PMX_BINCOUNT_HIST, dtype=np.uint64)
        totals = np.zeros(3, dtype=np.uint64)
        n = reader._L.pmx_dbam_bincount_hist(reader._h, hist.ctypes.data, totals.ctypes.data, 0, None)
        if n < 0:
            reader._raise(n)
        tail = np.zeros(max(int(n), 1), dtype=np.uint32)
        if n:
            m = reader._L.pmx_dbam_bincount_hist(reader._h, hist.ctypes.data, totals.ctypes.data, int(n), tail.ctypes.data)
            if m < 0:
                reader._raise(m)
            assert m == n
        return hist, totals, tail[:int(n)]

    def counts(self, reader) -> np.ndarray:
        """Every bin's count (``pmx_dbam_bincount_copy``), uint32."""
        out = np.zeros(int(self.nb.sum()), dtype=np.uint32)
        rc = reader._L.pmx_dbam_bincount_copy(reader._h, 0, out.size, out.ctypes.data)
        if rc:
            reader._raise(rc)
        return out

    def result(self, reader) -> BinCounts:
        hist, totals, tail = self.tables(reader)
        low = np.flatnonzero(hist)
        high, nhigh = np.unique(tail, return_counts=True)       # the host finishes the table: exact for any count
        c = BinCounts(self.bin_size, self.extend, _per_reference(self.names, self.use, self.nb),
                      np.concatenate((low, high.astype(np.int64))), np.concatenate((hist[low].astype(np.int64), nhigh)), int(totals[2]))
        if (c.B, c.T) != (int(totals[0]), int(totals[1])):
            raise RuntimeError("pmx_dbam_bincount_hist: the table does not add up to its totals")
        return c


def count_device(reader, mapq_criteria: int, references=None, bin_size: int = DEFAULT_BIN, extend: int = 0) -> BinCounts:
    """``begin`` + ``add`` + ``hist`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, mapq_criteria, references, bin_size, extend)
    acc.add(reader)
    return acc.result(reader)


def from_reader(reader, mapq_criteria: int = 0, references=None, bin_size: int = DEFAULT_BIN, extend: int = 0) -> BinCounts:
    """The bin counts of the reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the
    reader has selected).  A device reader counts on the GPU -- window by window for a stream reader, which is read once more
    when it is a regular file and raises ``InputUnseekable`` otherwise; a host reader through ``batches`` and ``count_host``."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        return count_over(reader, "fingerprint",
                          lambda: DeviceCount(reader, mapq_criteria, references, bin_size, extend)).result(reader)
    if int(bin_size) < 0 or int(extend) < 0:
        raise ValueError("bin_size and extend are not negative")
    use = _selected_mask(reader, references)
    _first, nb = layout(reader.lengths, use, bin_size)
    counts, reads = np.zeros(int(nb.sum()), dtype=np.int64), 0
    for batch in reader.batches(mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE):
        if len(batch[0]):
            c, n = count_host(*batch, reader.lengths, use, bin_size, extend)
            counts += c
            reads += n
    return BinCounts.from_counts(bin_size, extend, _per_reference(reader.references, use, nb), counts, reads)


def fingerprint_rows(name: str, c: BinCounts, control: Optional[BinCounts] = None, control_name: str = ""):
    """The first block of ``_fingerprint.tab``: (label, value) pairs; the floats with ``repr`` (they read back exactly)."""
    rows = [("Name", name), ("Bin size", c.bin_size), ("Extend", c.extend), ("Bins", c.B), ("Reads", c.reads),
            ("Mean", repr(float(c.mean))), ("X-intercept", repr(float(c.x_intercept))), ("AUC", repr(float(c.auc))),
            ("Synthetic AUC", repr(float(c.synthetic_auc))), ("Elbow", repr(float(c.elbow))),
            ("Synthetic JS distance", repr(float(c.synthetic_jsd)))]
    if control is not None:
        rows += [("Control", control_name), ("Control mean", repr(float(control.mean))), ("JS distance", repr(float(c.jsd_to(control))))]
    return rows


_FLOAT_ROWS = ("Mean", "X-intercept", "AUC", "Synthetic AUC", "Elbow", "Synthetic JS distance", "Control mean", "JS distance")


def write_fingerprint(path_base, name: str, c: BinCounts, control: Optional[BinCounts] = None, control_name: str = "") -> Path:
    """Writes ``<path_base>_fingerprint.tab`` (to a temporary file beside it, renamed into place) and returns its path: the
    label / value block, one row per chosen reference, and ``H`` as one row per count that occurs."""
    path = Path(str(path_base) + FINGERPRINT_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w") as fp:
            for label, value in fingerprint_rows(name, c, control, control_name):
                fp.write("{}\t{}\n".format(label, value))
            fp.write("\t".join(_REF_HEADER) + "\n")
            for chrom, nb in c.per_reference.items():
                fp.write("{}\t{}\n".format(chrom, nb))
            fp.write("\t".join(_HIST_HEADER) + "\n")
            for k, n in zip(c.values.tolist(), c.bins.tolist()):
                fp.write("{}\t{}\n".format(k, n))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def read_fingerprint(path) -> Tuple[str, BinCounts, Dict[str, object]]:
    """(name, BinCounts, the label / value block as written: floats as float, ``Control`` as str) of a ``_fingerprint.tab``."""
    with open(path) as fp:
        lines = [ln.rstrip("\n").split("\t") for ln in fp if ln.strip()]
    at_ref = lines.index(list(_REF_HEADER))
    at_hist = lines.index(list(_HIST_HEADER))
    head = {row[0]: row[1] if len(row) > 1 else "" for row in lines[:at_ref]}
    per = {row[0]: int(row[1]) for row in lines[at_ref + 1:at_hist]}
    table = np.array([[int(x) for x in row[:2]] for row in lines[at_hist + 1:]], dtype=np.int64).reshape(-1, 2)
    c = BinCounts(int(head["Bin size"]), int(head["Extend"]), per, table[:, 0], table[:, 1], int(head["Reads"]))
    block = {k: (float(v) if k in _FLOAT_ROWS else v) for k, v in head.items()}
    return head["Name"], c, block
