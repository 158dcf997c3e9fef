"""Library complexity: ENCODE's NRF, PBC1 and PBC2 beside NSC and RSC.

A read is what the run's filter keeps (``-q``; read2, unmapped, no reference and query length 0 dropped) EXCEPT that flagged
duplicates (0x400) are kept: complexity is a statement about duplicates.  Its key is ``(ref_id, pos1, read_len, reverse)``,
compared in full.  With N reads, D distinct keys, M1 keys seen once and M2 keys seen twice: NRF = D / N, PBC1 = M1 / D,
PBC2 = M1 / M2.  A device reader counts on the GPU (``pmx_dbam_complexity``, include/pymasc_amd_ingest.h); a host reader goes
through its ``batches`` and ``count_host`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, Sequence, Tuple

import numpy as np

from .native import PMX_BAM_DEFAULT_EXCLUDE, PMX_BAM_FLAG_DUPLICATE, PMX_COMPLEXITY_BINS, SideAccumulator, count_over

#: the filter of the complexity count: the run's, with flagged duplicates kept
COMPLEXITY_EXCLUDE = PMX_BAM_DEFAULT_EXCLUDE & ~PMX_BAM_FLAG_DUPLICATE
COMPLEXITY_SUFFIX = "_complexity.tab"
_LAST = PMX_COMPLEXITY_BINS - 1
_REF_HEADER = ("chrom", "reads", "distinct", "one", "two")
_HIST_HEADER = ("multiplicity", "positions")


def _ratio(num: int, den: int) -> float:
    """num / den; a zero denominator gives nan when the numerator is zero too, else inf."""
    if den:
        return num / den
    return float("nan") if num == 0 else float("inf")


class LibraryComplexity:
    """``per_reference``: ``{name: (N, D, M1, M2)}`` in header order, the chosen references only.  ``hist``: int64 array of
    ``PMX_COMPLEXITY_BINS``; ``hist[k]`` keys seen exactly k times for 1 <= k < 31, ``hist[31]`` keys seen at least 31 times,
    ``hist[0]`` the largest multiplicity.  A key never spans two references, so counts of disjoint sets of references, of the
    windows of a stream (as ``pmx_dbam_complexity`` cuts them) or of ranks add up (``+``)."""

    def __init__(self, per_reference: Dict[str, Tuple[int, int, int, int]], hist):
        self.per_reference = {str(k): tuple(int(x) for x in v) for k, v in per_reference.items()}
        self.hist = np.asarray(hist, dtype=np.int64).copy()
        if self.hist.shape != (PMX_COMPLEXITY_BINS,):
            raise ValueError("hist has {} bins".format(PMX_COMPLEXITY_BINS))

    def _sum(self, k: int) -> int:
        return sum(v[k] for v in self.per_reference.values())

    reads = property(lambda self: self._sum(0))
    distinct = property(lambda self: self._sum(1))
    m1 = property(lambda self: self._sum(2))
    m2 = property(lambda self: self._sum(3))
    nrf = property(lambda self: _ratio(self.distinct, self.reads))
    pbc1 = property(lambda self: _ratio(self.m1, self.distinct))
    pbc2 = property(lambda self: _ratio(self.m1, self.m2))
    max_multiplicity = property(lambda self: int(self.hist[0]))

    def __add__(self, other: "LibraryComplexity") -> "LibraryComplexity":
        if not isinstance(other, LibraryComplexity):
            return NotImplemented
        per = dict(self.per_reference)
        for name, v in other.per_reference.items():
            per[name] = tuple(a + b for a, b in zip(per.get(name, (0, 0, 0, 0)), v))
        hist = self.hist + other.hist
        hist[0] = max(int(self.hist[0]), int(other.hist[0]))
        return LibraryComplexity(per, hist)

    def __eq__(self, other) -> bool:
        return (isinstance(other, LibraryComplexity) and list(self.per_reference.items()) == list(other.per_reference.items())
                and np.array_equal(self.hist, other.hist))

    __hash__ = None

    def __repr__(self) -> str:
        return "LibraryComplexity(reads={}, distinct={}, m1={}, m2={}, max_multiplicity={})".format(
            self.reads, self.distinct, self.m1, self.m2, self.max_multiplicity)


def _chosen(reader_references: Sequence[str], references) -> np.ndarray:
    """uint8 mask over the header's references: the chosen ones (None: all); an unknown name is a ValueError."""
    names = list(reader_references)
    if references is None:
        return np.ones(max(len(names), 1), dtype=np.uint8)[:len(names)]
    want = [references] if isinstance(references, str) else list(references)
    for n in want:
        if n not in names:
            raise ValueError("unknown reference {}".format(n))
    want = set(want)
    return np.array([1 if n in want else 0 for n in names], dtype=np.uint8)


def _from_tables(names: Sequence[str], use: np.ndarray, per_ref: np.ndarray, hist: np.ndarray) -> LibraryComplexity:
    return LibraryComplexity({n: tuple(per_ref[i]) for i, n in enumerate(names) if use[i]}, hist)


def count_host(ref_id, pos1, read_len, reverse, nref: int) -> Tuple[np.ndarray, np.ndarray]:
    """The host checker, plain numpy: (per_ref int64 [nref, 4] = N, D, M1, M2 of every reference; hist) of the reads given as
    four columns.  ``np.unique`` over the rows with their counts; no GPU."""
    per_ref = np.zeros((int(nref), 4), dtype=np.int64)
    hist = np.zeros(PMX_COMPLEXITY_BINS, dtype=np.int64)
    ref_id = np.asarray(ref_id, dtype=np.int64).ravel()
    if ref_id.size == 0:
        return per_ref, hist
    rows = np.stack([ref_id, np.asarray(pos1, dtype=np.int64).ravel(), np.asarray(read_len, dtype=np.int64).ravel(),
                     np.asarray(reverse).ravel().astype(bool).astype(np.int64)], axis=1)
    keys, counts = np.unique(rows, axis=0, return_counts=True)
    refs = keys[:, 0]
    for k, w in enumerate((counts, None, counts == 1, counts == 2)):
        per_ref[:, k] = np.bincount(refs, weights=None if w is None else w.astype(np.float64), minlength=int(nref))[:int(nref)]
    hist[:] = np.bincount(np.minimum(counts, _LAST), minlength=PMX_COMPLEXITY_BINS)
    hist[0] = counts.max()
    return per_ref, hist


def count_device(reader, mapq_criteria: int, use: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """One ``pmx_dbam_complexity`` call on a device reader's handle (a stream reader: its current window)."""
    reader._check_open()
    nref = len(reader.references)
    per_ref = np.zeros((max(nref, 1), 4), dtype=np.uint64)
    hist = np.zeros(PMX_COMPLEXITY_BINS, dtype=np.uint64)
    mask = np.ascontiguousarray(use, dtype=np.uint8) if nref else np.zeros(1, dtype=np.uint8)
    rc = reader._L.pmx_dbam_complexity(reader._h, int(mapq_criteria), COMPLEXITY_EXCLUDE, mask.ctypes.data, per_ref.ctypes.data,
                                       hist.ctypes.data)
    if rc:
        reader._raise(rc)
    return per_ref[:nref].astype(np.int64), hist.astype(np.int64)


class WindowedCount(SideAccumulator):
    """The sum of a stream reader's ``pmx_dbam_complexity`` calls: ``DeviceStreamReader`` calls ``count`` when a window has
    been worked on (``add``), and once more behind the last window (``flush``: the records the library held back).  The sums
    live on the host: a new handle does not reset them (no ``begin``)."""

    def __init__(self, reader, mapq_criteria: int, references=None):
        self.mapq_criteria = int(mapq_criteria)
        self.names = tuple(reader.references)
        self.use = _selected_mask(reader, references)
        self.per_ref = np.zeros((len(self.names), 4), dtype=np.int64)
        self.hist = np.zeros(PMX_COMPLEXITY_BINS, dtype=np.int64)

    def count(self, reader) -> None:
        per_ref, hist = count_device(reader, self.mapq_criteria, self.use)
        self.per_ref += per_ref
        top = max(int(self.hist[0]), int(hist[0]))
        self.hist += hist
        self.hist[0] = top

    add = flush = count

    def result(self, reader=None) -> LibraryComplexity:
        return _from_tables(self.names, self.use, self.per_ref, self.hist)


def _selected_mask(reader, references) -> np.ndarray:
    """The chosen references among those the reader has selected (a reader without a selection: among all)."""
    use = _chosen(reader.references, references)
    selected = getattr(reader, "_selected", None)
    if selected is not None and references is None:
        use = np.array([1 if i in selected else 0 for i in range(len(reader.references))], dtype=np.uint8)
    elif selected is not None:
        for i, n in enumerate(reader.references):
            if use[i] and i not in selected:
                raise ValueError("reference {} was not selected".format(n))
    return use


def from_reader(reader, mapq_criteria: int = 0, references=None) -> LibraryComplexity:
    """The complexity of the reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the
    reader has selected).  A device reader counts on the GPU -- window by window for a stream reader, which is read once more
    when it is a regular file and raises ``InputUnseekable`` otherwise; a host reader through ``batches`` and ``count_host``."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        return count_over(reader, "complexity", lambda: WindowedCount(reader, mapq_criteria, references)).result()
    use = _selected_mask(reader, references)
    cols = [[], [], [], []]
    for batch in reader.batches(mapq_criteria, COMPLEXITY_EXCLUDE):
        keep = use[batch[0]].astype(bool) if len(batch[0]) else np.zeros(0, dtype=bool)
        for c, a in zip(cols, batch):
            c.append(np.asarray(a)[keep])
    if cols[0]:
        cols = [np.concatenate(c) for c in cols]
    per_ref, hist = count_host(*cols, len(reader.references))
    per_ref[~use.astype(bool)] = 0
    return _from_tables(reader.references, use, per_ref, hist)


def complexity_rows(name: str, c: LibraryComplexity):
    """The first block of ``_complexity.tab``: (label, value) pairs; the ratios with ``repr`` (they read back exactly)."""
    return [("Name", name), ("Reads", c.reads), ("Distinct positions", c.distinct), ("Positions with one read", c.m1),
            ("Positions with two reads", c.m2), ("Largest multiplicity", c.max_multiplicity), ("NRF", repr(float(c.nrf))),
            ("PBC1", repr(float(c.pbc1))), ("PBC2", repr(float(c.pbc2)))]


def write_complexity(path_base, name: str, c: LibraryComplexity) -> Path:
    """Writes ``<path_base>_complexity.tab`` (to a temporary file beside it, renamed into place) and returns its path: the
    label / value block, one row per chosen reference, and the non-empty bins of the multiplicity histogram (the last ``>=31``)."""
    path = Path(str(path_base) + COMPLEXITY_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w") as fp:
            for label, value in complexity_rows(name, c):
                fp.write("{}\t{}\n".format(label, value))
            fp.write("\t".join(_REF_HEADER) + "\n")
            for chrom, row in c.per_reference.items():
                fp.write("\t".join([chrom] + [str(x) for x in row]) + "\n")
            fp.write("\t".join(_HIST_HEADER) + "\n")
            for k in range(1, PMX_COMPLEXITY_BINS):
                if c.hist[k]:
                    fp.write("{}\t{}\n".format(">={}".format(_LAST) if k == _LAST else k, int(c.hist[k])))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def read_complexity(path) -> Tuple[str, LibraryComplexity, Dict[str, float]]:
    """(name, LibraryComplexity, {"NRF": ..., "PBC1": ..., "PBC2": ...} as written) of a ``_complexity.tab`` file."""
    with open(path) as fp:
        lines = [ln.rstrip("\n").split("\t") for ln in fp if ln.strip()]
    at_ref = lines.index(list(_REF_HEADER))
    at_hist = lines.index(list(_HIST_HEADER))
    head = {row[0]: row[1] for row in lines[:at_ref]}
    per = {row[0]: tuple(int(x) for x in row[1:5]) for row in lines[at_ref + 1:at_hist]}
    hist = np.zeros(PMX_COMPLEXITY_BINS, dtype=np.int64)
    for label, count in lines[at_hist + 1:]:
        hist[_LAST if label.startswith(">=") else int(label)] = int(count)
    hist[0] = int(head["Largest multiplicity"])
    return head["Name"], LibraryComplexity(per, hist), {k: float(head[k]) for k in ("NRF", "PBC1", "PBC2")}
