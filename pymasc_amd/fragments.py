"""Paired-end fragment sizes of an alignment file: ``--fragments`` / ``fragments=``, the histogram of fragment
sizes with median and spread per orientation, beside the fragment length the cross-correlation estimates (``_stats.tab``).

The definitions, which the device code (csrc/ingest/fragments_device.inc), the host path here and the tests state the same way.
They are this project's own, modelled on Picard's CollectInsertSizeMetrics and deepTools' bamPEFragmentSize; nothing here was
compared with either's output.

**The pair rule.**  A pair is counted at its read1 record, from that record's own fields; nothing is matched.  A record that passes
the run's filter (``-q``, ``PMX_BAM_DEFAULT_EXCLUDE``, ``ref_id >= 0``, query length > 0, on a chosen reference) counts in
``reads``.  With flag 0x1 it also counts in ``paired`` and in exactly one of the following, the first that holds:

1. flag 0x8: ``mate_unmapped``;
2. the mate's reference is not the record's own (BAM: ``next_refID != refID``; SAM: RNEXT is neither ``=`` nor byte-equal to RNAME):
   ``mate_elsewhere``;
3. ``tlen == 0``, ``tlen == -2^31`` or the mate's position is unknown (``mate_pos1 = next_pos + 1 = PNEXT <= 0``): ``no_size``;
4. otherwise it is a *fragment*: ``size = |tlen|``, ``start1 = min(pos1, mate_pos1)`` and an orientation -- ``TANDEM`` (2) when
   bit 0x10 equals bit 0x20 shifted down, ``FR`` (0) when the read is forward and ``tlen > 0`` or reverse and ``tlen < 0``, ``RF``
   (1) in every other case.  No reference span from the CIGAR is needed; the rule differs from Picard's only where one read
   contains the other's far end.

**Size bound.**  A fragment with ``size > max_size`` (1 .. 65536, default 2000) counts in ``over[orientation]`` and goes no
further.  Any other becomes a *row* ``(ref_id, start1, size, orientation)``, counted in ``rows``.

**Mask.**  An exclude mask drops a row when it would drop a read with the row's extent ``[start1, start1 + size - 1]`` -- the
fragment's extent, not read1's; the dropped rows count in ``masked``.

**Table.**  ``H[o][s - 1]`` is the number of rows left with orientation ``o`` and size ``s``, 64-bit.
``paired == mate_unmapped + mate_elsewhere + no_size + sum(over) + rows`` and ``rows - masked == sum(H)``.

**Statistics**, per orientation with ``n = sum_s H[o][s] > 0``, from exact integers and one float operation each: ``mean``,
``sd`` (``n - 1`` below; nan for ``n = 1``), ``median`` (the mean of the two middle values for even ``n``), ``q25`` / ``q75`` (the
smallest ``s`` whose cumulative count reaches ``ceil(q n)``), ``mad`` (the median of ``|s - median|``), ``mode`` (the smallest ``s``
with the largest count), ``min``, ``max``.

A device reader counts on the GPU (``pmx_dbam_fragments_*``, include/pymasc_amd_ingest.h); a host reader goes through its
``mate_batches`` and ``rows_host`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import ctypes
import math
import os
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Tuple

import numpy as np

from .complexity import _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, PMX_FRAGMENTS_COUNTERS, PMX_FRAGMENTS_MAX_SIZE, SideAccumulator, count_over

FRAGMENTS_SUFFIX = "_fragments.tab"
DEFAULT_MAX_SIZE = 2000
MAX_SIZE = PMX_FRAGMENTS_MAX_SIZE
BAD_MAX_SIZE = "max_size is {}: it must lie in [1, 65536]"
NO_MATES = "the input has no mate fields"
FR, RF, TANDEM = 0, 1, 2
ORIENTATIONS = ("FR", "RF", "TANDEM")
COUNTERS = ("reads", "paired", "mate_unmapped", "mate_elsewhere", "no_size", "over_fr", "over_rf", "over_tandem", "rows", "masked")
_LABELS = ("Reads", "Paired", "Mate unmapped", "Mate elsewhere", "No size", "Over FR", "Over RF", "Over TANDEM", "Rows", "Masked")
STATS = ("n", "mean", "sd", "median", "q25", "q75", "mad", "mode", "min", "max")
_STAT_HEADER = ("orientation",) + STATS
_SIZE_HEADER = ("size", "fr", "rf", "tandem")
_REF_HEADER = ("chrom", "length")
_NAN = float("nan")
assert len(COUNTERS) == PMX_FRAGMENTS_COUNTERS


def check_max_size(max_size) -> int:
    if isinstance(max_size, (bool, str)) or int(max_size) != max_size or not 1 <= int(max_size) <= MAX_SIZE:
        raise ValueError(BAD_MAX_SIZE.format(max_size))
    return int(max_size)


def _weighted_median2(values: List[int], counts: List[int], n: int) -> int:
    """Twice the median of the multiset (``values`` ascending with ``counts``, ``n`` elements): the sum of its two middle elements
    (the same one twice for odd ``n``), an exact integer."""
    lo_at, hi_at = (n - 1) // 2, n // 2
    lo = hi = None
    cum = 0
    for v, c in zip(values, counts):
        cum += c
        if lo is None and cum > lo_at:
            lo = v
        if cum > hi_at:
            hi = v
            break
    return lo + hi


def size_stats(hist_row) -> Optional[Dict[str, object]]:
    """The statistics of one orientation's counts (``hist_row[s - 1]`` = rows of size ``s``), or None without a row."""
    h = np.asarray(hist_row, dtype=np.uint64)
    at = np.flatnonzero(h)
    if at.size == 0:
        return None
    sizes = [int(x) + 1 for x in at.tolist()]
    counts = [int(x) for x in h[at].tolist()]
    n = sum(counts)
    s1 = sum(s * c for s, c in zip(sizes, counts))
    s2 = sum(s * s * c for s, c in zip(sizes, counts))
    med2 = _weighted_median2(sizes, counts, n)

    def quantile(num: int, den: int) -> int:
        need, cum = (num * n + den - 1) // den, 0
        for s, c in zip(sizes, counts):
            cum += c
            if cum >= need:
                return s
        return sizes[-1]
    dev: Dict[int, int] = {}                    # |2 s - 2 median| -> count
    for s, c in zip(sizes, counts):
        d = abs(2 * s - med2)
        dev[d] = dev.get(d, 0) + c
    dv = sorted(dev)
    mad4 = _weighted_median2(dv, [dev[d] for d in dv], n)
    top = max(counts)
    return {"n": n, "mean": s1 / n, "sd": math.sqrt((n * s2 - s1 * s1) / (n * (n - 1))) if n > 1 else _NAN, "median": med2 / 2,
            "q25": quantile(1, 4), "q75": quantile(3, 4), "mad": mad4 / 4, "mode": sizes[counts.index(top)], "min": sizes[0],
            "max": sizes[-1]}


class FragmentSizes:
    """``hist``: uint64 ``[3][max_size]``, ``hist[o][s - 1]`` the rows of orientation ``o`` (``FR``, ``RF``, ``TANDEM``) and size
    ``s``; ``counters``: the ten of ``COUNTERS`` in that order; ``per_reference``: ``{name: length}`` of the chosen references in
    header order.  ``stats(o)``: the statistics of one orientation (None without a row), each also a property of the FR rows
    (``median``, ``mean``, ...)."""

    def __init__(self, max_size: int, per_reference: Dict[str, int], hist, counters):
        self.max_size = check_max_size(max_size)
        self.per_reference = {str(k): int(v) for k, v in per_reference.items()}
        self.hist = np.asarray(hist, dtype=np.uint64).reshape(3, -1).copy()
        self.counters = {k: int(v) for k, v in zip(COUNTERS, [int(x) for x in np.asarray(counters).ravel().tolist()])}
        if self.hist.shape[1] != self.max_size or len(np.asarray(counters).ravel()) != len(COUNTERS):
            raise ValueError("hist holds 3 * max_size counts and counters ten")
        self._stats: Dict[int, Optional[dict]] = {}

    def stats(self, orientation: int = FR) -> Optional[Dict[str, object]]:
        o = int(orientation)
        if o not in self._stats:
            self._stats[o] = size_stats(self.hist[o])
        return self._stats[o]

    def _fr(self, key: str):
        st = self.stats(FR)
        return _NAN if st is None else st[key]

    n = property(lambda self: int(self.hist.sum(dtype=np.uint64)))
    over = property(lambda self: tuple(self.counters[k] for k in ("over_fr", "over_rf", "over_tandem")))
    mean = property(lambda self: self._fr("mean"))
    sd = property(lambda self: self._fr("sd"))
    median = property(lambda self: self._fr("median"))
    q25 = property(lambda self: self._fr("q25"))
    q75 = property(lambda self: self._fr("q75"))
    mad = property(lambda self: self._fr("mad"))
    mode = property(lambda self: self._fr("mode"))
    min = property(lambda self: self._fr("min"))
    max = property(lambda self: self._fr("max"))

    def check_identities(self) -> None:
        c = self.counters
        if c["paired"] != c["mate_unmapped"] + c["mate_elsewhere"] + c["no_size"] + sum(self.over) + c["rows"]:
            raise RuntimeError("fragment sizes: the counters of the pairs do not add up")
        if c["rows"] - c["masked"] != self.n:
            raise RuntimeError("fragment sizes: the table does not add up to rows - masked")

    def __eq__(self, other) -> bool:
        return (isinstance(other, FragmentSizes) and self.max_size == other.max_size and self.counters == other.counters
                and list(self.per_reference.items()) == list(other.per_reference.items()) and np.array_equal(self.hist, other.hist))

    __hash__ = None

    def __repr__(self) -> str:
        return "FragmentSizes(max_size={}, {})".format(self.max_size, ", ".join("{}={}".format(k, v) for k, v in self.counters.items()))


def _per_reference(names, lengths, use) -> Dict[str, int]:
    return {n: int(l) for n, l, u in zip(names, lengths, use) if u}


# ---- the host path: the checker, and what a run without device ingest uses ----

def classify(ref, pos1, flag, mate_ref, mate_pos1, tlen):
    """The pair rule on columns: (kind int8 -- 0 not paired, 1 mate_unmapped, 2 mate_elsewhere, 3 no_size, 4 a fragment --, size,
    start1, orientation); the last three mean something where kind is 4."""
    ref, pos1, flag = np.asarray(ref, dtype=np.int64), np.asarray(pos1, dtype=np.int64), np.asarray(flag, dtype=np.int64)
    mate_ref, mate_pos1 = np.asarray(mate_ref, dtype=np.int64), np.asarray(mate_pos1, dtype=np.int64)
    tlen = np.asarray(tlen, dtype=np.int64)
    kind = np.full(ref.size, 4, dtype=np.int8)
    kind[(tlen == 0) | (tlen == -(1 << 31)) | (mate_pos1 <= 0)] = 3
    kind[mate_ref != ref] = 2
    kind[(flag & 0x8) != 0] = 1
    kind[(flag & 0x1) == 0] = 0
    rev, mate_rev = (flag & 0x10) != 0, (flag & 0x20) != 0
    orient = np.where(rev == mate_rev, TANDEM, np.where((~rev & (tlen > 0)) | (rev & (tlen < 0)), FR, RF)).astype(np.uint8)
    return kind, np.abs(tlen), np.minimum(pos1, mate_pos1), orient


def rows_host(reader, mapq_criteria: int = 0, references=None, max_size: int = DEFAULT_MAX_SIZE
              ) -> Iterator[Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray, np.ndarray]]:
    """Per batch of a host reader's ``mate_batches``: (ref_id, start1, size int32, orientation uint8) of the rows left after the
    reader's mask, in file order, and the ten counters of the batch (int64, the order of ``COUNTERS``)."""
    max_size = check_max_size(max_size)
    if not hasattr(reader, "mate_batches"):
        raise ValueError(NO_MATES)
    use = np.asarray(_selected_mask(reader, references), dtype=bool)
    mask = getattr(reader, "_exclude", None)
    for ref, pos, _rlen, _rev, flag, mref, mpos, tlen in reader.mate_batches(int(mapq_criteria), PMX_BAM_DEFAULT_EXCLUDE):
        on = use[ref] if ref.size else np.zeros(0, dtype=bool)
        ref, pos, flag, mref, mpos, tlen = (x[on] for x in (ref, pos, flag, mref, mpos, tlen))
        kind, size, start1, orient = classify(ref, pos, flag, mref, mpos, tlen)
        c = np.zeros(len(COUNTERS), dtype=np.int64)
        c[0], c[1] = ref.size, int((kind != 0).sum())
        for k in (1, 2, 3):
            c[1 + k] = int((kind == k).sum())
        frag = kind == 4
        big = frag & (size > max_size)
        for o in range(3):
            c[5 + o] = int((big & (orient == o)).sum())
        row = frag & ~big
        r_ref, r_start, r_size, r_or = ref[row], start1[row].astype(np.int32), size[row].astype(np.int32), orient[row]
        c[8] = r_ref.size
        if mask is not None and r_ref.size:
            keep = mask.keep(r_ref, r_start, r_size)
            c[9] = int(r_ref.size - keep.sum())
            r_ref, r_start, r_size, r_or = r_ref[keep], r_start[keep], r_size[keep], r_or[keep]
        yield r_ref.astype(np.int32), r_start, r_size, r_or, c


def count_host(reader, mapq_criteria: int = 0, references=None, max_size: int = DEFAULT_MAX_SIZE) -> FragmentSizes:
    """The host checker, plain numpy: the table of the rows of ``rows_host``."""
    max_size = check_max_size(max_size)
    use = _selected_mask(reader, references)
    hist = np.zeros(3 * max_size, dtype=np.int64)
    counters = np.zeros(len(COUNTERS), dtype=np.int64)
    for _ref, _start, size, orient, c in rows_host(reader, mapq_criteria, references, max_size):
        counters += c
        if size.size:
            hist += np.bincount(orient.astype(np.int64) * max_size + size.astype(np.int64) - 1, minlength=3 * max_size)
    out = FragmentSizes(max_size, _per_reference(reader.references, reader.lengths, use), hist.reshape(3, max_size), counters)
    out.check_identities()
    return out


# ---- the device path ----

class DeviceCount(SideAccumulator):
    """The table a device reader's handle holds between ``pmx_dbam_fragments_begin`` and the next one: ``add`` counts what the
    handle holds now (a stream reader calls it for every window), ``result`` reads ``H`` and the counters back."""

    def __init__(self, reader, mapq_criteria: int, references=None, max_size: int = DEFAULT_MAX_SIZE):
        reader._check_open()
        self.mapq_criteria, self.max_size = int(mapq_criteria), check_max_size(max_size)
        self.names, self.lengths = tuple(reader.references), tuple(reader.lengths)
        self.use = _selected_mask(reader, references)
        self.begin(reader)

    def begin(self, reader) -> None:
        """A zeroed table on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        mask = np.ascontiguousarray(self.use, dtype=np.uint8) if self.names else np.zeros(1, dtype=np.uint8)
        rc = reader._L.pmx_dbam_fragments_begin(reader._h, self.max_size, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> int:
        """The rows of what the handle holds now that were added to the table."""
        out = ctypes.c_uint64()
        rc = reader._L.pmx_dbam_fragments_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(out))
        if rc:
            reader._raise(rc)
        return int(out.value)

    def result(self, reader) -> FragmentSizes:
        hist = np.zeros(3 * self.max_size, dtype=np.uint64)
        counters = np.zeros(len(COUNTERS), dtype=np.uint64)
        rc = reader._L.pmx_dbam_fragments_tables(reader._h, hist.ctypes.data, counters.ctypes.data)
        if rc:
            reader._raise(rc)
        out = FragmentSizes(self.max_size, _per_reference(self.names, self.lengths, self.use), hist.reshape(3, self.max_size), counters)
        out.check_identities()
        return out


def count_device(reader, mapq_criteria: int, references=None, max_size: int = DEFAULT_MAX_SIZE) -> FragmentSizes:
    """``begin`` + ``add`` + ``tables`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, mapq_criteria, references, max_size)
    acc.add(reader)
    return acc.result(reader)


def rows_device(reader, mapq_criteria: int = 0, references=None, max_size: int = DEFAULT_MAX_SIZE):
    """(ref_id, start1, size int32, orientation uint8) of the rows of what a device reader's handle holds now, after its mask
    (``pmx_dbam_fragments_rows``)."""
    reader._check_open()
    use = np.ascontiguousarray(_selected_mask(reader, references), dtype=np.uint8)
    args = (reader._h, int(mapq_criteria), PMX_BAM_DEFAULT_EXCLUDE, int(max_size), use.ctypes.data if use.size else None)
    n = reader._L.pmx_dbam_fragments_rows(*args, 0, None, None, None, None)
    if n < 0:
        reader._raise(n)
    cols = [np.zeros(max(int(n), 1), dtype=t) for t in (np.int32, np.int32, np.int32, np.uint8)]
    m = reader._L.pmx_dbam_fragments_rows(*args, int(n), *(c.ctypes.data for c in cols))
    if m < 0:
        reader._raise(m)
    assert m == n
    return tuple(c[:int(n)] for c in cols)


def from_reader(reader, mapq_criteria: int = 0, references=None, max_size: int = DEFAULT_MAX_SIZE) -> FragmentSizes:
    """The fragment sizes of the reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the
    reader has selected).  A device reader counts on the GPU -- window by window for a stream reader, which is read once more when
    it is a regular file and raises ``InputUnseekable`` otherwise; a host reader through ``count_host``.  A BED read file has no
    mate fields: ValueError (host) or ``PmxIOError`` (device)."""
    from .bam_device import DeviceBamReader
    max_size = check_max_size(max_size)
    if isinstance(reader, DeviceBamReader):
        return count_over(reader, "fragments", lambda: DeviceCount(reader, mapq_criteria, references, max_size)).result(reader)
    return count_host(reader, mapq_criteria, references, max_size)


# ---- the table ----

def _fmt(v) -> str:
    return repr(float(v)) if isinstance(v, float) else str(int(v))


def fragments_rows(name: str, c: FragmentSizes):
    """The first block of ``_fragments.tab``: (label, value) pairs."""
    return [("Name", name), ("Max size", c.max_size)] + [(label, c.counters[k]) for label, k in zip(_LABELS, COUNTERS)]


def write_fragments(path_base, name: str, c: FragmentSizes) -> Path:
    """Writes ``<path_base>_fragments.tab`` (to a temporary file beside it, renamed into place) and returns its path: the label /
    value block, one row per chosen reference, one statistics row per orientation that has rows (floats with ``repr``: they read
    back exactly), and one ``size / fr / rf / tandem`` line per size that occurs."""
    path = Path(str(path_base) + FRAGMENTS_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w") as fp:
            for label, value in fragments_rows(name, c):
                fp.write("{}\t{}\n".format(label, value))
            fp.write("\t".join(_REF_HEADER) + "\n")
            for chrom, n in c.per_reference.items():
                fp.write("{}\t{}\n".format(chrom, n))
            fp.write("\t".join(_STAT_HEADER) + "\n")
            for o, label in enumerate(ORIENTATIONS):
                st = c.stats(o)
                if st is not None:
                    fp.write("\t".join([label] + [_fmt(st[k]) for k in STATS]) + "\n")
            fp.write("\t".join(_SIZE_HEADER) + "\n")
            for s in np.flatnonzero(c.hist.any(axis=0)).tolist():
                fp.write("{}\t{}\t{}\t{}\n".format(s + 1, *(int(x) for x in c.hist[:, s].tolist())))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def read_fragments(path) -> Tuple[str, FragmentSizes, Dict[str, Dict[str, object]]]:
    """(name, FragmentSizes, ``{orientation label: the statistics row as written}``) of a ``_fragments.tab``."""
    with open(path) as fp:
        lines = [ln.rstrip("\n").split("\t") for ln in fp if ln.strip()]
    at_ref, at_stat, at_size = (lines.index(list(h)) for h in (_REF_HEADER, _STAT_HEADER, _SIZE_HEADER))
    head = {row[0]: row[1] if len(row) > 1 else "" for row in lines[:at_ref]}
    per = {row[0]: int(row[1]) for row in lines[at_ref + 1:at_stat]}
    max_size = int(head["Max size"])
    hist = np.zeros((3, max_size), dtype=np.uint64)
    for row in lines[at_size + 1:]:
        hist[:, int(row[0]) - 1] = [int(x) for x in row[1:4]]
    ints = ("n", "q25", "q75", "mode", "min", "max")
    stats = {row[0]: {k: (int(v) if k in ints else float(v)) for k, v in zip(STATS, row[1:])} for row in lines[at_stat + 1:at_size]}
    return head["Name"], FragmentSizes(max_size, per, hist, [int(head[label]) for label in _LABELS]), stats
