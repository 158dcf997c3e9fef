"""The strand-aware read profile around anchor sites and the TSS enrichment: ``--tss BED`` / ``tss=``, beside
NSC / RSC, NRF / PBC, the fingerprint and FRiP.

The definitions, which the device code (csrc/ingest/tss_device.inc), the host checker here and the tests state the same way.
They are this project's own: nothing here was compared with ENCODE's ATAC pipeline or with deepTools.

* An anchor is ``(reference, a, s)``: a 1-based position ``a`` and a strand ``s`` (``+`` or ``-``).  Anchors come as a BED6 file,
  plain, gzip or bgzip, read by the BED read readers (``bed_reads.DeviceBedReadsReader`` with device ingest, else
  ``bed_reads.BedReadsReader``; ``batches(0, 0)``, so every line is kept) against the alignment's own references and lengths, and
  those readers' rules apply unchanged: at least 6 fields, a chromosome the alignment lacks and a strand of ``.`` are their
  errors.  A ``+`` line ``chrom start end ... +`` is the anchor ``a = start + 1``, a ``-`` line the anchor ``a = end``: the 5' base
  of the feature, the TSS convention.  Anchors also come as an ordered ``{name: [(a, "+" | "-"), ...]}``; a name the alignment
  lacks is a ValueError.  Anchors may repeat, and each counts separately.  Anchors on references that are not chosen are dropped,
  and ``anchors`` counts the rest.  ``a < 1``, ``a`` beyond its reference's length and more than 2^20 anchors are a ValueError.
* The reads are the ones the correlation sees (the set ``--peaks`` uses): the run's filter, the chosen references, less the reads
  an exclude mask drops.  ``N`` is their number.  The extent ``[lo, hi]`` is the fingerprint's (7.16) with ``tss_extend``: ``0``
  is the read's own length, ``1`` its 5' base only (the ATAC cut-site convention); clipped to ``[1, len]``.
* The flank ``F`` is an integer, ``1 <= F <= 4095``, 2000 by default; the table has two rows of width ``W = 2F + 1``.  A read with
  the extent ``[lo, hi]`` on an anchor's reference covers, for that anchor, the offsets ``o = s * (p - a)`` for ``p`` in
  ``[lo, hi]`` with ``|o| <= F``.  For every such ``o``, ``same[o + F] += 1`` when the read's strand equals the anchor's,
  ``opposite[o + F] += 1`` otherwise.  ``pairs`` counts the (read, anchor) pairs with at least one such offset, ``n_near`` the
  reads in at least one pair, once each.  Every count is an integer.
* Statistics (host, float64, in this order): ``total = same + opposite``; ``E = max(1, min(100, F // 4))``;
  ``edge_sum = sum(total[:E]) + sum(total[W - E:])``; ``background = edge_sum / (2 * E)``; ``normalized[o] = total[o] /
  background``; ``TSS enrichment = max(normalized)``; ``Peak offset`` the first offset where that maximum is reached;
  ``At TSS = normalized[F]``.  With ``edge_sum == 0`` all three are nan.

A device reader counts on the GPU (``pmx_dbam_tss_*``, include/pymasc_amd_ingest.h); a host reader goes through its ``batches``
and ``count_host`` (plain numpy), which is also the device's checker.
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Dict, Tuple

import numpy as np

from .complexity import _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, SideAccumulator, count_over

TSS_SUFFIX = "_tss.tab"
MAX_FLANK = 4095
MAX_ANCHORS = 1 << 20
DEFAULT_FLANK = 2000
_ROW_HEADER = ("offset", "same", "opposite", "total", "normalized")
_FLOATS = ("Background", "TSS enrichment", "At TSS")
_NAN = float("nan")
_CHUNK = 1 << 16                    # reads whose pairs count_host expands at a time


def check_flank(flank) -> int:
    if isinstance(flank, bool) or int(flank) != flank or not 1 <= int(flank) <= MAX_FLANK:
        raise ValueError("the flank is {}: it must lie in [1, {}]".format(flank, MAX_FLANK))
    return int(flank)


def check_extend(extend) -> int:
    if isinstance(extend, bool) or int(extend) != extend or int(extend) < 0:
        raise ValueError("extend is not negative")
    return int(extend)


class Anchors:
    """Anchors bound to an alignment's ``references`` / ``lengths``: ``ref`` (int32, the reference's index), ``pos1`` (uint32,
    ``a``) and ``reverse`` (uint8, 1 for a ``-`` anchor), in the order they were read; ``source``: the file's path, or ""."""

    def __init__(self, references, lengths, ref, pos1, reverse, source: str = ""):
        self.references, self.lengths = tuple(references), tuple(int(x) for x in lengths)
        a = np.asarray(pos1, dtype=np.int64).ravel()
        self.ref = np.ascontiguousarray(ref, dtype=np.int32).ravel()
        self.reverse = np.ascontiguousarray(np.asarray(reverse).ravel() != 0, dtype=np.uint8)
        self.source = str(source)
        if not (self.ref.size == a.size == self.reverse.size):
            raise ValueError("ref, pos1 and reverse have one entry per anchor")
        if a.size > MAX_ANCHORS:
            raise ValueError("{} anchors: more than 2^20".format(a.size))
        if a.size:
            top = np.asarray(self.lengths, dtype=np.int64)[self.ref]
            bad = np.flatnonzero((a < 1) | (a > top))
            if bad.size:
                k = int(bad[0])
                raise ValueError("anchor {}: position {} is outside {} (1 .. {})".format(k, int(a[k]), self.references[self.ref[k]],
                                                                                         int(top[k])))
        self.pos1 = np.ascontiguousarray(a, dtype=np.uint32)

    def __len__(self) -> int:
        return int(self.ref.size)

    def chosen(self, use) -> int:
        """The anchors on the references ``use`` flags."""
        return int(np.asarray(use, dtype=bool)[self.ref].sum()) if len(self) else 0


class AnchorSource:
    """What ``tss=`` names -- a BED6 file's path or an ordered ``{name: [(a, "+" | "-"), ...]}`` -- for a whole call: ``resolve``
    binds it to an alignment's references and lengths, once for every distinct header."""

    def __init__(self, source, device_ingest: bool = False, device: int = 0):
        self.mapping = dict(source) if isinstance(source, dict) else None
        self.source = "" if self.mapping is not None else os.fspath(source)
        self.device_ingest, self.device = bool(device_ingest), int(device)
        self._bound: Dict[tuple, Anchors] = {}

    def resolve(self, references, lengths) -> Anchors:
        key = (tuple(references), tuple(int(x) for x in lengths))
        if key not in self._bound:
            self._bound[key] = self._read(*key)
        return self._bound[key]

    def _read(self, references, lengths) -> Anchors:
        if self.mapping is not None:
            ids = {n: i for i, n in enumerate(references)}
            ref, pos, rev = [], [], []
            for name, rows in self.mapping.items():
                if name not in ids:
                    raise ValueError("the anchors name {}, which is not among the alignment's references".format(name))
                for a, strand in rows:
                    if strand not in ("+", "-"):
                        raise ValueError("an anchor's strand is '+' or '-', not {!r}".format(strand))
                    ref.append(ids[name])
                    pos.append(int(a))
                    rev.append(strand == "-")
            return Anchors(references, lengths, ref, pos, rev)
        from .bed_reads import BedReadsReader, DeviceBedReadsReader
        if self.device_ingest:
            reader = DeviceBedReadsReader(self.source, references, lengths, self.device)
        else:
            reader = BedReadsReader(self.source, references, lengths)
        cols = [[], [], []]
        with reader:
            for ref, pos1, span, rev in reader.batches(0, 0):
                rev = np.asarray(rev).astype(bool)
                cols[0].append(np.asarray(ref, dtype=np.int32))
                cols[1].append(np.where(rev, pos1.astype(np.int64) + span.astype(np.int64) - 1, pos1.astype(np.int64)))
                cols[2].append(rev)
        ref, pos, rev = (np.concatenate(c) if c else np.zeros(0, dtype=np.int64) for c in cols)
        return Anchors(references, lengths, ref, pos, rev, self.source)


def open_anchors(source, references, lengths, device_ingest: bool = False, device: int = 0) -> Anchors:
    """The anchors of ``source`` (a BED6 file's path, an ordered ``{name: [(a, "+" | "-"), ...]}``, an ``AnchorSource`` or what
    this returned) bound to ``references`` / ``lengths``, the alignment's own."""
    if isinstance(source, Anchors):
        if (source.references, source.lengths) != (tuple(references), tuple(int(x) for x in lengths)):
            raise ValueError("the anchors were opened against other references")
        return source
    if not isinstance(source, AnchorSource):
        source = AnchorSource(source, device_ingest, device)
    return source.resolve(references, lengths)


class TssProfile:
    """``same`` / ``opposite``: int64 [2 * flank + 1], the reads' bases at every offset ``-flank .. flank`` from an anchor, by the
    read's strand relative to the anchor's; ``N``, ``n_near``, ``anchors``, ``pairs``, ``flank``, ``extend``; the statistics are
    computed from them on demand."""

    def __init__(self, same, opposite, N: int, n_near: int, anchors: int, pairs: int, flank: int, extend: int):
        self.same = np.asarray(same, dtype=np.int64).ravel().copy()
        self.opposite = np.asarray(opposite, dtype=np.int64).ravel().copy()
        self.N, self.n_near, self.anchors, self.pairs = int(N), int(n_near), int(anchors), int(pairs)
        self.flank, self.extend = int(flank), int(extend)
        if self.same.size != 2 * self.flank + 1 or self.opposite.size != self.same.size:
            raise ValueError("same and opposite have 2 * flank + 1 entries")

    total = property(lambda self: self.same + self.opposite)

    @property
    def background(self) -> float:
        """The mean of ``total`` over the ``E`` outermost offsets of either side."""
        total = self.total
        edge = max(1, min(100, self.flank // 4))
        edge_sum = int(total[:edge].sum()) + int(total[total.size - edge:].sum())
        return edge_sum / (2 * edge)

    @property
    def normalized(self) -> np.ndarray:
        background = self.background
        if background == 0:         # (edge_sum == 0)
            return np.full(self.same.size, _NAN)
        return np.array([int(x) / background for x in self.total.tolist()], dtype=np.float64)

    @property
    def enrichment(self) -> float:
        norm = self.normalized
        return _NAN if norm[0] != norm[0] else float(norm.max())

    @property
    def at_tss(self) -> float:
        return float(self.normalized[self.flank])

    @property
    def peak_offset(self):
        """The first offset where ``normalized`` reaches its maximum (an int), nan without a background."""
        norm = self.normalized
        return _NAN if norm[0] != norm[0] else int(np.argmax(norm)) - self.flank

    def _ints(self):
        return (self.N, self.n_near, self.anchors, self.pairs, self.flank, self.extend)

    def __eq__(self, other) -> bool:
        return (isinstance(other, TssProfile) and self._ints() == other._ints() and np.array_equal(self.same, other.same)
                and np.array_equal(self.opposite, other.opposite))

    __hash__ = None

    def __repr__(self) -> str:
        return "TssProfile(flank={}, extend={}, anchors={}, N={}, n_near={}, pairs={}, bases={})".format(
            self.flank, self.extend, self.anchors, self.N, self.n_near, self.pairs, int(self.total.sum()))


def count_host(ref_id, pos1, read_len, reverse, anchors: Anchors, use, flank: int, extend: int = 0):
    """The host checker, plain numpy: (table int64 [2, W] = same, opposite; N; n_near; pairs) of the reads given as four columns.
    Per reference the anchors are sorted by position, two searches give every read its anchors ``lo - F <= a <= hi + F``, the
    (read, anchor) pairs are written out (``_CHUNK`` reads at a time), and each pair adds +1 at its first offset and -1 behind its
    last to a table of differences, whose prefix sums are the rows."""
    F, W = int(flank), 2 * int(flank) + 1
    diff = np.zeros(2 * (W + 1), dtype=np.int64)
    ref = np.asarray(ref_id, dtype=np.int64).ravel()
    pos = np.asarray(pos1, dtype=np.int64).ravel()
    rl = np.asarray(read_len, dtype=np.int64).ravel()
    rev = np.asarray(reverse).ravel().astype(bool)
    span = np.full(ref.size, int(extend), dtype=np.int64) if extend else rl
    lo_all = np.maximum(np.where(rev, pos + rl - span, pos), 1)
    hi_all = np.where(rev, pos + rl - 1, pos + span - 1)
    n = n_near = pairs = 0
    for r in range(len(anchors.references)):
        if not use[r]:
            continue
        sel = ref == r
        n += int(sel.sum())
        mine = np.flatnonzero(anchors.ref == r)
        if not mine.size:
            continue
        order = np.argsort(anchors.pos1[mine], kind="stable")
        a_all = anchors.pos1[mine][order].astype(np.int64)
        minus_all = anchors.reverse[mine][order].astype(bool)
        lo, hi, rv = lo_all[sel], np.minimum(hi_all[sel], anchors.lengths[r]), rev[sel]
        ok = lo <= hi
        lo, hi, rv = lo[ok], hi[ok], rv[ok]
        j0 = np.searchsorted(a_all, lo - F, side="left")
        count = np.searchsorted(a_all, hi + F, side="right") - j0
        n_near += int((count > 0).sum())
        pairs += int(count.sum())
        for c0 in range(0, lo.size, _CHUNK):
            cnt = count[c0:c0 + _CHUNK]
            if not cnt.any():
                continue
            read = np.repeat(np.arange(c0, c0 + cnt.size), cnt)
            j = j0[read] + np.arange(read.size) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            a, minus = a_all[j], minus_all[j]
            o_lo = np.maximum(np.where(minus, a - hi[read], lo[read] - a), -F)
            o_hi = np.minimum(np.where(minus, a - lo[read], hi[read] - a), F)
            base = np.where(rv[read] != minus, W + 1, 0)
            diff += np.bincount(base + o_lo + F, minlength=diff.size) - np.bincount(base + o_hi + F + 1, minlength=diff.size)
    table = np.cumsum(diff.reshape(2, W + 1), axis=1)
    return table[:, :W], n, n_near, pairs


def _profile(reader, anchors, references, flank, extend, device_ingest: bool):
    """(the anchors bound to the reader's references, the chosen references' flags, flank, extend), checked."""
    flank, extend = check_flank(flank), check_extend(extend)
    bound = open_anchors(anchors, reader.references, reader.lengths, device_ingest, getattr(reader, "device", 0))
    return bound, np.asarray(_selected_mask(reader, references), dtype=np.uint8), flank, extend


class DeviceCount(SideAccumulator):
    """The table a device reader's handle holds between ``pmx_dbam_tss_begin`` and the next one: ``add`` counts what the handle
    holds now (a stream reader calls it for every window), ``result`` reads the profile back."""

    def __init__(self, reader, anchors, mapq_criteria: int, references=None, flank: int = DEFAULT_FLANK, extend: int = 0):
        reader._check_open()
        self.mapq_criteria = int(mapq_criteria)
        self.bound, self.use, self.flank, self.extend = _profile(reader, anchors, references, flank, extend, True)
        self.begin(reader)

    def begin(self, reader) -> None:
        """A zeroed table on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        b = self.bound
        mask = np.ascontiguousarray(self.use, dtype=np.uint8) if b.references else np.zeros(1, dtype=np.uint8)
        n = len(b)
        rc = reader._L.pmx_dbam_tss_begin(reader._h, n, b.ref.ctypes.data if n else None, b.pos1.ctypes.data if n else None,
                                          b.reverse.ctypes.data if n else None, self.flank, self.extend, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> Tuple[int, int]:
        out = np.zeros(2, dtype=np.uint64)
        rc = reader._L.pmx_dbam_tss_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, out.ctypes.data)
        if rc:
            reader._raise(rc)
        return int(out[0]), int(out[1])

    def copy(self, reader) -> np.ndarray:
        """uint64 [2, W]: same, opposite (``pmx_dbam_tss_copy``)."""
        out = np.zeros(2 * (2 * self.flank + 1), dtype=np.uint64)
        rc = reader._L.pmx_dbam_tss_copy(reader._h, out.ctypes.data)
        if rc:
            reader._raise(rc)
        return out.reshape(2, -1)

    def totals(self, reader) -> np.ndarray:
        """uint64 [4] = N, n_near, anchors, pairs of ``pmx_dbam_tss_totals``."""
        totals = np.zeros(4, dtype=np.uint64)
        rc = reader._L.pmx_dbam_tss_totals(reader._h, totals.ctypes.data)
        if rc:
            reader._raise(rc)
        return totals

    def result(self, reader) -> TssProfile:
        table, t = self.copy(reader), [int(x) for x in self.totals(reader)]
        if t[2] != self.bound.chosen(self.use):
            raise RuntimeError("pmx_dbam_tss_totals: the library kept {} anchors, not {}".format(t[2], self.bound.chosen(self.use)))
        return TssProfile(table[0].astype(np.int64), table[1].astype(np.int64), t[0], t[1], t[2], t[3], self.flank, self.extend)


def count_device(reader, anchors, mapq_criteria: int, references=None, flank: int = DEFAULT_FLANK, extend: int = 0) -> TssProfile:
    """``begin`` + ``add`` + ``copy`` / ``totals`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, anchors, mapq_criteria, references, flank, extend)
    acc.add(reader)
    return acc.result(reader)


def from_reader(reader, anchors, mapq_criteria: int = 0, references=None, flank: int = DEFAULT_FLANK, extend: int = 0) -> TssProfile:
    """The reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the reader has selected)
    piled up around ``anchors`` (``open_anchors``).  A device reader counts on the GPU -- window by window for a stream reader,
    which is read once more when it is a regular file and raises ``InputUnseekable`` otherwise; a host reader through ``batches``
    and ``count_host``."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        return count_over(reader, "tss", lambda: DeviceCount(reader, anchors, mapq_criteria, references, flank, extend)).result(reader)
    bound, use, flank, extend = _profile(reader, anchors, references, flank, extend, False)
    table = np.zeros((2, 2 * flank + 1), dtype=np.int64)
    n = n_near = pairs = 0
    for batch in reader.batches(mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE):
        if len(batch[0]):
            t, a, b, c = count_host(*batch, bound, use, flank, extend)
            table += t
            n, n_near, pairs = n + a, n_near + b, pairs + c
    return TssProfile(table[0], table[1], n, n_near, bound.chosen(use), pairs, flank, extend)


def tss_rows(name: str, c: TssProfile, anchor_file: str = ""):
    """The first block of ``_tss.tab``: (label, value) pairs; the floats with ``repr`` (they read back exactly)."""
    return [("Name", name), ("Anchor file", anchor_file), ("Flank", c.flank), ("Extend", c.extend), ("Anchors", c.anchors),
            ("Reads", c.N), ("Reads near anchors", c.n_near), ("Read-anchor pairs", c.pairs), ("Background", repr(float(c.background))),
            ("TSS enrichment", repr(float(c.enrichment))), ("At TSS", repr(float(c.at_tss))), ("Peak offset", c.peak_offset)]


def write_tss(path_base, name: str, c: TssProfile, anchor_file: str = "") -> Path:
    """Writes ``<path_base>_tss.tab`` (to a temporary file beside it, renamed into place) and returns its path: the label / value
    block, then ``offset same opposite total normalized`` for the offsets ``-flank .. flank``."""
    path = Path(str(path_base) + TSS_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w") as fp:
            for label, value in tss_rows(name, c, anchor_file):
                fp.write("{}\t{}\n".format(label, value))
            fp.write("\t".join(_ROW_HEADER) + "\n")
            rows = zip(range(-c.flank, c.flank + 1), c.same.tolist(), c.opposite.tolist(), c.total.tolist(), c.normalized.tolist())
            for o, s, p, t, x in rows:
                fp.write("{}\t{}\t{}\t{}\t{}\n".format(o, s, p, t, repr(float(x))))
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def read_tss(path) -> Tuple[str, TssProfile, Dict[str, object]]:
    """(name, TssProfile, the label / value block as written: ``Background``, ``TSS enrichment`` and ``At TSS`` as float,
    ``Peak offset`` as int or nan) of a ``_tss.tab``."""
    with open(path) as fp:
        rows = [ln.rstrip("\n").split("\t") for ln in fp if ln.strip()]
    at = rows.index(list(_ROW_HEADER))
    head = {row[0]: row[1] if len(row) > 1 else "" for row in rows[:at]}
    same = [int(row[1]) for row in rows[at + 1:]]
    opposite = [int(row[2]) for row in rows[at + 1:]]
    c = TssProfile(same, opposite, int(head["Reads"]), int(head["Reads near anchors"]), int(head["Anchors"]),
                   int(head["Read-anchor pairs"]), int(head["Flank"]), int(head["Extend"]))
    block = {k: (float(v) if k in _FLOATS else v) for k, v in head.items()}
    block["Peak offset"] = _NAN if head["Peak offset"] == "nan" else int(head["Peak offset"])
    return head["Name"], c, block
