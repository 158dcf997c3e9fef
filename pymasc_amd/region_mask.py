"""Excluded regions (ENCODE's blacklist): ``--exclude-regions BED`` / ``exclude_regions=``.

The rules, which the device code (csrc/ingest/region_mask_device.inc, pmx_bits_clear_regions_dev_ex), the host checker here and
the tests all state the same way:

* The mask is BED read by the text-track readers (``inputs.open_track``: plain, gzip, bgzip; BED3 and wider; every line counts),
  or an ordered ``{name: [(start, end), ...]}``.  Intervals are 0-based, half-open: ``(b, e)`` covers 1-based positions
  ``b + 1 .. e``.  Lines may be unsorted, overlap and abut; per chromosome they are clipped to the chromosome's length, sorted and
  merged (abutting lines join) -- on the device by ``pmx_dbam_set_exclude`` when a device reader takes the mask, by ``merge`` here
  for the host readers.
* A name that is not among the alignment's references is skipped, with one warning that counts them; no name matching at all is
  a ValueError.
* A read that passed the reader's filter is left out when its extent ``[pos1, pos1 + read_len - 1]`` overlaps a merged interval:
  ``b + 1 <= pos1 + read_len - 1 and pos1 <= e``.  It is removed before the feeders.
* A track's ``M`` is cleared on 1-based positions ``max(1, b + 2 - L) .. e`` of every merged interval, ``L`` the run's read length:
  the positions where a read of length L would touch the interval.  The read filter, the clear on the device and the cut of the
  cache pass (``MaskedTrack``) all take the same clipped, merged intervals: ``ResolvedMask.merged``.  Only ``pymasc-precalc``, which
  has no alignment header, cuts with the lines merged as they are.
"""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import Dict, Optional, Sequence, Tuple

import numpy as np

logger = logging.getLogger(__name__)

_EMPTY = np.zeros(0, dtype=np.uint32)


def merge(begin, end, length: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """The lines ``(begin[i], end[i])`` of one chromosome, clipped to ``length`` (None: not clipped), empty ones dropped, sorted
    by begin and merged: a line that overlaps or abuts the running maximum of the ends before it joins that group.  uint32
    arrays, begins and ends ascending."""
    b = np.asarray(begin, dtype=np.int64).reshape(-1)
    e = np.asarray(end, dtype=np.int64).reshape(-1)
    if length is not None:
        e = np.minimum(e, int(length))
    ok = b < e
    b, e = b[ok], e[ok]
    if b.size == 0:
        return _EMPTY, _EMPTY
    order = np.argsort(b, kind="stable")
    b, e = b[order], e[order]
    top = np.maximum.accumulate(e)
    head = np.ones(b.size, dtype=bool)
    head[1:] = b[1:] > top[:-1]
    starts = np.flatnonzero(head)
    last = np.concatenate((starts[1:] - 1, [b.size - 1]))
    return b[starts].astype(np.uint32), top[last].astype(np.uint32)


def overlaps(pos, read_len, mb, me) -> np.ndarray:
    """True for every read of one chromosome whose extent ``[pos, pos + read_len - 1]`` overlaps a merged interval of ``mb`` /
    ``me`` (``merge``): the last interval with ``b + 1 <= pos + read_len - 1`` is the only candidate, and it overlaps when
    ``pos <= e``."""
    pos = np.asarray(pos, dtype=np.int64)
    if mb.size == 0 or pos.size == 0:
        return np.zeros(pos.size, dtype=bool)
    last = pos + np.maximum(np.asarray(read_len, dtype=np.int64), 1) - 1
    k = np.searchsorted(mb.astype(np.int64), last - 1, side="right") - 1
    return (k >= 0) & (me.astype(np.int64)[np.maximum(k, 0)] >= pos)


def mask_stem(path) -> str:
    """``/dir/blacklist.bed.gz`` -> ``blacklist``: the mask's part of the default cache name."""
    name = Path(os.fspath(path)).name
    for z in (".gz", ".bgz"):
        if name.lower().endswith(z):
            name = name[:-len(z)]
    return Path(name).stem if Path(name).suffix else name


def stats_path(track_path, mask_source, k=None) -> Optional[Path]:
    """The default cache of a masked track: ``<track stem>_<mask file stem>_mappability.json`` beside the track -- never the
    unmasked track's ``<track stem>_mappability.json``.  A dict mask has no file stem: None (no default cache)."""
    from .mappability import default_stats_path
    if isinstance(mask_source, ExcludeMask):
        mask_source = mask_source.source
    if mask_source is None or isinstance(mask_source, dict):
        return None
    plain = default_stats_path(track_path, k)
    tail = "_mappability.json"
    return plain.parent / (plain.name[:-len(tail)] + "_" + mask_stem(mask_source) + tail)


class ExcludeMask:
    """The lines of a mask by chromosome name, as they were read (``open_mask``); ``resolve`` binds them to an alignment's
    references.  ``source``: the path it was read from, None for a dict."""

    def __init__(self, lines: Dict[str, Tuple[np.ndarray, np.ndarray]], source=None, what: str = "excluded regions"):
        self.lines = lines
        self.source = source
        self.what = what            # what the messages call the file (a peak file is read and resolved here too)
        self._merged: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}
        self._warned = False        # the skipped names were reported (once per mask, however many files resolve it)

    def merged(self, name: str, length: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """The merged intervals of ``name`` (``merge``; empty arrays for a name the mask does not hold)."""
        key = (name, length)
        if key not in self._merged:
            b, e = self.lines.get(name, (_EMPTY, _EMPTY))
            self._merged[key] = merge(b, e, length)
        return self._merged[key]

    def track_intervals(self, name: str) -> Tuple[np.ndarray, np.ndarray]:
        """The merged lines of ``name`` as they are, for a cut without an alignment header (``pymasc-precalc``)."""
        return self.merged(name)

    def resolve(self, references: Sequence[str], lengths: Sequence[int]) -> "ResolvedMask":
        """The mask of an alignment file: names that are not among ``references`` are skipped (one warning with their count);
        ValueError when no name matches at all."""
        refs = list(references)
        known = set(refs)
        skipped = [n for n in self.lines if n not in known]
        if len(skipped) == len(self.lines):
            raise ValueError("no chromosome of the {}{} is among the alignment's references (e.g. {} vs {}): "
                             "check the naming ('chr1' vs '1')".format(
                                 self.what, "" if self.source is None else " '{}'".format(self.source),
                                 ", ".join(repr(n) for n in skipped[:3]) or "none", ", ".join(repr(n) for n in refs[:3]) or "none"))
        if skipped and not self._warned:
            self._warned = True
            logger.warning("{}: {} chromosome name(s) are not among the alignment's references and are skipped."
                           "".format(self.what[:1].upper() + self.what[1:], len(skipped)))
        return ResolvedMask(self, refs, [int(x) for x in lengths])


class ResolvedMask:
    """An ``ExcludeMask`` bound to the references of one alignment file: what the readers and the calculator take."""

    def __init__(self, mask: ExcludeMask, references, lengths):
        self.mask = mask
        self.references = tuple(references)
        self.lengths = tuple(lengths)

    def lines(self, ref_id: int, clip: bool = False) -> Tuple[np.ndarray, np.ndarray]:
        """The lines of reference ``ref_id`` as they were read, one row per line in file order, unmerged (none for a reference
        the file does not name); ``clip``: the ends clipped to the reference's length (a line may be empty then)."""
        b, e = self.mask.lines.get(self.references[ref_id], (_EMPTY, _EMPTY))
        return (b, np.minimum(e, min(max(self.lengths[ref_id], 0), 2**32 - 1)).astype(np.uint32)) if clip else (b, e)

    def csr(self, use=None):
        """(offsets int64[nref + 1], begin uint32, end uint32): every reference's lines as read, in reference order -- the
        arguments of ``pmx_dbam_set_exclude``, which clips, sorts and merges them on the device, and of
        ``pmx_dbam_peakcount_begin``, which keeps them apart.  ``use`` (one flag per reference; None: all): a reference that is
        not in it has no lines."""
        parts = [self.lines(r) if use is None or use[r] else (_EMPTY, _EMPTY) for r in range(len(self.references))]
        offsets = np.zeros(len(parts) + 1, dtype=np.int64)
        if parts:
            offsets[1:] = np.cumsum([p[0].size for p in parts])
        begin = np.concatenate([p[0] for p in parts] or [_EMPTY]).astype(np.uint32)
        end = np.concatenate([p[1] for p in parts] or [_EMPTY]).astype(np.uint32)
        return offsets, np.ascontiguousarray(begin), np.ascontiguousarray(end)

    def merged(self, ref_id: int) -> Tuple[np.ndarray, np.ndarray]:
        """The merged intervals of reference ``ref_id``, clipped to its length: what the read filter uses."""
        return self.mask.merged(self.references[ref_id], self.lengths[ref_id])

    def merged_table(self):
        """(ref_id int32, begin uint32, end uint32) of every merged interval in (reference, begin) order: what
        ``pmx_dbam_exclude_intervals`` returns for the same mask."""
        rows = [(np.full(self.merged(r)[0].size, r, dtype=np.int32),) + self.merged(r) for r in range(len(self.references))]
        if not rows:
            return np.zeros(0, np.int32), _EMPTY, _EMPTY
        return tuple(np.concatenate([row[k] for row in rows]) for k in range(3))

    def keep(self, ref, pos, read_len) -> np.ndarray:
        """The host checker of the device filter: True for every read of a batch (``ref`` ids, 1-based ``pos``, ``read_len``)
        that overlaps no merged interval of its reference."""
        ref = np.asarray(ref)
        out = np.ones(ref.size, dtype=bool)
        for r in np.unique(ref).tolist():
            if r < 0 or r >= len(self.references):
                continue
            mb, me = self.merged(int(r))
            if mb.size:
                sel = np.flatnonzero(ref == r)
                out[sel] = ~overlaps(np.asarray(pos)[sel], np.asarray(read_len)[sel], mb, me)
        return out

    def track_intervals(self, name: str) -> Tuple[np.ndarray, np.ndarray]:
        """The merged intervals a track's vector of chromosome ``name`` is cleared with: those of the read filter, clipped to the
        reference's length; none for a name that is not a reference."""
        if name not in self.references:
            return _EMPTY, _EMPTY
        return self.merged(self.references.index(name))


def open_mask(source, device_ingest: bool = False, device: int = 0, what: str = "excluded regions") -> ExcludeMask:
    """The mask of ``source``: an ``ExcludeMask`` as it is, an ordered ``{name: [(start, end), ...]}``, or the path of a BED
    file, read through ``inputs.open_track`` (on ``device`` with ``device_ingest``).  ValueError for a malformed dict interval.
    ``what``: what the messages call it (``pymasc_amd.peaks`` reads a peak file here: the first three columns of every line)."""
    if isinstance(source, ExcludeMask):
        return source
    if isinstance(source, dict):
        lines = {}
        for name, ivs in source.items():
            arr = np.asarray(list(ivs), dtype=np.int64).reshape(-1, 2)
            if arr.size and (arr.min() < 0 or arr.max() >= 2**32):
                raise ValueError("{} of '{}': positions must lie in [0, 2^32)".format(what, name))
            lines[str(name)] = (arr[:, 0].astype(np.uint32), arr[:, 1].astype(np.uint32))
        return ExcludeMask(lines, what=what)
    from .inputs import open_track
    path = os.fspath(source)
    if not os.path.isfile(path):
        raise FileNotFoundError("{}: no such file: '{}'".format(what, path))
    lines = {}
    with open_track(path, device_ingest, device) as t:
        for name in t.chromsizes:
            b, e, _v = t.fetch_arrays(0.0, name)
            lines[name] = (np.asarray(b, dtype=np.uint32).copy(), np.asarray(e, dtype=np.uint32).copy())
    return ExcludeMask(lines, source=path, what=what)


def resolve_lines(mask: ExcludeMask, references: Sequence[str], lengths: Sequence[int], use=None):
    """``mask.resolve`` with the lines kept apart (a peak file): (the ``ResolvedMask``, its ``csr(use)``) -- one
    row per line, in file order within a reference and the references in header order, unmerged and unclipped.  The names, the
    warning and the ValueError are ``resolve``'s; the clipping is ``ResolvedMask.lines(r, clip=True)`` or the device's."""
    resolved = mask.resolve(references, lengths)
    return resolved, resolved.csr(use)


def cut_intervals(begin, end, mb, me, read_len: int) -> Tuple[np.ndarray, np.ndarray]:
    """The track intervals ``[begin, end)`` (0-based, any order) less the 1-based positions ``max(1, b + 2 - L) .. e`` of every
    merged interval ``(b, e)``: 0-based ``[max(0, b + 1 - L), e)``.  The pieces come in the order of the intervals."""
    begin = np.asarray(begin, dtype=np.int64)
    end = np.asarray(end, dtype=np.int64)
    if mb.size == 0 or begin.size == 0:
        return begin, end
    cb, ce = merge(np.maximum(mb.astype(np.int64) + 1 - int(read_len), 0), me)     # (padded neighbours may meet)
    cb, ce = cb.astype(np.int64), ce.astype(np.int64)
    gb = np.concatenate(([0], ce))                     # the gaps between the cuts: [gb[k], ge[k])
    ge = np.concatenate((cb, [np.iinfo(np.int64).max]))
    lo = np.searchsorted(ge, begin, side="right")      # the first gap that ends behind the interval's begin
    hi = np.searchsorted(gb, end, side="left")         # the first gap that begins at or behind its end
    cnt = np.maximum(hi - lo, 0)
    which = np.repeat(np.arange(begin.size), cnt)
    gap = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
    pb = np.maximum(begin[which], gb[gap])
    pe = np.minimum(end[which], ge[gap])
    ok = pb < pe
    return pb[ok], pe[ok]


class MaskedTrack:
    """A track reader seen through a mask, for the mappable-length pass (``mappability.MappabilityStats``): ``fetch_arrays`` /
    ``fetch`` give the track's intervals with ``cut_intervals`` applied; everything else is the reader's."""

    def __init__(self, track, mask, read_len: int):
        """``mask``: a ``ResolvedMask`` (a run: the clipped intervals of its references) or an ``ExcludeMask`` (no header)."""
        self._track, self._mask, self._read_len = track, mask, int(read_len)

    def __getattr__(self, name):
        return getattr(self._track, name)

    def fetch_arrays(self, valfilter: float, chrom: str):
        bulk = getattr(self._track, "fetch_arrays", None)
        if bulk is not None:
            b, e, _v = bulk(valfilter, chrom)
        else:
            iv = np.asarray([(x, y) for x, y, _v in self._track.fetch(valfilter, chrom)], dtype=np.int64).reshape(-1, 2)
            b, e = iv[:, 0], iv[:, 1]
        pb, pe = cut_intervals(b, e, *self._mask.track_intervals(chrom), self._read_len)
        return pb, pe, np.ones(pb.size, dtype=np.float32)

    def fetch(self, valfilter: float, chrom: str):
        b, e, v = self.fetch_arrays(valfilter, chrom)
        return iter(zip(b.tolist(), e.tolist(), v.tolist()))
