"""BED read files: tagAlign (ENCODE) and ``bedtools bamtobed`` output, BED6 with one line per read.

* ``is_bed_reads(path)``: the name decides -- ``.tagAlign`` or ``.bed`` in any letter case, optionally followed by ``.gz`` /
  ``.bgz``; the compression (plain, gzip, BGZF) is told from the bytes by the readers;
* ``chrom_sizes_of(chrom_sizes)``: the references of such a file, which has no header, from a ``.chrom.sizes`` / ``.fai`` file,
  a BAM / SAM file's header (``plot.load_chrom_sizes``) or an ordered ``{name: length}``;
* ``BedReadsReader`` (host, libpymasc_io.so ``pmx_bed_open``) has ``SamReader``'s surface; it is the checker of the device
  reader, the path without a GPU and the path of a rank of several;
* ``DeviceBedReadsReader`` (libpymasc_ingest.so ``pmx_dbed_open``) is a ``DeviceBamReader`` whose table is parsed and sorted on
  the GPU.

Both deliver the reads sorted stably by (reference in the order of the sizes, start), ties in file order, so an unsorted file
gives what the same lines stably sorted give.  A line ``chrom start end name score strand`` is the read at ``start + 1`` of
length ``end - start`` on the strand given, with MAPQ ``min(score, 255)`` (``.``: 255); there is no duplicate or read-2 flag.
"""
from __future__ import annotations

import ctypes
import os
from typing import Tuple

from .bam_device import DeviceBamReader
from .native import PmxIOError, load_ingest_library, load_io_library
from .sam import SamReader

_SUFFIXES = (".tagalign", ".bed")
_COMPRESSED = (".gz", ".bgz")


def is_bed_reads(path) -> bool:
    """The file's name ends in ``.tagAlign`` or ``.bed`` (any letter case), optionally followed by ``.gz`` or ``.bgz``."""
    name = os.path.basename(os.fspath(path)).lower()
    for c in _COMPRESSED:
        if name.endswith(c):
            name = name[:-len(c)]
            break
    return name.endswith(_SUFFIXES)


def chrom_sizes_of(chrom_sizes) -> Tuple[Tuple[str, ...], Tuple[int, ...]]:
    """(references, lengths) in order from a path (``plot.load_chrom_sizes``: a ``.chrom.sizes`` / ``.fai`` text, or the header of
    a BAM / SAM file) or from an ordered mapping ``{name: length}``.  ValueError when they cannot be read or name nothing."""
    if isinstance(chrom_sizes, dict):
        sizes = dict(chrom_sizes)
    else:
        from .plot import PlotInputError, load_chrom_sizes
        try:
            sizes = load_chrom_sizes(chrom_sizes)
        except PlotInputError as e:
            raise ValueError("chromosome sizes: {}".format(e))
    if not sizes:
        raise ValueError("chromosome sizes: no chromosome named")
    return tuple(str(n) for n in sizes), tuple(int(v) for v in sizes.values())


def _c_sizes(references, lengths):
    names = (ctypes.c_char_p * len(references))(*[n.encode() for n in references])
    lens = (ctypes.c_int64 * len(lengths))(*[int(v) for v in lengths])
    return len(references), names, lens


class BedReadsReader(SamReader):
    """A BED read file (plain, gzip or BGZF) parsed and put in (reference, start) order on the host; ``SamReader``'s surface
    (the handle is a pmx_sam).  ``references`` / ``lengths``: the chromosome sizes, in their order."""

    def __init__(self, path, references, lengths, threads: int = 0):
        self._L = load_io_library()
        self.path = os.fspath(path)
        self._h = self._open_handle("pmx_bed_open", self.path.encode(), int(threads), *_c_sizes(references, lengths))
        self.references: Tuple[str, ...] = tuple(references)
        self.lengths: Tuple[int, ...] = tuple(int(v) for v in lengths)

    def fetch(self, reference: str, *args, **kwargs):
        raise ValueError("fetch() needs an index: {} is a BED read file".format(self.path))

    def mate_batches(self, *args, **kwargs):
        raise ValueError("{}: the input has no mate fields".format(self.path))


class DeviceBedReadsReader(DeviceBamReader):
    """A BED read file copied to HBM, parsed and put in (reference, start) order there; the surface of ``DeviceBamReader``.
    ``references`` / ``lengths``: the chromosome sizes; ``select`` chooses chromosomes among the records, as for a file without
    an index."""

    def __init__(self, path, references, lengths, device: int = 0, threads: int = 0, select=None):
        self._L = load_ingest_library()
        self.path = os.fspath(path)
        self.indexed = False
        self._attach(self._open_handle("pmx_dbed_open", self.path.encode(), int(device), int(threads),
                                       *_c_sizes(references, lengths)), select)


class SizesHeader:
    """What ``inputs.open_header`` gives for a BED read file: the references and lengths of its chromosome sizes, after a check
    that the file can be read (none of it is)."""

    def __init__(self, path, references, lengths):
        p = os.fspath(path)
        try:
            with open(p, "rb"):
                pass
        except OSError as e:
            raise PmxIOError(-1, "{}: {}".format(p, e.strerror or e))
        self.path = p
        self.references: Tuple[str, ...] = tuple(references)
        self.lengths: Tuple[int, ...] = tuple(lengths)

    def close(self) -> None:
        pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False
