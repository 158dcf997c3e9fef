"""The mappability track of a genome FASTA: exact k-mer uniqueness, computed at open.

Position p of a chromosome is uniquely mappable when the k-mer F that starts there exists (k valid bases A C G T of any case,
inside the record), is no palindrome (F != revcomp(F)), and no other existing position has F or revcomp(F) as its k-mer -- the
rule of the CRG and Umap single-read tracks, with exact matches (Umap's definition).  The track of a chromosome is its maximal
runs of unique positions with value 1.0, and then reads like any other track.

* ``is_fasta(path)``: the name decides -- ``.fa``, ``.fasta``, ``.fna`` or ``.fas`` in any letter case, optionally followed by
  ``.gz`` / ``.bgz``; the compression (plain, gzip, BGZF) is told from the bytes;
* ``KmerTrackReader(path, k)`` (host, libpymasc_io.so ``pmx_kmer_open``) sorts the positions by their canonical k-mer on host
  threads: the checker of the device generator and the path without a GPU;
* ``DeviceKmerTrackReader(path, k, device)`` (libpymasc_ingest.so ``pmx_dkm_open``) hashes, sorts and groups the k-mers on the
  GPU; its intervals stay in HBM (``fetch_device``), as a ``DeviceBigWigReader``'s do;
* ``fasta_sizes(path)``: the names and lengths of the records, from ``<path>.fai`` when it exists, else from a scan of the
  header lines on the host (no track is computed).

Both readers report the records' true lengths as ``chromsizes`` (not extents) and ``kind == "kmer"``.
"""
from __future__ import annotations

import gzip
import os
from typing import Dict

import numpy as np

from .bigwig_device import DeviceBigWigReader
from .native import (HostTrackReader, PmxIOError, existing_path, load_ingest_library,  # noqa: F401  (PmxIOError re-exported)
                     load_io_library)

_SUFFIXES = (".fa", ".fasta", ".fna", ".fas")
_COMPRESSED = (".gz", ".bgz")


def is_fasta(path) -> bool:
    """The file's name ends in ``.fa``, ``.fasta``, ``.fna`` or ``.fas`` (any letter case), optionally followed by ``.gz`` or
    ``.bgz``."""
    name = os.path.basename(os.fspath(path)).lower()
    for c in _COMPRESSED:
        if name.endswith(c):
            name = name[:-len(c)]
            break
    return name.endswith(_SUFFIXES)


def fasta_stem(path) -> str:
    """The file name without its FASTA suffix and compression suffix: ``hg38.fa.gz`` -> ``hg38``."""
    name = os.path.basename(os.fspath(path))
    low = name.lower()
    for c in _COMPRESSED:
        if low.endswith(c):
            name, low = name[:-len(c)], low[:-len(c)]
            break
    for s in _SUFFIXES:
        if low.endswith(s):
            return name[:-len(s)]
    return name


def fasta_sizes(path) -> Dict[str, int]:
    """{name: length} of the records in file order: from ``<path>.fai`` (samtools faidx) when it exists, else from the header
    lines of a host scan (plain or gzip / BGZF) that counts the sequence bytes of every record without checking them."""
    p = os.fspath(path)
    fai = p + ".fai"
    if os.path.exists(fai):
        out = {}
        with open(fai) as fh:
            for line in fh:
                f = line.rstrip("\r\n").split("\t")
                if len(f) >= 2 and f[0]:
                    out[f[0]] = int(f[1])
        return out
    with open(p, "rb") as fh:
        magic = fh.read(2)
    opener = gzip.open if magic == b"\x1f\x8b" else open
    out: Dict[str, int] = {}
    name = None
    with opener(p, "rb") as fh:
        for line in fh:
            line = line.rstrip(b"\n")
            if line.endswith(b"\r"):
                line = line[:-1]
            if line.startswith(b">"):
                name = line[1:].replace(b"\t", b" ").split(b" ")[0].decode("utf-8", "replace")
                out[name] = 0
            elif name is not None:
                out[name] += len(line)
    return out


def _check_k(k) -> int:
    if k is None:
        raise ValueError("a genome FASTA needs the k-mer length (the read length)")
    k = int(k)
    if not 16 <= k <= 1024:
        raise ValueError("k = {}: the k-mer length must lie in [16, 1024]".format(k))
    return k


class KmerTrackReader(HostTrackReader):
    chromsizes_are_extents = False

    def __init__(self, path, k: int, threads: int = 0):
        self.path = existing_path(path)
        self.k = _check_k(k)
        self._L = load_io_library()
        self._attach(self._open_handle("pmx_kmer_open", self.path.encode(), self.k, int(threads)))


class DeviceKmerTrackReader(DeviceBigWigReader):
    """The genome is packed, hashed, sorted and grouped on GPU ``device``; the handle is a pmx_dbw (kind 2), so
    ``fetch_device``, ``fetch_arrays`` and ``fetch`` are DeviceBigWigReader's.  ``budget_bytes``: device bytes the sort passes
    may use (0: half of the free memory less inputs.DEVICE_INGEST_MARGIN); ``hash_bits`` < 64 keeps only the low bits of the
    hash, a test knob that forces collisions (resolved exactly).  No host fallback: without a GPU the constructor raises."""
    chromsizes_are_extents = False

    def __init__(self, path, k: int, device: int = 0, budget_bytes: int = 0, hash_bits: int = 64, threads: int = 0):
        self.path = existing_path(path)
        self.k = _check_k(k)
        self._L = load_ingest_library()
        self._attach(self._open_handle("pmx_dkm_open", self.path.encode(), self.k, int(device), int(threads),
                                       int(budget_bytes), int(hash_bits)))


def open_kmer_track(path, k, device_ingest: bool, device: int = 0):
    """``DeviceKmerTrackReader`` on ``device`` with ``device_ingest``, else ``KmerTrackReader``."""
    if device_ingest:
        return DeviceKmerTrackReader(path, k, device=device)
    return KmerTrackReader(path, k)


def write_bed(track, out_path) -> int:
    """The track as BED3 in the order of its chromosomes; gzip (mtime 0, so that equal tracks give equal bytes) when the name
    ends in .gz.  Returns the number of intervals written."""
    out_path = os.fspath(out_path)
    n = 0
    parts = []
    for chrom in track.chromsizes:
        b, e, _v = track.fetch_arrays(0.0, chrom)
        if len(b):
            lines = np.char.add(np.char.add(np.char.add(chrom + "\t", b.astype(str)), "\t"), e.astype(str))
            parts.append("\n".join(lines.tolist()) + "\n")
            n += len(b)
    data = "".join(parts).encode()
    if out_path.lower().endswith(".gz"):
        with open(out_path, "wb") as raw:
            with gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as fh:
                fh.write(data)
    else:
        with open(out_path, "wb") as fh:
            fh.write(data)
    return n
