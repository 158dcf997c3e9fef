"""TEST INFRASTRUCTURE ONLY -- a stand-in for the ``pyBigWig`` module, written for this project.

The reference's ``reader/bigwig.pyx`` does a plain ``import pyBigWig`` and uses three things of it:
``open(path)``, ``.chroms()`` and ``.intervals(chrom, start, end)`` (plus ``.close()``).  This module
offers exactly those over a JSON file, so that oracle/make_ref_mscc_vectors.py can run the reference's
own compiled ``successive`` MSCC calculator on synthetic tracks where the real pyBigWig is not installed:

    {"chroms": {name: size, ...}, "intervals": {name: [[begin, end, value], ...], ...}}

Like pyBigWig it returns values as float32 (widened to Python floats), clips to the query range, and
returns ``None`` for a chromosome that holds no interval.  Only the reference's reader imports it, and only when the
generator (or the test that re-runs it) has put this directory on ``sys.path``; ``pymasc_amd`` never does.
"""
import builtins
import json
import struct


class _Track:
    def __init__(self, path):
        with builtins.open(path) as fh:
            doc = json.load(fh)
        self._chroms = {str(k): int(v) for k, v in doc["chroms"].items()}
        self._intervals = doc.get("intervals", {})

    def chroms(self):
        return dict(self._chroms)

    def intervals(self, chrom, start=0, end=None):
        if chrom not in self._chroms:
            raise RuntimeError("Invalid interval bounds!")      # (what pyBigWig raises for an unknown chromosome)
        end = self._chroms[chrom] if end is None else end
        out = [(max(int(b), start), min(int(e), end), struct.unpack("f", struct.pack("f", v))[0])
               for b, e, v in self._intervals.get(chrom, ()) if int(b) < end and int(e) > start]
        return tuple(out) or None

    def close(self):
        self._intervals = {}


def open(path, mode="r"):
    return _Track(path)
