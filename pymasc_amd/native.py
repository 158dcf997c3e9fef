"""What every reader over libpymasc_io.so (include/pymasc_amd_io.h, host) and libpymasc_ingest.so
(include/pymasc_amd_ingest.h, device) shares: the two libraries' prototypes as data and the one loader that declares them,
``PmxIOError`` / ``raise_last``, and the reader bases -- ``NativeReader`` (handle, close, context manager),
``AlignmentReader`` (the accessors of the pmx_bam / pmx_sam / pmx_dbam handle families) and ``TrackReader`` (``chromsizes``,
``kind`` and ``sorted`` of the pmx_track / pmx_dbw handles) --, and what the counts taken beside the correlation share on a device
reader: ``SIDE_KINDS``, ``SideAccumulator`` and ``count_over``.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

PMX_BAM_FLAG_UNMAPPED = 0x4
PMX_BAM_FLAG_REVERSE = 0x10
PMX_BAM_FLAG_READ2 = 0x80
PMX_BAM_FLAG_DUPLICATE = 0x400
PMX_BAM_DEFAULT_EXCLUDE = PMX_BAM_FLAG_READ2 | PMX_BAM_FLAG_UNMAPPED | PMX_BAM_FLAG_DUPLICATE
PMX_COMPLEXITY_BINS = 32        # (include/pymasc_amd_ingest.h)
PMX_BINCOUNT_HIST = 4096
PMX_FRAGMENTS_MAX_SIZE = 65536
PMX_FRAGMENTS_COUNTERS = 10
PMX_IO_ERR_NOTFOUND = -4        # (PMX_DBAM_ERR_NOTFOUND has the same value)
TRACK_KINDS = ("bigwig", "bigbed", "kmer")      # pmx_track_kind / pmx_dbw_kind


class PmxIOError(IOError):
    """An error reported by libpymasc_io.so or libpymasc_ingest.so; ``code`` is the PMX_IO_ERR_* value."""

    def __init__(self, code: int, msg: str):
        super().__init__("[pmx_io {}] {}".format(code, msg))
        self.code = code
        self.msg = msg

    def __reduce__(self):           # (pickled as its two arguments: the ranks of a run pass it to each other)
        return type(self), (self.code, self.msg)


_int, _str, _vp, _i32, _i64, _u32, _u64, _f32 = (ctypes.c_int, ctypes.c_char_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                 ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float)
_out, _pu64 = ctypes.POINTER(_vp), ctypes.POINTER(_u64)
_sizes = [_i32, ctypes.POINTER(_str), ctypes.POINTER(_i64)]     # nref, names, lengths of a BED read file's references


def _alignment_protos(p: str) -> dict:
    """The accessors every alignment handle family has under its prefix (pmx_bam / pmx_sam / pmx_dbam)."""
    return {
        p + "_close": (None, [_vp]),
        p + "_nref": (_i32, [_vp]),
        p + "_ref_name": (_str, [_vp, _i32]),
        p + "_ref_len": (_i64, [_vp, _i32]),
        p + "_header_text": (_str, [_vp, ctypes.POINTER(_u32)]),
        p + "_readlen_hist": (_i64, [_vp, _u32, _i64, _vp, _vp, _vp]),
        p + "_readlen_counters": (_int, [_vp, _pu64]),
    }


def _decode_protos(p: str) -> dict:
    """decode-then-fetch (pmx_sam / pmx_dbam)."""
    return {
        p + "_decode": (_i64, [_vp, _u32, _u32, _i32]),
        p + "_fetch": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    }


def _track_protos(p: str) -> dict:
    """The accessors of a track handle under its prefix (pmx_track / pmx_dbw); fetch differs and is listed with the library."""
    return {
        p + "_close": (None, [_vp]),
        p + "_nchrom": (_i32, [_vp]),
        p + "_chrom_name": (_str, [_vp, _i32]),
        p + "_chrom_len": (_i64, [_vp, _i32]),
        p + "_sorted": (_int, [_vp]),
        p + "_kind": (_int, [_vp]),
    }


#: every symbol include/pymasc_amd_io.h declares: name -> (restype, argtypes)
IO_PROTOTYPES = {
    "pmx_io_last_error": (_str, []),
    "pmx_io_version": (_int, []),
    "pmx_bam_open": (_int, [_str, _int, _out]),
    **_alignment_protos("pmx_bam"),
    "pmx_bam_next_batch": (_i64, [_vp, _u32, _u32, _i64, _vp, _vp, _vp, _vp]),
    "pmx_bam_next_mates": (_i64, [_vp, _u32, _u32, _i64] + [_vp] * 8),
    "pmx_bam_counters": (_int, [_vp] + [_pu64] * 4),
    "pmx_bam_index_load": (_int, [_vp, _str]),
    "pmx_bam_has_index": (_int, [_vp]),
    "pmx_bam_fetch_ref": (_int, [_vp, _i32]),
    "pmx_sam_open": (_int, [_str, _int, _out]),
    "pmx_sam_open_header": (_int, [_str, _out]),
    "pmx_bed_open": (_int, [_str, _int] + _sizes + [_out]),
    **_alignment_protos("pmx_sam"),
    **_decode_protos("pmx_sam"),
    "pmx_sam_fetch_mates": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "pmx_sam_counters": (_int, [_vp] + [_pu64] * 5),
    "pmx_bigwig_open": (_int, [_str, _out]),
    "pmx_ttrack_open": (_int, [_str, _int, _out]),
    "pmx_kmer_open": (_int, [_str, _i32, _int, _out]),
    **_track_protos("pmx_track"),
    "pmx_track_fetch": (_i64, [_vp, _str, _f32, _i64, _vp, _vp, _vp]),
}

#: every symbol include/pymasc_amd_ingest.h declares: name -> (restype, argtypes)
INGEST_PROTOTYPES = {
    "pmx_dbam_last_error": (_str, []),
    "pmx_dbam_version": (_int, []),
    "pmx_dbam_open": (_int, [_str, _int, _int, _out]),
    "pmx_dbam_open_indexed": (_int, [_str, _str, _int, _int, _out]),
    "pmx_dsam_open": (_int, [_str, _int, _int, _out]),
    "pmx_dbed_open": (_int, [_str, _int, _int] + _sizes + [_out]),
    "pmx_dbam_open_stream": (_int, [_int, _int, _int, _u64, _out]),
    "pmx_dbam_stream_next": (_i64, [_vp]),
    "pmx_dbam_stream_info": (_int, [_vp, _pu64]),
    "pmx_dbam_select": (_int, [_vp, ctypes.POINTER(_i32), _i32]),
    **_alignment_protos("pmx_dbam"),
    **_decode_protos("pmx_dbam"),
    "pmx_dbam_device_arrays": (_int, [_vp] + [_out] * 4),
    "pmx_dbam_runs": (_i64, [_vp, _i64, _vp, _vp, _vp, _vp]),
    "pmx_dbam_complexity": (_int, [_vp, _u32, _u32, _vp, _vp, _vp]),
    "pmx_dbam_bincount_begin": (_int, [_vp, _u32, _u32, _vp]),
    "pmx_dbam_bincount_add": (_int, [_vp, _u32, _u32, _pu64]),
    "pmx_dbam_bincount_hist": (_i64, [_vp, _vp, _vp, _i64, _vp]),
    "pmx_dbam_bincount_copy": (_int, [_vp, _i64, _i64, _vp]),
    "pmx_dbam_peakcount_begin": (_int, [_vp, _i32, _vp, _vp, _vp, _u32, _vp]),
    "pmx_dbam_peakcount_add": (_int, [_vp, _u32, _u32, _vp]),
    "pmx_dbam_peakcount_copy": (_int, [_vp, _i64, _i64, _vp]),
    "pmx_dbam_peakcount_totals": (_int, [_vp, _vp, _vp]),
    "pmx_dbam_coverage_begin": (_int, [_vp, _u32, _vp]),
    "pmx_dbam_coverage_add": (_int, [_vp, _u32, _u32, _pu64]),
    "pmx_dbam_coverage_finish": (_int, [_vp, _vp]),
    "pmx_dbam_coverage_runs": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "pmx_dbam_coverage_text": (_i64, [_vp, _i64, _i64, _vp, _i64]),
    "pmx_dbam_coverage_ranges": (_i64, [_vp, _vp, _i64]),
    "pmx_dbam_coverage_sections": (_i64, [_vp, _i64, _i64, _u32, _u32, _vp, _i64, _vp, _i64]),
    "pmx_dbam_coverage_zoom_begin": (_int, [_vp, _u32, _u32, _vp, _vp]),
    "pmx_dbam_coverage_zoom_records": (_i64, [_vp, _u32, _u32, _vp, _i64, _vp, _i64]),
    "pmx_ddeflate_bound": (_u64, [_u64]),
    "pmx_ddeflate": (_i64, [_int, _vp, _vp, _i64, _vp, _i64, _vp]),
    "pmx_dbam_coverage_sections_z": (_i64, [_vp, _i64, _i64, _u32, _u32, _vp, _i64, _vp, _i64, _vp]),
    "pmx_dbam_coverage_zoom_records_z": (_i64, [_vp, _u32, _u32, _vp, _i64, _vp, _i64, _vp]),
    "pmx_dbam_coverage_signal": (_int, [_vp, _u32, ctypes.c_double, _vp]),
    "pmx_dbam_coverage_compare": (_int, [_vp, _vp, _u32, _int, ctypes.c_double, ctypes.c_double, ctypes.c_double, _vp]),
    "pmx_dbam_coverage_poisson": (_int, [_vp, _vp, _u32, ctypes.c_double, _u32, _u32, _vp, ctypes.c_uint64, _vp]),
    "pmx_dbam_coverage_call": (_int, [_vp, ctypes.c_double, _u32, _u32, _vp]),
    "pmx_dbam_coverage_call_rows": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "pmx_dbam_coverage_call_text": (_i64, [_vp, _i64, _i64, _vp, _i64]),
    "pmx_dbam_coverage_qvalue": (_int, [_vp, _vp]),
    "pmx_dbam_coverage_qvalue_rows": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
    "pmx_dbam_coverage_qvalue_cutoff": (_int, [_vp, ctypes.c_double, _vp]),
    "pmx_dbam_coverage_signal_runs": (_int, [_vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "pmx_dbam_coverage_signal_text": (_i64, [_vp, _i64, _i64, _vp, _i64]),
    "pmx_dbam_coverage_signal_ranges": (_i64, [_vp, _vp, _i64]),
    "pmx_dbam_coverage_signal_sections": (_i64, [_vp, _i64, _i64, _u32, _u32, _vp, _i64, _vp, _i64, _vp]),
    "pmx_dbam_coverage_signal_zoom_begin": (_int, [_vp, _u32, _u32, _vp, _vp]),
    "pmx_dbam_coverage_signal_zoom_records": (_i64, [_vp, _u32, _u32, _vp, _i64, _vp, _i64]),
    "pmx_dbam_coverage_signal_sections_z": (_i64, [_vp, _i64, _i64, _u32, _u32, _vp, _i64, _vp, _i64, _vp, _vp]),
    "pmx_dbam_coverage_signal_zoom_records_z": (_i64, [_vp, _u32, _u32, _vp, _i64, _vp, _i64, _vp]),
    "pmx_dbam_gcbias_begin": (_int, [_vp, _vp, _u32, _vp]),
    "pmx_dbam_gcbias_add": (_int, [_vp, _u32, _u32, _vp]),
    "pmx_dbam_gcbias_tables": (_i64, [_vp, _vp, _vp, _i64, _vp]),
    "pmx_dbam_fragments_begin": (_int, [_vp, _u32, _vp]),
    "pmx_dbam_fragments_add": (_int, [_vp, _u32, _u32, _pu64]),
    "pmx_dbam_fragments_tables": (_int, [_vp, _vp, _vp]),
    "pmx_dbam_fragments_timings": (_int, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "pmx_dbam_fragments_rows": (_i64, [_vp, _u32, _u32, _u32, _vp, _i64, _vp, _vp, _vp, _vp]),
    "pmx_dbam_coverage_add_fragments": (_int, [_vp, _u32, _u32, _u32, _pu64]),
    "pmx_dbam_tss_begin": (_int, [_vp, _i64, _vp, _vp, _vp, _u32, _u32, _vp]),
    "pmx_dbam_tss_add": (_int, [_vp, _u32, _u32, _vp]),
    "pmx_dbam_tss_copy": (_int, [_vp, _vp]),
    "pmx_dbam_tss_totals": (_int, [_vp, _vp]),
    "pmx_dgc_open": (_int, [_str, _int, _int, _out]),
    "pmx_dgc_close": (None, [_vp]),
    "pmx_dgc_nrec": (_i32, [_vp]),
    "pmx_dgc_rec_name": (_str, [_vp, _i32]),
    "pmx_dgc_rec_len": (_i64, [_vp, _i32]),
    "pmx_dbam_set_exclude": (_int, [_vp, _i32, _vp, _vp, _vp]),
    "pmx_dbam_exclude_intervals": (_i64, [_vp, _i64, _vp, _vp, _vp]),
    "pmx_dbam_excluded": (_int, [_vp, _pu64, _pu64]),
    "pmx_dbam_counters": (_int, [_vp] + [_pu64] * 6),
    "pmx_dbam_timings": (_int, [_vp, ctypes.POINTER(ctypes.c_double)]),
    "pmx_dbam_inflated": (_int, [_vp, _u64, _u64, _vp]),
    "pmx_dbw_open": (_int, [_str, _int, _int, _out]),
    "pmx_dtt_open": (_int, [_str, _int, _int, _out]),
    "pmx_dkm_open": (_int, [_str, _i32, _int, _int, _i64, _i32, _out]),
    **_track_protos("pmx_dbw"),
    "pmx_dbw_fetch": (_i64, [_vp, _str, _f32]),
    "pmx_dbw_device_arrays": (_int, [_vp] + [_out] * 3),
    "pmx_dbw_copy": (_int, [_vp, _i64, _i64, _vp, _vp, _vp]),
}

_loaded: Dict[str, ctypes.CDLL] = {}


def load_library(name: str, env: str, prototypes: dict, last_error: str):
    """dlopen ``name`` beside this file (or the path the environment variable ``env`` gives), once, and declare
    ``prototypes``; ``last_error`` names the function ``raise_last`` reads the message from."""
    path = os.environ.get(env, os.path.join(_HERE, name))
    if name not in _loaded:
        if not os.path.exists(path):
            raise PmxIOError(-1, "{} not found: run `python pymasc_amd/build.py`".format(path))
        L = ctypes.CDLL(path)
        for fn, (restype, argtypes) in prototypes.items():
            getattr(L, fn).restype = restype
            getattr(L, fn).argtypes = argtypes
        L.last_error = getattr(L, last_error)
        _loaded[name] = L
    return _loaded[name]


def load_io_library():
    """libpymasc_io.so (built by pymasc_amd/build.py:build_io) with its prototypes declared."""
    return load_library("libpymasc_io.so", "PYMASC_AMD_IO_LIB", IO_PROTOTYPES, "pmx_io_last_error")


def load_ingest_library():
    """libpymasc_ingest.so (built by pymasc_amd/build.py:build_ingest) with its prototypes declared."""
    return load_library("libpymasc_ingest.so", "PYMASC_AMD_INGEST_LIB", INGEST_PROTOTYPES, "pmx_dbam_last_error")


def raise_last(lib, code: int):
    """The library's last error of this thread as a ``PmxIOError``."""
    raise PmxIOError(int(code), lib.last_error().decode("utf-8", "replace"))


def existing_path(path) -> str:
    """``path`` as a string, or the reference's IOError when there is no such file (bigwig.pyx:127-128)."""
    path_str = os.fspath(path)
    if not os.path.exists(path_str):
        raise IOError("input file '{0}' dose not exist.".format(path_str))
    return path_str


class NativeReader:
    """What every reader over a library handle shares: ``closed``, ``close()``, the context manager and ``__del__``.
    ``_h`` is the handle (None until the open succeeds and after close), ``_P`` the prefix of the handle family's functions
    (``_fn("close")`` is the library's close function), ``_WHAT`` what the closed-reader ValueError calls the reader."""
    _h = None
    _P = ""
    _WHAT = "reader"

    def _fn(self, name: str):
        return getattr(self._L, self._P + "_" + name)

    def _raise(self, code: int):
        raise_last(self._L, code)

    def _open_handle(self, fn: str, *args):
        """``self._L.<fn>(*args, &handle)``; returns the handle or raises the library's error."""
        h = ctypes.c_void_p()
        rc = getattr(self._L, fn)(*args, ctypes.byref(h))
        if rc:
            self._raise(rc)
        return h

    def _check_open(self) -> None:
        if self._h is None:
            raise ValueError("I/O operation on closed " + self._WHAT)

    @property
    def closed(self) -> bool:
        return self._h is None

    def close(self) -> None:
        if self._h is not None:
            self._fn("close")(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class AlignmentReader(NativeReader):
    """The accessors the alignment handle families share (pmx_bam, pmx_sam, pmx_dbam): the header's ``references`` /
    ``lengths``, ``header_text``, ``counters`` (``_COUNTERS`` names the family's words), ``read_length_histogram``, and for
    the families that decode first and fetch then (pmx_sam, pmx_dbam) ``decode`` / ``_fetch``."""
    _WHAT = "BAM reader"
    _COUNTERS: Tuple[str, ...] = ()

    def _load_references(self) -> None:
        n = self._fn("nref")(self._h)
        self.references: Tuple[str, ...] = tuple(self._fn("ref_name")(self._h, i).decode() for i in range(n))
        self.lengths: Tuple[int, ...] = tuple(int(self._fn("ref_len")(self._h, i)) for i in range(n))

    @property
    def header_text(self) -> str:
        ln = ctypes.c_uint32()
        t = self._fn("header_text")(self._h, ctypes.byref(ln))
        return (t or b"").decode("utf-8", "replace")

    def counters(self) -> dict:
        v = [ctypes.c_uint64() for _ in self._COUNTERS]
        rc = self._fn("counters")(self._h, *[ctypes.byref(x) for x in v])
        if rc:
            self._raise(rc)
        return dict(zip(self._COUNTERS, (int(x.value) for x in v)))

    def read_length_histogram(self, mapq_criteria: int = 0):
        """The read-length histogram with the estimator's filter (PyMaSC core/readlen.pyx:estimate_readlen): one pass over
        every record, beside (not inside) a ``batches`` iteration and without touching the arrays of the last ``decode``.
        Returns a ``pymasc_amd.readlen.ReadLengthHistogram``; its first-occurrence keys are offsets in the uncompressed
        stream (BAM) or of lines in the text (SAM, BED)."""
        from .readlen import histogram_from_library
        self._check_open()
        return histogram_from_library(self._fn("readlen_hist"), self._fn("readlen_counters"), self._h, mapq_criteria,
                                      self._raise)

    def library_complexity(self, mapq_criteria: int = 0, references=None):
        """NRF / PBC1 / PBC2 of the reads at ``mapq_criteria`` over ``references`` (None: all the reader has selected), flagged
        duplicates kept: a ``pymasc_amd.complexity.LibraryComplexity`` (``complexity.from_reader``).  A device reader counts on
        the GPU with arrays of its own: the arrays of the last ``decode`` stay as they are."""
        from .complexity import from_reader
        self._check_open()
        return from_reader(self, mapq_criteria, references)

    def bin_counts(self, mapq_criteria: int = 0, references=None, bin_size: int = 500, extend: int = 0):
        """The reads at ``mapq_criteria`` (flagged duplicates, read2 and unmapped reads dropped) counted per genome bin of
        ``bin_size`` bases over ``references`` (None: all the reader has selected): a ``pymasc_amd.fingerprint.BinCounts``
        (``fingerprint.from_reader``).  ``extend``: every read covers that many bases from its 5' end (0: its own
        length).  A device reader counts on the GPU with arrays of its own: the arrays of the last ``decode`` stay as they are."""
        from .fingerprint import from_reader
        self._check_open()
        return from_reader(self, mapq_criteria, references, bin_size, extend)

    def peak_counts(self, peaks, mapq_criteria: int = 0, references=None, extend: int = 0):
        """The reads of ``bin_counts`` counted per line of ``peaks`` (a peak file's path, an ordered ``{name: [(start, end),
        ...]}`` or ``peaks.open_peaks``' result) and in at least one line: a ``pymasc_amd.peaks.PeakCounts`` with ``frip`` and
        ``enrichment`` (``peaks.from_reader``).  ``extend`` as for ``bin_counts``.  A device reader counts on the
        GPU with arrays of its own: the arrays of the last ``decode`` stay as they are."""
        from .peaks import from_reader
        self._check_open()
        return from_reader(self, peaks, mapq_criteria, references, extend)

    def coverage(self, mapq_criteria: int = 0, references=None, extend: int = 0):
        """The reads of ``bin_counts`` piled up base by base into runs of constant depth: a ``pymasc_amd.coverage.Coverage``
        (``coverage.from_reader``).  ``extend`` as for ``bin_counts``.  A device reader counts on the GPU with
        arrays of its own: the arrays of the last ``decode`` stay as they are."""
        from .coverage import from_reader
        self._check_open()
        return from_reader(self, mapq_criteria, references, extend)

    def gc_bias(self, genome, mapq_criteria: int = 0, references=None, window: int = 100):
        """The reads of ``bin_counts`` against the windows of ``genome`` per G + C content of the window: a
        ``pymasc_amd.gcbias.GcBias`` (``gcbias.from_reader``).  ``genome``: a FASTA file's path, or for a device
        reader an open ``gcbias.DeviceGenome``.  A device reader counts on the GPU with arrays of its own: the arrays of the last
        ``decode`` stay as they are."""
        from .gcbias import from_reader
        self._check_open()
        return from_reader(self, genome, mapq_criteria, references, window)

    def fragment_sizes(self, mapq_criteria: int = 0, references=None, max_size: int = 2000):
        """The paired-end fragment sizes of the reads of ``bin_counts`` that are paired, per orientation, from each read1 record's
        own mate fields: a ``pymasc_amd.fragments.FragmentSizes`` (``fragments.from_reader``).  A device reader
        counts on the GPU with arrays of its own: the arrays of the last ``decode`` stay as they are."""
        from .fragments import from_reader
        self._check_open()
        return from_reader(self, mapq_criteria, references, max_size)

    def tss_profile(self, anchors, mapq_criteria: int = 0, references=None, flank: int = 2000, extend: int = 0):
        """The reads of ``bin_counts`` piled up around ``anchors`` (a BED6 file's path, an ordered ``{name: [(a, "+" | "-"), ...]}``
        or ``tss.open_anchors``' result) by offset and by strand relative to the anchor's, ``flank`` bases either side: a
        ``pymasc_amd.tss.TssProfile`` with ``enrichment`` (``tss.from_reader``).  ``extend`` as for
        ``bin_counts`` (1: the 5' base only).  A device reader counts on the GPU with arrays of its own: the arrays of the last
        ``decode`` stay as they are."""
        from .tss import from_reader
        self._check_open()
        return from_reader(self, anchors, mapq_criteria, references, flank, extend)

    # ---- excluded regions (pymasc_amd.region_mask) ----
    _exclude = None
    _dropped = 0

    def set_exclude(self, mask) -> None:
        """From now on the reads that overlap ``mask`` (a ``region_mask.ResolvedMask`` of this reader's references; None: no
        mask) are left out of ``batches`` / ``feed`` / ``library_complexity``, after the reader's own filter.  A host reader
        applies ``mask.keep`` to every batch; a device reader hands the mask to the library."""
        self._check_open()
        self._exclude = mask
        self._dropped = 0

    def excluded(self) -> int:
        """Reads left out because of the mask since the last pass (``feed`` / ``batches`` / ``decode``) began."""
        return int(self._dropped)

    def _drop_excluded(self, ref, pos, rlen, rev):
        """A host batch less the reads the mask leaves out."""
        if self._exclude is None or ref.size == 0:
            return ref, pos, rlen, rev
        keep = self._exclude.keep(ref, pos, rlen)
        self._dropped += int(ref.size - keep.sum())
        return ref[keep], pos[keep], rlen[keep], rev[keep]

    def decode(self, mapq_criteria: int = 0, flag_exclude: int = PMX_BAM_DEFAULT_EXCLUDE, reference: int = -1) -> int:
        """Runs the record walk + filter; returns the number of kept records (they stay with the handle, for ``_fetch``)."""
        self._check_open()
        n = self._fn("decode")(self._h, int(mapq_criteria), int(flag_exclude), int(reference))
        if n < 0:
            self._raise(n)
        return int(n)

    def _fetch(self, first: int, n: int):
        ref = np.empty(n, dtype=np.int32)
        pos = np.empty(n, dtype=np.int32)
        rlen = np.empty(n, dtype=np.int32)
        rev = np.empty(n, dtype=np.uint8)
        rc = self._fn("fetch")(self._h, first, n, ref.ctypes.data, pos.ctypes.data, rlen.ctypes.data, rev.ctypes.data)
        if rc:
            self._raise(rc)
        return ref, pos, rlen, rev.astype(bool)


#: the counts taken beside the correlation, in the order a stream reader serves them (it decides which error surfaces first)
SIDE_KINDS = ("complexity", "fingerprint", "peaks", "coverage", "gcbias", "fragments", "tss")


class SideAccumulator:
    """What a device reader's side count is to ``DeviceStreamReader._windows``: ``add(reader)`` counts what the handle holds now
    (every window of a stream, the whole of any other device reader); ``begin(reader)`` starts again on a new handle (a regular
    file opened for another pass); ``flush(reader)`` comes behind the last window.  Here the last two do nothing."""

    def begin(self, reader) -> None:
        pass

    def flush(self, reader) -> None:
        pass


def count_over(reader, kind: str, make):
    """The accumulator ``make()`` of ``kind`` (one of ``SIDE_KINDS``) over everything a device reader reads: armed for one pass
    of a stream reader's windows (a regular file is read once more, any other source raises ``InputUnseekable``), one ``add``
    for a whole-file reader."""
    if not hasattr(reader, "_windows"):
        acc = make()
        acc.add(reader)
        return acc
    acc = reader._arm(kind, make())
    try:
        for _ in reader._windows():
            pass
    finally:
        reader._disarm(kind)
    return acc


class TrackReader(NativeReader):
    """What the host (pmx_track) and the device (pmx_dbw) track readers share: ``_attach`` loads ``kind`` and ``chromsizes``;
    ``sorted``, ``fetch`` over the subclass's ``fetch_arrays``, ``disable_progress_bar``."""
    _WHAT = "track reader"

    def _attach(self, h) -> None:
        self._h = h
        self.kind = TRACK_KINDS[self._fn("kind")(h)]
        self.chromsizes: Dict[str, int] = {self._fn("chrom_name")(h, i).decode(): int(self._fn("chrom_len")(h, i))
                                           for i in range(self._fn("nchrom")(h))}

    def _check_chrom(self, chrom: str) -> None:
        self._check_open()
        if chrom not in self.chromsizes:
            raise KeyError(chrom)

    @property
    def sorted(self) -> bool:
        """The intervals of the last fetch are non-empty, ascending and disjoint (true before the first fetch)."""
        return bool(self._fn("sorted")(self._h))

    def fetch(self, valfilter: float, chrom: str):
        begin, end, value = self.fetch_arrays(valfilter, chrom)
        return iter(zip(begin.tolist(), end.tolist(), value.tolist()))

    def disable_progress_bar(self) -> None:
        pass


class HostTrackReader(TrackReader):
    """A track of libpymasc_io.so, whatever it was opened from (the handle is a pmx_track)."""
    _P = "pmx_track"

    def fetch_arrays(self, valfilter: float, chrom: str) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """(begin, end, value) arrays of the chromosome's intervals with value >= valfilter, in the track's order."""
        self._check_chrom(chrom)
        name = chrom.encode()
        n = self._L.pmx_track_fetch(self._h, name, float(valfilter), 0, None, None, None)
        if n == PMX_IO_ERR_NOTFOUND:
            raise KeyError(chrom)
        if n < 0:
            self._raise(n)
        begin = np.empty(n, dtype=np.uint32)
        end = np.empty(n, dtype=np.uint32)
        value = np.empty(n, dtype=np.float32)
        if n:
            m = self._L.pmx_track_fetch(self._h, name, float(valfilter), n, begin.ctypes.data, end.ctypes.data,
                                        value.ctypes.data)
            if m < 0:
                self._raise(m)
            assert m == n
        return begin, end, value
