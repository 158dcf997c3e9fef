"""Fragment-length estimate and the ChIP-seq quality scores NSC, RSC, FWHM and VSN, written to ``<name>_stats.tab``.

What PyMaSC computes from the cross-correlation curves once they exist (PyMaSC/stats.py, interfaces/stats.py,
utils/calc.py:24-46, output/stats.py:48-130), reimplemented on the host.  Per curve (each chromosome, then the merged
genome-wide curve, for NCC and for MSCC):

  avr_cc        the curve smoothed by a ``smooth_window`` moving average; the first and last ``smooth_window // 2``
                points average a partial window that grows towards the inside (utils/calc.py:24-46)
  cc_min        the background: element ``min(bg_avr_width, len) // 2`` of the sorted last ``bg_avr_width`` values
  ccrl          cc at the read length (index ``read_len - 1``)
  est_lib_len   ``argmax(avr_cc) + 1``; when that lies within ``mask_size`` of the read length (the phantom peak) it is
                taken again with ``avr_cc[read_len - 1 - mask_size : read_len + mask_size]`` masked out
  fwhm          width of the smoothed peak at half height over cc_min, walked out from ``length - 1`` with the peak
                height read at ``avr_cc[length - 2]`` (the reference's index); a side that runs off the curve gives
                twice the other side's half width; both sides failing gives ``False``
  nsc, rsc, vsn ``ccfl / cc_min``, ``(ccfl - cc_min) / (ccrl - cc_min)``, ``2 ccfl fwhm / (forward + reverse)``

each at the expected length (``library_length``, when given) and at the estimated length.  A failed FWHM is ``False``,
as in the reference, and VSN then is ``0.0``: the file says ``False`` / ``0.0`` exactly where PyMaSC's does.

Genome-wide, the per-chromosome curves are merged by ``tables.merge_cc`` (Fisher z, weights n - 3; n = chromosome length
for NCC, ``mappable_len[read_len - 1]`` for MSCC); read counts (and, for MSCC, the mappable lengths by lag) are summed;
NCC's genome length also counts the chromosomes without reads.  When an MSCC curve exists, its genome-wide estimate is
the length at which the genome-wide NCC "estimated" scores are taken.  Per chromosome the reference does not do this:
``BothGenomeWideResultModel`` derives from ``NCCGenomeWideResultModel``, so PyMaSC/stats.py:622 is the branch taken
and each chromosome's NCC keeps its own estimate.  The same holds here (none of it reaches ``_stats.tab``).

Differences from the reference, both where it would fail with a bare exception: a peak height not above cc_min is a
ValueError (the reference's ``assert``), and a merged curve with no finite value at a shift is NaN there (the reference
divides by a zero weight sum); a strand without reads then gives ReadsTooFew as usual.

There is no kernel here: the input is O(chromosomes x max_shift) float64 values, read once per run after the GPU work.
"""
from __future__ import annotations

import logging
import math
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Mapping, Optional, Tuple, Union

import numpy as np

from .exceptions import ReadsTooFew
from .result import BothGenomeWideResult, EmptyResult, MSCCGenomeWideResult, NCCGenomeWideResult
from .tables import merge_cc

logger = logging.getLogger(__name__)

STATS_SUFFIX = "_stats.tab"

#: an estimate this close to the read length is reported as suspicious when no mask is applied
_NEAR_READLEN = 5
#: how many leading shifts are compared with the background
_HEAD = 10

_SUMMARY_LABELS = ("Name", "Read length", "Expected library length", "Estimated library length")
_ROW_FIELDS = ("genomelen", "forward_reads", "reverse_reads", "cc_min", "ccrl", "ccfl", "ccfl_est", "nsc", "rsc",
               "nsc_est", "rsc_est", "fwhm", "vsn", "fwhm_est", "vsn_est")
_NCC_LABELS = ("Genome length", "Forward reads", "Reverse reads", "Minimum NCC", "NCC at read length",
               "NCC at expected library length", "NCC at estimated library length", "NSC", "RSC", "Estimated NSC",
               "Estimated RSC", "FWHM", "VSN", "Estimated FWHM", "Estimated VSN")
_MSCC_LABELS = ("DMP length", "Forward reads in DMP", "Reverse reads in DMP", "Minimum MSCC", "MSCC at read length",
                "MSCC at expected library length", "MSCC at estimated library length", "MSCC NSC", "MSCC RSC",
                "Estimated MSCC NSC", "Estimated MSCC RSC", "MSCC FWHM", "MSCC VSN", "Estimated MSCC FWHM",
                "Estimated MSCC VSN")
#: every label of ``_stats.tab``, in file order (34 rows)
STATS_LABELS = _SUMMARY_LABELS + _NCC_LABELS + _MSCC_LABELS


@dataclass(frozen=True)
class Params:
    """PyMaSC's statistics options (utils/parsearg.py:235-260): -r, -l, -w, --bg-avr-width, --mask-size, --chi2-pval."""
    read_len: int
    library_length: Optional[int] = None
    smooth_window: int = 15
    bg_avr_width: int = 50
    mask_size: int = 5
    chi2_pval: float = 0.05


@dataclass(frozen=True)
class Metrics:
    """Scores at one fragment length; all None when no length was asked for.  ``fwhm`` is False when it failed."""
    fragment_length: Optional[int] = None
    ccfl: Optional[float] = None
    fwhm: Union[int, bool, None] = None
    nsc: Optional[float] = None
    rsc: Optional[float] = None
    vsn: Optional[float] = None


@dataclass(frozen=True, eq=False)
class CurveStats:
    """Statistics of one NCC or MSCC curve.  For MSCC ``genomelen`` / ``forward_reads`` / ``reverse_reads`` are arrays by
    lag and the reported value is the element at ``read_len - 1``.  ``cc_lower`` / ``cc_upper``: the 99 % interval of a
    merged genome-wide curve, None per chromosome."""
    kind: str                        # "NCC" or "MSCC"
    read_len: int
    genomelen: Union[int, np.ndarray]
    forward_reads: Union[int, np.ndarray]
    reverse_reads: Union[int, np.ndarray]
    cc: np.ndarray
    avr_cc: np.ndarray
    cc_min: float
    ccrl: float
    est_lib_len: int
    expected: Metrics
    estimated: Metrics
    cc_lower: Optional[np.ndarray] = None
    cc_upper: Optional[np.ndarray] = None

    def _repr(self, v) -> int:
        return int(v) if self.kind == "NCC" else int(np.asarray(v)[self.read_len - 1])

    @property
    def genomelen_repr(self) -> int:
        return self._repr(self.genomelen)

    @property
    def forward_reads_repr(self) -> int:
        return self._repr(self.forward_reads)

    @property
    def reverse_reads_repr(self) -> int:
        return self._repr(self.reverse_reads)


@dataclass(frozen=True, eq=False)
class GenomeStats:
    """What ``genome_wide_stats`` returns: the genome-wide and per-chromosome statistics of each curve the result has
    (None / empty where it has none).  Chromosomes without reads have no entry."""
    params: Params
    whole_ncc: Optional[CurveStats]
    whole_mscc: Optional[CurveStats]
    ncc: Dict[str, CurveStats]
    mscc: Dict[str, CurveStats]

    @property
    def read_len(self) -> int:
        return self.params.read_len

    @property
    def expected_lib_len(self) -> Optional[int]:
        return self.params.library_length

    @property
    def est_lib_len(self) -> int:
        """The run's fragment-length estimate: MSCC's when there is an MSCC curve, NCC's otherwise."""
        return (self.whole_mscc if self.whole_mscc is not None else self.whole_ncc).est_lib_len


# ---- one curve -----------------------------------------------------------------------------------------------------

def moving_average(cc: np.ndarray, window: int) -> np.ndarray:
    """Centred moving average of ``window`` points; the ``window // 2`` points at each edge average the first (last)
    ``window // 2 + i`` values instead (i = distance from the edge)."""
    avr = np.correlate(cc, np.repeat(1, window) / float(window), mode="same")
    half = window // 2
    for i in range(half):
        avr[i] = np.mean(cc[:half + i])
        avr[-(i + 1)] = np.mean(cc[-(half + i):])
    return avr


def _background(cc: np.ndarray, width: int, warn: bool) -> float:
    tail = np.sort(cc[-width:])
    cc_min = tail[min(width, cc.size) // 2]
    if warn and np.median(cc[:_HEAD]) < cc_min:
        logger.warning("The background coefficient (%r) is above the median of the first %d shifts: the curve may not "
                       "have decayed yet; a larger max_shift may help.", float(cc_min), _HEAD)
    return cc_min


def _estimate(avr: np.ndarray, p: Params, warn: bool) -> int:
    est = int(np.argmax(avr)) + 1
    suspicious = False
    if p.mask_size and abs(est - p.read_len) <= p.mask_size:
        logger.warning("Estimated library length %d is within %d of the read length %d: masking the phantom peak "
                       "(read length +/- %d) and estimating again.", est, p.mask_size, p.read_len, p.mask_size)
        lo = max(0, p.read_len - 1 - p.mask_size)
        hi = min(len(avr), p.read_len + p.mask_size)
        masked = avr.copy()
        masked[lo:hi] = -np.inf
        est = int(np.argmax(masked)) + 1
        suspicious = est - 1 in (lo - 1, hi)             # the new maximum sits right at an edge of the mask
    elif warn and abs(est - p.read_len) <= _NEAR_READLEN:
        suspicious = True
    if warn and suspicious:
        logger.error("Estimated library length %d is close to the read length %d: check the curves.", est, p.read_len)
    return est


def _fwhm(avr: np.ndarray, cc_min: float, length: int) -> Union[int, bool]:
    if np.isnan(cc_min):
        return False
    top = length - 1
    if top < 0:
        raise ValueError("fragment length must be at least 1, got {}".format(length))
    height = avr[top - 1]                                   # the reference reads the peak one shift early
    if not height > cc_min:
        raise ValueError("FWHM at length {}: the smoothed curve ({!r}) is not above the background ({!r})"
                         .format(length, float(height), float(cc_min)))
    half = cc_min + (height - cc_min) / 2
    fwd, fwd_failed = 0, False
    while avr[top + fwd] > half:
        fwd += 1
        if top + fwd == avr.size:
            logger.warning("FWHM at length %d: the forward side of the peak runs off the curve; a larger max_shift "
                           "may help.", length)
            fwd, fwd_failed = fwd - 1, True
            break
    back, back_failed = 0, False
    while avr[top - back] > half:
        back += 1
        if back > top:
            logger.warning("FWHM at length %d: the backward side of the peak runs off the curve.", length)
            back, back_failed = back - 1, True
            break
    if fwd_failed and back_failed:
        logger.error("FWHM at length %d: both sides of the peak run off the curve; no width.", length)
        return False
    if fwd_failed:
        logger.warning("FWHM at length %d: using twice the backward half width.", length)
        return back * 2 + 1
    if back_failed:
        logger.warning("FWHM at length %d: using twice the forward half width.", length)
        return fwd * 2 + 1
    return back + fwd + 1


def _metrics(cc, avr, cc_min, ccrl, length, fwd_repr, rev_repr) -> Metrics:
    ccfl = cc[length - 1]
    fwhm = _fwhm(avr, cc_min, length)
    with np.errstate(divide="ignore", invalid="ignore"):
        nsc = ccfl / cc_min
        rsc = (ccfl - cc_min) / (ccrl - cc_min)
        vsn = 2 * ccfl * fwhm / (fwd_repr + rev_repr)
    return Metrics(length, ccfl, fwhm, nsc, rsc, vsn)


def curve_stats(kind: str, cc, genomelen, forward_reads, reverse_reads, p: Params, warn: bool = False,
                est_lib_len: Optional[int] = None, interval=(None, None)) -> CurveStats:
    """Statistics of one curve.  ``est_lib_len``: the length the "estimated" scores are taken at instead of this curve's
    own estimate (which ``CurveStats.est_lib_len`` still reports)."""
    cc = np.asarray(cc, dtype=np.float64)
    avr = moving_average(cc, p.smooth_window)
    cc_min = _background(cc, p.bg_avr_width, warn)
    own = _estimate(avr, p, warn)
    ccrl = cc[p.read_len - 1]
    rl = p.read_len - 1
    fwd_repr = int(forward_reads) if kind == "NCC" else int(np.asarray(forward_reads)[rl])
    rev_repr = int(reverse_reads) if kind == "NCC" else int(np.asarray(reverse_reads)[rl])
    expected = (Metrics() if p.library_length is None else
                _metrics(cc, avr, cc_min, ccrl, p.library_length, fwd_repr, rev_repr))
    estimated = _metrics(cc, avr, cc_min, ccrl, own if est_lib_len is None else est_lib_len, fwd_repr, rev_repr)
    return CurveStats(kind, p.read_len, genomelen, forward_reads, reverse_reads, cc, avr, cc_min, ccrl, own, expected,
                      estimated, interval[0], interval[1])


# ---- genome-wide ---------------------------------------------------------------------------------------------------

def _cc_of(r) -> np.ndarray:
    if getattr(r, "cc", None) is None:
        r.calc_cc()
    return np.asarray(r.cc, dtype=np.float64)


def _chrom_stats(kind, chroms, p: Params):
    """(per-chromosome stats of the chromosomes with reads, genome length of those without)."""
    out: Dict[str, CurveStats] = {}
    empty_len = 0
    for c, r in chroms.items():
        if r is None:
            continue
        if isinstance(r, EmptyResult):
            empty_len += int(r.genomelen)
            continue
        if kind == "NCC":
            glen, fw, rv = r.genomelen, r.forward_sum, r.reverse_sum
        else:
            glen = np.array(r.mappable_len, dtype=np.int64)
            fw, rv = np.asarray(r.forward_sum, dtype=np.int64), np.asarray(r.reverse_sum, dtype=np.int64)
        out[c] = curve_stats(kind, _cc_of(r), glen, fw, rv, p)
    return out, empty_len


def _whole(kind, chroms: Mapping[str, CurveStats], empty_len: int, p: Params, warn: bool, est_lib_len=None, reads=None):
    if not chroms:
        return None
    rows = list(chroms.values())
    merged, lo, hi = merge_cc([s.genomelen_repr for s in rows], [s.cc for s in rows])
    glen = np.sum(np.asarray([s.genomelen for s in rows], dtype=np.int64), axis=0)
    if reads is not None:
        fw, rv = (np.asarray(x, dtype=np.int64) for x in reads)
    else:
        fw = np.sum(np.asarray([s.forward_reads for s in rows], dtype=np.int64), axis=0)
        rv = np.sum(np.asarray([s.reverse_reads for s in rows], dtype=np.int64), axis=0)
    if kind == "NCC":                # chromosomes without reads count towards NCC's genome length only
        glen, fw, rv = int(glen) + empty_len, int(fw), int(rv)
    return curve_stats(kind, merged, glen, fw, rv, p, warn, est_lib_len, (lo, hi))


def _strand_balance(s: CurveStats, pval: float) -> None:
    """χ² test of forward vs reverse counts against 1:1, one degree of freedom (survival function erfc(sqrt(x / 2)))."""
    a, b = s.forward_reads_repr, s.reverse_reads_repr
    if a == 0 and b == 0:
        return
    n = a + b
    x = ((a - n / 2.) ** 2 + (b - n / 2.) ** 2) / n
    p = math.erfc(math.sqrt(x / 2))
    if p <= pval:
        logger.warning("%s forward/reverse read counts are imbalanced: +/- = %d / %d, chi-squared p-value %.5g <= %s",
                       s.kind, a, b, p, pval)
    else:
        logger.info("%s forward/reverse read counts +/- = %d / %d, chi-squared p-value %.5g > %s", s.kind, a, b, p, pval)


def check_params(read_len, library_length=None, smooth_window=15, max_shift=None) -> None:
    """ValueError for options the statistics cannot use.  PyMaSC logs a ``library_length`` above ``max_shift`` and ignores
    it; here it is an error, as are a ``library_length`` or ``smooth_window`` below 1."""
    if read_len is not None and read_len < 1:
        raise ValueError("read_len must be at least 1, got {}".format(read_len))
    if library_length is not None:
        if library_length < 1:
            raise ValueError("library_length must be at least 1, got {}".format(library_length))
        if max_shift is not None and library_length > max_shift:
            raise ValueError("library_length {} is longer than max_shift {}".format(library_length, max_shift))
    if smooth_window < 1:
        raise ValueError("smooth_window must be at least 1, got {}".format(smooth_window))


def genome_wide_stats(result, read_len: int, library_length: Optional[int] = None, smooth_window: int = 15,
                      bg_avr_width: int = 50, mask_size: int = 5, chi2_pval: float = 0.05,
                      output_warnings: bool = True, mscc_reads=None) -> GenomeStats:
    """Statistics of a genome-wide result: ``NCCGenomeWideResult``, ``MSCCGenomeWideResult`` or ``BothGenomeWideResult``,
    the stand-alone dataclasses or the reference's own classes (pymasc_amd.result binds whichever is present).
    ``output_warnings``: the genome-wide curves' warnings (background above the first shifts, estimate near the read
    length); the per-chromosome curves never give them.  Raises ReadsTooFew when a genome-wide curve has no forward or
    no reverse read (for MSCC only when there is no NCC curve; with one, it is a warning).  ``mscc_reads``: the genome-wide
    (forward, reverse) mappable read counts by shift, in place of the sums over the chromosomes, for a result whose
    per-chromosome counts are not known (a ``_nreads.tab`` written without MSCC columns, as ``--skip-ncc`` writes it)."""
    check_params(read_len, library_length, smooth_window)
    p = Params(int(read_len), None if library_length is None else int(library_length), int(smooth_window),
               int(bg_avr_width), int(mask_size), float(chi2_pval))
    if isinstance(result, BothGenomeWideResult):
        ncc_rows, mscc_rows = result.chroms, result.mappable_chroms
    elif isinstance(result, MSCCGenomeWideResult):
        ncc_rows, mscc_rows = None, result.chroms
    elif isinstance(result, NCCGenomeWideResult):
        ncc_rows, mscc_rows = result.chroms, None
    else:
        raise TypeError("unsupported genome-wide result: {!r}".format(type(result)))

    mscc, whole_mscc = {}, None
    if mscc_rows is not None:
        mscc, empty = _chrom_stats("MSCC", mscc_rows, p)
        whole_mscc = _whole("MSCC", mscc, empty, p, output_warnings, reads=mscc_reads)
    ncc, whole_ncc = {}, None
    if ncc_rows is not None:
        ncc, empty = _chrom_stats("NCC", ncc_rows, p)
        whole_ncc = _whole("NCC", ncc, empty, p, output_warnings,
                           whole_mscc.est_lib_len if whole_mscc is not None else None)
    if whole_ncc is None and whole_mscc is None:
        raise ReadsTooFew("no chromosome has reads")

    if whole_ncc is not None:
        for n, strand in ((whole_ncc.forward_reads, "forward"), (whole_ncc.reverse_reads, "reverse")):
            if n == 0:
                logger.error("There is no %s read.", strand)
                raise ReadsTooFew("there is no {} read".format(strand))
        _strand_balance(whole_ncc, p.chi2_pval)
    if whole_mscc is not None:
        for n, strand in ((whole_mscc.forward_reads, "forward"), (whole_mscc.reverse_reads, "reverse")):
            if np.sum(n) == 0:
                if whole_ncc is None:
                    logger.error("There is no %s read in mappable regions.", strand)
                    raise ReadsTooFew("there is no {} read in mappable regions".format(strand))
                logger.warning("There is no %s read in mappable regions.", strand)
        _strand_balance(whole_mscc, p.chi2_pval)
    return GenomeStats(p, whole_ncc, whole_mscc, ncc, mscc)


# ---- _stats.tab ----------------------------------------------------------------------------------------------------

def _fmt(v) -> str:
    if v is None:
        return "nan"
    if isinstance(v, (bool, np.bool_)):
        return str(bool(v))
    if isinstance(v, (int, np.integer)):
        return repr(int(v))
    if isinstance(v, (float, np.floating)):
        return repr(float(v))
    return str(v)


def _curve_row(s: Optional[CurveStats]) -> List[str]:
    if s is None:
        return ["nan"] * len(_ROW_FIELDS)
    e, x = s.expected, s.estimated
    return [_fmt(v) for v in (s.genomelen_repr, s.forward_reads_repr, s.reverse_reads_repr, s.cc_min, s.ccrl, e.ccfl,
                              x.ccfl, e.nsc, e.rsc, x.nsc, x.rsc, e.fwhm, e.vsn, x.fwhm, x.vsn)]


def stats_rows(name: str, stats: GenomeStats) -> List[Tuple[str, str]]:
    """The (label, value) rows of ``_stats.tab`` in file order (output/stats.py:48-130)."""
    values = [name, _fmt(stats.read_len), _fmt(stats.expected_lib_len), _fmt(stats.est_lib_len)]
    values += _curve_row(stats.whole_ncc) + _curve_row(stats.whole_mscc)
    return list(zip(STATS_LABELS, values))


def write_stats(outfile: Union[str, os.PathLike], stats: GenomeStats) -> Path:
    """Writes ``<outfile>_stats.tab`` (the suffix is appended to the whole path, as PyMaSC does) and returns its path; the
    Name row is the last component of ``outfile``."""
    base = Path(outfile)
    path = Path(str(base) + STATS_SUFFIX)
    with open(path, "w") as fp:
        for label, value in stats_rows(base.name, stats):
            fp.write("{}\t{}\n".format(label, value))
    return path


def load_stats(path) -> Dict[str, str]:
    """label -> value (as text) of a ``_stats.tab`` file."""
    with open(path) as fp:
        return dict(line.rstrip("\n").split("\t", 1) for line in fp if "\t" in line)
