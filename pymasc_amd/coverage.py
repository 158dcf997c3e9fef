"""The fragment pileup as a bedGraph track: ``--coverage`` / ``coverage=``, what a ChIP-seq user builds next from
the estimated fragment length, taken from the reads that are in device memory already.

The definitions, which the device code (csrc/ingest/coverage_device.inc), the host checker here and the tests state the same way.
They are this project's own: nothing here was compared with ``bedtools genomecov``, deepTools or MACS2.

* The reads are the ones the correlation sees: the run's filter, the chosen references, less the reads an exclude mask drops.
* The extent is the fingerprint's (7.16) with ``extend``: ``L = extend``, or the read's own length at 0; a forward read covers
  ``[pos1, pos1 + L - 1]``, a reverse read ``[pos1 + read_len - L, pos1 + read_len - 1]``; both clipped to ``[1, len]`` of the
  reference.  A read with nothing left after the clip adds nothing and is not in ``reads``.
* With ``extend = "pair"`` (``PAIR``) the reads are replaced by the FR rows of ``pymasc_amd.fragments`` (pairs
  counted at read1, ``size <= max_size``, masked by the fragment's extent): a row covers ``[start1, start1 + size - 1]``, clipped
  the same way, and ``reads`` is the number of rows piled.
* ``depth[r][p]`` is the number of kept reads whose clipped extent holds position ``p`` of reference ``r``, a 32-bit count.
* Per chosen reference, in header order, the maximal intervals of constant depth greater than 0 are the runs
  ``(start0, end0, depth)``, 0-based and half-open as in bedGraph.  Two reads that abut at equal depth form one run; depth 0 is not
  written; a reference without reads has no run.
* Totals: ``reads`` (the reads that added something), ``runs``, ``covered_bases = sum (end0 - start0)``,
  ``fragment_bases = sum depth * (end0 - start0)`` (the sum of the clipped extents' lengths), ``max_depth``.

The file is ``<name>_coverage.bedGraph``: a ``track`` line, then ``chrom<TAB>start0<TAB>end0<TAB>depth`` per run, plain text.

A device reader counts on the GPU and formats the lines there (``pmx_dbam_coverage_*``, include/pymasc_amd_ingest.h); a host reader
goes through its ``batches`` and ``HostCount`` (plain numpy), which is also the device's checker.

The same runs as a bigWig file, ``<name>_coverage.bw`` (``write_bigwig``, ``read_bigwig``): see the second half of
this module.

The pileup as a signal track (``--coverage-bin`` / ``--coverage-normalize``; ``Signal``, ``Coverage.signal``,
``DeviceCount.signal``): the mean depth per bin of ``B`` bases times a scale factor, float32, equal neighbours merged.

* Reference ``r`` of length ``len`` has the bins ``j = 0 .. ceil(len / B) - 1``; bin ``j`` covers ``[j * B, min((j + 1) * B, len))``
  and has the width ``w_j`` (only the last bin can be short); ``S_j`` is the integer sum of the depth over its bases (below 2^47:
  exact as a u64 and as a float64); ``B`` is an integer from 1 to 65536.
* ``v_j = f32((f64(S_j) * scale) / f64(w_j))``: one float64 multiply, one float64 divide, one conversion to float32, each rounded
  to nearest even: ``np.float32((float(S) * scale) / float(w))``.
* ``scale`` is a finite float64 of at least 2^-64 (no value is a float32 denormal) with ``scale * max_depth < 2^40`` (so
  ``v * 10^6 < 2^63`` and the device's text is integer arithmetic); anything else is a ``ValueError`` (``check_scale``).
* Consecutive bins of one reference are one run when they have the same ``S`` and the same width -- the rule is on ``S``, not on
  ``v``: two different ``S`` that round to one float32 stay two runs --; bins with ``S = 0`` are in no run.  A run is ``(ref,
  start0, end0, v)``, in header order.  With ``B = 1`` the signal runs are the depth runs with ``v = f32(f64(depth) * scale)``.
  Totals: ``runs``, ``covered_bases`` (the runs' widths summed), the smallest and the largest ``v``.
* Normalisation (``scale_of``, float64): ``none``: 1.0; ``cpm``: ``1e6 / reads``; ``rpgc``: ``genome_size / fragment_bases``
  (``genome_size``: ``coverage_genome_size``, else the sum of the chosen references' lengths); times ``coverage_scale``, one
  multiplication.  With no kept read the factor is 1.0 and the track is empty.
* bedGraph text: ``value`` is the decimal expansion of the exact value of ``v`` rounded to six decimals, ties to even, without
  trailing zeros and without a trailing ``.`` (``format_value``: ``'%.6f' % float(v)``, stripped); with scale 1 and ``B = 1`` the
  lines equal the depth track's.  The track line is the depth track's followed by `` bin=<B> normalize=<word> scale=<repr>``.
* bigWig: the layout of 7.18.1 with ``v`` as an item's third word.  ``z_0`` is ``zoom_base`` (a multiple of ``B``), else ``B * p``
  with ``p`` the smallest power of two with ``B * p >= max(32, 10 * covered_bases / runs)`` (the signal's counts).  A zoom bin of
  level 0 takes the signal runs that overlap it in ascending start order, each by ``ov`` bases: ``validCount = sum ov``, min and max
  over ``v``, ``sum``: ``acc += f64(ov) * f64(v)``, ``sumSquares``: ``acc += f64(ov) * (f64(v) * f64(v))``, both float64 from 0.0,
  every multiply and add rounded on its own (no fused multiply-add).  A bin of level ``k + 1`` adds its up to four bins of level
  ``k`` in index order the same way.  The records hold the four floats as float32, rounded to nearest.  Total summary:
  ``validCount = covered_bases``, min, max, then ``sum`` and ``sumSquares`` as float64: per data section its runs in order with the
  two products above from 0.0, the sections' partial sums then added in file order on the host from 0.0.

Treatment against control (``--coverage-control``; ``Coverage.compare``, ``DeviceCount.compare``): two pileups
over the same chosen references as one signal track.

* ``S_t[j]`` and ``S_c[j]`` are the integer depth sums per bin of ``B`` bases of the two pileups, with the bins, the widths ``w_j``
  and the bound on ``S`` above; ``B`` is 1 .. 65536.  ``a_t``, ``a_c`` and the pseudocount ``p`` are float64.
* Per bin, in float64, each operation rounded to nearest even on its own (no fused multiply-add): ``t = (f64(S_t) * a_t) /
  f64(w)``, ``c = (f64(S_c) * a_c) / f64(w)``; ``subtract``: ``v = f32(t - c)``; ``ratio``: ``v = f32((t + p) / (c + p))``;
  ``log2``: ``v = f32(lg2((t + p) / (c + p)))``.
* ``lg2(x)`` of a positive normal float64 is a stated algorithm (``lg2``): ``(m, e) = frexp(x)`` with ``m`` in [0.5, 1); if ``m <
  0.7071067811865476`` (the float64 of sqrt(1/2)): ``m = 2 m``, ``e = e - 1``; ``f = m - 1.0``; ``s = f / (2.0 + f)``; ``z = s * s``;
  ``P = c_10``, then for ``k = 9 .. 0``: ``P = P * z + c_k`` with ``c_k = 1.0 / (2 k + 1)`` as a float64 division, the multiply and
  the add rounded separately; ``ln = (2.0 * s) * P``; ``lg2 = f64(e) + ln * 1.4426950408889634``.
* Consecutive bins of one reference are one run when they have the same ``S_t``, the same ``S_c`` and the same width (the rule is
  on the sums, not on ``v``); bins with both sums 0 are in no run; a bin only the control covers is in one.  Totals: ``runs``,
  ``covered_bases``, the smallest and the largest ``v`` as signed floats.
* Factors (``factors_of``, float64): with ``cpm`` or ``rpgc`` each track takes ``scale_of`` of its own totals; with ``none``
  ``a_t = 1.0`` and ``a_c = reads_t / reads_c`` (both 1.0 when either has no kept read); ``coverage_scale`` then multiplies both.
* Refused (``check_factors``, a ``ValueError``): a factor or, for ``log2`` / ``ratio``, ``p`` below 2^-64 or not finite;
  ``a * max_depth >= 2^40`` for either track; ``p >= 2^40``; for ``ratio`` ``(a_t * max_depth_t + p) / p >= 2^40``.  ``subtract``
  ignores ``p``.
* bedGraph text: a negative ``v`` is ``-`` followed by the text of ``|v|``, unless that is ``0`` (never ``-0``); the track line
  is the signal's (``scale=`` is ``a_t``) followed by `` control=<the control's basename> compare=<op> pseudocount=<repr>``.
  bigWig: the layout and sum orders above; min and max are signed.

Peaks called from the track (``--coverage-call``; ``Signal.call``, ``DeviceCount.call``, ``Peaks``): a threshold
caller over the signal runs, whichever of the above made them.  The definitions are this project's own: nothing here was compared
with MACS2.

* The input is the runs ``(ref, start0, end0, v)`` of a track: within a reference they ascend and do not overlap, and the bases in
  no run are uncovered.  ``cutoff`` is a finite float64 (negative is legal), ``max_gap`` an integer 0 .. 2^31 - 1, ``min_length`` an
  integer 1 .. 2^31 - 1 (``check_call``).  Values compare as floats: ``f64(v)`` against ``cutoff`` and ``f64(v)`` against
  ``f64(v')``; ``-0.0`` equals ``0.0``.
* A run passes when ``f64(v) >= cutoff``; equality passes.
* Take the passing runs of one reference in order.  Two consecutive passing runs ``a``, ``b`` are linked when ``b.start0 - a.end0
  <= max_gap``, whatever lies between them (failing runs or uncovered bases); runs of different references are never linked.  A
  candidate is a maximal chain: ``start`` is its first run's ``start0``, ``end`` its last run's ``end0``.
* A candidate is a peak when ``end - start >= min_length``.  Peaks are in header order, then ascending.
* Per peak: ``value``, the largest ``v`` of its passing runs, float32; ``summit = s + (e - s) // 2``, 0-based, where ``(s, e)`` is
  the first passing run with that value; ``runs``, the number of its passing runs.  Only integers, a maximum and a first-argmax
  appear, so the result does not depend on any order; a mean or an area over a peak would be a float sum and is left out.
* Totals (``CALL_TOTALS``): ``passing_runs``, ``candidates``, ``peaks``, ``peak_bases`` (``end - start`` over the peaks),
  ``passing_bases`` (the widths of the passing runs inside peaks).
* The file is ``<name>_coverage_peaks.narrowPeak``, without a header line, one line per peak: ``chrom``, ``start``, ``end``,
  ``peak_<n>`` (``n`` 1-based in file order), ``score``, ``.``, ``value``, ``-1``, ``-1``, ``summit - start``, TAB-separated.
  ``score = trunc(min(max(f64(value) * 10.0, 0.0), 1000.0))`` (``call_score``); ``value`` is written by ``format_value``.  On a
  p-score track (below) column 8 holds the text of ``value`` as well, in place of ``-1``.

The treatment scored against the control (``--coverage-poisson``; ``Coverage.poisson``, ``DeviceCount.poisson``):
-log10 of a Poisson upper tail per bin against a local lambda, as one signal track.  The definitions are this project's own: nothing
here was compared with MACS2.  Everything is integer arithmetic or float64, each float64 operation rounded to nearest even on its
own (no fused multiply-add).

* Two pileups over the same chosen references (``compare``'s check); ``B`` (1 .. 65536) with the bins, the widths ``w_j`` and the
  sums ``S_t[j]``, ``S_c[j]`` above; reference ``r`` has the bins ``0 .. n_r - 1`` and the length ``len_r``.  ``a_c`` is a float64
  factor checked by ``check_scale`` against the control's ``max_depth``; the treatment is not scaled, because the score counts reads
  (``a_c = factors_of("none", ...)[1]`` scales the control to the treatment's library size).  ``W_s`` and ``W_l`` are two window
  sizes in bases, each 0 (off) .. 2^31 - 1 (``check_lambda_windows``; the defaults are 1000 and 10000).
* ``k[j] = S_t[j] // w_j``, an integer division.
* Window mean, for ``W > 0``: ``h = (W // B) // 2`` bins; ``lo = max(0, j - h)`` and ``hi = min(n_r - 1, j + h)``, inside the bin
  range of ``j``'s own reference (a window never crosses into another reference); ``N = sum S_c[lo .. hi]`` as u64;
  ``D = min(len_r, (hi + 1) * B) - lo * B``; ``c_W = (f64(N) * a_c) / f64(D)``.  ``h = 0`` gives the bin's own value; a window that is
  off contributes nothing.
* Lambda: ``c_0 = (f64(S_c[j]) * a_c) / f64(w_j)``; ``l_bg = (f64(sum of every S_c) * a_c) / f64(sum of the chosen lengths)``;
  ``l[j] = max(l_bg, c_0, c_Ws, c_Wl)`` (``poisson_lambda``).  A control without a covered base is refused, so ``l > 0`` and normal
  everywhere.
* ``ln(x) = lg2(x) * 0.6931471805599453`` with ``lg2`` the stated algorithm above; ``F[0] = F[1] = 0.0``,
  ``F[i] = F[i - 1] + ln(f64(i))``, a sequential sum (``lnfact(n)``), computed here for ``n = max_depth_t + 1`` entries and handed
  to the library as an array.  A ``max_depth_t`` above 2^20 is refused.
* Score (``poisson_values``): if ``f64(k) <= l`` then ``v = 0.0`` -- the bin is not enriched, and equality counts as not enriched.
  Otherwise ``S = 1.0``, ``T = 1.0`` and for ``i = 1, 2, ...``: ``r = l / f64(k + i)``; ``T = T * r``; ``S' = S + T``; stop when
  ``S' == S``, else ``S = S'`` (the ratio is below 1 and falling, so the loop ends).  Then ``A = f64(k) * ln(l)``;
  ``C = (l - A) + F[k]``; ``v = f32(C * 0.4342944819032518 - lg2(S) * 0.3010299956639812)``: -log10 of ``P(X >= k | l)``, with
  ``0 <= v < 2^40``.
* Runs: a bin with ``S_t = 0`` is in no run.  A kept bin begins a run when it is the first bin of its reference, when the bin before
  it is not kept, or when ``k`` or the bits of ``l`` differ from the bin before: the rule is on ``(k, l)``, not on ``v`` and not on
  the width.  Rows are ``(ref, start0, end0, v)`` in header order; the totals are the signal's four.
* The track line is the signal's (``normalize=none scale=1.0``) followed by `` control=<the control's basename>
  poisson=<W_s>,<W_l>`` (``poisson_tail``).

Benjamini-Hochberg q-scores for the p-score track (``--coverage-qvalue``, ``--coverage-call-q``;
``Signal.qvalues``, ``DeviceCount.qvalue``, ``QTable``): the correction over every base of the chosen genome.  The definitions are
this project's own: nothing here was compared with MACS2.  Everything is integer arithmetic or float64, each float64 operation
rounded to nearest even on its own (no fused multiply-add).

* Input: the runs ``(ref, start0, end0, v)`` of a p-score track, ``v`` float32: ``+0.0`` or the float32 of a positive number, so
  ``v >= 0`` and never a NaN.  A track whose smallest value is negative is refused.
* Tests: ``N`` = the sum of the lengths of the chosen references, u64 (the ``L`` of ``l_bg`` above).  Every base of the chosen
  genome is one test; a base in no run has p = 1 and counts in ``N`` only.
* Distinct values: ``u_1 > u_2 > ... > u_m`` are the distinct values of the runs, compared as floats.  ``W_i`` = the sum of
  ``end0 - start0`` over the runs with the value ``u_i``, u64.
* Rank: ``r_1 = 1``, ``r_i = 1 + W_1 + ... + W_(i-1)``, u64.  ``r_i <= N`` always.
* Raw score: ``x_i = f64(u_i) + (lg2(f64(r_i)) - lg2(f64(N))) * 0.3010299956639812`` with ``lg2`` the stated algorithm above.
  ``r_i`` and ``N`` are below 2^53, so the conversions are exact.
* Monotone, clamped: ``Q_i = max(0.0, min(x_1 .. x_i))`` and ``q_i = f32(Q_i)``.  ``min`` and ``max`` are associative and exact
  and the sums are integers, so no result depends on any order.  ``q`` is non-increasing in ``i``, hence non-decreasing in the
  p-score.
* Table: ``m`` rows ``(u_i, W_i, q_i)``, descending in ``u`` (``QTable``).
* Cutoff: ``pcut(X)`` for a finite float64 ``X`` is ``f64(u_i)`` of the largest ``i`` with ``f64(q_i) >= X``, the smallest
  p-score whose q-score reaches ``X``; ``2^40`` when no row reaches ``X`` (``v < 2^40``, so ``call`` then finds nothing);
  ``X <= 0`` gives ``f64(u_m)``.
* Lookup: the q-score of a peak is ``q_i`` of the row with ``u_i == value``.  A peak's value is the value of one of its runs, so
  the row exists: a miss is an internal error, not a ``-1``.  With a table, column 9 of a narrowPeak line is the text of the
  peak's q-score (``format_value``); the coverage file itself stays the p-score track.
"""
from __future__ import annotations

import ctypes
import os
import re
import struct
import zlib
from pathlib import Path
from typing import Dict, Iterator, Tuple

import numpy as np

from .complexity import _selected_mask
from .native import PMX_BAM_DEFAULT_EXCLUDE, SideAccumulator, count_over, load_ingest_library, raise_last

COVERAGE_SUFFIX = "_coverage.bedGraph"
TILE = 4096                 # slots per scan tile of the device code (PMX_COVERAGE_TILE of include/pymasc_amd_ingest.h)
TEXT_CHUNK = 1 << 18        # runs per call of pmx_dbam_coverage_text when a file is written
DEFLATE_CHUNK = 1 << 20     # runs per call of pmx_dbam_coverage_sections_z: 1024 sections of 1024 runs, four workgroups on each of 256 CUs
MAX_READS = 1 << 31
TOTALS = ("reads", "runs", "covered_bases", "fragment_bases", "max_depth")
PAIR = "pair"               # ``extend``: the FR pairs at their own extent
NORMALIZE = ("none", "cpm", "rpgc")
MAX_BIN = 1 << 16           # the widest bin of a signal track
MIN_SCALE, MAX_VALUE = 2.0 ** -64, 2.0 ** 40       # scale >= MIN_SCALE and scale * max_depth < MAX_VALUE
SIGNAL_TOTALS = ("runs", "covered_bases", "min", "max")
COMPARE = ("log2", "ratio", "subtract")     # ``coverage_compare``; an operation's index is its ``op`` of pmx_dbam_coverage_compare
CALL_SUFFIX = "_coverage_peaks.narrowPeak"
CALL_TOTALS = ("passing_runs", "candidates", "peaks", "peak_bases", "passing_bases")
QVALUE_TOTALS = ("rows", "tests", "covered_bases", "positive_bases")
CALL_GAP, CALL_LENGTH = 30, 200             # the defaults of ``coverage_call_gap`` and ``coverage_call_length``
MAX_CALL_INT = (1 << 31) - 1                # the largest ``max_gap`` and ``min_length``
LAMBDA_WINDOWS = (1000, 10000)              # the defaults of ``coverage_lambda``: the small and the large window of the p-score track
MAX_WINDOW = (1 << 31) - 1                  # the largest window
MAX_POISSON_DEPTH = 1 << 20                 # the largest ``max_depth`` of a treatment that is scored
LN_2, LOG10_E, LOG10_2 = 0.6931471805599453, 0.4342944819032518, 0.3010299956639812
_TRACK = re.compile(r'^track type=bedGraph name="(.*)" description="pymasc_amd fragment pileup extend=(\d+|read|pair) reads=(\d+)"$')


def check_extend(extend):
    """``extend`` as the pileup takes it: ``"pair"`` or an integer of at least 0."""
    if extend == PAIR:
        return PAIR
    if isinstance(extend, (str, bool)) or int(extend) != extend or int(extend) < 0:
        raise ValueError("extend is \"pair\" or an integer that is not negative")
    return int(extend)


def check_bin(b) -> int:
    """``coverage_bin`` as the signal takes it: an integer from 1 to 65536."""
    try:
        ok = not isinstance(b, (str, bool)) and int(b) == b and 1 <= int(b) <= MAX_BIN
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("coverage_bin is an integer from 1 to 65536")
    return int(b)


def check_scale(scale, max_depth: int = 0) -> float:
    """The signal's scale factor: a finite float64 of at least 2^-64 with ``scale * max_depth`` below 2^40 (the refusals of
    ``pmx_dbam_coverage_signal``, made here for both paths)."""
    if isinstance(scale, (str, bool)):
        raise ValueError("the scale is a number")
    scale = float(scale)
    if not np.isfinite(scale) or scale < MIN_SCALE:
        raise ValueError("the scale is a finite number of at least 2^-64 (below it a value could be a float32 denormal)")
    if scale * float(int(max_depth)) >= MAX_VALUE:
        raise ValueError("scale * max_depth is 2^40 or more (a value's text is made in 64-bit integers)")
    return scale


def check_factor(scale) -> float:
    """``coverage_scale`` as the run takes it: a finite number above 0 (the final factor is checked by ``check_scale``)."""
    if isinstance(scale, (str, bool)) or not np.isfinite(float(scale)) or float(scale) <= 0.0:
        raise ValueError("coverage_scale is a finite number above 0")
    return float(scale)


def check_genome_size(size, normalize: str = "rpgc"):
    """``coverage_genome_size``: None or a positive integer, and only with ``rpgc``."""
    if size is None:
        return None
    if isinstance(size, (str, bool)) or int(size) != size or int(size) < 1:
        raise ValueError("coverage_genome_size is a positive integer")
    if normalize != "rpgc":
        raise ValueError("coverage_genome_size needs coverage_normalize=\"rpgc\"")
    return int(size)


def check_normalize(normalize) -> str:
    if normalize not in NORMALIZE:
        raise ValueError("coverage_normalize is \"none\", \"cpm\" or \"rpgc\"")
    return normalize


def scale_of(normalize: str, reads: int, fragment_bases: int, lengths, coverage_scale: float = 1.0, genome_size=None) -> float:
    """The final scale factor, float64: ``none``: 1.0; ``cpm``: ``1e6 / reads``; ``rpgc``: ``genome_size / fragment_bases``
    (``genome_size`` None: the sum of the chosen references' ``lengths``); times ``coverage_scale``, one multiplication.  With no
    kept read the normalisation is 1.0 (the track is empty)."""
    check_normalize(normalize)
    genome_size = check_genome_size(genome_size, normalize)
    coverage_scale = check_factor(coverage_scale)
    factor = 1.0
    if normalize == "cpm" and int(reads):
        factor = 1e6 / float(int(reads))
    elif normalize == "rpgc" and int(fragment_bases):
        factor = float(sum(int(l) for l in lengths) if genome_size is None else genome_size) / float(int(fragment_bases))
    return factor * coverage_scale


def format_value(v) -> str:
    """A value as the bedGraph text holds it: the exact value of the float32 rounded to six decimals (ties to even), without
    trailing zeros and without a trailing ``.``.  A negative value is ``-`` followed by the text of ``|v|``, unless that is ``0``
    (never ``-0``)."""
    text = ("%.6f" % abs(float(v))).rstrip("0").rstrip(".")
    return "-" + text if float(v) < 0 and text != "0" else text


def signal_tail(bin: int, normalize: str, scale: float) -> str:
    """What a signal's track line has behind the depth track's."""
    return " bin={} normalize={} scale={!r}".format(int(bin), normalize, float(scale))


def compare_tail(control, op: str, pseudo: float) -> str:
    """What a compared track's line has behind a signal's: the control's basename, the operation and the pseudocount."""
    return " control={} compare={} pseudocount={!r}".format(os.path.basename(os.fspath(control)), check_compare(op), float(pseudo))


def check_compare(op) -> str:
    if op not in COMPARE:
        raise ValueError("coverage_compare is \"log2\", \"ratio\" or \"subtract\"")
    return op


def check_pseudocount(p, op: str = "log2") -> float:
    """``coverage_pseudocount``: for ``log2`` and ``ratio`` a finite number of at least 2^-64 and below 2^40; ``subtract`` ignores
    it (any number)."""
    if isinstance(p, (str, bool)):
        raise ValueError("coverage_pseudocount is a number")
    p = float(p)
    if check_compare(op) == "subtract":
        return p
    if not np.isfinite(p) or p < MIN_SCALE:
        raise ValueError("coverage_pseudocount is a finite number of at least 2^-64")
    if p >= MAX_VALUE:
        raise ValueError("coverage_pseudocount is 2^40 or more")
    return p


def check_factors(op: str, a_t, a_c, pseudo, max_depth_t: int = 0, max_depth_c: int = 0):
    """(a_t, a_c, p) as ``pmx_dbam_coverage_compare`` takes them, its refusals made here for both paths: each factor by
    ``check_scale`` with its own track's ``max_depth``, ``p`` by ``check_pseudocount``, and for ``ratio``
    ``(a_t * max_depth_t + p) / p`` below 2^40."""
    a_t, a_c, p = check_scale(a_t, max_depth_t), check_scale(a_c, max_depth_c), check_pseudocount(pseudo, op)
    if op == "ratio" and (a_t * float(int(max_depth_t)) + p) / p >= MAX_VALUE:
        raise ValueError("(factor * max_depth + pseudocount) / pseudocount is 2^40 or more (a value's text is made in 64-bit integers)")
    return a_t, a_c, p


def factors_of(normalize: str, totals_t, totals_c, lengths, scale: float = 1.0, genome_size=None) -> Tuple[float, float]:
    """(a_t, a_c), float64, from the two pileups' totals by name (``reads``, ``fragment_bases``): with ``cpm`` or ``rpgc`` each
    track takes ``scale_of`` of its own totals; with ``none`` ``a_t = 1.0`` and ``a_c = reads_t / reads_c`` (one division: the
    control is scaled to the treatment's library size), both 1.0 when either file has no kept read; ``scale`` then multiplies
    both."""
    if check_normalize(normalize) != "none":
        return tuple(scale_of(normalize, t["reads"], t["fragment_bases"], lengths, scale, genome_size) for t in (totals_t, totals_c))
    check_genome_size(genome_size, normalize)
    scale = check_factor(scale)
    rt, rc = int(totals_t["reads"]), int(totals_c["reads"])
    a_c = float(rt) / float(rc) if rt and rc else 1.0
    return 1.0 * scale, a_c * scale


_LG2_C = [1.0 / (2 * k + 1) for k in range(11)]


def lg2(x):
    """The base-2 logarithm of positive normal float64 values as the compared track states it, in numpy: every
    operation is one float64 operation rounded on its own, so the device, this and the tests' restatement agree to the bit.
    ``(m, e) = frexp(x)``; ``m < 0.7071067811865476``: ``m = 2 m, e = e - 1``; ``f = m - 1``; ``s = f / (2 + f)``; ``z = s * s``;
    ``P = c_10``, ``P = P * z + c_k`` for ``k = 9 .. 0`` with ``c_k = 1 / (2 k + 1)``; ``lg2 = e + ((2 s) * P) * 1.4426950408889634``."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    low = m < 0.7071067811865476
    m = np.where(low, 2.0 * m, m)
    e = np.where(low, e - 1, e)
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    P = np.full_like(z, _LG2_C[10])
    for k in range(9, -1, -1):
        P = P * z
        P = P + _LG2_C[k]
    ln = (2.0 * s) * P
    return e.astype(np.float64) + ln * 1.4426950408889634


def compare_values(S_t, S_c, w, op: str, a_t: float, a_c: float, pseudo: float) -> np.ndarray:
    """``v`` (float32) of bins with the sums ``S_t``, ``S_c`` and the widths ``w``, in the stated order of operations."""
    w = np.asarray(w, dtype=np.float64)
    t = (np.asarray(S_t, dtype=np.float64) * a_t) / w
    c = (np.asarray(S_c, dtype=np.float64) * a_c) / w
    if op == "subtract":
        return (t - c).astype(np.float32)
    x = (t + pseudo) / (c + pseudo)
    return (x if op == "ratio" else lg2(x)).astype(np.float32)


def check_lambda_windows(windows=LAMBDA_WINDOWS) -> Tuple[int, int]:
    """``coverage_lambda`` as the p-score track takes it: (small, large), two integers from 0 (off) to 2^31 - 1."""
    try:
        small, large = windows
        ok = all(not isinstance(x, (str, bool)) and int(x) == x and 0 <= int(x) <= MAX_WINDOW for x in (small, large))
    except (TypeError, ValueError, OverflowError):
        ok = False
    if not ok:
        raise ValueError("coverage_lambda is two integers, each from 0 (off) to 2^31 - 1")
    return int(small), int(large)


def poisson_tail(control, small: int, large: int) -> str:
    """What a p-score track's line has behind a signal's: the control's basename and the two windows."""
    small, large = check_lambda_windows((small, large))
    return " control={} poisson={},{}".format(os.path.basename(os.fspath(control)), small, large)


def lnfact(n) -> np.ndarray:
    """``F[0 .. n - 1]``, float64, of the p-score track: ``F[0] = F[1] = 0.0``, ``F[i] = F[i - 1] + ln(f64(i))``
    with ``ln(x) = lg2(x) * 0.6931471805599453``, a sequential sum (``np.cumsum`` adds one element after the other).  ``n`` is
    ``max_depth + 1`` of the treatment: 1 to 2^20 + 1."""
    if isinstance(n, (str, bool)) or int(n) != n or not 1 <= int(n) <= MAX_POISSON_DEPTH + 1:
        raise ValueError("the table of ln(i!) has 1 to 2^20 + 1 entries (the treatment's max_depth is at most 2^20)")
    terms = np.zeros(int(n), dtype=np.float64)
    if n > 2:
        terms[2:] = lg2(np.arange(2, int(n), dtype=np.float64)) * LN_2
    return np.cumsum(terms)


def poisson_series(k, lam) -> Tuple[np.ndarray, np.ndarray]:
    """(S, steps) of the series of pairs with ``f64(k) > lam``: ``S = T = 1.0``; for ``i = 1, 2, ...``: ``T = T * (lam / f64(k + i))``,
    ``S' = S + T``, stop when ``S' == S``, else ``S = S'``.  A masked loop: the pairs that have stopped are left out."""
    k, lam = np.asarray(k, dtype=np.int64).ravel(), np.asarray(lam, dtype=np.float64).ravel()
    S, T, steps = np.ones(k.size, dtype=np.float64), np.ones(k.size, dtype=np.float64), np.zeros(k.size, dtype=np.int64)
    live, i = np.arange(k.size), 0
    while live.size:
        i += 1
        T[live] = T[live] * (lam[live] / (k[live] + i).astype(np.float64))
        S2 = S[live] + T[live]
        go = S2 > S[live]                                   # (T >= 0: S' >= S, so this is S' != S)
        steps[live] = i
        S[live[go]] = S2[go]
        live = live[go]
    return S, steps


def poisson_values(k, lam, F) -> np.ndarray:
    """``v`` (float32) of pairs ``(k, lam)`` with the table ``F`` (``lnfact``; ``F[k]`` exists for every ``k``), in the stated order
    of operations: 0.0 where ``f64(k) <= lam``; elsewhere ``f32(((lam - f64(k) * ln(lam)) + F[k]) * 0.4342944819032518 - lg2(S) *
    0.3010299956639812)`` with ``S`` of ``poisson_series``."""
    k, lam = np.asarray(k, dtype=np.int64).ravel(), np.asarray(lam, dtype=np.float64).ravel()
    F = np.asarray(F, dtype=np.float64)
    out = np.zeros(k.size, dtype=np.float32)
    at = np.flatnonzero(k.astype(np.float64) > lam)
    if at.size:
        kk, ll = k[at], lam[at]
        S, _steps = poisson_series(kk, ll)
        A = kk.astype(np.float64) * (lg2(ll) * LN_2)
        C = (ll - A) + F[kk]
        out[at] = (C * LOG10_E - lg2(S) * LOG10_2).astype(np.float32)
    return out


def poisson_lambda(S_c, width, bin: int, length: int, a_c: float, lam_bg: float, small: int, large: int) -> np.ndarray:
    """``l[j]`` (float64) of the bins of one reference of ``length`` bases from the control's sums ``S_c`` and the widths: the
    largest of ``lam_bg``, ``c_0`` and the means over the windows that are on, each ``(f64(N) * a_c) / f64(D)``."""
    S_c, width = np.asarray(S_c, dtype=np.int64), np.asarray(width, dtype=np.int64)
    n = S_c.size
    P = np.concatenate(([0], np.cumsum(S_c, dtype=np.int64)))      # P[i]: the sum of the bins in front of i
    lam = np.maximum(lam_bg, (S_c.astype(np.float64) * a_c) / width.astype(np.float64))
    j = np.arange(n, dtype=np.int64)
    for W in (small, large):
        if W:
            h = (int(W) // int(bin)) // 2
            lo, hi = np.maximum(j - h, 0), np.minimum(j + h, n - 1)
            N = P[hi + 1] - P[lo]
            D = np.minimum(int(length), (hi + 1) * int(bin)) - lo * int(bin)
            lam = np.maximum(lam, (N.astype(np.float64) * a_c) / D.astype(np.float64))
    return lam


def check_poisson(a_c, small, large, max_depth_t: int, max_depth_c: int, control_bases: int):
    """(a_c, small, large) as ``pmx_dbam_coverage_poisson`` takes them, its refusals made here for both paths: the windows by
    ``check_lambda_windows``, a treatment's ``max_depth`` above 2^20, ``a_c`` by ``check_scale`` with the control's ``max_depth``,
    a control without a covered base."""
    small, large = check_lambda_windows((small, large))
    if int(max_depth_t) > MAX_POISSON_DEPTH:
        raise ValueError("the treatment's max_depth is above 2^20")
    a_c = check_scale(a_c, max_depth_c)
    if not int(control_bases):
        raise ValueError("the control has no covered base: there is no background to score against")
    return a_c, small, large


def check_call(cutoff, max_gap=30, min_length=200) -> Tuple[float, int, int]:
    """(cutoff, max_gap, min_length) as the peak caller takes them (the refusals of ``pmx_dbam_coverage_call``, made here for both
    paths): a finite number (negative is legal), an integer from 0 to 2^31 - 1, an integer from 1 to 2^31 - 1."""
    if isinstance(cutoff, (str, bool)) or cutoff is None:
        raise ValueError("coverage_call (the cutoff) is a number")
    try:
        cutoff = float(cutoff)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("coverage_call (the cutoff) is a number") from None
    if not np.isfinite(cutoff):
        raise ValueError("coverage_call (the cutoff) is a finite number")
    for what, x, low in (("coverage_call_gap", max_gap, 0), ("coverage_call_length", min_length, 1)):
        try:
            ok = not isinstance(x, (str, bool)) and int(x) == x and low <= int(x) <= MAX_CALL_INT
        except (TypeError, ValueError, OverflowError):
            ok = False
        if not ok:
            raise ValueError("{} is an integer from {} to 2^31 - 1".format(what, low))
    return cutoff, int(max_gap), int(min_length)


def call_score(value) -> np.ndarray:
    """The narrowPeak score of float32 values: ``trunc(min(max(f64(value) * 10.0, 0.0), 1000.0))``, int64."""
    x = np.asarray(value, dtype=np.float32).astype(np.float64) * 10.0
    return np.trunc(np.minimum(np.maximum(x, 0.0), 1000.0)).astype(np.int64)


def check_q(x, what: str = "coverage_call_q") -> float:
    """``X`` of ``pcut(X)``: a finite number."""
    if isinstance(x, (str, bool)) or x is None:
        raise ValueError("{} is a number".format(what))
    try:
        x = float(x)
    except (TypeError, ValueError, OverflowError):
        raise ValueError("{} is a number".format(what)) from None
    if not np.isfinite(x):
        raise ValueError("{} is a finite number".format(what))
    return x


class QTable:
    """The q-scores of a p-score track: ``p`` the distinct values ``u_i`` (float32, descending), ``bases`` their
    covered bases ``W_i`` (uint64), ``q`` their q-scores (float32, non-increasing), ``tests`` the number ``N`` of tests.  Two are
    equal when their columns are, bit for bit, with ``tests``."""

    def __init__(self, p, bases, q, tests: int):
        self.p = np.asarray(p, dtype=np.float32).ravel()
        self.bases = np.asarray(bases, dtype=np.uint64).ravel()
        self.q = np.asarray(q, dtype=np.float32).ravel()
        self.tests = int(tests)
        if not (self.p.size == self.bases.size == self.q.size):
            raise ValueError("the three columns have one length")
        if self.p.size and (self.p.min() < 0 or np.any(np.diff(self.p.view(np.uint32).astype(np.int64)) >= 0)):
            raise ValueError("the values are not negative and descend")

    @property
    def totals(self):
        """(rows, tests, covered bases, bases with q > 0), the order of ``pmx_dbam_coverage_qvalue``."""
        return int(self.p.size), self.tests, int(self.bases.sum(dtype=np.uint64)), int(self.bases[self.q > 0].sum(dtype=np.uint64))

    def lookup(self, values) -> np.ndarray:
        """``q_i`` (float32) of the rows with ``u_i == value``; a value without a row is an internal error."""
        bits = np.asarray(values, dtype=np.float32).ravel().view(np.uint32)
        asc = self.p.view(np.uint32)[::-1]                      # (v >= +0.0: the bits order as the floats do)
        at = np.searchsorted(asc, bits)
        if bits.size and (np.any(at >= asc.size) or np.any(asc[np.minimum(at, max(asc.size - 1, 0))] != bits)):
            raise RuntimeError("a value has no row in the q-score table")
        return self.q[::-1][at] if bits.size else np.zeros(0, dtype=np.float32)

    def cutoff(self, X) -> float:
        """``pcut(X)``: the smallest p-score whose q-score reaches ``X``, ``2^40`` when none does."""
        X = check_q(X, "X")
        n = int(np.count_nonzero(self.q.astype(np.float64) >= X))       # (q is non-increasing: the rows that reach X are the first n)
        return float(self.p[n - 1]) if n else MAX_VALUE

    def __eq__(self, other) -> bool:
        return (isinstance(other, QTable) and self.tests == other.tests and self.p.size == other.p.size
                and np.array_equal(self.p.view(np.uint32), other.p.view(np.uint32)) and np.array_equal(self.bases, other.bases)
                and np.array_equal(self.q.view(np.uint32), other.q.view(np.uint32)))

    __hash__ = None

    def __repr__(self) -> str:
        return "QTable(rows={}, tests={}, covered_bases={}, positive_bases={})".format(*self.totals)


class Peaks:
    """The peaks called from a signal track: ``rows``: ``{name: (start, end, summit, value, runs)}`` (uint32,
    uint32, uint32, float32, uint32) of the references that have a peak, in header order; ``cutoff``, ``max_gap``, ``min_length``;
    ``totals``: by name (``CALL_TOTALS``).  Two are equal when their rows are, bit for bit, with the three parameters, the
    totals and the q-score table."""

    def __init__(self, rows, cutoff: float, max_gap: int, min_length: int, totals, pscore: bool = False, qtable=None):
        """``pscore``: the track is a p-score track: column 8 of a line holds the value's text, not ``-1``.
        ``qtable``: its ``QTable`` (7.18.7): column 9 holds the text of the peak's q-score, not ``-1``."""
        if qtable is not None and not (isinstance(qtable, QTable) and pscore):
            raise ValueError("qtable is the QTable of a p-score track")
        self.qtable = qtable
        self.pscore = bool(pscore)
        types = (np.uint32, np.uint32, np.uint32, np.float32, np.uint32)
        self.rows = {str(k): tuple(np.asarray(x, dtype=t).ravel() for x, t in zip(v, types)) for k, v in rows.items()}
        self.cutoff, self.max_gap, self.min_length = check_call(cutoff, max_gap, min_length)
        self.totals = {k: int(totals[k]) for k in CALL_TOTALS}
        if any(len(v) != 5 or not (v[0].size == v[1].size == v[2].size == v[3].size == v[4].size > 0) for v in self.rows.values()):
            raise ValueError("every reference has five columns of one length, and at least one peak")

    n_peaks = property(lambda self: sum(int(v[0].size) for v in self.rows.values()))
    peak_bases = property(lambda self: sum(int((e.astype(np.int64) - s.astype(np.int64)).sum()) for s, e, *_x in self.rows.values()))

    def lines(self):
        """``{name: [(start, end), ...]}`` of the peaks, in file order: what ``peaks.open_peaks`` takes."""
        return {n: list(zip(v[0].tolist(), v[1].tolist())) for n, v in self.rows.items()}

    def text_chunks(self, chunk: int = 1 << 16) -> Iterator[bytes]:
        """The narrowPeak lines, ``chunk`` peaks at a time; the peak numbers run through the file."""
        no = 0
        for name, (s, e, m, v, _r) in self.rows.items():
            for a in range(0, s.size, chunk):
                z = slice(a, a + chunk)
                q9 = ["-1"] * int(v[z].size) if self.qtable is None else [format_value(x) for x in self.qtable.lookup(v[z])]
                yield "".join("{}\t{}\t{}\tpeak_{}\t{}\t.\t{}\t{}\t{}\t{}\n".format(name, x, y, no + a + i + 1, sc, format_value(val),
                                                                                 format_value(val) if self.pscore else "-1", q, c - x)
                               for i, (x, y, c, val, sc, q) in enumerate(zip(s[z].tolist(), e[z].tolist(), m[z].tolist(), v[z],
                                                                             call_score(v[z]).tolist(), q9))).encode()
            no += s.size

    def __eq__(self, other) -> bool:
        return (isinstance(other, Peaks) and (self.cutoff, self.max_gap, self.min_length, self.pscore) == (other.cutoff, other.max_gap,
                                                                                                            other.min_length, other.pscore)
                and self.totals == other.totals and list(self.rows) == list(other.rows)
                and (self.qtable is None) == (other.qtable is None) and (self.qtable is None or self.qtable == other.qtable)
                and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for k in self.rows for a, b in zip(self.rows[k], other.rows[k])))

    __hash__ = None

    def __repr__(self) -> str:
        return "Peaks(cutoff={!r}, max_gap={}, min_length={}, {})".format(self.cutoff, self.max_gap, self.min_length,
                                                                          ", ".join("{}={}".format(k, v) for k, v in self.totals.items()))


class Signal:
    """A signal track: ``runs``: ``{name: (start0, end0, value)}`` (uint32, uint32, float32) of the chosen references that have a
    run, in header order; ``bin``, ``scale``; ``refs`` as for ``Coverage``; ``reads``, ``extend`` and ``normalize`` (the word) are
    what the track line says.  Two signals are equal when their runs are, bit for bit, with ``bin`` and ``scale``."""

    def __init__(self, runs, bin: int, scale: float, refs=None, reads: int = 0, extend=0, normalize: str = "none", more: str = "",
                 pscore: bool = False):
        """``more``: what the track line says behind a signal's (``compare_tail`` of a compared track); ``pscore``: the values are
        p-scores (``Coverage.poisson``), which ``call`` hands on to its ``Peaks``."""
        self.more, self.pscore = str(more), bool(pscore)
        self.runs = {str(k): (np.asarray(v[0], dtype=np.uint32).ravel(), np.asarray(v[1], dtype=np.uint32).ravel(),
                              np.asarray(v[2], dtype=np.float32).ravel()) for k, v in runs.items()}
        self.bin, self.scale = check_bin(bin), float(scale)
        self.refs = None if refs is None else [(str(n), int(l)) for n, l in refs]
        self.reads, self.extend, self.normalize = int(reads), check_extend(extend), check_normalize(normalize)
        if any(not (v[0].size == v[1].size == v[2].size > 0) for v in self.runs.values()):
            raise ValueError("every reference has as many starts as ends and values, and at least one run")

    n_runs = property(lambda self: sum(int(v[0].size) for v in self.runs.values()))
    covered_bases = property(lambda self: sum(int((e.astype(np.int64) - s.astype(np.int64)).sum()) for s, e, _v in self.runs.values()))
    min = property(lambda self: min((float(v.min()) for _s, _e, v in self.runs.values()), default=0.0))
    max = property(lambda self: max((float(v.max()) for _s, _e, v in self.runs.values()), default=0.0))

    @property
    def totals(self):
        """(runs, covered_bases, the smallest value, the largest value), the order of ``pmx_dbam_coverage_signal``."""
        return self.n_runs, self.covered_bases, self.min, self.max

    def rows(self):
        """Every run as a plain tuple (name, start0, end0, value), in file order."""
        return [(n, *r) for n, v in self.runs.items() for r in zip(*(x.tolist() for x in v))]

    def text_chunks(self, chunk: int = 1 << 16) -> Iterator[bytes]:
        """The bedGraph lines, ``chunk`` runs at a time."""
        for name, (s, e, v) in self.runs.items():
            for a in range(0, s.size, chunk):
                yield "".join("{}\t{}\t{}\t{}\n".format(name, x, y, format_value(z))
                               for x, y, z in zip(s[a:a + chunk].tolist(), e[a:a + chunk].tolist(), v[a:a + chunk])).encode()

    tail = property(lambda self: signal_tail(self.bin, self.normalize, self.scale) + self.more)

    def qvalues(self) -> QTable:
        """The q-scores of a p-score track, in numpy: the path of host readers and the checker of
        ``pmx_dbam_coverage_qvalue``.  ``N`` is the sum of ``refs``' lengths; the distinct values descend, ``W`` their covered
        bases, ``r = 1 +`` the bases in front, ``x = f64(u) + (lg2(f64(r)) - lg2(f64(N))) * 0.3010299956639812``,
        ``q = f32(max(0.0, the running minimum of x))``."""
        if not self.pscore:
            raise ValueError("the track is not a p-score track (Coverage.poisson makes one)")
        if self.refs is None:
            raise ValueError("the track does not know its chosen references' lengths: the number of tests is their sum")
        tests = sum(l for _n, l in self.refs)
        if not self.runs:
            return QTable([], [], [], tests)
        v = np.concatenate([x for _s, _e, x in self.runs.values()])
        w = np.concatenate([e.astype(np.uint64) - s.astype(np.uint64) for s, e, _x in self.runs.values()])
        if v.min() < 0:
            raise ValueError("the smallest value of the track is negative: not a p-score")
        bits = v.view(np.uint32)
        order = np.argsort(bits, kind="stable")[::-1]           # (v >= +0.0: the bits order as the floats do)
        sb, sw = bits[order], w[order]
        heads = np.flatnonzero(np.concatenate(([True], sb[1:] != sb[:-1])))
        u, W = sb[heads].view(np.float32), np.add.reduceat(sw, heads)
        r = np.uint64(1) + np.concatenate((np.zeros(1, dtype=np.uint64), np.cumsum(W, dtype=np.uint64)[:-1]))
        d = lg2(r.astype(np.float64)) - lg2(np.full(1, tests, dtype=np.float64))[0]
        x = u.astype(np.float64) + d * LOG10_2
        mn = np.minimum.accumulate(x)
        return QTable(u, W, np.where(mn > 0.0, mn, 0.0).astype(np.float32), tests)

    def call(self, cutoff, max_gap: int = CALL_GAP, min_length: int = CALL_LENGTH, qtable=None) -> Peaks:
        """The peaks of the track, in numpy: the path of host readers and the checker of
        ``pmx_dbam_coverage_call``.  A run passes when ``f64(v) >= cutoff``; consecutive passing runs of a reference are linked
        when the second begins at most ``max_gap`` bases behind the first's end; a maximal chain of at least ``min_length`` bases
        from its first start to its last end is a peak, with the largest ``v`` of its passing runs, the middle ``s + (e - s) // 2``
        of the first run that has it, and the number of its passing runs.  ``qtable``: the track's ``QTable``, handed on to
        the ``Peaks`` for column 9."""
        cutoff, max_gap, min_length = check_call(cutoff, max_gap, min_length)
        rows, tot = {}, dict.fromkeys(CALL_TOTALS, 0)
        for name, (s, e, v) in self.runs.items():
            at = np.flatnonzero(v.astype(np.float64) >= cutoff)
            if not at.size:
                continue
            ps, pe, pv = s[at].astype(np.int64), e[at].astype(np.int64), v[at]
            begins = np.ones(at.size, dtype=bool)
            begins[1:] = ps[1:] - pe[:-1] > max_gap
            first = np.flatnonzero(begins)
            count = np.diff(np.append(first, at.size))
            start, end = ps[first], pe[first + count - 1]
            tot["passing_runs"] += int(at.size)
            tot["candidates"] += int(first.size)
            keep = end - start >= min_length
            if not keep.any():
                continue
            f64 = pv.astype(np.float64)
            top = np.repeat(np.maximum.reduceat(f64, first), count)
            hit = np.flatnonzero(f64 == top)                     # (-0.0 == 0.0; every chain has one)
            chain = np.repeat(np.arange(first.size), count)
            _c, where = np.unique(chain[hit], return_index=True)    # the first hit of every chain
            arg = hit[where][keep]
            rows[name] = (start[keep], end[keep], ps[arg] + (pe[arg] - ps[arg]) // 2, pv[arg], count[keep])
            tot["peaks"] += int(keep.sum())
            tot["peak_bases"] += int((end - start)[keep].sum())
            tot["passing_bases"] += int(np.add.reduceat(pe - ps, first)[keep].sum())
        return Peaks(rows, cutoff, max_gap, min_length, tot, self.pscore, qtable)

    def __eq__(self, other) -> bool:
        return (isinstance(other, Signal) and (self.bin, self.scale, self.pscore) == (other.bin, other.scale, other.pscore)
                and list(self.runs) == list(other.runs)
                and all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for k in self.runs for a, b in zip(self.runs[k], other.runs[k])))

    __hash__ = None

    def __repr__(self) -> str:
        return "Signal(bin={}, scale={!r}, runs={}, covered_bases={}, min={!r}, max={!r})".format(self.bin, self.scale, *self.totals)


def _same_refs(mine, theirs) -> None:
    """Both pileups of a compared or scored track know their chosen references, and they are the same."""
    if mine is None or theirs is None:
        raise ValueError("a pileup does not know its chosen references' lengths (it was read from a bedGraph file)")
    if mine != theirs:
        raise ValueError("the chosen references of the control differ in name, length or order")


def _entries(begins, keep_of, bin: int, length: int):
    """(at, ends) of the kept entries of a reference: the bins where ``begins`` is set begin an entry, which ends where the next one
    begins, the last at ``length``; ``keep_of(at)``: which of them are kept."""
    at = np.flatnonzero(begins)
    ends = np.append(at[1:] * bin, length)
    keep = keep_of(at)
    return at[keep], ends[keep]


def _by_reference(names, ref, *cols):
    """``{name: columns}`` of rows given as columns: split where the reference column ``ref`` (ids into ``names``) changes."""
    cut = np.flatnonzero(np.diff(ref)) + 1 if ref.size else np.zeros(0, dtype=np.int64)
    edges = np.concatenate(([0], cut, [ref.size])).astype(np.int64) if ref.size else np.zeros(1, dtype=np.int64)
    return {names[int(ref[a])]: tuple(x[a:z] for x in cols) for a, z in zip(edges[:-1], edges[1:])}


def _pull(reader, fn, head, rest_none=(), rest_of=lambda size: (), bound: bool = False) -> bytes:
    """The bytes of an entry point that is called twice: ``fn(handle, *head, None, 0, *rest_none)`` gives their number,
    ``fn(handle, *head, buffer, size, *rest_of(size))`` fills a buffer of it.  ``bound``: the number is an upper bound (a compressed
    pull), and the second call says how many bytes it wrote."""
    size = fn(reader._h, *head, None, 0, *rest_none)
    if size < 0:
        reader._raise(size)
    buf = np.zeros(max(int(size), 1), dtype=np.uint8)
    got = fn(reader._h, *head, buf.ctypes.data, int(size), *rest_of(int(size)))
    if got < 0:
        reader._raise(got)
    assert got <= size if bound else got == size
    return buf[:int(got)].tobytes()


class Coverage:
    """``runs``: ``{name: (start0, end0, depth)}``, uint32, of the chosen references that have a run, in header order;
    ``reads``: the reads that added; ``extend`` (0: every read's own length; ``"pair"``: the FR pairs at their own extent)."""

    def __init__(self, runs, reads: int, extend: int, refs=None):
        """``refs``: the chosen references as ``[(name, length), ...]`` in header order, where they are known (a count knows them, a
        bedGraph file does not); ``write_bigwig`` needs them, and two pileups compare equal without them."""
        self.runs = {str(k): tuple(np.asarray(x, dtype=np.uint32).ravel() for x in v) for k, v in runs.items()}
        self.reads, self.extend = int(reads), check_extend(extend)
        self.refs = None if refs is None else [(str(n), int(l)) for n, l in refs]
        if any(len(v) != 3 or not (v[0].size == v[1].size == v[2].size > 0) for v in self.runs.values()):
            raise ValueError("every reference has as many starts as ends and depths, and at least one run")

    n_runs = property(lambda self: sum(int(v[0].size) for v in self.runs.values()))
    covered_bases = property(lambda self: sum(int((e.astype(np.int64) - s.astype(np.int64)).sum()) for s, e, _d in self.runs.values()))
    fragment_bases = property(lambda self: sum(int(((e.astype(np.int64) - s.astype(np.int64)) * d.astype(np.int64)).sum())
                                               for s, e, d in self.runs.values()))
    max_depth = property(lambda self: max((int(d.max()) for _s, _e, d in self.runs.values()), default=0))

    @property
    def totals(self) -> Tuple[int, int, int, int, int]:
        """(reads, runs, covered_bases, fragment_bases, max_depth), the order of ``pmx_dbam_coverage_finish``."""
        return self.reads, self.n_runs, self.covered_bases, self.fragment_bases, self.max_depth

    def rows(self):
        """Every run as a plain tuple (name, start0, end0, depth), in file order."""
        return [(n, *r) for n, v in self.runs.items() for r in zip(*(x.tolist() for x in v))]

    def text_chunks(self, chunk: int = 1 << 16) -> Iterator[bytes]:
        """The bedGraph lines, formatted with numpy, ``chunk`` runs at a time."""
        for name, (s, e, d) in self.runs.items():
            head = name + "\t"
            for a in range(0, s.size, chunk):
                cols = [x[a:a + chunk].astype("U10") for x in (s, e, d)]
                lines = np.char.add(np.char.add(np.char.add(np.char.add(np.char.add(head, cols[0]), "\t"), cols[1]), "\t"), cols[2])
                yield ("\n".join(lines.tolist()) + "\n").encode()

    def signal(self, bin: int = 1, scale: float = 1.0, normalize: str = "none") -> Signal:
        """The signal track of the pileup, in numpy: the runs are split at the bin edges and their ``overlap * depth`` added per
        bin (``np.add.at``); a bin begins a run where ``S`` or the width differs from the bin before.  ``bin`` above 1 needs
        ``refs`` (the last bin of a reference is clipped to its length).  ``normalize``: the word the track line says."""
        bin, scale = check_bin(bin), check_scale(scale, self.max_depth)
        if bin > 1 and self.refs is None:
            raise ValueError("the pileup does not know its chosen references' lengths (it was read from a bedGraph file)")
        lengths = dict(self.refs or [])
        out = {}
        for name, (s, e, d) in self.runs.items():
            if bin == 1:
                out[name] = (s, e, ((d.astype(np.float64) * scale) / 1.0).astype(np.float32))
                continue
            length = lengths[name]
            total, width = self._bin_sums(name, bin, length)
            begins = np.ones(total.size, dtype=bool)
            begins[1:] = (total[1:] != total[:-1]) | (width[1:] != width[:-1])
            at, ends = _entries(begins, lambda at: total[at] != 0, bin, length)
            if at.size:
                out[name] = (at * bin, ends, ((total[at].astype(np.float64) * scale) / width[at].astype(np.float64)).astype(np.float32))
        return Signal(out, bin, scale, self.refs, self.reads, self.extend, normalize)

    def _bin_sums(self, name: str, bin: int, length: int):
        """(S, width) of every bin of ``bin`` bases of the reference ``name`` of ``length`` bases, int64: the runs are split at the
        bin edges and their ``overlap * depth`` added per bin."""
        total = np.zeros(-(-length // bin), dtype=np.int64)
        width = np.full(total.size, bin, dtype=np.int64)
        if total.size:
            width[-1] = length - (total.size - 1) * bin
        if name in self.runs:
            s, e, d = (x.astype(np.int64) for x in self.runs[name])
            j0, j1 = s // bin, (e - 1) // bin
            n = j1 - j0 + 1                                 # the bins of every run
            run = np.repeat(np.arange(s.size), n)
            j = j0[run] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
            w = np.minimum(e[run], (j + 1) * bin) - np.maximum(s[run], j * bin)
            np.add.at(total, j, w * d[run])
        return total, width

    def compare(self, other: "Coverage", bin: int = 1, op: str = "log2", a_t: float = 1.0, a_c: float = 1.0, pseudo: float = 1.0,
                normalize: str = "none", control="") -> Signal:
        """This pileup (the treatment) against ``other`` (the control) as one signal track, in numpy: the path of
        host readers and the checker of ``pmx_dbam_coverage_compare``.  Both know the same chosen references.  Per bin ``t = (S_t *
        a_t) / w``, ``c = (S_c * a_c) / w`` and ``v`` by ``op`` (``compare_values``); a bin begins a run where ``S_t``, ``S_c`` or
        the width differs from the bin before; the bins with both sums 0 are in no run.  The result's ``scale`` is ``a_t``;
        ``normalize`` and ``control`` are what the track line says."""
        bin = check_bin(bin)
        a_t, a_c, pseudo = check_factors(op, a_t, a_c, pseudo, self.max_depth, other.max_depth)
        _same_refs(self.refs, other.refs)
        out = {}
        for name, length in self.refs:
            if name not in self.runs and name not in other.runs:
                continue
            St, width = self._bin_sums(name, bin, length)
            Sc, _w = other._bin_sums(name, bin, length)
            begins = np.ones(St.size, dtype=bool)
            begins[1:] = (St[1:] != St[:-1]) | (Sc[1:] != Sc[:-1]) | (width[1:] != width[:-1])
            at, ends = _entries(begins, lambda at: (St[at] != 0) | (Sc[at] != 0), bin, length)
            if at.size:
                out[name] = (at * bin, ends, compare_values(St[at], Sc[at], width[at], op, a_t, a_c, pseudo))
        return Signal(out, bin, a_t, self.refs, self.reads, self.extend, normalize, compare_tail(control, op, pseudo))

    def poisson(self, other: "Coverage", bin: int = 1, a_c: float = 1.0, small: int = LAMBDA_WINDOWS[0], large: int = LAMBDA_WINDOWS[1],
                control="") -> Signal:
        """This pileup (the treatment) scored against ``other`` (the control) as one signal track of p-scores,
        in numpy: the path of host readers and the checker of ``pmx_dbam_coverage_poisson``.  Per bin ``k = S_t // w`` and ``l``
        (``poisson_lambda``); a bin with ``S_t = 0`` is in no run, a kept bin begins a run where its reference begins, where the
        bin before is not kept or where ``k`` or the bits of ``l`` differ from it; ``v`` by ``poisson_values``.  The result's
        ``scale`` is 1.0 (the treatment is not scaled) and its ``pscore`` is set; ``control`` is what the track line says."""
        bin = check_bin(bin)
        a_c, small, large = check_poisson(a_c, small, large, self.max_depth, other.max_depth, other.fragment_bases)
        _same_refs(self.refs, other.refs)
        F = lnfact(self.max_depth + 1)
        out = {name: (start, end, poisson_values(k, lam, F)) for name, start, end, k, lam in self.poisson_pairs(other, bin, a_c, small, large)}
        return Signal(out, bin, 1.0, self.refs, self.reads, self.extend, "none", poisson_tail(control, small, large), True)

    def poisson_pairs(self, other: "Coverage", bin: int, a_c: float, small: int, large: int):
        """(name, start0, end0, k, l) of the runs of ``poisson``, reference by reference: the pairs ``poisson_values`` scores."""
        lam_bg = (float(other.fragment_bases) * a_c) / float(sum(l for _n, l in self.refs))
        for name, length in self.refs:
            if name not in self.runs:
                continue
            St, width = self._bin_sums(name, bin, length)
            Sc, _w = other._bin_sums(name, bin, length)
            k, lam = St // width, poisson_lambda(Sc, width, bin, length, a_c, lam_bg, small, large)
            kept, bits = St != 0, lam.view(np.uint64)
            begins = np.ones(St.size, dtype=bool)
            begins[1:] = (kept[1:] != kept[:-1]) | (kept[1:] & ((k[1:] != k[:-1]) | (bits[1:] != bits[:-1])))
            at, ends = _entries(begins, lambda at: kept[at], bin, length)
            if at.size:
                yield name, at * bin, ends, k[at], lam[at]

    def call(self, cutoff, max_gap: int = CALL_GAP, min_length: int = CALL_LENGTH) -> Peaks:
        """The peaks of the depth track: ``Signal.call`` of the signal at bin 1 and scale 1.0."""
        return self.signal(1, 1.0).call(cutoff, max_gap, min_length)

    def __eq__(self, other) -> bool:
        return (isinstance(other, Coverage) and (self.reads, self.extend) == (other.reads, other.extend)
                and list(self.runs) == list(other.runs)
                and all(np.array_equal(a, b) for k in self.runs for a, b in zip(self.runs[k], other.runs[k])))

    __hash__ = None

    def __repr__(self) -> str:
        return "Coverage(extend={}, reads={}, runs={}, covered_bases={}, fragment_bases={}, max_depth={})".format(self.extend, *self.totals)


class HostCount:
    """The host checker, plain numpy, and the path of host readers: a difference array per chosen reference that has a read (one
    slot per base and a closing one); ``add`` marks a batch of reads given as four columns with ``np.add.at``, ``result`` takes the running sum and
    cuts it into runs where a slot is not 0."""

    def __init__(self, names, lengths, use, extend=0):
        """``extend`` ``"pair"``: ``add`` is given the FR rows of ``fragments.rows_host`` as forward reads of ``size`` bases."""
        self.label = check_extend(extend)
        extend = 0 if self.label == PAIR else self.label
        self.names, self.lengths = tuple(names), tuple(max(int(x), 0) for x in lengths)
        self.use = np.asarray(use, dtype=bool)
        if not self.use.any():
            raise ValueError("no chosen reference")
        self.extend, self.reads = int(extend), 0
        self.steps = {r: None for r in range(len(self.names)) if self.use[r]}      # (allocated with the reference's first read)

    def add(self, ref_id, pos1, read_len, reverse) -> int:
        ref = np.asarray(ref_id, dtype=np.int64).ravel()
        pos = np.asarray(pos1, dtype=np.int64).ravel()
        rl = np.asarray(read_len, dtype=np.int64).ravel()
        rev = np.asarray(reverse).ravel().astype(bool)
        span = np.full(ref.size, self.extend, dtype=np.int64) if self.extend else rl
        lo_all = np.maximum(np.where(rev, pos + rl - span, pos), 1)
        hi_all = np.where(rev, pos + rl - 1, pos + span - 1)
        added = 0
        for r in np.unique(ref).tolist():
            if r not in self.steps:
                continue
            sel = ref == r
            lo, hi = lo_all[sel], np.minimum(hi_all[sel], self.lengths[r])
            on = lo <= hi
            if self.steps[r] is None:
                self.steps[r] = np.zeros(self.lengths[r] + 1, dtype=np.int32)
            steps = self.steps[r]
            np.add.at(steps, lo[on] - 1, 1)
            np.add.at(steps, hi[on], -1)
            added += int(on.sum())
        self.reads += added
        if self.reads >= MAX_READS:
            raise ValueError("2^31 reads or more: the depth is a 32-bit count")
        return added

    def result(self) -> Coverage:
        runs = {}
        for r, steps in self.steps.items():
            at = np.flatnonzero(steps) if steps is not None else np.zeros(0, dtype=np.int64)
            if at.size:
                depth = np.cumsum(steps[at], dtype=np.int64)
                keep = depth[:-1] > 0
                runs[self.names[r]] = (at[:-1][keep], at[1:][keep], depth[:-1][keep])
        return Coverage(runs, self.reads, self.label, [(self.names[r], self.lengths[r]) for r in self.steps])


def count_host(ref_id, pos1, read_len, reverse, names, lengths, use, extend: int = 0) -> Coverage:
    """The pileup of the reads given as four columns over the references ``names`` / ``lengths`` chosen by ``use``."""
    acc = HostCount(names, lengths, use, extend)
    acc.add(ref_id, pos1, read_len, reverse)
    return acc.result()


class DeviceCount(SideAccumulator):
    """The pileup a device reader's handle holds between ``pmx_dbam_coverage_begin`` and the next one: ``add`` marks what the handle
    holds now (a stream reader calls it for every window), ``finish`` turns the table into runs, ``runs`` / ``text`` read them
    back, ``result`` is all of it as a ``Coverage``."""

    def __init__(self, reader, mapq_criteria: int, references=None, extend=0, max_size: int = 2000):
        """``extend`` ``"pair"``: ``add`` marks the FR rows of at most ``max_size`` bases (``pmx_dbam_coverage_add_fragments``)."""
        reader._check_open()
        self.mapq_criteria, self.extend, self.max_size = int(mapq_criteria), check_extend(extend), int(max_size)
        self.names = tuple(reader.references)
        self.use = _selected_mask(reader, references)
        self.refs = [(n, max(int(l), 0)) for n, l, u in zip(self.names, reader.lengths, self.use) if u]
        self.totals = None
        self.begin(reader)

    @staticmethod
    def _fn(reader, what: str, signal: bool):
        """The entry point ``what`` over the depth runs or, with ``signal``, its twin over the signal runs."""
        return getattr(reader._L, ("pmx_dbam_coverage_signal_" if signal else "pmx_dbam_coverage_") + what)

    def begin(self, reader) -> None:
        """A zeroed table on the reader's handle (a stream reader calls it again when a pass opens a new handle)."""
        mask = np.ascontiguousarray(self.use, dtype=np.uint8) if self.names else np.zeros(1, dtype=np.uint8)
        self.totals = self.sig = self.called = self.qtab = None
        rc = reader._L.pmx_dbam_coverage_begin(reader._h, 0 if self.extend == PAIR else self.extend, mask.ctypes.data)
        if rc:
            reader._raise(rc)

    def add(self, reader) -> int:
        added = ctypes.c_uint64()
        if self.extend == PAIR:
            rc = reader._L.pmx_dbam_coverage_add_fragments(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, self.max_size,
                                                           ctypes.byref(added))
        else:
            rc = reader._L.pmx_dbam_coverage_add(reader._h, self.mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(added))
        if rc:
            reader._raise(rc)
        return int(added.value)

    def finish(self, reader) -> Dict[str, int]:
        """The totals of ``pmx_dbam_coverage_finish`` by name (``TOTALS``); a second call gives the first one's."""
        if self.totals is None:
            out = np.zeros(5, dtype=np.uint64)
            rc = reader._L.pmx_dbam_coverage_finish(reader._h, out.ctypes.data)
            if rc:
                reader._raise(rc)
            self.totals = dict(zip(TOTALS, (int(x) for x in out)))
        return self.totals

    def signal(self, reader, bin: int = 1, scale: float = 1.0, normalize: str = "none") -> Dict[str, float]:
        """Makes the signal runs on the handle (``pmx_dbam_coverage_signal``), beside the depth runs and in place of an earlier
        signal, and returns their totals by name (``SIGNAL_TOTALS``).  Every method below takes ``signal=True`` to work on them.
        ``normalize``: the word the track line says."""
        bin, scale = check_bin(bin), check_scale(scale, self.finish(reader)["max_depth"])
        return self._track(reader, "signal", (bin, scale), bin, scale, check_normalize(normalize))

    def _track(self, reader, what: str, args, bin: int, scale: float, normalize: str, more: str = "", pscore: bool = False) -> Dict[str, float]:
        """A track into the handle's signal slot by ``pmx_dbam_coverage_<what>(handle, *args, totals)``, in place of the one before
        and its peaks; what a ``Signal`` of it says beside its runs is kept in ``sig``.  Returns the totals by name."""
        out = np.zeros(4, dtype=np.float64)
        self.sig = self.called = self.qtab = None
        rc = getattr(reader._L, "pmx_dbam_coverage_" + what)(reader._h, *args, out.ctypes.data)
        if rc:
            reader._raise(rc)
        self.sig = dict(bin=bin, scale=scale, normalize=normalize, more=more, pscore=pscore,
                        totals=dict(runs=int(out[0]), covered_bases=int(out[1]), min=float(out[2]), max=float(out[3])))
        return self.sig["totals"]

    def compare(self, reader, control_acc: "DeviceCount", control_reader, bin: int = 1, op: str = "log2", a_t: float = 1.0,
                a_c: float = 1.0, pseudo: float = 1.0, normalize: str = "none", control="") -> Dict[str, float]:
        """Makes the compared track of this pileup (the treatment) and the finished pileup ``control_acc`` on
        ``control_reader``'s handle (``pmx_dbam_coverage_compare``) in this handle's signal slot and returns
        its totals by name (``SIGNAL_TOTALS``): ``signal=True`` on every method below serves it.  The control's handle is
        not changed and may be closed afterwards.  ``normalize`` and ``control``: what the track line says."""
        bin = check_bin(bin)
        a_t, a_c, pseudo = check_factors(op, a_t, a_c, pseudo, self.finish(reader)["max_depth"], control_acc.finish(control_reader)["max_depth"])
        _same_refs(self.refs, control_acc.refs)
        return self._track(reader, "compare", (control_reader._h, bin, COMPARE.index(op), a_t, a_c, pseudo), bin, a_t, check_normalize(normalize),
                           compare_tail(control, op, pseudo))

    def poisson(self, reader, control_acc: "DeviceCount", control_reader, bin: int = 1, a_c: float = 1.0, small: int = LAMBDA_WINDOWS[0],
                large: int = LAMBDA_WINDOWS[1], control="") -> Dict[str, float]:
        """Makes the p-score track of this pileup (the treatment) against the finished pileup ``control_acc`` on
        ``control_reader``'s handle (``pmx_dbam_coverage_poisson``) in this handle's signal slot and returns its
        totals by name (``SIGNAL_TOTALS``): ``signal=True`` on every method below serves it, and ``call`` writes column 8.  The
        table ``lnfact`` is computed here.  The control's handle is not changed and may be closed afterwards."""
        bin = check_bin(bin)
        mine, theirs = self.finish(reader), control_acc.finish(control_reader)
        a_c, small, large = check_poisson(a_c, small, large, mine["max_depth"], theirs["max_depth"], theirs["fragment_bases"])
        _same_refs(self.refs, control_acc.refs)
        F = np.ascontiguousarray(lnfact(mine["max_depth"] + 1))
        return self._track(reader, "poisson", (control_reader._h, bin, a_c, small, large, F.ctypes.data, F.size), bin, 1.0, "none",
                           poisson_tail(control, small, large), True)

    def _count(self, reader, signal: bool) -> int:
        if signal and self.sig is None:
            raise ValueError("no signal: call signal first")
        return self.sig["totals"]["runs"] if signal else self.finish(reader)["runs"]

    def runs(self, reader, first: int = 0, n=None, signal: bool = False):
        """(reference int32, start0, end0, depth uint32) of the runs ``[first, first + n)`` (``pmx_dbam_coverage_runs``); with
        ``signal`` the last column is the float32 value."""
        n = self._count(reader, signal) - int(first) if n is None else int(n)
        out = [np.zeros(max(n, 1), dtype=t) for t in (np.int32, np.uint32, np.uint32, np.float32 if signal else np.uint32)]
        rc = self._fn(reader, "runs", signal)(reader._h, int(first), n, *(x.ctypes.data for x in out))
        if rc:
            reader._raise(rc)
        return tuple(x[:n] for x in out)

    def text(self, reader, first: int = 0, n=None, signal: bool = False) -> bytes:
        """The bedGraph lines of the runs ``[first, first + n)``, formatted on the device (``pmx_dbam_coverage_text``: the size,
        then the bytes)."""
        n = self._count(reader, signal) - int(first) if n is None else int(n)
        return _pull(reader, self._fn(reader, "text", signal), (int(first), n))

    def text_chunks(self, reader, chunk: int = TEXT_CHUNK, signal: bool = False) -> Iterator[bytes]:
        total = self._count(reader, signal)
        for first in range(0, total, int(chunk)):
            yield self.text(reader, first, min(int(chunk), total - first), signal)

    def ranges(self, reader, signal: bool = False) -> np.ndarray:
        """The first run of every chosen reference in header order, one more entry closing them (``pmx_dbam_coverage_ranges``)."""
        self.finish(reader)
        out = np.zeros(len(self.refs) + 1, dtype=np.int64)
        got = self._fn(reader, "ranges", signal)(reader._h, out.ctypes.data, out.size)
        if got < 0:
            reader._raise(got)
        assert got == out.size
        return out

    def sections(self, reader, first: int, n: int, chrom_id: int, items: int, signal: bool = False):
        """(bytes, table) of the runs ``[first, first + n)`` of one reference as bedGraph sections of a bigWig file stamped with
        ``chrom_id`` (``pmx_dbam_coverage_sections``: the size, then the bytes); ``table[section] = (id, start, id, end, bytes)``.
        With ``signal`` (bytes, table, sums): ``sums[section] = (sum, sum of squares)``, float64."""
        return self._sections(reader, first, n, chrom_id, items, signal, False)

    def _sections(self, reader, first, n, chrom_id, items, signal, z):
        """``sections``, or with ``z`` ``sections_z``: what an entry point writes behind the table is the streams' lengths (``z``), then
        the sums (``signal``), a row per section each."""
        rows = -(-int(n) // int(items))
        table = np.zeros((max(rows, 1), 5), dtype=np.uint32)
        more = [np.zeros(max(rows, 1), dtype=np.uint32)] * bool(z) + [np.zeros((max(rows, 1), 2), dtype=np.float64)] * bool(signal)
        blob = _pull(reader, self._fn(reader, "sections_z" if z else "sections", signal), (int(first), int(n), int(chrom_id), int(items)),
                     (None, 0) + (None,) * len(more), lambda size: (table.ctypes.data, len(table)) + tuple(x.ctypes.data for x in more), z)
        assert not z or len(blob) == int(more[0][:rows].sum(dtype=np.int64))
        return (blob, table[:rows]) + tuple(x[:rows] for x in more)

    def _section_chunks(self, pull, reader, k, chrom_id, items, chunk, signal):
        ranges = self.ranges(reader, signal)
        step = max(int(chunk) // int(items), 1) * int(items)
        for first in range(int(ranges[k]), int(ranges[k + 1]), step):
            yield pull(reader, first, min(step, int(ranges[k + 1]) - first), chrom_id, items, signal)

    def section_chunks(self, reader, k: int, chrom_id: int, items: int, chunk: int = TEXT_CHUNK, signal: bool = False):
        """``sections`` of the ``k``-th chosen reference, about ``chunk`` runs at a time (whole sections)."""
        return self._section_chunks(self.sections, reader, k, chrom_id, items, chunk, signal)

    def sections_z(self, reader, first: int, n: int, chrom_id: int, items: int, signal: bool = False):
        """``sections`` with every section compressed on the device (``pmx_dbam_coverage_sections_z``): (the zlib
        streams end to end, the table of ``sections`` -- column 4 stays the raw size --, the streams' lengths); with ``signal``
        the sums of ``sections`` behind them."""
        return self._sections(reader, first, n, chrom_id, items, signal, True)

    def section_chunks_z(self, reader, k: int, chrom_id: int, items: int, chunk: int = DEFLATE_CHUNK, signal: bool = False):
        """``sections_z`` of the ``k``-th chosen reference, about ``chunk`` runs at a time (whole sections)."""
        return self._section_chunks(self.sections_z, reader, k, chrom_id, items, chunk, signal)

    def zoom_begin(self, reader, z0: int, levels: int, ids, signal: bool = False) -> Tuple[int, int]:
        """Fills the zoom bins on the device (``pmx_dbam_coverage_zoom_begin``); ``ids[k]``: the chromosome id of the ``k``-th
        chosen reference.  Returns (the sum of depth^2 over the covered bases, the smallest depth); (0, 0) with ``signal``."""
        chrom_id = np.zeros(max(len(self.names), 1), dtype=np.uint32)
        chrom_id[np.flatnonzero(self.use)] = np.asarray(ids, dtype=np.uint32)
        out = np.zeros(2, dtype=np.uint64)
        rc = self._fn(reader, "zoom_begin", signal)(reader._h, int(z0), int(levels), chrom_id.ctypes.data, out.ctypes.data)
        if rc:
            reader._raise(rc)
        return int(out[0]), int(out[1])

    def zoom_records(self, reader, level: int, items: int, signal: bool = False):
        """(bytes, table) of a level's records, 32 bytes each, in sections of ``items`` (``pmx_dbam_coverage_zoom_records``);
        ``table[section] = (first id, first start, last id, last end, bytes)``.  The last level frees the bins."""
        tables = []

        def table_of(size):         # (the rows follow from the size)
            tables.append(np.zeros((max(-(-(size // 32) // int(items)), 1), 5), dtype=np.uint32))
            return tables[0].ctypes.data, len(tables[0])
        blob = _pull(reader, self._fn(reader, "zoom_records", signal), (int(level), int(items)), (None, 0), table_of)
        return blob, tables[0][:-(-(len(blob) // 32) // int(items))]

    def zoom_records_z(self, reader, level: int, items: int, signal: bool = False):
        """``zoom_records`` with every section compressed on the device (``pmx_dbam_coverage_zoom_records_z``): (streams, table,
        the streams' lengths).  The last level frees the bins."""
        size = self._fn(reader, "zoom_records", signal)(reader._h, int(level), int(items), None, 0, None, 0)     # (the raw bytes: the rows)
        rows = -(-(max(int(size), 0) // 32) // int(items))      # (what fails there fails in the pull, which raises it)
        table, zsizes = np.zeros((max(rows, 1), 5), dtype=np.uint32), np.zeros(max(rows, 1), dtype=np.uint32)
        blob = _pull(reader, self._fn(reader, "zoom_records_z", signal), (int(level), int(items)), (None, 0, None),
                     lambda size: (table.ctypes.data, len(table), zsizes.ctypes.data), True)
        assert len(blob) == int(zsizes[:rows].sum(dtype=np.int64))
        return blob, table[:rows], zsizes[:rows]

    def result(self, reader) -> Coverage:
        totals = self.finish(reader)
        c = Coverage(_by_reference(self.names, *self.runs(reader)), totals["reads"], self.extend, self.refs)
        if c.totals != tuple(totals[k] for k in TOTALS):
            raise RuntimeError("pmx_dbam_coverage_finish: the runs do not add up to the totals")
        return c

    def signal_result(self, reader) -> Signal:
        """The signal runs on the handle as a ``Signal``."""
        g = Signal(_by_reference(self.names, *self.runs(reader, signal=True)), self.sig["bin"], self.sig["scale"], self.refs, self.finish(reader)["reads"], self.extend, self.sig["normalize"],
                   self.sig["more"], self.sig["pscore"])
        if g.totals != tuple(self.sig["totals"][k] for k in SIGNAL_TOTALS):
            raise RuntimeError("pmx_dbam_coverage_signal: the runs do not add up to the totals")
        return g

    def call(self, reader, cutoff, max_gap: int = CALL_GAP, min_length: int = CALL_LENGTH) -> Dict[str, int]:
        """Calls the peaks of the signal runs on the handle (``pmx_dbam_coverage_call``) and returns the totals by
        name (``CALL_TOTALS``); the peak table stays on the handle until the next ``call``, ``signal``, ``compare`` or ``begin``.
        A handle without a signal gets ``signal(reader, 1, 1.0)`` first: the peaks of the depth track."""
        cutoff, max_gap, min_length = check_call(cutoff, max_gap, min_length)
        if self.sig is None:
            self.signal(reader, 1, 1.0)
        out = np.zeros(5, dtype=np.uint64)
        self.called = None
        rc = reader._L.pmx_dbam_coverage_call(reader._h, cutoff, max_gap, min_length, out.ctypes.data)
        if rc:
            reader._raise(rc)
        self.called = dict(cutoff=cutoff, max_gap=max_gap, min_length=min_length, pscore=self.sig["pscore"],
                           totals=dict(zip(CALL_TOTALS, (int(x) for x in out))))
        return self.called["totals"]

    def _peaks(self) -> int:
        if self.called is None:
            raise ValueError("no peaks: call call first")
        return self.called["totals"]["peaks"]

    def call_rows(self, reader, first: int = 0, n=None):
        """(reference int32, start, end, summit uint32, value float32, runs uint32) of the peaks ``[first, first + n)``
        (``pmx_dbam_coverage_call_rows``)."""
        n = self._peaks() - int(first) if n is None else int(n)
        out = [np.zeros(max(n, 1), dtype=t) for t in (np.int32, np.uint32, np.uint32, np.uint32, np.float32, np.uint32)]
        rc = reader._L.pmx_dbam_coverage_call_rows(reader._h, int(first), n, *(x.ctypes.data for x in out))
        if rc:
            reader._raise(rc)
        return tuple(x[:n] for x in out)

    def call_text(self, reader, first: int = 0, n=None) -> bytes:
        """The narrowPeak lines of the peaks ``[first, first + n)``, formatted on the device (``pmx_dbam_coverage_call_text``: the
        size, then the bytes); peak ``first + i`` is ``peak_<first + i + 1>``."""
        n = self._peaks() - int(first) if n is None else int(n)
        return _pull(reader, reader._L.pmx_dbam_coverage_call_text, (int(first), n))

    def call_text_chunks(self, reader, chunk: int = TEXT_CHUNK) -> Iterator[bytes]:
        total = self._peaks()
        for first in range(0, total, int(chunk)):
            yield self.call_text(reader, first, min(int(chunk), total - first))

    def qvalue(self, reader) -> Dict[str, int]:
        """Builds the q-score table of the p-score track on the handle (``pmx_dbam_coverage_qvalue``) and returns
        its totals by name (``QVALUE_TOTALS``).  The table stays on the handle until the next ``signal``, ``compare``, ``poisson``
        or ``begin``; while it is there ``call_text`` writes column 9.  A peak table that is there is dropped: ``call`` again."""
        out = np.zeros(4, dtype=np.uint64)
        self.called = self.qtab = None
        rc = reader._L.pmx_dbam_coverage_qvalue(reader._h, out.ctypes.data)
        if rc:
            reader._raise(rc)
        self.qtab = dict(zip(QVALUE_TOTALS, (int(x) for x in out)))
        return self.qtab

    def qvalue_rows(self, reader, first: int = 0, n=None):
        """(p float32, bases uint64, q float32) of the rows ``[first, first + n)`` (``pmx_dbam_coverage_qvalue_rows``)."""
        if n is None:
            if self.qtab is None:
                raise ValueError("no table: call qvalue first")
            n = self.qtab["rows"] - int(first)
        n = int(n)
        out = [np.zeros(max(n, 1), dtype=t) for t in (np.float32, np.uint64, np.float32)]
        rc = reader._L.pmx_dbam_coverage_qvalue_rows(reader._h, int(first), n, *(x.ctypes.data for x in out))
        if rc:
            reader._raise(rc)
        return tuple(x[:n] for x in out)

    def qvalue_cutoff(self, reader, X) -> float:
        """``pcut(X)`` of the table on the handle, searched on the device (``pmx_dbam_coverage_qvalue_cutoff``)."""
        out = ctypes.c_double()
        rc = reader._L.pmx_dbam_coverage_qvalue_cutoff(reader._h, check_q(X, "X"), ctypes.byref(out))
        if rc:
            reader._raise(rc)
        return float(out.value)

    def qvalue_result(self, reader) -> QTable:
        """The table on the handle as a ``QTable``."""
        t = QTable(*self.qvalue_rows(reader), self.qtab["tests"])
        if t.totals != tuple(self.qtab[k] for k in QVALUE_TOTALS):
            raise RuntimeError("pmx_dbam_coverage_qvalue: the rows do not add up to the totals")
        return t

    def call_result(self, reader) -> Peaks:
        """The peak table on the handle as a ``Peaks``, with the q-score table when the handle holds one."""
        ref, start, end, summit, value, runs = self.call_rows(reader)
        tot = self.called["totals"]
        p = Peaks(_by_reference(self.names, ref, start, end, summit, value, runs), self.called["cutoff"], self.called["max_gap"], self.called["min_length"], tot, self.called["pscore"],
                  None if self.qtab is None else self.qvalue_result(reader))
        inside = int(runs.sum(dtype=np.int64))
        if (p.n_peaks, p.peak_bases) != (tot["peaks"], tot["peak_bases"]) or not (tot["peaks"] <= tot["candidates"] <= tot["passing_runs"]) \
                or inside > tot["passing_runs"] or not (inside <= tot["passing_bases"] <= tot["peak_bases"]):
            raise RuntimeError("pmx_dbam_coverage_call: the peaks do not add up to the totals")
        return p


def count_device(reader, mapq_criteria: int, references=None, extend=0, max_size: int = 2000) -> Coverage:
    """``begin`` + ``add`` + ``finish`` + ``runs`` on a device reader's handle (what it holds now)."""
    acc = DeviceCount(reader, mapq_criteria, references, extend, max_size)
    acc.add(reader)
    return acc.result(reader)


def device_count_of(reader, mapq_criteria: int = 0, references=None, extend=0, max_size: int = 2000) -> DeviceCount:
    """The finished ``DeviceCount`` of everything a device reader reads: one ``add`` for a whole-file reader, every window of a
    stream reader (read once more when it is a regular file, ``InputUnseekable`` otherwise)."""
    acc = count_over(reader, "coverage", lambda: DeviceCount(reader, mapq_criteria, references, extend, max_size))
    acc.finish(reader)
    return acc


def from_reader(reader, mapq_criteria: int = 0, references=None, extend=0, max_size: int = 2000) -> Coverage:
    """The pileup of the reads of ``reader`` at ``mapq_criteria`` over ``references`` (names; None: every reference the reader has
    selected).  A device reader counts on the GPU (``device_count_of``); a host reader through ``batches`` and ``HostCount``.
    ``extend`` ``"pair"``: the FR pairs of at most ``max_size`` bases at their own extent; a host reader through
    ``fragments.rows_host``."""
    from .bam_device import DeviceBamReader
    if isinstance(reader, DeviceBamReader):
        return device_count_of(reader, mapq_criteria, references, extend, max_size).result(reader)
    acc = HostCount(reader.references, reader.lengths, _selected_mask(reader, references), extend)
    if acc.label == PAIR:
        from .fragments import FR, rows_host
        for ref, start1, size, orient, _c in rows_host(reader, mapq_criteria, references, max_size):
            fr = orient == FR
            if fr.any():
                acc.add(ref[fr], start1[fr], size[fr], np.zeros(int(fr.sum()), dtype=bool))
        return acc.result()
    for batch in reader.batches(mapq_criteria, PMX_BAM_DEFAULT_EXCLUDE):
        if len(batch[0]):
            acc.add(*batch)
    return acc.result()


def track_line(name: str, extend, reads: int, tail: str = "") -> bytes:
    """``tail``: what a signal track says behind the depth track's line (``signal_tail``)."""
    return 'track type=bedGraph name="{}" description="pymasc_amd fragment pileup extend={} reads={}"{}\n'.format(
        name, PAIR if extend == PAIR else int(extend) if int(extend) else "read", int(reads), tail).encode()


def write_track(path_base, name: str, extend, reads: int, chunks, tail: str = "") -> Path:
    """Writes ``<path_base>_coverage.bedGraph`` (to a temporary file beside it, renamed into place) and returns its path: the
    track line (with ``tail`` behind it), then the bytes of ``chunks`` (the lines of the runs)."""
    path = Path(str(path_base) + COVERAGE_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "wb") as fp:
            fp.write(track_line(name, extend, reads, tail))
            for chunk in chunks:
                fp.write(chunk)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def write_coverage(path_base, name: str, c, reader=None, signal: bool = False) -> Path:
    """``write_track`` of a ``Coverage`` or a ``Signal`` (the lines formatted on the host) or, with ``reader``, of a finished
    ``DeviceCount`` on that reader's handle: the lines are formatted on the device and pulled ``TEXT_CHUNK`` runs at a time;
    ``signal``: the lines of the signal it made last (``DeviceCount.signal``)."""
    if reader is None:
        return write_track(path_base, name, c.extend, c.reads, c.text_chunks(), c.tail if isinstance(c, Signal) else "")
    if signal and c.sig is None:
        raise ValueError("no signal: call signal first")
    tail = signal_tail(c.sig["bin"], c.sig["normalize"], c.sig["scale"]) + c.sig["more"] if signal else ""
    return write_track(path_base, name, c.extend, c.finish(reader)["reads"], c.text_chunks(reader, signal=signal), tail)


def read_coverage(path) -> Tuple[str, Coverage]:
    """(name, Coverage) of a ``_coverage.bedGraph`` as ``write_coverage`` writes it."""
    with open(path) as fp:
        head = _TRACK.match(fp.readline().rstrip("\n"))
        if head is None:
            raise ValueError("'{}' does not begin with the track line of a fragment pileup".format(path))
        cols: Dict[str, list] = {}
        for ln in fp:
            chrom, s, e, d = ln.rstrip("\n").split("\t")
            cols.setdefault(chrom, []).append((int(s), int(e), int(d)))
    runs = {k: tuple(zip(*v)) for k, v in cols.items()}
    extend = head.group(2)
    return head.group(1), Coverage(runs, int(head.group(3)), 0 if extend == "read" else PAIR if extend == PAIR else int(extend))


# ---------------------------------------------------------------------------------------------------------------------------------
# The pileup as a bigWig file: ``--coverage-format bigwig`` / ``coverage_format="bigwig"``
# ---------------------------------------------------------------------------------------------------------------------------------
#
# bbi version 4, little-endian, in this one layout: the 64-byte header, the zoom headers (24 bytes each), the 40-byte total summary,
# the chromosome B+ tree, the u64 section count, the data sections, their R-tree, then per zoom level a u32 record count, the
# level's sections and their R-tree, and the magic again.  fieldCount, definedFieldCount, autoSqlOffset and extensionOffset are 0.
#
# * Chromosomes: the chosen references with their lengths, keyed in bytewise name order; a chromosome's id is its rank in that
#   order, so the sections are written reference by reference in NAME order (``chr10`` before ``chr2``), each from its own range of
#   the runs: no run is sorted.  A chosen reference without a run is in the tree and has no section.
# * Data sections: type 1 (bedGraph), ``items_per_section`` runs each, the last one of a reference shorter, none holding two
#   references; a depth is written as float32, exact up to 2^24 and rounded to nearest above.
# * Zoom level ``k`` has the reduction ``z_k = z_0 * 4^k``: bin ``j`` of a reference covers ``[j * z, min((j + 1) * z, len))``; a bin
#   with a covered base (depth > 0) gives one record (id, start, end, validCount = its covered bases, then min, max, sum and sum of
#   squares of the depth over those bases as float32, each rounded to nearest even from the exact integer); empty bins are not
#   written.  The records are packed ``items_per_section`` to a section in (id, start) order; such a section may hold the last
#   records of one reference and the first of the next, which its R-tree item says with two ids.  ``z_0`` is ``zoom_base``, else the
#   smallest power of two that is at least ``10 * covered_bases / runs`` and 32.  Levels exist for ``k < 10`` while ``z_k`` is at
#   most half the longest chosen length; no run gives no level.
# * Total summary: validCount = covered_bases, the smallest and largest depth, sum = fragment_bases, and the sum of squares.
# * With ``compress`` every section goes through zlib on the host (a pool of at most ``min(16, cpus)`` threads) and
#   ``uncompressBufSize`` is the largest raw section; otherwise it is 0.  With ``compress="device"`` the sections
#   are compressed by the GPU's own DEFLATE encoder before they leave it: the source hands zlib streams and their lengths, and the
#   file differs from zlib's in its compressed bytes only.
#
# Sections, their tables and the zoom records come from a ``DeviceCount`` on its reader's handle (the GPU) or from ``HostParts``
# (numpy); everything else is the code below, so the two files are the same byte for byte when nothing is compressed.

BIGWIG_SUFFIX = "_coverage.bw"
FORMATS = ("bedgraph", "bigwig")
SUFFIXES = dict(zip(FORMATS, (COVERAGE_SUFFIX, BIGWIG_SUFFIX)))
BW_MAGIC, BW_CHROM_MAGIC, BW_RTREE_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0
ZOOM_LEVELS = 10            # at most (PMX_COVERAGE_ZOOM_LEVELS of include/pymasc_amd_ingest.h)
CHROM_BLOCK = 256           # keys per node of the chromosome tree
EXACT_DEPTH = 1 << 24       # below it a depth is exact as float32
ZOOM_RECORD = np.dtype([("id", "<u4"), ("start", "<u4"), ("end", "<u4"), ("valid", "<u4"), ("min", "<f4"), ("max", "<f4"), ("sum", "<f4"),
                        ("sumsq", "<f4")])


DEVICE = "device"           # ``compress``: the sections are compressed on the GPU
DEVICE_ITEMS = 2048         # items per section at most with it: a zoom section of 32-byte records must fit a chunk of the encoder
DEFLATE_MAX_CHUNK = 1 << 16     # PMX_DEFLATE_MAX_CHUNK of include/pymasc_amd_ingest.h


def check_compress(compress):
    """``coverage_compress`` as the run takes it: False, True (zlib on the host) or ``"device"``."""
    if compress == DEVICE or compress is True or compress is False:
        return compress
    if isinstance(compress, str):
        raise ValueError("coverage_compress is False, True or \"device\"")
    return bool(compress)


def check_format(fmt, compress=False) -> str:
    """``coverage_format`` as the run takes it; ``compress`` (``check_compress``) only with ``"bigwig"``."""
    compress = check_compress(compress)
    if fmt not in FORMATS:
        raise ValueError("coverage_format is \"bedgraph\" or \"bigwig\"")
    if compress and fmt != "bigwig":
        raise ValueError("coverage_compress needs coverage_format=\"bigwig\"")
    return fmt


def sumsq_fits(max_depth: int, fragment_bases: int) -> bool:
    """Whether every sum of depth^2 over covered bases is exact in 64 bits: it is at most ``max_depth * fragment_bases``, which
    must be below 2^64 (the check of ``pmx_dbam_coverage_zoom_begin``, made here for both paths before a byte is written)."""
    return int(max_depth) * int(fragment_bases) < 1 << 64


def zoom_plan(lengths, covered_bases: int, runs: int, zoom_base=None, bin: int = 1) -> Tuple[int, int]:
    """(z_0, levels) of a pileup over references of ``lengths``; ``bin`` above 1 (a signal's): ``zoom_base`` is a multiple of it,
    and without one ``z_0 = bin * p`` with the smallest power of two ``p`` that makes it at least ``10 * covered_bases / runs`` and
    32."""
    if zoom_base is not None and (isinstance(zoom_base, bool) or int(zoom_base) != zoom_base or not 1 <= int(zoom_base) < 1 << 31):
        raise ValueError("zoom_base is an integer of at least 1 and below 2^31")
    if zoom_base is not None and int(zoom_base) % int(bin):
        raise ValueError("zoom_base is a multiple of the signal's bin")
    if not runs:
        return 0, 0
    z0 = 32 if int(bin) == 1 else int(bin)
    if zoom_base is not None:
        z0 = int(zoom_base)
    else:
        while z0 * int(runs) < 10 * int(covered_bases) or z0 < 32:
            z0 *= 2
    longest, levels = max(lengths, default=0), 0
    while levels < ZOOM_LEVELS and 2 * z0 * 4 ** levels <= longest:
        levels += 1
    return z0, levels


def _section_table(ids, starts, ends, n: int, items: int, unit: int, head: int) -> np.ndarray:
    """``table[section] = (first id, first start, last id, last end, bytes)`` of ``n`` rows packed ``items`` to a section."""
    first = np.arange(0, n, items, dtype=np.int64)
    last = np.minimum(first + items, n) - 1
    t = np.zeros((first.size, 5), dtype=np.uint32)
    if n:
        t[:, 0], t[:, 1], t[:, 2], t[:, 3] = ids[first], starts[first], ids[last], ends[last]
        t[:, 4] = head + unit * (last - first + 1)
    return t


class HostParts:
    """The numpy twin of the device's bigWig entry points, over a ``Coverage`` that knows its chosen references: the path of host
    readers and the device's checker.  It has what ``assemble_bigwig`` takes from a source: ``refs``, ``totals``,
    ``section_chunks``, ``zoom_begin`` and ``zoom_records``."""

    def __init__(self, c):
        """``c``: a ``Coverage``, or a ``Signal`` (then ``bin`` is its bin, ``section_chunks`` also hands the sections' sums and the
        zoom levels are summed in float64 in the stated order)."""
        if c.refs is None:
            raise ValueError("the pileup does not know its chosen references' lengths (it was read from a bedGraph file)")
        if any(n not in dict(c.refs) for n in c.runs):
            raise ValueError("a run on a reference that is not among the chosen ones")
        self.c, self.refs = c, list(c.refs)
        self.bin = c.bin if isinstance(c, Signal) else None
        self.totals = dict(zip(TOTALS if self.bin is None else SIGNAL_TOTALS, c.totals))
        self._levels = []

    def section_chunks(self, k: int, chrom_id: int, items: int, chunk: int = TEXT_CHUNK):
        s, e, d = self.c.runs.get(self.refs[k][0], (np.zeros(0, dtype=np.uint32),) * 3)
        step = max(int(chunk) // int(items), 1) * int(items)
        for a in range(0, s.size, step):
            sa, ea, da = s[a:a + step], e[a:a + step], d[a:a + step]
            m = sa.size
            i = np.arange(m, dtype=np.int64)
            table = _section_table(np.full(m, chrom_id, dtype=np.uint32), sa, ea, m, items, 12, 24)
            out = np.zeros(6 * len(table) + 3 * m, dtype="<u4")
            at = 6 * (i // items + 1) + 3 * i
            out[at], out[at + 1], out[at + 2] = sa, ea, da.astype(np.float32).view(np.uint32)
            first = np.arange(0, m, items, dtype=np.int64)
            head = 6 * (first // items) + 3 * first
            out[head], out[head + 1], out[head + 2] = chrom_id, table[:, 1], table[:, 3]
            out[head + 5] = 1 | ((table[:, 4] - 24) // 12 << 16)
            if self.bin is None:
                yield out.tobytes(), table
                continue
            ov, v = (ea.astype(np.int64) - sa.astype(np.int64)).astype(np.float64), da.astype(np.float64)
            sums = np.zeros((len(table), 2), dtype=np.float64)
            np.add.at(sums[:, 0], i // items, ov * v)               # (np.add.at adds one element after the other, in order)
            np.add.at(sums[:, 1], i // items, ov * (v * v))
            yield out.tobytes(), table, sums

    @staticmethod
    def _reduce(j, cnt, mn, mx, sm, sq):
        """The bins ``j`` (ascending, with repeats) reduced to one row per distinct bin."""
        at = np.flatnonzero(np.concatenate(([True], j[1:] != j[:-1]))) if j.size else np.zeros(0, dtype=np.int64)
        if not j.size:
            return j, cnt, mn, mx, sm, sq
        return (j[at], np.add.reduceat(cnt, at), np.minimum.reduceat(mn, at), np.maximum.reduceat(mx, at), np.add.reduceat(sm, at),
                np.add.reduceat(sq, at))

    @staticmethod
    def _reduce_signal(j, cnt, mn, mx, sm, sq):
        """``_reduce`` for a signal: the two float64 sums are added one after the other, in order, from 0.0."""
        if not j.size:
            return j, cnt, mn, mx, sm, sq
        first = np.concatenate(([True], j[1:] != j[:-1]))
        at, g = np.flatnonzero(first), np.cumsum(first) - 1
        a, b = np.zeros(at.size, dtype=np.float64), np.zeros(at.size, dtype=np.float64)
        np.add.at(a, g, sm)
        np.add.at(b, g, sq)
        return j[at], np.add.reduceat(cnt, at), np.minimum.reduceat(mn, at), np.maximum.reduceat(mx, at), a, b

    def _zoom_begin_signal(self, z0: int, levels: int, ids) -> Tuple[int, int]:
        order = np.argsort(np.asarray(ids))
        empty = (np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.float32))
        level = []
        for k in order.tolist():
            s, e, v = self.c.runs.get(self.refs[k][0], empty)
            s, e = s.astype(np.int64), e.astype(np.int64)
            if not levels:
                continue
            j0, j1 = s // z0, (e - 1) // z0
            n = j1 - j0 + 1
            run = np.repeat(np.arange(s.size), n)
            j = j0[run] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
            w = np.minimum(e[run], (j + 1) * z0) - np.maximum(s[run], j * z0)
            ov, vv = w.astype(np.float64), v[run].astype(np.float64)
            level.append(self._reduce_signal(j, w.astype(np.uint64), v[run], v[run], ov * vv, ov * (vv * vv)))
        self._ids, self._z0, self._levels = [int(ids[k]) for k in order.tolist()], int(z0), [level] if levels else []
        self._lens = [self.refs[k][1] for k in order.tolist()]
        for _ in range(1, levels):
            self._levels.append([self._reduce_signal(r[0] // 4, *r[1:]) for r in self._levels[-1]])
        return 0, 0

    def zoom_begin(self, z0: int, levels: int, ids) -> Tuple[int, int]:
        if self.bin is not None:
            return self._zoom_begin_signal(z0, levels, ids)
        order = np.argsort(np.asarray(ids))                 # the chosen references in id order
        empty = (np.zeros(0, dtype=np.uint32),) * 3
        level, sumsq, low = [], 0, None
        for k in order.tolist():
            s, e, d = (x.astype(np.int64) for x in self.c.runs.get(self.refs[k][0], empty))
            sumsq += int(((e - s).astype(np.uint64) * d.astype(np.uint64) * d.astype(np.uint64)).sum(dtype=np.uint64))
            if d.size:
                low = int(d.min()) if low is None else min(low, int(d.min()))
            if not levels:
                continue
            j0, j1 = s // z0, (e - 1) // z0
            n = j1 - j0 + 1                                 # the bins of every run
            run = np.repeat(np.arange(s.size), n)
            j = j0[run] + np.arange(int(n.sum())) - np.repeat(np.cumsum(n) - n, n)
            w = (np.minimum(e[run], (j + 1) * z0) - np.maximum(s[run], j * z0)).astype(np.uint64)
            dd = d[run].astype(np.uint64)
            level.append(self._reduce(j, w, dd, dd, w * dd, w * dd * dd))
        self._ids, self._z0, self._levels = [int(ids[k]) for k in order.tolist()], int(z0), [level] if levels else []
        self._lens = [self.refs[k][1] for k in order.tolist()]
        for _ in range(1, levels):                          # four bins into one
            self._levels.append([self._reduce(r[0] // 4, *r[1:]) for r in self._levels[-1]])
        return sumsq, low or 0

    def zoom_records(self, level: int, items: int):
        z = self._z0 * 4 ** level
        rows = self._levels[level]
        rec = np.zeros(sum(r[0].size for r in rows), dtype=ZOOM_RECORD)
        a = 0
        for cid, length, (j, cnt, mn, mx, sm, sq) in zip(self._ids, self._lens, rows):
            v = rec[a:a + j.size]
            v["id"], v["start"], v["end"], v["valid"] = cid, j * z, np.minimum((j + 1) * z, length), cnt
            v["min"], v["max"], v["sum"], v["sumsq"] = (x.astype(np.float32) for x in (mn, mx, sm, sq))
            a += j.size
        return rec.tobytes(), _section_table(rec["id"], rec["start"], rec["end"], rec.size, items, 32, 0)


class _DeviceParts:
    """A finished ``DeviceCount`` on its reader's handle as a source of ``assemble_bigwig``; ``signal``: the signal it made last."""

    def __init__(self, acc: "DeviceCount", reader, signal: bool = False):
        self.acc, self.reader, self.refs, self.sg = acc, reader, list(acc.refs), bool(signal)
        if self.sg and acc.sig is None:
            raise ValueError("no signal: call signal first")
        self.bin = acc.sig["bin"] if self.sg else None
        self.totals = dict(acc.sig["totals"]) if self.sg else dict(acc.finish(reader))

    def section_chunks(self, k, chrom_id, items):
        return self.acc.section_chunks(self.reader, k, chrom_id, items, signal=self.sg)

    def zoom_begin(self, z0, levels, ids):
        return self.acc.zoom_begin(self.reader, z0, levels, ids, self.sg)

    def zoom_records(self, level, items):
        return self.acc.zoom_records(self.reader, level, items, self.sg)

    def section_chunks_z(self, k, chrom_id, items):
        return self.acc.section_chunks_z(self.reader, k, chrom_id, items, signal=self.sg)

    def zoom_records_z(self, level, items):
        return self.acc.zoom_records_z(self.reader, level, items, self.sg)


def _chrom_tree(names, ids, lengths, at: int) -> bytes:
    """The chromosome B+ tree, which begins at ``at``: ``names`` (bytes, ascending) with their ids and lengths, ``CHROM_BLOCK`` keys
    per node, a node's children behind it."""
    key = max(len(n) for n in names)
    tiers = [[(n, struct.pack("<II", i, l)) for n, i, l in zip(names, ids, lengths)]]      # (key, value) of every item, per tier
    while len(tiers[-1]) > CHROM_BLOCK:
        tiers.append([(tiers[-1][a][0], None) for a in range(0, len(tiers[-1]), CHROM_BLOCK)])
    out = [struct.pack("<IIIIQQ", BW_CHROM_MAGIC, CHROM_BLOCK, key, 8, len(names), 0)]
    pos, where = at + 32, {}
    for t in reversed(range(len(tiers))):                                                   # where every tier's nodes begin
        where[t] = pos
        pos += 4 * -(-len(tiers[t]) // CHROM_BLOCK) + (key + 8) * len(tiers[t])
    for t in reversed(range(len(tiers))):
        for k in range(0, len(tiers[t]), CHROM_BLOCK):
            items = tiers[t][k:k + CHROM_BLOCK]
            out.append(struct.pack("<BBH", t == 0, 0, len(items)))
            for x, (name, value) in enumerate(items, k):                                    # (item x of a tier points to node x of the one below)
                out.append(name.ljust(key, b"\0") + (value if t == 0 else struct.pack("<Q", where[t - 1] + (4 + (key + 8) * CHROM_BLOCK) * x)))
    return b"".join(out)


_RT_LEAF = np.dtype([("c0", "<u4"), ("s0", "<u4"), ("c1", "<u4"), ("e1", "<u4"), ("off", "<u8"), ("size", "<u8")])
_RT_NODE = np.dtype([("c0", "<u4"), ("s0", "<u4"), ("c1", "<u4"), ("e1", "<u4"), ("off", "<u8")])


def _rtree(table: np.ndarray, offsets: np.ndarray, sizes: np.ndarray, block: int, per_slot: int, at: int, data_end: int) -> bytes:
    """The R-tree over the sections of ``table`` (rows ``(id, start, id, end, ...)`` in (id, start) order) that lie at ``offsets``
    with ``sizes`` bytes; the index itself begins at ``at``.  Built bottom-up, ``block`` items per node, a node's children behind it;
    a node's bounds are its first item's beginning and the largest (id, end) among its items.  No section: one empty leaf."""
    n = len(table)
    leaf = np.zeros(n, dtype=_RT_LEAF)
    leaf["c0"], leaf["s0"], leaf["c1"], leaf["e1"], leaf["off"], leaf["size"] = table[:, 0], table[:, 1], table[:, 2], table[:, 3], offsets, sizes
    tiers = [leaf]                                          # the items of every tier, bottom-up
    while len(tiers[-1]) > block:
        below = tiers[-1]
        first = np.arange(0, len(below), block)
        hi = np.maximum.reduceat((below["c1"].astype(np.uint64) << np.uint64(32)) | below["e1"].astype(np.uint64), first)
        node = np.zeros(first.size, dtype=_RT_NODE)
        node["c0"], node["s0"], node["c1"], node["e1"] = below["c0"][first], below["s0"][first], hi >> np.uint64(32), hi & np.uint64(0xffffffff)
        tiers.append(node)
    pos = at + 48
    for t in reversed(range(len(tiers))):                   # the root first; every item above the leaves learns where its node is
        items = tiers[t]
        nodes = max(-(-len(items) // block), 1)
        if t + 1 < len(tiers):
            k = np.arange(len(tiers[t + 1]), dtype=np.uint64)
            tiers[t + 1]["off"] = np.uint64(pos) + k * np.uint64(4 + items.dtype.itemsize * block)
        pos += 4 * nodes + items.dtype.itemsize * len(items)
    top = tiers[-1]
    hi = int(((top["c1"].astype(np.uint64) << np.uint64(32)) | top["e1"].astype(np.uint64)).max()) if n else 0
    out = [struct.pack("<IIQIIIIQII", BW_RTREE_MAGIC, block, n, int(top["c0"][0]) if n else 0, int(top["s0"][0]) if n else 0, hi >> 32,
                       hi & 0xffffffff, data_end, per_slot, 0)]
    for t in reversed(range(len(tiers))):
        items = tiers[t]
        for a in range(0, max(len(items), 1), block):
            part = items[a:a + block]
            out.append(struct.pack("<BBH", t == 0, 0, len(part)) + part.tobytes())
    return b"".join(out)


class _SectionWriter:
    """Writes sections at the file's end and remembers where: raw, each through zlib in a pool of threads, or (``"device"``) as the
    zlib streams the source made of them."""

    def __init__(self, fp, compress):
        self.fp, self.largest, self.pool = fp, 0, None
        if compress is True:
            from multiprocessing.pool import ThreadPool
            self.pool = ThreadPool(max(min(16, os.cpu_count() or 1), 1))

    def close(self) -> None:
        if self.pool is not None:
            self.pool.close()
            self.pool.join()

    def write_streams(self, blob: bytes, table: np.ndarray, zsizes: np.ndarray):
        """The sections as the streams of ``blob``, ``zsizes`` bytes each, written as they are; ``table[:, 4]``: their raw sizes."""
        sizes = np.asarray(zsizes).astype(np.int64)
        assert len(sizes) == len(table) and int(sizes.sum()) == len(blob)
        self.largest = max(self.largest, int(table[:, 4].max()) if len(table) else 0)
        at = self.fp.tell()
        self.fp.write(blob)
        return at + np.cumsum(sizes) - sizes, sizes

    def write(self, blob: bytes, table: np.ndarray):
        """The sections of ``blob`` (``table[:, 4]``: their raw sizes); returns their (offsets, sizes) in the file."""
        raw = table[:, 4].astype(np.int64)
        ends = np.cumsum(raw)
        assert (int(ends[-1]) if raw.size else 0) == len(blob)
        self.largest = max(self.largest, int(raw.max()) if raw.size else 0)
        at = self.fp.tell()
        if self.pool is None:
            self.fp.write(blob)
            return at + ends - raw, raw
        view = memoryview(blob)
        parts = self.pool.map(zlib.compress, [view[int(z - r):int(z)] for z, r in zip(ends, raw)], chunksize=64)
        sizes = np.array([len(p) for p in parts], dtype=np.int64)
        self.fp.write(b"".join(parts))
        return at + np.cumsum(sizes) - sizes, sizes


def assemble_bigwig(fp, src, compress=False, items_per_section: int = 1024, index_block: int = 256, zoom_base=None) -> None:
    """Writes the bigWig file of the source ``src`` (``HostParts``, or a ``DeviceCount`` with its reader) into the seekable binary
    file ``fp``, from its beginning.  ``compress``: False, True (every section through zlib on the host) or ``"device"`` (the source
    compresses them: it has ``section_chunks_z`` and ``zoom_records_z``, which hand ``(streams, table, lengths)``)."""
    items, block = int(items_per_section), int(index_block)
    compress = check_compress(compress)
    if not 1 <= items <= 65535 or not 2 <= block <= 65535:
        raise ValueError("items_per_section lies in [1, 65535] and index_block in [2, 65535]")
    device = compress == DEVICE
    if device and items > DEVICE_ITEMS:
        raise ValueError("compress=\"device\" takes at most {} items per section".format(DEVICE_ITEMS))
    if device and not (hasattr(src, "section_chunks_z") and hasattr(src, "zoom_records_z")):
        raise ValueError("compress=\"device\" needs a pileup counted by a device reader: this source has no section_chunks_z "
                         "(a host reader or device_ingest=False; use compress=True for zlib on the host)")
    refs, tot = src.refs, src.totals
    sbin = getattr(src, "bin", None)                                   # a signal's bin; None: the depth runs
    if not refs:
        raise ValueError("no chosen reference")
    if sbin is None and not sumsq_fits(tot["max_depth"], tot["fragment_bases"]):
        raise ValueError("max_depth * fragment_bases is 2^64 or more: the zoom levels' sums of squares would not be exact")
    z0, levels = zoom_plan([l for _n, l in refs], tot["covered_bases"], tot["runs"], zoom_base, sbin or 1)
    names = [n.encode() for n, _l in refs]
    order = sorted(range(len(refs)), key=lambda k: names[k])           # bytewise name order: a chromosome's id is its rank
    if any(names[a] == names[b] for a, b in zip(order, order[1:])):
        raise ValueError("two chosen references have the same name")
    ids = [0] * len(refs)
    for rank, k in enumerate(order):
        ids[k] = rank
    sumsq, low = src.zoom_begin(z0, levels, ids)
    # the pass over the runs against finish's totals: d <= d^2 <= max_depth * d for every covered base
    if sbin is None and not (low <= tot["max_depth"] and tot["fragment_bases"] <= sumsq <= tot["max_depth"] * tot["fragment_bases"]
                             and bool(low) == bool(tot["runs"])):
        raise RuntimeError("the zoom pass does not agree with the pileup's totals")
    writer = _SectionWriter(fp, compress)
    try:
        fp.seek(0)
        fp.write(bytes(64 + 24 * levels))
        summary_at = fp.tell()
        if sbin is None:
            fp.write(struct.pack("<Qdddd", tot["covered_bases"], float(low), float(tot["max_depth"]), float(tot["fragment_bases"]), float(sumsq)))
        else:
            fp.write(bytes(40))                                         # (a signal's two sums are known behind its sections)
        total, squares = 0.0, 0.0
        tree_at = fp.tell()
        fp.write(_chrom_tree([names[k] for k in order], range(len(order)), [refs[k][1] for k in order], tree_at))
        data_at = fp.tell()
        fp.write(bytes(8))
        tables, offsets, sizes, n_runs = [], [], [], 0
        for rank, k in enumerate(order):
            for part in (src.section_chunks_z if device else src.section_chunks)(k, rank, items):
                table = part[1]
                if sbin is not None:                                    # the sections' partial sums, added in file order
                    part, sums = part[:-1], part[-1]
                    for a, b in sums.tolist():
                        total += a
                        squares += b
                o, s = writer.write_streams(*part) if device else writer.write(*part)
                tables.append(table)
                offsets.append(o)
                sizes.append(s)
                n_runs += (int(table[:, 4].sum(dtype=np.int64)) - 24 * len(table)) // 12
        if n_runs != tot["runs"]:
            raise RuntimeError("the sections hold {} runs, the pileup {}".format(n_runs, tot["runs"]))
        table = np.concatenate(tables) if tables else np.zeros((0, 5), dtype=np.uint32)
        index_at, n_sections = fp.tell(), len(table)
        fp.write(_rtree(table, np.concatenate(offsets) if offsets else np.zeros(0), np.concatenate(sizes) if sizes else np.zeros(0),
                        block, items, index_at, index_at))
        zooms = []
        for level in range(levels):
            part = (src.zoom_records_z if device else src.zoom_records)(level, items)
            table = part[1]
            at = fp.tell()
            fp.write(struct.pack("<I", int(table[:, 4].sum(dtype=np.int64)) // 32))
            o, s = writer.write_streams(*part) if device else writer.write(*part)
            zindex_at = fp.tell()
            fp.write(_rtree(table, o, s, block, items, zindex_at, zindex_at))
            zooms.append((z0 * 4 ** level, at, zindex_at))
        fp.write(struct.pack("<I", BW_MAGIC))
        fp.seek(0)
        fp.write(struct.pack("<IHHQQQHHQQIQ", BW_MAGIC, 4, levels, tree_at, data_at, index_at, 0, 0, 0, summary_at,
                             writer.largest if compress else 0, 0))
        for z, at, zindex_at in zooms:
            fp.write(struct.pack("<IIQQ", z, 0, at, zindex_at))
        if sbin is not None:
            fp.seek(summary_at)
            fp.write(struct.pack("<Qdddd", tot["covered_bases"], float(tot["min"]), float(tot["max"]), total, squares))
        fp.seek(data_at)
        fp.write(struct.pack("<Q", n_sections))
        fp.seek(0, os.SEEK_END)
    finally:
        writer.close()


def deflate_bound(n: int) -> int:
    """The longest zlib stream the device encoder writes for ``n`` raw bytes (``pmx_ddeflate_bound``)."""
    return int(load_ingest_library().pmx_ddeflate_bound(int(n)))


def deflate_device(chunks, device: int = 0):
    """Every chunk (bytes of at most ``DEFLATE_MAX_CHUNK``) as one zlib stream made by the GPU's DEFLATE encoder (``pmx_ddeflate``;
    DESIGN.md 7.18.2): a list of bytes that ``zlib.decompress`` turns back into the chunks."""
    L = load_ingest_library()
    chunks = [bytes(c) for c in chunks]
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    src = np.frombuffer(b"".join(chunks) or b"\0", dtype=np.uint8)
    cap = sum(int(L.pmx_ddeflate_bound(len(c))) for c in chunks)
    dst, sizes = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(max(len(chunks), 1), dtype=np.uint32)
    got = L.pmx_ddeflate(int(device), src.ctypes.data, offsets.ctypes.data, len(chunks), dst.ctypes.data, cap, sizes.ctypes.data)
    if got < 0:
        raise_last(L, got)
    ends = np.cumsum(sizes[:len(chunks)], dtype=np.int64)
    assert (int(ends[-1]) if len(chunks) else 0) == got
    return [dst[int(z - n):int(z)].tobytes() for z, n in zip(ends, sizes)]


def bigwig_source(c, reader=None, signal: bool = False):
    """What ``assemble_bigwig`` reads: ``HostParts`` of a ``Coverage`` or a ``Signal``, or a finished ``DeviceCount`` on ``reader``'s
    handle (``signal``: the signal it made last)."""
    return HostParts(c) if reader is None else _DeviceParts(c, reader, signal)


def write_bigwig(path_base, name: str, c, reader=None, compress=False, items_per_section: int = 1024, index_block: int = 256,
                 zoom_base=None, signal: bool = False) -> Path:
    """Writes ``<path_base>_coverage.bw`` (to a temporary file beside it, renamed into place) and returns its path: the pileup of
    a ``Coverage`` that knows its chosen references (sections and zoom records made with numpy) or, with ``reader``, of a finished
    ``DeviceCount`` on that reader's handle (made on the GPU).  A bigWig file has no place for ``name``, the reads or the extent.
    A depth is exact as float32 up to 2^24 and rounded to nearest above.  ``compress``: as for ``assemble_bigwig``; ``"device"`` needs
    ``reader``.  ``c`` may be a ``Signal``; with ``reader``, ``signal`` writes the signal the count made last."""
    path = Path(str(path_base) + BIGWIG_SUFFIX)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "w+b") as fp:
            assemble_bigwig(fp, bigwig_source(c, reader, signal), compress, items_per_section, index_block, zoom_base)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def write_file(path, chunks) -> Path:
    """Writes the bytes of ``chunks`` to ``path`` (through a temporary file beside it, renamed into place)."""
    path = Path(path)
    tmp = "{}.tmp.{}".format(path, os.getpid())
    try:
        with open(tmp, "wb") as fp:
            for chunk in chunks:
                fp.write(chunk)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.unlink(tmp)
    return path


def write_called(path_base, chunks) -> Path:
    """Writes ``<path_base>_coverage_peaks.narrowPeak`` (through a temporary file, renamed into place) and returns its path: the
    bytes of ``chunks`` -- ``Peaks.text_chunks()`` or ``DeviceCount.call_text_chunks(reader)`` --, no header line, so that
    ``peaks.open_peaks`` reads the file as it is."""
    return write_file(str(path_base) + CALL_SUFFIX, chunks)


def read_bigwig(path) -> Coverage:
    """The pileup of a ``_coverage.bw``, read through the host ``BigWigReader``: the runs by reference in the file's (name) order
    and ``refs`` from its chromosome tree.  The file does not hold the reads or the extent: both are 0.  A value that is not a whole
    number from 1 to 2^24 - 1 is a ValueError (such a file is not a pileup this module wrote, or holds a depth float32 rounded)."""
    from .bigwig import BigWigReader
    with BigWigReader(path) as r:
        refs = list(r.chromsizes.items())
        runs = {}
        for chrom, _length in refs:
            s, e, v = r.fetch_arrays(0.0, chrom)
            if v.size:
                if not bool(np.all((v >= 1) & (v < EXACT_DEPTH) & (v == np.floor(v)))):
                    raise ValueError("'{}': a value on '{}' is not a whole number from 1 to 2^24 - 1".format(path, chrom))
                runs[chrom] = (s, e, v.astype(np.uint32))
    return Coverage(runs, 0, 0, refs)
