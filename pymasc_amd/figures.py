"""PyMaSC's figure: one PDF of cross-correlation plots drawn from the statistics of a run (``stats.GenomeStats``).

The pages, in order, as PyMaSC's output/figure.py draws them:

  1. the genome-wide NCC with its 99 % band, the background ``min(cc)`` and marks at the read length and at the
     expected and estimated library lengths, NSC / RSC in a box;
  2. the same, zoomed to ``[0, 2 x est]`` around MSCC's estimate: only with both curves and ``2 x est < max_shift + 1``;
  3. the genome-wide MSCC with its smoothed curve and band;
  4. ``Naive CC vs MSCC``: both genome-wide curves less their minima (drawn whenever there is an MSCC curve);
  5. one such comparison per chromosome with a curve, in sorted order; a chromosome whose curves are all NaN is skipped.

Drawn with matplotlib's object-oriented API (``Figure`` and ``backend_pdf.PdfPages``), never ``pyplot``: no global state, no
GUI backend, no display.  matplotlib is imported when a figure is drawn, not with this module.  The PDF carries no creation
date, so that the same statistics give the same bytes.

There is no kernel here: a few thousand float64 values per page, drawn once per run.
"""
from __future__ import annotations

import logging
import os
from pathlib import Path
from typing import List, Optional, Tuple

import numpy as np

from .stats import CurveStats, GenomeStats

logger = logging.getLogger(__name__)

PDF_SUFFIX = ".pdf"
XLABEL = "Reverse Strand Shift"
BAND_COLOR = "lightskyblue"


def _title(what: str, name: Optional[str]) -> str:
    return what + (" for " + name if name else "")


def _new_figure():
    from matplotlib.figure import Figure
    fig = Figure()
    return fig, fig.add_subplot()


def _headroom(ax) -> Tuple[float, float, float]:
    """Raise the top of the y range by 10 % (lower it by 5 % when it is not above 0); (lower, upper, height)."""
    lower, upper = ax.get_ylim()
    lower, upper = ax.set_ylim((lower, upper * 1.1 if upper > 0 else upper * 0.95))
    return lower, upper, upper - lower


def _mark(ax, x, color, label_y, label, point_y=None, point_label=None, offset=0.0) -> None:
    """A dashed vertical line at ``x`` with ``label`` at height ``label_y``; with ``point_y``, a ring on the curve there and
    ``point_label`` beside it, ``offset`` above it."""
    ax.axvline(x, color=color, linestyle="dashed", linewidth=0.5)
    ax.annotate(label, (x, label_y))
    if point_y and point_label:
        ax.scatter(x, point_y, facecolors="none", edgecolors=color)
        ax.annotate(point_label, (x, point_y + offset))


def _box(ax, text: str) -> None:
    """A rounded box in the bottom right corner of the axes."""
    ax.annotate(text, xy=(1, ax.get_ylim()[0]), textcoords="axes fraction", xytext=(0.95, 0.05),
                bbox=dict(boxstyle="round", fc="w", alpha=0.9), horizontalalignment="right")


def _usable(s: Optional[CurveStats]) -> bool:
    return s is not None and s.cc is not None and not np.all(np.isnan(s.cc))


# ---- the pages -----------------------------------------------------------------------------------------------------

def ncc_page(s: CurveStats, name: Optional[str], xlim=None):
    """Page 1 (and, with ``xlim``, page 2): the genome-wide NCC."""
    fig, ax = _new_figure()
    ax.set_title(_title("Cross-Correlation", name))
    ax.set_xlabel(XLABEL)
    ax.set_ylabel("Cross-Correlation")
    x = np.arange(len(s.cc))
    if s.cc_lower is not None and s.cc_upper is not None:
        ax.fill_between(x, s.cc_lower, s.cc_upper, color=BAND_COLOR, alpha=0.5, linewidth=0)
    ax.plot(x, s.cc, color="black", linewidth=0.5)
    if xlim is not None:
        ax.set_xlim(xlim)
    _lower, upper, height = _headroom(ax)

    ax.axhline(s.cc_min, linestyle="dashed", linewidth=0.5)
    ax.text(0, s.cc_min, "min(cc) = {:.5f}".format(s.cc_min))
    _mark(ax, s.read_len - 1, "red", upper - height / 25, "read length: {}".format(s.read_len),
          s.ccrl, " cc(read length) = {:.5f}".format(s.ccrl), height / 50)
    est = s.estimated
    if est.fragment_length and est.ccfl is not None:
        _mark(ax, est.fragment_length - 1, "blue", upper - height / 10,
              "estimated lib len: {}".format(est.fragment_length),
              est.ccfl, " cc(est lib len) = {:.5f}".format(est.ccfl), height / 50)
    exp = s.expected
    if exp.fragment_length and exp.ccfl is not None:
        _mark(ax, exp.fragment_length - 1, "green", upper - height / 6,
              "expected lib len: {}".format(exp.fragment_length),
              exp.ccfl, " cc(lib length) = {:.5f}".format(exp.ccfl), -height / 25)

    lines = ["{} = {:.5f}".format(label, v) for label, v in
             (("NSC", exp.nsc), ("RSC", exp.rsc), ("Est NSC", est.nsc), ("Est RSC", est.rsc)) if v]
    if lines:
        _box(ax, "\n".join(lines))
    return fig


def mscc_page(s: CurveStats, name: Optional[str], smooth_window: int):
    """Page 3: the genome-wide MSCC, its moving average and band, and the library lengths on it."""
    fig, ax = _new_figure()
    ax.set_title(_title("MSCC and Library Length Estimation", name))
    ax.set_xlabel(XLABEL)
    ax.set_ylabel("Mappability Sensitive Cross-Correlation")
    x = np.arange(len(s.cc))
    if s.cc_lower is not None and s.cc_upper is not None:
        ax.fill_between(x, s.cc_lower, s.cc_upper, color=BAND_COLOR, alpha=0.5, linewidth=0)
    ax.plot(x, s.cc, color="black", linewidth=0.5, label="MSCC")
    ax.plot(x, s.avr_cc, alpha=0.8, label="Smoothed", color="pink")
    _lower, upper, height = _headroom(ax)

    n = len(s.cc)
    if s.est_lib_len and s.est_lib_len <= n:
        y = s.cc[s.est_lib_len - 1]
        _mark(ax, s.est_lib_len - 1, "blue", upper - height / 2, "estimated lib len: {}".format(s.est_lib_len),
              y, " cc(est lib len) = {:.5f}".format(y), height / 50)
    lib = s.expected.fragment_length
    if lib and lib <= n:
        y = s.cc[lib - 1]
        _mark(ax, lib - 1, "green", upper - height / 1.75, "expected lib len: {}".format(lib),
              y, " cc(lib length) = {:.5f}".format(y), -height / 25)
    ax.legend(loc="best")
    _box(ax, "Mov avr win size = {}".format(smooth_window))
    return fig


def comparison_page(ncc: Optional[CurveStats], mscc: Optional[CurveStats], title: str):
    """Pages 4 and 5: NCC and MSCC less their minima on one axis; None when neither curve has a finite value."""
    has_ncc, has_mscc = _usable(ncc), _usable(mscc)
    if not (has_ncc or has_mscc):
        return None
    fig, ax = _new_figure()
    ax.set_title(title)
    ax.set_xlabel(XLABEL)
    ax.set_ylabel("Relative Cross-Correlation from each minimum")
    if ncc is not None:
        ax.plot(np.arange(len(ncc.cc)), ncc.cc - ncc.cc_min, color="black", linewidth=0.5, label="Naive CC")
    if mscc is not None:
        ax.plot(np.arange(len(mscc.cc)), mscc.cc - mscc.cc_min, alpha=0.8 if has_ncc else 1, linewidth=0.5,
                label="MSCC")
    _lower, upper, height = _headroom(ax)

    first = ncc if ncc is not None else mscc
    _mark(ax, first.read_len, "red", upper - height / 25, "read length: {}".format(first.read_len))
    if mscc is not None:
        if mscc.est_lib_len:
            _mark(ax, mscc.est_lib_len, "blue", upper - height / 10, "estimated lib len: {}".format(mscc.est_lib_len))
        ax.legend(loc="best")
    lib = first.expected.fragment_length
    if lib:
        _mark(ax, lib, "green", upper - height / 6, "expected lib len: {}".format(lib))
    return fig


# ---- the document --------------------------------------------------------------------------------------------------

def figure_pages(stats: GenomeStats, name: Optional[str]) -> list:
    """The pages of the PDF, in order, as matplotlib ``Figure`` objects (nothing is written)."""
    pages: List = []
    ncc, mscc = stats.whole_ncc, stats.whole_mscc
    if ncc is not None:
        pages.append(ncc_page(ncc, name))
    if mscc is not None:
        if ncc is not None and mscc.est_lib_len * 2 < len(ncc.cc):
            pages.append(ncc_page(ncc, name, (0, mscc.est_lib_len * 2)))
        pages.append(mscc_page(mscc, name, stats.params.smooth_window))
        page = comparison_page(ncc, mscc, "Naive CC vs MSCC")
        if page is not None:
            pages.append(page)
    for chrom in sorted(set(stats.ncc) | set(stats.mscc)):
        page = comparison_page(stats.ncc.get(chrom), stats.mscc.get(chrom),
                               _title("{} Cross-Correlation".format(chrom), name))
        if page is None:
            logger.debug("Skip the plot of %s: no usable reads.", chrom)
            continue
        pages.append(page)
    return pages


def write_pdf(path, stats: GenomeStats, name: Optional[str]) -> Path:
    """Writes the pages of ``figure_pages`` to ``path``, one per PDF page; returns the path."""
    from matplotlib.backends.backend_pdf import PdfPages
    path = Path(path)
    logger.info("Output '{}'".format(path))
    pages = figure_pages(stats, name)
    with PdfPages(os.fspath(path), metadata={"CreationDate": None}) as pdf:
        for fig in pages:
            pdf.savefig(fig)
    return path
