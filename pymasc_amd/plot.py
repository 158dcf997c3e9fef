"""The ``pymasc-plot`` command: ``python -m pymasc_amd.plot out/sample -s hg38.chrom.sizes -m hg38_36mer_mappability.json``.

Redraws a run's figure and recomputes its ``_stats.tab`` from the tables the run saved, with the statistics options of this
call (PyMaSC's plot.py; options and defaults from utils/parsearg.py ``get_plot_parser``).  No alignment file, no track and no
GPU is read: ``_cc.tab`` / ``_mscc.tab`` hold the per-chromosome curves, ``_nreads.tab`` the read counts, ``-s`` the
chromosome lengths (a ``.chrom.sizes`` / ``.fai`` file, or the header of a BAM or SAM file through the host readers) and the
JSON cache of ``-m`` the mappable lengths by lag.  From them the per-chromosome results are rebuilt (``NCCResult`` /
``MSCCResult`` with their ``cc`` set from the tables) and handed to ``stats.genome_wide_stats``.  Writes, in
``<outdir>/<name>``: ``<name>.pdf`` (pymasc_amd.figures), ``<name>_stats.tab``, and ``<name>_cc.tab`` / ``<name>_mscc.tab``
for the tables given (their per-chromosome columns as loaded and the merged ``whole`` column).

The chromosomes are those present in every table given.  A chromosome that ``_nreads.tab`` lists with no read at all is the
reference's layout for a chromosome without reads, not a disagreement; any other difference is logged with the common set.
Every chromosome of ``-s`` that passes ``-i`` / ``-e`` and has no column counts as a chromosome without reads
(``EmptyNCCResult``), so that ``Genome length`` is what ``pymasc`` reports for the same chromosomes.

Deliberate differences from the reference:

- ``-i`` / ``-e`` take effect: the reference computes the filtered list and then uses every column.
- ``-f mscc`` takes effect: the reference checks for ``"masc"``, which is not one of the choices.
- The base path gets the suffixes appended whole (``b.sam`` -> ``b.sam_cc.tab``, as this project names its outputs); the
  reference takes the path's stem.
- ``-s`` is needed with ``--masc`` alone too: the genome length of ``_stats.tab`` comes from it either way.

Exit status 2 for argument errors, before any file is read; 1 after a critical log when a table, the cache or ``-s``
cannot be used or no chromosome has reads.  Parsing, ``--help``, ``--version`` and argument errors import neither torch, nor
matplotlib, nor the native libraries; no GPU is used at all.
"""
from __future__ import annotations

import argparse
import csv
import json
import logging
import os
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import List, Optional, Tuple

from . import cli

logger = logging.getLogger(__name__)

#: what -f can name: "all" stands for the other three
FORCE_CHOICES = ("all", "stats", "cc", "mscc")
LIBLEN_TOO_LONG = "Specified expected library length > max shift. Ignore expected length setting."     # as pymasc logs it


class PlotInputError(Exception):
    """A table, the cache or the sizes file cannot be used: logged as critical, exit status 1."""


# ---- arguments -------------------------------------------------------------------------------------------------------
def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="python -m pymasc_amd.plot",
        description="Draw the figure and recompute _stats.tab from the tables of a pymasc run, without its alignment\n"
                    "file and without a GPU.",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.shared_options(parser)

    inp = parser.add_argument_group("inputs")
    inp.add_argument("statfile", nargs="?", type=Path,
                     help="base path of the tables: fills in --stats, --cc, --masc and --nreads with <base>_stats.tab, "
                          "<base>_cc.tab, <base>_mscc.tab and <base>_nreads.tab where those files exist")
    inp.add_argument("--stats", type=Path, help="the _stats.tab file (read length, expected library length, name)")
    inp.add_argument("--cc", type=Path, help="the _cc.tab file (naive cross-correlation)")
    inp.add_argument("--masc", type=Path, help="the _mscc.tab file (mappability-sensitive cross-correlation)")
    inp.add_argument("--nreads", type=Path, help="the _nreads.tab file (read counts)")
    inp.add_argument("-s", "--sizes", type=Path,
                     help="chromosome lengths: a tab-separated name / length file (.chrom.sizes, .fai) or a BAM or SAM "
                          "file (plain or bgzip'd), whose header is read")
    inp.add_argument("-m", "--mappability-stats", type=Path,
                     help="the mappable-length cache (JSON) of the track; a path not ending in .json is taken as the "
                          "track, whose cache is <track without extension>_mappability.json")

    cli.chromfilter_options(parser.add_argument_group("chromosomes"))
    cli.stats_options(parser.add_argument_group("statistics"))

    out = parser.add_argument_group("outputs")
    out.add_argument("-n", "--name", help="base name of the outputs (default: the Name row of the stats file)")
    out.add_argument("-o", "--outdir", default=".", type=Path,
                     help="directory the outputs are written to, created if missing (default .)")
    out.add_argument("-f", "--force-overwrite", nargs="*", type=str.lower, choices=FORCE_CHOICES, default=[],
                     help="write these outputs even where they would replace their own input: all, stats, cc, mscc")
    return parser


def parse_args(argv=None) -> argparse.Namespace:
    """The options, completed from the base path and checked without reading any file (exit 2 on an error)."""
    from .mappability import default_stats_path
    from .stats import STATS_SUFFIX
    from .tables import CC_SUFFIX, MSCC_SUFFIX, NREADS_SUFFIX

    parser = get_parser()
    args = parser.parse_args(argv)
    if args.statfile is not None:
        for attr, suffix in (("stats", STATS_SUFFIX), ("cc", CC_SUFFIX), ("masc", MSCC_SUFFIX),
                             ("nreads", NREADS_SUFFIX)):
            path = Path(str(args.statfile) + suffix)
            if getattr(args, attr) is None and path.exists():
                setattr(args, attr, path)

    if args.stats is None:
        parser.error("no statistics file: give a base path or --stats")
    if args.nreads is None:
        parser.error("no read-count table: give a base path or --nreads")
    if args.cc is None and args.masc is None:
        parser.error("neither a cross-correlation table (--cc) nor a mappability-sensitive one (--masc)")
    for opt, path in (("--stats", args.stats), ("--nreads", args.nreads), ("--cc", args.cc), ("--masc", args.masc)):
        if path is not None and not path.is_file():
            parser.error("argument {}: no such file: '{}'".format(opt, path))
    if args.sizes is None:
        parser.error("the chromosome lengths are needed: give -s/--sizes")
    if not args.sizes.is_file():
        parser.error("argument -s/--sizes: no such file: '{}'".format(args.sizes))
    if args.masc is not None:
        if args.mappability_stats is not None and not args.mappability_stats.name.endswith(".json"):
            args.mappability_stats = default_stats_path(args.mappability_stats)
        if args.mappability_stats is None or not args.mappability_stats.is_file():
            parser.error("--masc needs the mappable-length cache of the track: give -m/--mappability-stats "
                         "(no such file: '{}')".format(args.mappability_stats))
    if args.name is not None and not _file_name(args.name):
        parser.error("argument -n/--name: an output name is a file name: {!r}".format(args.name))
    args.force_overwrite = set(FORCE_CHOICES[1:]) if "all" in args.force_overwrite else set(args.force_overwrite)
    return args


def _file_name(name: str) -> bool:
    return bool(name) and os.sep not in name and not (os.altsep and os.altsep in name) and name not in (".", "..")


# ---- inputs ----------------------------------------------------------------------------------------------------------
def load_chrom_sizes(path) -> dict:
    """name -> length, in file order: the header of a BAM or SAM file (plain or bgzip'd), else the first two tab-separated
    columns of each line of a text file (``.chrom.sizes``, ``.fai``).  PlotInputError when neither can be read."""
    path = os.fspath(path)
    try:
        with open(path, "rb") as fh:
            head = fh.read(2)
    except OSError as e:
        raise PlotInputError("cannot read '{}': {}".format(path, e))
    if head[:1] == b"@" or head == b"\x1f\x8b":             # SAM text, or BGZF: a BAM file or a bgzip'd SAM file
        from . import inputs
        from .bam import PmxIOError
        try:
            with inputs.open_header(path) as reader:
                sizes = dict(zip(reader.references, reader.lengths))
        except (PmxIOError, OSError) as e:
            raise PlotInputError("cannot read the header of '{}': {}".format(path, e))
        if not sizes:
            raise PlotInputError("the header of '{}' names no chromosome".format(path))
        return sizes
    sizes = {}
    try:
        with open(path) as fh:
            for n, line in enumerate(fh, 1):
                if not line.strip():
                    continue
                cols = line.rstrip("\r\n").split("\t")
                try:
                    length = int(cols[1])
                except (IndexError, ValueError):
                    raise PlotInputError("'{}' line {}: not a chromosome name and a length: {!r}".format(path, n, line))
                if not cols[0] or length < 0:
                    raise PlotInputError("'{}' line {}: not a chromosome name and a length: {!r}".format(path, n, line))
                sizes[cols[0]] = length
    except (OSError, UnicodeDecodeError) as e:
        raise PlotInputError("cannot read '{}': {}".format(path, e))
    if not sizes:
        raise PlotInputError("'{}' names no chromosome".format(path))
    return sizes


def _load_cc(path) -> dict:
    from . import tables
    try:
        cols = tables.load_cc_table(path)
    except (OSError, ValueError, IndexError, csv.Error) as e:
        raise PlotInputError("cannot parse '{}': {}".format(path, e))
    if not cols or not next(iter(cols.values())):
        raise PlotInputError("'{}' holds no chromosome column or no shift".format(path))
    return cols


def _load_nreads(path):
    from . import tables
    try:
        return tables.load_nreads_table(path, whole=True)
    except (OSError, ValueError, IndexError, KeyError, csv.Error) as e:
        raise PlotInputError("cannot parse '{}': {}".format(path, e))


def _load_lag_tables(path) -> dict:
    try:
        with open(path) as fh:
            refs = json.load(fh)["references"]
    except (OSError, ValueError, KeyError, TypeError) as e:
        raise PlotInputError("cannot read the mappable lengths of '{}': {!r}".format(path, e))
    if not isinstance(refs, dict):
        raise PlotInputError("'{}': 'references' is not an object".format(path))
    return refs


def _summary(path):
    """(name, read length, expected library length or None) of a ``_stats.tab`` file."""
    from . import stats
    try:
        rows = stats.load_stats(path)
        name = rows["Name"]
        read_len = int(rows["Read length"])
        lib = rows["Expected library length"]
        lib = None if lib == "nan" else int(lib)
    except (OSError, ValueError, KeyError) as e:
        raise PlotInputError("cannot read the statistics file '{}': {!r}".format(path, e))
    if not _file_name(name):
        raise PlotInputError("'{}': the Name row {!r} is not a file name".format(path, name))
    if read_len < 1:
        raise PlotInputError("'{}': read length {} is not positive".format(path, read_len))
    return name, read_len, lib


# ---- the rebuilt result ----------------------------------------------------------------------------------------------
def _common_chroms(cc, masc, fw, rv, mfw, mrv):
    """The chromosomes of every table given, sorted; a warning when the tables disagree.  Mappable read counts without
    per-chromosome columns (only ``whole``) leave the MSCC columns unconstrained."""
    sets, counted = [], set()
    if cc is not None:
        sets.append(set(cc))
        counted |= {c for c in fw if fw[c] or rv.get(c)}
        sets.append(set(fw) & set(rv))
    if masc is not None:
        sets.append(set(masc))
        if mfw:
            counted |= {c for c in mfw if any(mfw[c]) or any(mrv.get(c, ()))}
            sets.append(set(mfw) & set(mrv))
    common = set.intersection(*sets)
    columns = set().union(*(set(t) for t in (cc, masc) if t is not None))
    if (columns | counted) - common:
        logger.warning("Chromosome names in the tables differ; using the ones they share: {}".format(sorted(common)))
    return sorted(common)


@dataclass
class Rebuilt:
    """What ``rebuild_result`` returns.  ``mscc_reads``: the genome-wide (forward, reverse) mappable read counts by shift,
    for ``stats.genome_wide_stats``, when ``_nreads.tab`` has them only in its ``whole`` column (``pymasc --skip-ncc``
    writes it so, as PyMaSC does); the per-chromosome MSCC results then hold zero counts.  None otherwise."""
    result: object
    used: List[str]
    mscc_reads: Optional[Tuple[object, object]] = None


def rebuild_result(read_len, sizes, cc=None, masc=None, nreads=None, lag_tables=None, chromfilter=None) -> Rebuilt:
    """The genome-wide result the tables stand for: ``NCCResult`` / ``MSCCResult`` per chromosome with ``cc`` set from the
    table columns, placeholders for the chromosomes of ``sizes`` without a column.  ``nreads``: what
    ``tables.load_nreads_table(path, whole=True)`` returns.  PlotInputError for a chromosome missing from ``sizes`` or
    ``lag_tables``, for counts missing from ``nreads`` and for tables that disagree in length."""
    import numpy as np
    from . import result as R
    from .chromfilter import NoTargetChromosomesError, filter_references

    fw, rv, mfw, mrv = (dict(d) for d in nreads)
    for d in (fw, rv):
        d.pop("whole", None)
    whole_m = (mfw.pop("whole", None), mrv.pop("whole", None))
    nshift = {len(next(iter(t.values()))) for t in (cc, masc) if t is not None}
    if len(nshift) != 1:
        raise PlotInputError("the correlation tables do not cover the same shifts")
    nshift = nshift.pop()
    max_shift = nshift - 1
    if read_len > nshift:
        raise PlotInputError("read length {} is longer than the tables' {} shifts".format(read_len, nshift))

    try:
        used = filter_references(_common_chroms(cc, masc, fw, rv, mfw, mrv), chromfilter)
    except NoTargetChromosomesError:
        used = []
    for c in used:
        if c not in sizes:
            raise PlotInputError("chromosome '{}' is not in the chromosome sizes".format(c))
        if masc is not None and c not in lag_tables:
            raise PlotInputError("chromosome '{}' is not in the mappable-length cache".format(c))

    mscc_reads = None
    if masc is not None and not mfw:
        if whole_m[0] is None or whole_m[1] is None:
            raise PlotInputError("the read-count table has no mappable read counts")
        if len(whole_m[0]) < nshift or len(whole_m[1]) < nshift:
            raise PlotInputError("the mappable read counts are shorter than the table")
        mscc_reads = tuple(np.asarray(x[:nshift], dtype=np.int64) for x in whole_m)
        zeros = [0] * nshift
        mfw = mrv = {c: zeros for c in used}

    ncc_rows, mscc_rows = {}, {}
    for c in used:
        if cc is not None:
            r = R.NCCResult(max_shift=max_shift, read_len=read_len, genomelen=int(sizes[c]), forward_sum=int(fw[c]),
                            reverse_sum=int(rv[c]), forward_read_len_sum=None, reverse_read_len_sum=None, ccbins=None)
            r.cc = np.asarray(cc[c], dtype=np.float64)
            ncc_rows[c] = r
        if masc is not None:
            lag = tuple(int(x) for x in lag_tables[c])
            if len(mfw[c]) < nshift or len(mrv[c]) < nshift or len(lag) < read_len:
                raise PlotInputError("the read counts or mappable lengths of '{}' are shorter than the table".format(c))
            r = R.MSCCResult(max_shift=max_shift, read_len=read_len, genomelen=int(sizes[c]),
                             forward_sum=np.asarray(mfw[c][:nshift], dtype=np.int64),
                             reverse_sum=np.asarray(mrv[c][:nshift], dtype=np.int64), forward_read_len_sum=None,
                             reverse_read_len_sum=None, ccbins=None, mappable_len=lag)
            r.cc = np.asarray(masc[c], dtype=np.float64)
            mscc_rows[c] = r

    # chromosomes without a column: counted in the genome length as pymasc counts chromosomes without reads
    try:
        kept = filter_references(list(sizes), chromfilter)
    except NoTargetChromosomesError:
        kept = []
    for c in kept:
        if c in ncc_rows or c in mscc_rows:
            continue
        if cc is not None:
            ncc_rows[c] = R.EmptyNCCResult.create_empty(int(sizes[c]), max_shift, read_len)
        if masc is not None:
            mscc_rows[c] = R.EmptyMSCCResult.create_empty(int(sizes[c]), max_shift, read_len)

    genomelen = sum(int(sizes[c]) for c in set(ncc_rows) | set(mscc_rows))
    fsum = sum(int(fw[c]) for c in used) if cc is not None else 0
    rsum = sum(int(rv[c]) for c in used) if cc is not None else 0
    if cc is not None and masc is not None:
        result = R.BothGenomeWideResult(genomelen, None, None, fsum, rsum, ncc_rows, mscc_rows)
    elif cc is not None:
        result = R.NCCGenomeWideResult(genomelen, None, None, fsum, rsum, ncc_rows)
    else:
        result = R.MSCCGenomeWideResult(genomelen, None, None, mscc_rows)
    return Rebuilt(result, used, mscc_reads)


# ---- outputs ---------------------------------------------------------------------------------------------------------
def _writable(source, output: Path, key: str, force) -> bool:
    """False (with a warning) when ``output`` is the input ``source`` itself and -f does not name ``key``."""
    if source is None or Path(source).resolve() != output.resolve():
        return True
    if key in force:
        logger.warning("-f {}: the input '{}' will be overwritten.".format(key, output))
        return True
    logger.warning("'{}' is an input: not overwritten; -f {} writes it.".format(output, key))
    return False


def main(argv=None) -> int:
    try:
        args = parse_args(argv)
    except SystemExit as e:         # --help, --version, argument errors
        return e.code if isinstance(e.code, int) else 2
    cli.setup_logging(args.log_level)
    cli.log_version()

    from . import figures, stats, tables
    from .exceptions import ReadsTooFew
    try:
        name, read_len, library_length = _summary(args.stats)
        sizes = load_chrom_sizes(args.sizes)
        cc = _load_cc(args.cc) if args.cc is not None else None
        masc = _load_cc(args.masc) if args.masc is not None else None
        nreads = _load_nreads(args.nreads)
        lag_tables = _load_lag_tables(args.mappability_stats) if masc is not None else None
        rebuilt = rebuild_result(read_len, sizes, cc, masc, nreads, lag_tables, args.chromfilter)
    except PlotInputError as e:
        logger.critical("Failed to load the tables: {}".format(e))
        return 1

    name = args.name or name
    if args.library_length is not None:
        library_length = args.library_length
    max_shift = len(next(iter((cc or masc).values()))) - 1
    if library_length is not None and library_length > max_shift:
        logger.error(LIBLEN_TOO_LONG)
        library_length = None
    try:
        gstats = stats.genome_wide_stats(rebuilt.result, read_len, library_length, args.smooth_window,
                                         args.bg_avr_width, args.mask_size, args.chi2_pval, mscc_reads=rebuilt.mscc_reads)
    except (ReadsTooFew, ValueError) as e:
        logger.critical("Failed to process the tables: {}".format(e))
        return 1

    base = args.outdir / name
    try:
        args.outdir.mkdir(parents=True, exist_ok=True)
        if _writable(args.stats, Path(str(base) + stats.STATS_SUFFIX), "stats", args.force_overwrite):
            stats.write_stats(base, gstats)
        used = rebuilt.used
        ts = tables.TableSet(None if gstats.whole_ncc is None else gstats.whole_ncc.cc,
                             {c: cc[c] for c in used} if cc is not None else {},
                             None if gstats.whole_mscc is None else gstats.whole_mscc.cc,
                             {c: masc[c] for c in used} if masc is not None else {},
                             None, None, tuple(used))
        # the table writers name a table after the stem of the path they are given: a suffix keeps a dotted name whole
        table_path = Path(str(base) + ".tab")
        if cc is not None and _writable(args.cc, Path(str(base) + tables.CC_SUFFIX), "cc", args.force_overwrite):
            tables.write_cc_table(table_path, ts)
        if masc is not None and _writable(args.masc, Path(str(base) + tables.MSCC_SUFFIX), "mscc",
                                          args.force_overwrite):
            tables.write_mscc_table(table_path, ts)
        figures.write_pdf(Path(str(base) + figures.PDF_SUFFIX), gstats, name)
    except OSError as e:
        logger.critical("Failed to write the outputs: {}".format(e))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
