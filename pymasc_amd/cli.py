"""The ``pymasc`` command: ``python -m pymasc_amd reads... -m track.bw -d 1000 ...``.

The options, their defaults and their checks are PyMaSC's (utils/parsearg.py ``get_pymasc_parser``, pymasc.py ``_parse_args``);
the run is one ``pipeline.run_files`` call with ``stats=True``.  ``-p N`` is N ranks, one per GPU: without a
launcher the command starts them itself (``launch.spawn_ranks``) and never touches a GPU; under torchrun (``WORLD_SIZE`` set)
each process is one rank.

Parsing, ``--help``, ``--version``, argument errors and the ``-p N`` parent import neither torch nor the native libraries:
``pipeline`` is imported only in the process that does the work.
"""
from __future__ import annotations

import argparse
import logging
import os
import signal
import sys
from itertools import zip_longest
from pathlib import Path
from typing import Optional

from . import __version__, launch

logger = logging.getLogger(__name__)

READLEN_ESTIMATORS = ("MEAN", "MEDIAN", "MODE", "MIN", "MAX")     # pymasc_amd.readlen.ESTIMATORS
LOG_LEVELS = ("DEBUG", "INFO", "WARNING", "ERROR", "CRITICAL")
NO_FILE_LEFT = "no input file is left to run"                     # pipeline.run_files' ValueError after step 2
TRACK_ERRORS = ("BWIOError", "JSONIOError")
DIST_BACKEND_ENV = "PMX_DIST_BACKEND"
_log_handler = None                 # the root handler setup_logging installed


# ---- parser pieces shared with pymasc_amd.precalc and pymasc_amd.plot ------------------------------------------------
class _NaturalNumber(argparse.Action):
    """An int option that must be at least 1: an argparse error (exit 2) otherwise."""

    def __call__(self, parser, namespace, values, option_string=None):
        if values < 1:
            parser.error("argument {} must be > 0.".format("/".join(self.option_strings)))
        setattr(namespace, self.dest, values)


class _Extend(_NaturalNumber):
    """--coverage-extend: a natural number, or one of the words ``_extend`` lets through."""

    def __call__(self, parser, namespace, values, option_string=None):
        if isinstance(values, str):
            setattr(namespace, self.dest, values)
        else:
            super().__call__(parser, namespace, values, option_string)


def _extend(text: str):
    """``auto`` / ``read`` / ``pair`` as they are, anything else as an int (argparse reports what is neither)."""
    return text if text in ("auto", "read", "pair") else int(text)


class _LogLevel(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, getattr(logging, values))


class _Color(argparse.Action):
    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values == "TRUE")


def _chromfilter_action(include: bool):
    """-i / -e: append ``(include, [patterns])`` to the one ordered ``chromfilter`` list (pymasc_amd.chromfilter)."""
    class _Append(argparse.Action):
        def __call__(self, parser, namespace, values, option_string=None):
            groups = list(getattr(namespace, self.dest) or [])
            groups.append((include, list(values)))
            setattr(namespace, self.dest, groups)
    return _Append


def shared_options(parser: argparse.ArgumentParser) -> None:
    """-v, --disable-progress, --color and --version: the options every command takes."""
    parser.add_argument("-v", "--log-level", type=str.upper, choices=LOG_LEVELS, default=logging.INFO, action=_LogLevel,
                        help="lowest level of the messages printed on stderr (default INFO)")
    parser.add_argument("--disable-progress", action="store_true", help="accepted for compatibility; nothing to disable")
    parser.add_argument("--color", type=str.upper, choices=("TRUE", "FALSE"), default=True, action=_Color,
                        help="accepted for compatibility; messages are printed without colour")
    parser.add_argument("--version", action="version", version="pymasc_amd " + __version__)


def ranks_option(group) -> None:
    group.add_argument("-p", "--process", type=int, default=1, action=_NaturalNumber,
                       help="how many ranks to run, each on a GPU of its own (default 1)")


def track_options(group) -> None:
    group.add_argument("-m", "--mappability", metavar="TRACK", type=Path,
                       help="mappability track: BigWig, bigBed (every interval counts as 1), or bedGraph / BED / WIG text, "
                            "plain or gzip / bgzip-compressed; "
                            "positions with a value of at least 1 count as mappable; or a genome FASTA "
                            "(.fa / .fasta / .fna / .fas, optionally .gz / .bgz), whose exact k-mer uniqueness track "
                            "is computed with k = the read length")
    group.add_argument("--mappability-stats", metavar="JSON", type=Path,
                       help="where the mappable-length cache is read and written (default: the track's path with "
                            "_mappability.json in place of its extension)")


def exclude_option(group) -> None:
    group.add_argument("--exclude-regions", metavar="BED", type=Path,
                       help="leave out the regions of this BED file (plain or gzip / bgzip-compressed; ENCODE's blacklist): reads "
                            "that overlap one are dropped before the correlation, and the mappability track is cleared where a "
                            "read would touch one; the mappable-length cache is then <track>_<BED name>_mappability.json")


def missing_exclude_file(args) -> Optional[str]:
    """The argparse message for an --exclude-regions file that does not exist, or None."""
    if args.exclude_regions is not None and not os.path.isfile(args.exclude_regions):
        return "argument --exclude-regions: no such file: '{}'".format(args.exclude_regions)
    return None


def shift_option(group) -> None:
    group.add_argument("-d", "--max-shift", type=int, default=1000, action=_NaturalNumber,
                       help="largest strand shift, in bases, the correlation is computed for (default 1000)")


def stats_options(group) -> None:
    """-l, --chi2-pval, -w, --mask-size and --bg-avr-width: the options of ``stats.genome_wide_stats``."""
    group.add_argument("-l", "--library-length", type=int, action=_NaturalNumber,
                       help="fragment length you expect; _stats.tab reports the correlation there too")
    group.add_argument("--chi2-pval", type=float, default=0.05,
                       help="significance level of the test for unequal forward and reverse read counts (default 0.05)")
    group.add_argument("-w", "--smooth-window", type=int, default=15, action=_NaturalNumber,
                       help="width of the moving average applied to the masked curve before its peak is sought "
                            "(default 15)")
    group.add_argument("--mask-size", type=int, default=5,
                       help="when the peak lies this close to the read length, hide that neighbourhood and look again; "
                            "below 1 turns it off (default 5)")
    group.add_argument("--bg-avr-width", type=int, default=50, action=_NaturalNumber,
                       help="the background level is the median over this many of the largest shifts (default 50)")


def chromfilter_options(group) -> None:
    """-i / -e, appending to one ordered ``chromfilter`` list."""
    group.add_argument("-i", "--include-chrom", nargs="+", dest="chromfilter", metavar="PATTERN",
                       action=_chromfilter_action(True),
                       help="keep the chromosomes matching these fnmatch patterns (case-sensitive); -i and -e apply in "
                            "the order given and may repeat")
    group.add_argument("-e", "--exclude-chrom", nargs="+", dest="chromfilter", metavar="PATTERN",
                       action=_chromfilter_action(False),
                       help="drop the chromosomes matching these fnmatch patterns (case-sensitive); see -i")


def setup_logging(level: int, rank: int = 0) -> None:
    """One stderr handler on the root logger (replaced, not added to, when called again); ranks other than 0 log ERROR and
    above only, so that a run over several ranks prints one set of messages."""
    global _log_handler
    root = logging.getLogger()
    if _log_handler is not None:
        root.removeHandler(_log_handler)
    _log_handler = logging.StreamHandler(sys.stderr)
    _log_handler.setFormatter(logging.Formatter("[%(asctime)s | %(levelname)s] %(name)s : %(message)s", "%Y-%m-%d %H:%M:%S"))
    root.addHandler(_log_handler)
    root.setLevel(level if rank == 0 else max(level, logging.ERROR))


def log_version() -> None:
    logger.info("pymasc_amd version {} with Python{}.{}.{}".format(__version__, *sys.version_info[:3]))


def readable_track(path) -> bool:
    """The -m file is a readable file; logged as the reference's BWIOError is when it is not."""
    p = os.fspath(path)
    if os.path.isfile(p) and os.access(p, os.R_OK):
        return True
    reason = "no such file" if not os.path.exists(p) else ("not a file" if not os.path.isfile(p) else "not readable")
    logger.critical("Cannot read the mappability track '{}': {}".format(p, reason))
    return False


# ---- pymasc -----------------------------------------------------------------------------------------------------------
def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="python -m pymasc_amd",
        description="Strand cross-correlation of aligned reads, naive and mappability-masked, on AMD Instinct GPUs:\n"
                    "the _cc, _mscc, _nreads and _stats tables of every input file.",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    shared_options(parser)

    run = parser.add_argument_group("how to run")
    ranks_option(run)
    run.add_argument("--successive", action="store_true",
                     help="accepted for compatibility; the bit-vector path gives the same integers")
    run.add_argument("--skip-ncc", action="store_true",
                     help="write only the mappability-masked correlation (needs -m)")
    run.add_argument("--skip-plots", action="store_true",
                     help="do not log the missing figure of each file; no figure is ever drawn")

    reads = parser.add_argument_group("reads")
    reads.add_argument("reads", nargs="+", type=Path, help="BAM or SAM files (plain or bgzip'd), sorted by coordinate; '-' reads standard input, and a FIFO or /dev/fd/N "
                            "is read as a stream too (both need -r/--read-length); files named .tagAlign or .bed (optionally "
                            ".gz / .bgz) are BED read files, sorted or not (need --chrom-sizes)")
    reads.add_argument("--chrom-sizes", metavar="FILE", type=Path,
                       help="chromosome names and lengths of the BED read files, in reference order: a .chrom.sizes or .fai "
                            "file, or a BAM / SAM file whose header gives them (BAM and SAM inputs keep their own)")
    reads.add_argument("-r", "--read-length", type=int, action=_NaturalNumber,
                       help="use this read length instead of estimating one from the files")
    reads.add_argument("--readlen-estimator", type=str.upper, default="MEDIAN", choices=READLEN_ESTIMATORS,
                       help="statistic of the observed read lengths taken as the estimate, in any case (default MEDIAN)")
    reads.add_argument("-q", "--mapq", type=int, default=1,
                       help="reads with a mapping quality below this are left out (default 1)")
    chromfilter_options(reads)

    track = parser.add_argument_group("mappability")
    track_options(track)
    exclude_option(track)

    fit = parser.add_argument_group("correlation and statistics")
    shift_option(fit)
    stats_options(fit)

    out = parser.add_argument_group("outputs")
    out.add_argument("-n", "--name", nargs="*", default=[],
                     help="base names of the outputs, paired with the files in order (default: each file's stem)")
    out.add_argument("-o", "--outdir", default=".", type=Path, help="directory the tables are written to (default .)")
    out.add_argument("--complexity", action="store_true",
                     help="also write <name>_complexity.tab for every file: the library complexity NRF, PBC1 and PBC2 (ENCODE) of "
                          "the reads at -q on the chosen chromosomes, flagged duplicates kept, counted per "
                          "(chromosome, position, read length, strand), with per-chromosome counts and the multiplicity histogram")
    out.add_argument("--fingerprint", action="store_true",
                     help="also write <name>_fingerprint.tab for every file: the reads the correlation sees counted per genome bin, "
                          "the fingerprint's AUC, X-intercept and elbow, the Jensen-Shannon distance to a Poisson model, and the "
                          "number of bins at every count")
    out.add_argument("--fingerprint-bin", metavar="N", type=int, action=_NaturalNumber,
                     help="width of the genome bins, in bases (default 500); implies --fingerprint")
    out.add_argument("--fingerprint-extend", metavar="N", type=int, action=_NaturalNumber,
                     help="count every read as N bases from its 5' end instead of its own length; implies --fingerprint")
    out.add_argument("--fingerprint-control", metavar="FILE", type=Path,
                     help="an alignment file (a control / input sample) counted the same way: the table then holds the "
                          "Jensen-Shannon distance between the two; implies --fingerprint")
    out.add_argument("--peaks", metavar="FILE", type=Path,
                     help="also write <name>_peaks.tab for every file: the reads the correlation sees counted per line of this peak "
                          "file (narrowPeak, broadPeak, gappedPeak or any BED3+; plain, gzip or bgzip; the first three columns), the "
                          "fraction of reads in peaks (FRiP) and its enrichment over the share of the genome the peaks cover")
    out.add_argument("--peaks-extend", metavar="N", type=int, action=_NaturalNumber,
                     help="count every read as N bases from its 5' end instead of its own length; needs --peaks")
    out.add_argument("--coverage", action="store_true",
                     help="also write <name>_coverage.bedGraph for every file: the reads the correlation sees, each extended from "
                          "its 5' end to the estimated fragment length, piled up base by base on the GPU and written as runs of "
                          "constant depth (plain text; binning and scaling: --coverage-bin, --coverage-normalize).  The GPU table takes 4 bytes per base of the chosen "
                          "chromosomes: 12.4 GB for hg38")
    out.add_argument("--coverage-extend", metavar="N|auto|read|pair", type=_extend, action=_Extend,
                     help="extend every read to N bases from its 5' end; auto (the default): to the run's own fragment-length "
                          "estimate, on one more read of the file, so not for '-' or a pipe; read: no extension, the read's own "
                          "length; pair: instead of reads, every properly oriented (FR) pair at its own extent, from read1's mate "
                          "fields, up to --fragments-max bases; implies --coverage")
    out.add_argument("--coverage-format", choices=("bedgraph", "bigwig"),
                     help="bedgraph (the default): the text track; bigwig: <name>_coverage.bw instead, the same runs as a bigWig "
                          "file a genome browser opens, with zoom levels (count, min, max, sum and sum of squares of the depth per "
                          "bin), its sections and zoom records made on the GPU.  The depth is a 32-bit float there: exact up to "
                          "2^24 and rounded to nearest above; implies --coverage")
    out.add_argument("--coverage-compress", action="store_true",
                     help="put every section of the bigWig file through zlib (on the host); needs --coverage-format bigwig")
    out.add_argument("--coverage-deflate", choices=("host", "device"),
                     help="where the sections of the bigWig file are compressed; implies --coverage-compress, so it needs "
                          "--coverage-format bigwig.  host (what --coverage-compress alone does): zlib on host threads; device: the "
                          "GPU's own DEFLATE encoder, before the sections leave it, for inputs read by device ingest.  A section "
                          "holds 1024 items here; the device encoder takes at most 2048 items per section.  Its compressed bytes "
                          "differ from zlib's; the decoded file does not")
    out.add_argument("--coverage-bin", metavar="N", type=int, action=_NaturalNumber,
                     help="write the pileup as a signal track: the mean depth per bin of N bases (1 to 65536; default 1), a 32-bit "
                          "float, equal neighbouring bins merged into one run, made on the GPU; implies --coverage")
    out.add_argument("--coverage-normalize", choices=("none", "cpm", "rpgc"),
                     help="scale the signal track: cpm: by 10^6 / the reads piled up; rpgc: by the genome size / the bases piled up, so "
                          "that the mean depth over the genome is 1 (the genome size: --coverage-genome-size, else the chosen "
                          "chromosomes' lengths); none (the default); implies --coverage")
    out.add_argument("--coverage-scale", metavar="X", type=float,
                     help="multiply the signal track by X (above 0; default 1) on top of --coverage-normalize; implies --coverage")
    out.add_argument("--coverage-genome-size", metavar="N", type=int, action=_NaturalNumber,
                     help="the genome size of --coverage-normalize rpgc, which it needs; implies --coverage")
    out.add_argument("--coverage-control", metavar="FILE",
                     help="an alignment file (a regular file, not a stream) with the control's reads: the track is every input "
                          "against it, bin by bin (--coverage-compare), both scaled by --coverage-normalize (none: the control to "
                          "the input's number of reads), made on the GPU; its chromosomes must be the input's; implies --coverage")
    out.add_argument("--coverage-compare", choices=("log2", "ratio", "subtract"),
                     help="what the track holds with --coverage-control, which it needs: log2 (the default) or ratio of "
                          "(input + pseudocount) / (control + pseudocount), or input - control")
    out.add_argument("--coverage-pseudocount", metavar="X", type=float,
                     help="the pseudocount of --coverage-compare log2 and ratio (at least 2^-64 and below 2^40; default 1); needs "
                          "--coverage-control")
    out.add_argument("--coverage-call", metavar="X", type=float,
                     help="also write <name>_coverage_peaks.narrowPeak: the peaks of the track the coverage file holds (depth, signal or "
                          "treatment against control), called on the GPU -- runs of at least X (any finite number), linked over gaps "
                          "of at most --coverage-call-gap bases and kept from --coverage-call-length bases; the score is the track's "
                          "value, no p-value is computed, and --peaks reads the file in a second run; implies --coverage")
    out.add_argument("--coverage-call-gap", metavar="N", type=int,
                     help="the largest gap between two runs of one peak (0 .. 2^31 - 1; default 30); needs --coverage-call")
    out.add_argument("--coverage-call-length", metavar="N", type=int,
                     help="the smallest peak (1 .. 2^31 - 1; default 200); needs --coverage-call")
    out.add_argument("--coverage-poisson", action="store_true",
                     help="with --coverage-control, which it needs: the track holds -log10 of the Poisson upper tail P(X >= k | lambda) "
                          "per bin instead of a compare operation, made on the GPU: k is the input's mean depth per bin as a whole "
                          "number (the input is not scaled), lambda the largest of the control's mean over the genome, at the bin "
                          "and over the two windows of --coverage-lambda, the control scaled to the input's number of reads; "
                          "--coverage-call then thresholds the score and writes it in column 8 too.  Not with --coverage-compare, "
                          "--coverage-pseudocount, --coverage-normalize other than none or --coverage-scale other than 1")
    out.add_argument("--coverage-lambda", metavar=("S", "L"), type=int, nargs=2,
                     help="the small and the large window of --coverage-poisson around every bin, in bases (each 0 .. 2^31 - 1, 0: "
                          "off; default 1000 10000); needs --coverage-poisson")
    out.add_argument("--coverage-qvalue", action="store_true",
                     help="with --coverage-poisson and one of --coverage-call / --coverage-call-q, which it needs: the "
                          "Benjamini-Hochberg q-scores of the p-score track over every base of the chosen chromosomes, made on the "
                          "GPU; column 9 of the narrowPeak holds -log10 q of every peak.  The coverage file stays the p-score track")
    out.add_argument("--coverage-call-q", metavar="X", type=float,
                     help="call the peaks at the smallest p-score whose q-score (-log10 q) reaches X (any finite number; 2: q <= "
                          "0.01) and write both scores; needs --coverage-poisson, not with --coverage-call, implies --coverage-qvalue; "
                          "--coverage-call-gap and --coverage-call-length apply")
    out.add_argument("--gc-bias", metavar="FASTA", type=Path,
                     help="also write <name>_gcbias.tab for every file: the reads the correlation sees, each placed on the window "
                          "of this genome (FASTA; plain, gzip or bgzip) that begins at its 5' end, counted per G + C content of the "
                          "window beside the genome's windows of that content, with AT / GC dropout; windows with an N or inside "
                          "--exclude-regions are left out")
    out.add_argument("--gc-window", metavar="N", type=int, action=_NaturalNumber,
                     help="length of the genome windows, 1 to 1024 bases (default 100); needs --gc-bias")
    out.add_argument("--fragments", action="store_true",
                     help="also write <name>_fragments.tab for every paired-end file: the fragment sizes of the pairs among the reads "
                          "the correlation sees, each counted at its read1 record from that record's mate fields, with median, "
                          "spread and the histogram per orientation (FR, RF, TANDEM); not for BED / tagAlign input")
    out.add_argument("--fragments-max", metavar="N", type=int, action=_NaturalNumber,
                     help="largest fragment size counted, 1 to 65536 bases (default 2000); larger pairs are only counted as over; "
                          "implies --fragments")
    out.add_argument("--tss", metavar="BED", type=Path,
                     help="also write <name>_tss.tab for every file: the reads the correlation sees piled up around the anchor sites "
                          "of this BED6 file (plain, gzip or bgzip; a + line anchors at start + 1, a - line at end: the TSS), by "
                          "offset and by strand relative to the anchor's, with the TSS enrichment over the table's outer edges")
    out.add_argument("--tss-flank", metavar="N", type=int, action=_NaturalNumber,
                     help="bases either side of an anchor, 1 to 4095 (default 2000); needs --tss")
    out.add_argument("--tss-extend", metavar="N", type=int, action=_NaturalNumber,
                     help="count every read as N bases from its 5' end instead of its own length (1: the cut site); needs --tss")
    return parser


def check_names(paths, names) -> None:
    """pipeline._basenames' rules, without importing pipeline (it brings torch): ValueError for more names than files, an
    empty name or one with a path separator, and two files with the same base name."""
    names = list(names or [])
    if len(names) > len(paths):
        raise ValueError("{} names for {} input files".format(len(names), len(paths)))
    seen = {}
    for f, n in zip_longest(paths, names):
        if n is None:
            n = Path(f).stem
        elif not n or os.sep in n or (os.altsep and os.altsep in n) or n in (".", ".."):
            raise ValueError("an output name is a file name: {!r}".format(n))
        if n in seen:
            raise ValueError("'{}' and '{}' would both write '{}_*': give them different names".format(seen[n], f, n))
        seen[n] = f


def parse_args(argv=None) -> argparse.Namespace:
    """The options, with every check that needs no file and no log (exit 2 on an error)."""
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.skip_ncc and args.mappability is None:
        parser.error("argument --skip-ncc: needs a track (-m/--mappability)")
    stdin = sum(str(p) == "-" for p in args.reads)
    if stdin > 1:
        parser.error("argument reads: '-' (standard input) may be named once")
    if stdin and args.process > 1:
        parser.error("argument -p/--process: '-' (standard input) is read by one process: use -p 1")
    try:
        check_names([str(p) for p in args.reads], args.name)
    except ValueError as e:
        parser.error("argument -n/--name: {}".format(e))
    if args.chrom_sizes is not None and not os.path.isfile(args.chrom_sizes):
        parser.error("argument --chrom-sizes: no such file: '{}'".format(args.chrom_sizes))
    if missing_exclude_file(args):
        parser.error(missing_exclude_file(args))
    if args.fingerprint_control is not None and not os.path.isfile(args.fingerprint_control):
        parser.error("argument --fingerprint-control: no such file: '{}'".format(args.fingerprint_control))
    if args.fingerprint_bin is not None or args.fingerprint_extend is not None or args.fingerprint_control is not None:
        args.fingerprint = True
    if args.peaks_extend is not None and args.peaks is None:
        parser.error("argument --peaks-extend: needs a peak file (--peaks)")
    if args.peaks is not None and not os.path.isfile(args.peaks):
        parser.error("argument --peaks: no such file: '{}'".format(args.peaks))
    if args.coverage_bin is not None and args.coverage_bin > 65536:
        parser.error("argument --coverage-bin: the bin is {}: it must lie in [1, 65536]".format(args.coverage_bin))
    if args.coverage_scale is not None and not 0.0 < args.coverage_scale < float("inf"):
        parser.error("argument --coverage-scale: must be a finite number above 0")
    if args.coverage_genome_size is not None and args.coverage_normalize != "rpgc":
        parser.error("argument --coverage-genome-size: needs --coverage-normalize rpgc")
    if args.coverage_control is None and (args.coverage_compare is not None or args.coverage_pseudocount is not None):
        parser.error("argument --coverage-compare / --coverage-pseudocount: needs --coverage-control")
    if args.coverage_control is not None:
        if args.coverage_control == "-" or not os.path.isfile(args.coverage_control):
            parser.error("argument --coverage-control: '{}' is not a regular file".format(args.coverage_control))
        if (args.coverage_pseudocount is not None and args.coverage_compare != "subtract"
                and not 2.0 ** -64 <= args.coverage_pseudocount < 2.0 ** 40):
            parser.error("argument --coverage-pseudocount: must be a finite number of at least 2^-64 and below 2^40")
    if args.coverage_lambda is not None and not args.coverage_poisson:
        parser.error("argument --coverage-lambda: needs --coverage-poisson")
    if args.coverage_poisson:
        if args.coverage_control is None:
            parser.error("argument --coverage-poisson: needs --coverage-control")
        if args.coverage_compare is not None or args.coverage_pseudocount is not None:
            parser.error("argument --coverage-poisson: not with --coverage-compare / --coverage-pseudocount (the score is not a compare "
                         "operation)")
        if args.coverage_normalize not in (None, "none") or args.coverage_scale not in (None, 1.0):
            parser.error("argument --coverage-poisson: not with --coverage-normalize other than none or --coverage-scale other than 1 "
                         "(the input is not scaled: the score counts reads)")
        if args.coverage_lambda is not None and not all(0 <= x < 1 << 31 for x in args.coverage_lambda):
            parser.error("argument --coverage-lambda: each window must lie in [0, 2^31 - 1]")
    if args.coverage_call_q is not None:
        if args.coverage_call is not None:
            parser.error("argument --coverage-call-q: not with --coverage-call (the cutoff is the p-score whose q-score reaches X)")
        if not args.coverage_poisson:
            parser.error("argument --coverage-call-q: needs --coverage-poisson")
        if not float("-inf") < args.coverage_call_q < float("inf"):
            parser.error("argument --coverage-call-q: must be a finite number")
    if args.coverage_qvalue:
        if not args.coverage_poisson:
            parser.error("argument --coverage-qvalue: needs --coverage-poisson")
        if args.coverage_call is None and args.coverage_call_q is None:
            parser.error("argument --coverage-qvalue: needs --coverage-call or --coverage-call-q")
    if args.coverage_call is None and args.coverage_call_q is None and (args.coverage_call_gap is not None or args.coverage_call_length is not None):
        parser.error("argument --coverage-call-gap / --coverage-call-length: needs --coverage-call")
    if args.coverage_call is not None or args.coverage_call_q is not None:
        if args.coverage_call is not None and not float("-inf") < args.coverage_call < float("inf"):
            parser.error("argument --coverage-call: must be a finite number")
        if args.coverage_call_gap is not None and not 0 <= args.coverage_call_gap < 1 << 31:
            parser.error("argument --coverage-call-gap: must lie in [0, 2^31 - 1]")
        if args.coverage_call_length is not None and not 1 <= args.coverage_call_length < 1 << 31:
            parser.error("argument --coverage-call-length: must lie in [1, 2^31 - 1]")
    signal = (args.coverage_bin, args.coverage_normalize, args.coverage_scale, args.coverage_genome_size, args.coverage_control,
              args.coverage_call)
    if args.coverage_extend is not None or args.coverage_format is not None or any(x is not None for x in signal):
        args.coverage = True
    if args.coverage_deflate is not None:
        if args.coverage_format != "bigwig":
            parser.error("argument --coverage-deflate: needs --coverage-format bigwig")
        args.coverage_compress = True
    if args.coverage_compress and args.coverage_format != "bigwig":
        parser.error("argument --coverage-compress: needs --coverage-format bigwig")
    if args.coverage and args.coverage_extend in (None, "auto"):
        from .stream_device import is_stream_path
        streams = [str(p) for p in args.reads if is_stream_path(str(p))]
        if streams:
            parser.error("argument --coverage-extend: auto reads the file once more, which {} cannot be: give a number or 'read'"
                         "".format(", ".join(streams)))
    if args.fragments_max is not None:
        if args.fragments_max > 65536:
            parser.error("argument --fragments-max: max_size is {}: it must lie in [1, 65536]".format(args.fragments_max))
        args.fragments = True
    if args.tss_flank is not None and args.tss is None:
        parser.error("argument --tss-flank: needs an anchor file (--tss)")
    if args.tss_extend is not None and args.tss is None:
        parser.error("argument --tss-extend: needs an anchor file (--tss)")
    if args.tss_flank is not None and args.tss_flank > 4095:
        parser.error("argument --tss-flank: the flank is {}: it must lie in [1, 4095]".format(args.tss_flank))
    if args.tss is not None and not os.path.isfile(args.tss):
        parser.error("argument --tss: no such file: '{}'".format(args.tss))
    if args.gc_window is not None and args.gc_bias is None:
        parser.error("argument --gc-window: needs a genome (--gc-bias)")
    if args.gc_window is not None and args.gc_window > 1024:
        parser.error("argument --gc-window: the window is {}: it must lie in [1, 1024]".format(args.gc_window))
    if args.gc_bias is not None and not os.path.isfile(args.gc_bias):
        parser.error("argument --gc-bias: no such file: '{}'".format(args.gc_bias))
    if args.chrom_sizes is None:
        from .bed_reads import is_bed_reads     # (no torch, no native library)
        bed = [str(p) for p in args.reads if is_bed_reads(p)]
        if bed:
            parser.error("argument --chrom-sizes: needed by the BED read file(s) {}".format(", ".join(bed)))
    return args


def _raise_on_sigterm(signum, frame):
    raise SystemExit(128 + signum)


def main(argv=None) -> int:
    argv = list(sys.argv[1:] if argv is None else argv)
    try:
        args = parse_args(argv)
    except SystemExit as e:         # --help, --version, argument errors
        return e.code if isinstance(e.code, int) else 2
    rank = int(os.environ.get("RANK", "0"))
    setup_logging(args.log_level, rank)
    if args.mappability is not None and not readable_track(args.mappability):
        return 1
    if launch.needs_spawn(args.process):
        # the ranks are this command again, in fresh processes; a SIGTERM here (a time limit) becomes SystemExit, and
        # spawn_ranks' cleanup stops the ranks it started before the parent goes
        signal.signal(signal.SIGTERM, _raise_on_sigterm)
        return launch.spawn_ranks([sys.executable, "-m", "pymasc_amd", *argv], args.process)
    return _rank_main(args, rank)


def _rank_main(args, rank: int) -> int:
    log_version()
    if args.mappability_stats is not None and args.mappability_stats == args.mappability:
        args.mappability_stats = None
    if args.library_length is not None and args.library_length > args.max_shift:
        logger.error("Specified expected library length > max shift. Ignore expected length setting.")
        args.library_length = None
    if args.successive:
        logger.info("--successive: the bit-vector path computes the same integers as the successive algorithm; "
                    "running it.")
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if "WORLD_SIZE" in os.environ and args.process != world:
        logger.warning("-p {} but WORLD_SIZE={}: using WORLD_SIZE.".format(args.process, world))
    if world <= 1:
        return _run(args, None, rank)

    backend = os.environ.get(DIST_BACKEND_ENV, "nccl")
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    import torch
    import torch.distributed as dist
    ndev = torch.cuda.device_count()
    need = local_world if backend == "nccl" else 1          # gloo: the ranks may share devices (LOCAL_RANK % count)
    if ndev < need:                 # the same decision on every rank of the node, taken before the rendezvous
        logger.error("{} ranks on this node with the {} backend need {} GPU(s); {} visible."
                     "".format(local_world, backend, need, ndev))
        return 1
    device = local_rank if backend == "nccl" else local_rank % ndev
    if backend == "nccl":
        torch.cuda.set_device(device)
        dist.init_process_group("nccl", device_id=torch.device("cuda", device))
    else:
        dist.init_process_group(backend)
    try:
        return _run(args, device, rank)
    finally:
        dist.destroy_process_group()


def _rank0_track_error(error: BaseException) -> bool:
    """The RuntimeError that sharding.on_rank0 raises on the other ranks when rank 0's track or cache failed."""
    return isinstance(error, RuntimeError) and any("failed on rank 0 [{}:".format(n) in str(error) for n in TRACK_ERRORS)


def _run(args, device, rank: int) -> int:
    from . import pipeline
    from .mappability import BWIOError, JSONIOError
    extra = {} if args.chrom_sizes is None else {"chrom_sizes": str(args.chrom_sizes)}   # (BED read files only)
    if args.complexity:
        extra["complexity"] = True
    if args.exclude_regions is not None:
        extra["exclude_regions"] = str(args.exclude_regions)
    if args.fingerprint:
        extra["fingerprint"] = True
        for key, value in (("fingerprint_bin", args.fingerprint_bin), ("fingerprint_extend", args.fingerprint_extend),
                           ("fingerprint_control", args.fingerprint_control)):
            if value is not None:
                extra[key] = str(value) if key == "fingerprint_control" else value
    if args.peaks is not None:
        extra["peaks"] = str(args.peaks)
        if args.peaks_extend is not None:
            extra["peaks_extend"] = args.peaks_extend
    if args.coverage:
        extra["coverage"] = True
        if args.coverage_extend not in (None, "auto"):
            extra["coverage_extend"] = 0 if args.coverage_extend == "read" else args.coverage_extend
        if args.coverage_format is not None:
            extra["coverage_format"] = args.coverage_format
        if args.coverage_compress:
            extra["coverage_compress"] = "device" if args.coverage_deflate == "device" else True
        for key in ("coverage_bin", "coverage_normalize", "coverage_scale", "coverage_genome_size", "coverage_control", "coverage_compare",
                    "coverage_pseudocount", "coverage_call", "coverage_call_gap", "coverage_call_length", "coverage_call_q"):
            if getattr(args, key) is not None:
                extra[key] = getattr(args, key)
        if args.coverage_poisson:
            extra["coverage_poisson"] = True
            if args.coverage_lambda is not None:
                extra["coverage_lambda"] = tuple(args.coverage_lambda)
        if args.coverage_qvalue:
            extra["coverage_qvalue"] = True
    if args.fragments:
        extra["fragments"] = True
    if args.fragments_max is not None:          # (it also bounds a pair pileup)
        extra["fragments_max"] = args.fragments_max
    if args.tss is not None:
        extra["tss"] = str(args.tss)
        if args.tss_flank is not None:
            extra["tss_flank"] = args.tss_flank
        if args.tss_extend is not None:
            extra["tss_extend"] = args.tss_extend
    if args.gc_bias is not None:
        extra["gc_bias"] = str(args.gc_bias)
        if args.gc_window is not None:
            extra["gc_window"] = args.gc_window
    try:
        results = pipeline.run_files(
            [str(p) for p in args.reads], str(args.outdir), args.max_shift, read_len=args.read_length,
            mapq_criteria=args.mapq,
            mappability_path=None if args.mappability is None else str(args.mappability),
            mappability_stats_path=None if args.mappability_stats is None else str(args.mappability_stats),
            skip_ncc=args.skip_ncc, device=device, readlen_estimator=args.readlen_estimator,
            chromfilter=args.chromfilter, stats=True, library_length=args.library_length,
            smooth_window=args.smooth_window, mask_size=args.mask_size, bg_avr_width=args.bg_avr_width,
            chi2_pval=args.chi2_pval, names=args.name or None, **extra)
    except (BWIOError, JSONIOError, pipeline.GenomeError):
        return 1                    # logged where it was raised (mappability.MappabilityStats, pipeline._GcGenome)
    except RuntimeError as e:
        if rank == 0 or not _rank0_track_error(e):
            raise
        logger.debug(str(e))        # rank 0 logged the cause and exits 1 too
        return 1
    except ValueError as e:
        if str(e) != NO_FILE_LEFT:
            raise
        if rank == 0:               # (every rank raises it: one message)
            logger.error("No input file could be run.")
        return 1
    if not args.skip_plots:
        for f in results:
            if f.written:           # rank 0, a file that ran
                logger.error("Skip output plots '{}'".format(Path(args.outdir) / (f.basename + ".pdf")))
    if not any(f.error is None for f in results):
        if rank == 0:
            logger.error("No input file could be run.")
        return 1
    return 0
