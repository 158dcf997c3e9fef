"""The ``pymasc-precalc`` command: ``python -m pymasc_amd.precalc -m track.bw -d 1000 -r 1000``.

Writes the mappable-length cache (``<track>_mappability.json`` or ``--mappability-stats``) that ``pymasc`` runs load, as
PyMaSC's calcmappablelen.py does: ``MappabilityStats`` computes the lag tables of every chromosome and saves them.  The cache
is looked up with the host reader of the track (its header is all that takes); a valid cache that already covers the range
is left as it is and no GPU is touched.  Otherwise the track is read by the device reader when there is a GPU.  ``-p`` is
accepted and ignored: the lag tables come from one GPU.
``--exclude-regions BED`` writes the cache of the masked track, ``<track>_<BED name>_mappability.json``, for reads of exactly
``-r`` bases: the cleared positions depend on the read length.
A genome FASTA (``kmer_track.is_fasta``) takes ``-r`` as the k of its k-mer track and needs it given: the default of 1000
means nothing there (an argparse error, exit 2).  Its cache is ``<stem>_k<K>_mappability.json``; the names and lengths that
check it come from ``<fasta>.fai`` or a scan of the header lines, so a valid cache costs no generation.
"""
from __future__ import annotations

import argparse
import logging
import sys

from . import cli
from .kmer_track import is_fasta

logger = logging.getLogger(__name__)


class _Given(cli._NaturalNumber):
    """-r: also notes that it was given (a genome FASTA has no use for the default)."""

    def __call__(self, parser, namespace, values, option_string=None):
        super().__call__(parser, namespace, values, option_string)
        namespace.max_readlen_given = True


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="python -m pymasc_amd.precalc",
        description="Compute the mappable length of every chromosome of a track at every shift, and save it as the\n"
                    "JSON cache that `python -m pymasc_amd -m <track>` loads.",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.shared_options(parser)
    cli.ranks_option(parser.add_argument_group("how to run"))
    track = parser.add_argument_group("mappability")
    cli.track_options(track)
    cli.exclude_option(track)
    lags = parser.add_argument_group("lag range")
    cli.shift_option(lags)
    lags.add_argument("-r", "--max-readlen", type=int, default=1000, action=_Given,
                      help="longest read length the cache has to serve (default 1000); for a genome FASTA, the k-mer "
                           "length of its track, which must be given")
    return parser


def main(argv=None) -> int:
    parser = get_parser()
    try:
        args = parser.parse_args(argv)
        if not args.mappability:
            parser.error("argument -m/--mappable: expected 1 argument(s)")
        if is_fasta(args.mappability) and not getattr(args, "max_readlen_given", False):
            parser.error("argument -r/--max-readlen: a genome FASTA needs it (the k of its k-mer track)")
        if cli.missing_exclude_file(args):
            parser.error(cli.missing_exclude_file(args))
    except SystemExit as e:         # --help, --version, argument errors
        return e.code if isinstance(e.code, int) else 2
    cli.setup_logging(args.log_level)
    cli.log_version()
    if args.mappability_stats is not None and args.mappability_stats == args.mappability:
        args.mappability_stats = None
    logger.debug("-p {} is not used: the lag tables are computed on one GPU.".format(args.process))
    if not cli.readable_track(args.mappability):
        return 1

    from . import inputs
    from .mappability import BWIOError, JSONIOError, MappabilityStats
    track_path = str(args.mappability)
    opened = []
    fasta = is_fasta(track_path)
    try:
        try:
            opened.append(_FastaSizes(track_path, args.max_readlen) if fasta else inputs.open_track(track_path, False))
        except (OSError, ValueError) as e:
            logger.critical("Cannot open the mappability track '{}': {}".format(track_path, e))
            return 1
        map_path = None if args.mappability_stats is None else str(args.mappability_stats)
        mask_path = None if args.exclude_regions is None else str(args.exclude_regions)
        masked = None if mask_path is None else args.max_readlen
        if mask_path is not None and map_path is None:      # the masked track's own cache, never the unmasked one
            from .region_mask import stats_path
            map_path = str(stats_path(track_path, mask_path, args.max_readlen if fasta else None))
        mask = []

        def feeder(t):
            """``t`` less the excluded regions, which are read when the first track needs them: a valid cache reads no mask."""
            if mask_path is None:
                return t
            from .region_mask import MaskedTrack, open_mask
            if not mask:
                mask.append(open_mask(mask_path, inputs.default_device_ingest(1)))
            return MaskedTrack(t, mask[0], masked)
        stats = MappabilityStats(opened[0], max_shift=args.max_shift, readlen=args.max_readlen, map_path=map_path,
                                 track_path=track_path, masked_read_len=masked)
        try:
            if not stats.is_called:             # no valid cache: the intervals are read on the GPU when there is one
                if fasta:                       # the k-mer track, generated now (on the GPU when there is one)
                    try:
                        opened.append(inputs.open_track(track_path, inputs.default_device_ingest(1), k=args.max_readlen))
                    except (OSError, ValueError) as e:
                        logger.critical("Cannot open the mappability track '{}': {}".format(track_path, e))
                        return 1
                    stats.feeder = opened[-1]
                elif inputs.default_device_ingest(1):
                    try:
                        opened.append(inputs.open_track(track_path, True))
                    except OSError as e:
                        logger.critical("Cannot open the mappability track '{}' on the GPU: {}".format(track_path, e))
                        return 1
                    stats.feeder = opened[-1]
                try:
                    stats.feeder = feeder(stats.feeder)
                except (OSError, ValueError) as e:
                    logger.critical("Cannot read the excluded regions '{}': {}".format(mask_path, e))
                    return 1
                stats.calc_mappability()
            stats.save_mappability_stats()
        finally:
            stats.close()
    except (BWIOError, JSONIOError):
        return 1                    # logged where it was raised
    finally:
        for t in opened:
            t.close()
    return 0


class _FastaSizes:
    """The records of a genome FASTA (``kmer_track.fasta_sizes``) and the k of its track: what checking the cache needs."""
    kind = "kmer"

    def __init__(self, path, k):
        from .kmer_track import _check_k, fasta_sizes
        self.k = _check_k(k)
        self.chromsizes = fasta_sizes(path)

    def close(self):
        pass


if __name__ == "__main__":
    sys.exit(main())
