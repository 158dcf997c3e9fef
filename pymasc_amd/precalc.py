"""The ``pymasc-precalc`` command: ``python -m pymasc_amd.precalc -m track.bw -d 1000 -r 1000``.

Writes the mappable-length cache (``<track>_mappability.json`` or ``--mappability-stats``) that ``pymasc`` runs load, as
PyMaSC's calcmappablelen.py does: ``MappabilityStats`` computes the lag tables of every chromosome and saves them.  The cache
is looked up with the host reader of the track (its header is all that takes); a valid cache that already covers the range
is left as it is and no GPU is touched.  Otherwise the track is read by the device reader when there is a GPU.  ``-p`` is
accepted and ignored: the lag tables come from one GPU.
"""
from __future__ import annotations

import argparse
import logging
import sys

from . import cli

logger = logging.getLogger(__name__)


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="python -m pymasc_amd.precalc",
        description="Compute the mappable length of every chromosome of a track at every shift, and save it as the\n"
                    "JSON cache that `python -m pymasc_amd -m <track>` loads.",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.shared_options(parser)
    cli.ranks_option(parser.add_argument_group("how to run"))
    cli.track_options(parser.add_argument_group("mappability"))
    lags = parser.add_argument_group("lag range")
    cli.shift_option(lags)
    lags.add_argument("-r", "--max-readlen", type=int, default=1000, action=cli._NaturalNumber,
                      help="longest read length the cache has to serve (default 1000)")
    return parser


def main(argv=None) -> int:
    parser = get_parser()
    try:
        args = parser.parse_args(argv)
        if not args.mappability:
            parser.error("argument -m/--mappable: expected 1 argument(s)")
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
    try:
        try:
            opened.append(inputs.open_track(track_path, False))
        except OSError as e:
            logger.critical("Cannot open the mappability track '{}': {}".format(track_path, e))
            return 1
        stats = MappabilityStats(opened[0], max_shift=args.max_shift, readlen=args.max_readlen,
                                 map_path=None if args.mappability_stats is None else str(args.mappability_stats),
                                 track_path=track_path)
        try:
            if not stats.is_called:             # no valid cache: the intervals are read on the GPU when there is one
                if inputs.default_device_ingest(1):
                    try:
                        opened.append(inputs.open_track(track_path, True))
                    except OSError as e:
                        logger.critical("Cannot open the mappability track '{}' on the GPU: {}".format(track_path, e))
                        return 1
                    stats.feeder = opened[-1]
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


if __name__ == "__main__":
    sys.exit(main())
