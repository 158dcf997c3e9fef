"""The ``mapgen`` command: ``python -m pymasc_amd.mapgen genome.fa -k 36 -o genome_k36.bed[.gz]``.

Computes the exact k-mer uniqueness track of a genome FASTA -- on the GPU when there is one
(``DeviceKmerTrackReader``), else on host threads (``KmerTrackReader``) -- and writes it as BED3 in the FASTA's record order,
gzip-compressed (mtime 0: equal tracks give equal bytes) when the output name ends in ``.gz``.  Passing the written file to
``-m`` gives the tables that ``-m genome.fa`` gives.
"""
from __future__ import annotations

import argparse
import logging
import sys

from . import cli

logger = logging.getLogger(__name__)


def get_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(
        prog="python -m pymasc_amd.mapgen",
        description="Write the exact k-mer uniqueness track of a genome FASTA as BED: the positions whose k-mer occurs\n"
                    "once in the genome, on either strand.",
        formatter_class=argparse.RawDescriptionHelpFormatter)
    cli.shared_options(parser)
    parser.add_argument("fasta", metavar="GENOME", help="genome FASTA (.fa / .fasta / .fna / .fas, plain, gzip or bgzip)")
    parser.add_argument("-k", "--kmer", type=int, required=True, action=cli._NaturalNumber,
                        help="k-mer length: the read length the track serves (16 to 1024)")
    parser.add_argument("-o", "--output", metavar="BED", required=True, help="BED3 output; gzip when it ends in .gz")
    return parser


def main(argv=None) -> int:
    parser = get_parser()
    try:
        args = parser.parse_args(argv)
        if not 16 <= args.kmer <= 1024:
            parser.error("argument -k/--kmer must lie in [16, 1024].")
    except SystemExit as e:         # --help, --version, argument errors
        return e.code if isinstance(e.code, int) else 2
    cli.setup_logging(args.log_level)
    cli.log_version()
    if not cli.readable_track(args.fasta):
        return 1
    from . import inputs, kmer_track
    try:
        track = kmer_track.open_kmer_track(args.fasta, args.kmer, inputs.default_device_ingest(1))
    except (OSError, ValueError) as e:
        logger.critical("Cannot compute the k-mer track of '{}': {}".format(args.fasta, e))
        return 1
    try:
        n = kmer_track.write_bed(track, args.output)
    finally:
        track.close()
    logger.info("{} unique intervals of k = {} written to '{}'".format(n, args.kmer, args.output))
    return 0


if __name__ == "__main__":
    sys.exit(main())
