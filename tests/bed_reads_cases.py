"""TEST INFRASTRUCTURE: BED read files (tagAlign) -- the golden reads written as tagAlign lines, plain / gzip / BGZF copies, a
shuffled copy and its stably sorted twin, the chromosome sizes, and the line-rule cases with the line they must name."""
import csv
import gzip
import os
import random

import numpy as np

from . import fixtures as fx
from . import io_writers as W

GOLD = os.path.join(fx.GOLDEN, "ENCFF000RMB-test")
STEM = "ENCFF000RMB-test"


def golden_sizes():
    """[(name, length)] of the golden BAM's header, in its order."""
    out = []
    for line in open(GOLD + ".refs.tsv").read().splitlines():
        n, v = line.split("\t")
        out.append((n, int(v)))
    return out


def golden_lines():
    """The golden reads as tagAlign lines: chrom, pos - 1, pos - 1 + qlen, N, mapq, strand (flags are 0 / 16 only)."""
    out = []
    with open(GOLD + ".reads.tsv", newline="") as fh:
        for r in csv.DictReader(fh, dialect="excel-tab"):
            flag = int(r["flag"])
            assert flag in (0, 16) and r["rname"] != "*"
            b = int(r["pos"]) - 1
            out.append("{}\t{}\t{}\tN\t{}\t{}\n".format(r["rname"], b, b + int(r["qlen"]), r["mapq"], "-" if flag & 16 else "+"))
    return out


def stable_sorted(lines, names):
    """The read lines in (reference in `names` order, start) order, ties in their order: what the readers deliver."""
    ids = {n: i for i, n in enumerate(names)}
    keyed = [l for l in lines if l.strip() and not l.startswith(("#", "track", "browser"))]
    return sorted(keyed, key=lambda l: (ids[l.split()[0]], int(l.split()[1])))


def write_sizes(path, sizes):
    with open(path, "w") as fh:
        fh.write("".join("{}\t{}\n".format(n, v) for n, v in sizes))
    return str(path)


def write_copies(directory, stem, text: bytes, bgzf_block=3000):
    """plain, gzip (two members) and BGZF copies of `text`: {kind: path}."""
    d = str(directory)
    half = len(text) // 2
    paths = {"plain": os.path.join(d, stem + ".tagAlign"), "gzip": os.path.join(d, stem + ".tagAlign.gz"),
             "bgzf": os.path.join(d, stem + ".bgzf.tagAlign.bgz")}
    open(paths["plain"], "wb").write(text)
    open(paths["gzip"], "wb").write(gzip.compress(text[:half]) + gzip.compress(text[half:]))
    open(paths["bgzf"], "wb").write(W.bgzf_compress(text, block=bgzf_block))
    return paths


def shuffled(lines, seed=1):
    out = list(lines)
    random.Random(seed).shuffle(out)
    return out


def tie_lines():
    """Reads with equal starts on both strands and different lengths and MAPQs, in an order that a sort must keep per start."""
    return ["chr2\t500\t536\ta\t30\t-\n", "chr1\t100\t136\tb\t30\t+\n", "chr1\t100\t130\tc\t20\t+\n",
            "chr1\t100\t140\td\t.\t-\n", "chr2\t500\t520\te\t1000\t+\n", "chr1\t50\t86\tf\t0\t-\n",
            "chr1\t100\t136\tg\t7\t-\n", "chr2\t500\t536\th\t30\t+\n", "chr1\t100\t101\ti\t255\t+\n"]


TIE_SIZES = [("chr1", 10000), ("chr2", 20000)]

# (name, text, the 1-based line named, a word of the reason); sizes TIE_SIZES
ERROR_CASES = [
    ("unknown_chrom", "chr1\t1\t5\tn\t0\t+\nchrX\t1\t5\tn\t0\t+\n", 2, "chrom"),
    ("end_le_start", "chr1\t1\t5\tn\t0\t+\n\nchr1\t5\t5\tn\t0\t+\n", 3, "end"),
    ("bad_strand", "chr1\t1\t5\tn\t0\t.\n", 1, "strand"),
    ("bad_score", "chr1\t1\t5\tn\t0\t+\nchr1\t1\t5\tn\t1.5\t-\n", 2, "score"),
    ("negative_score", "chr1\t1\t5\tn\t-1\t+\n", 1, "score"),
    ("five_fields", "# c\nchr1\t1\t5\tn\t0\n", 2, "fields"),
    ("start_2_31", "chr1\t2147483648\t2147483649\tn\t0\t+\n", 1, "2^31"),
    ("end_2_31", "chr1\t0\t2147483648\tn\t0\t+\n", 1, "2^31"),
    ("span_2_28", "chr1\t0\t268435456\tn\t0\t+\n", 1, "2^28"),
    ("negative_start", "chr1\t-1\t5\tn\t0\t+\n", 1, "2^31"),
    ("late_track", "chr1\t1\t5\tn\t0\t+\ntrack name=x\n", 2, "track"),
    ("second_track", "track name=x\nbrowser position chr1\ntrack name=y\nchr1\t1\t5\tn\t0\t+\n", 3, "track"),
    ("first_error_wins", "chr1\t1\t5\tn\t0\t+\nchr1\t1\t5\tn\t0\t*\nchrZ\t1\t5\tn\t0\t+\n", 2, "strand"),
]

# accepted: comments, browser and one leading track line, CRLF, spaces, extra fields, no final newline
ACCEPTED_TEXT = ("track name=reads description=\"x y\"\r\n# a comment\r\nbrowser position chr1:1-100\r\n"
                 "chr1  10 46   r1 30  +   extra\tfields\r\n\r\n   \r\nchr1\t5\t41\tr2\t.\t-\r\n#\r\nchr2\t0\t36\tr3\t0\t+")


def synthetic_lines(rng: np.random.Generator, n: int, nref: int, big=True):
    """n reads over nref chromosomes (names c0..), starts up to near 2^31 on the first few when `big`; returns (sizes, lines)."""
    lens = rng.integers(50_000, 2_000_000, size=nref)
    if big:
        lens[: min(3, nref)] = 2147483000
    sizes = [("c{}".format(i), int(v)) for i, v in enumerate(lens)]
    ref = rng.integers(0, nref, size=n)
    span = rng.integers(20, 120, size=n)
    start = (rng.random(n) * (lens[ref] - span)).astype(np.int64)
    mapq = rng.integers(0, 60, size=n)
    strand = rng.integers(0, 2, size=n)
    # a few exact ties
    k = n // 50
    start[-k:] = start[:k]
    ref[-k:] = ref[:k]
    lines = ["c{}\t{}\t{}\tN\t{}\t{}\n".format(r, s, s + l, q, "-" if st else "+")
             for r, s, l, q, st in zip(ref.tolist(), start.tolist(), span.tolist(), mapq.tolist(), strand.tolist())]
    return sizes, lines
