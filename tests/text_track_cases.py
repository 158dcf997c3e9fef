"""Text mappability tracks for the reader tests (tests/test_text_track.py on the host, tests/test_gpu_text_track.py on the
device): the golden bedGraph in every compression, BED / WIG twins of its mappable intervals, synthetic tracks and the
malformed cases with the line each must name."""
import gzip
import os

import numpy as np

from . import fixtures as fx
from . import io_writers as W

BEDGRAPH = os.path.join(fx.GOLDEN, "hg19_36mer-test.bedGraph")
BIGWIG = os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig")


def golden_text() -> bytes:
    return open(BEDGRAPH, "rb").read()


def compress(data: bytes, how: str) -> bytes:
    if how == "gzip":
        return gzip.compress(data)
    if how == "bgzf":
        return W.bgzf_compress(data)
    return data


def golden_variants(d):
    """The golden bedGraph as plain text, gzip (two concatenated members) and BGZF: {kind: path}."""
    t = golden_text()
    half = t.index(b"\n", len(t) // 2) + 1
    out = {"plain": d / "hg19_36mer-test.bedGraph"}
    out["plain"].write_bytes(t)
    out["gzip"] = d / "gz" / "hg19_36mer-test.bedGraph.gz"
    out["gzip"].parent.mkdir(exist_ok=True)
    out["gzip"].write_bytes(gzip.compress(t[:half]) + gzip.compress(t[half:]))
    out["bgzf"] = d / "bgzf" / "hg19_36mer-test.bedGraph.gz"
    out["bgzf"].parent.mkdir(exist_ok=True)
    out["bgzf"].write_bytes(W.bgzf_compress(t, block=4096))
    return out


def mappable(chrom="chr1"):
    """The golden intervals with value >= 1: [(begin, end)]."""
    return [(b, e) for b, e, v in fx.load_bedgraph()[chrom] if v >= 1.0]


def bed_text() -> bytes:
    return b"".join(b"chr1\t%d\t%d\tname%d\t0\t+\n" % (b, e, i) for i, (b, e) in enumerate(mappable()))


def wig_variable_text() -> bytes:
    """variableStep blocks, one per run of equal span: "pos value" lines, pos 1-based."""
    out, span = [b"track type=wiggle_0 name=twin\n"], None
    for b, e in mappable():
        if e - b != span:
            span = e - b
            out.append(b"variableStep chrom=chr1 span=%d\n" % span)
        out.append(b"%d 1\n" % (b + 1))
    return b"".join(out)


def wig_fixed_text(gap: int) -> bytes:
    """One fixedStep block per mappable interval, its single line at start; step = span + gap."""
    out = []
    for b, e in mappable():
        out.append(b"fixedStep chrom=chr1 start=%d step=%d span=%d\n1.0\n" % (b + 1, e - b + gap, e - b))
    return b"".join(out)


FIXED_MULTI = (b"fixedStep chrom=chrA start=11 step=10 span=4\n1\n0.5\n2\n"
               b"fixedStep chrom=chrA start=101 step=3\n7\n8\n",
               [(10, 14, 1.0), (20, 24, 0.5), (30, 34, 2.0), (100, 101, 7.0), (103, 104, 8.0)])


def synthetic(seed, nchrom=5, per=400, overlap=False):
    """{chrom: [(begin, end, value)]} ascending and disjoint (overlap=False) with values in {0, 0.25, .., 1.5}."""
    rng = np.random.default_rng(seed)
    tracks = {}
    for c in range(nchrom):
        pos, iv = int(rng.integers(0, 1000)), []
        for _ in range(per):
            pos += int(rng.integers(0, 50))
            ln = int(rng.integers(1, 200))
            iv.append((pos, pos + ln, float(rng.integers(0, 7)) * 0.25))
            pos += ln
        tracks["chr%d" % (c + 1)] = iv
    return tracks


def bedgraph_of(tracks, order=None) -> bytes:
    out = []
    for c in (order or list(tracks)):
        out.extend("{}\t{}\t{}\t{!r}\n".format(c, b, e, v) for b, e, v in tracks[c])
    return "".join(out).encode()


def big_bedgraph(seed, nlines, nchrom=24) -> bytes:
    """An hg38-shaped bedGraph of about `nlines` lines: runs and gaps drawn from the golden track's run statistics."""
    from pymasc_amd import synth
    runs, gaps = synth.fixture_run_lengths(BEDGRAPH)
    rng = np.random.default_rng(seed)
    names = [n for n, _ in synth.HG38[:nchrom]]
    per = -(-nlines // (2 * len(names)))
    parts = []
    for n in names:
        r = rng.choice(runs, per)
        g = rng.choice(gaps, per)
        edges = np.empty(2 * per + 1, dtype=np.int64)
        edges[0] = int(rng.integers(0, 10000))
        steps = np.empty(2 * per, dtype=np.int64)
        steps[0::2] = g
        steps[1::2] = r
        edges[1:] = edges[0] + np.cumsum(steps)
        val = np.tile(np.array(["0", "1"]), per)
        lines = np.char.add(np.char.add(np.char.add(np.char.add(n + "\t", edges[:-1].astype(str)), "\t"),
                                        np.char.add(edges[1:].astype(str), "\t")), val)
        parts.append("\n".join(lines.tolist()) + "\n")
    return "".join(parts).encode()


#: values whose (float)strtod the readers must reproduce (the device's fast path and its host re-parse)
ROUNDING = ["1", "1.0", "1e0", "0.99999997", "0.9999999701976776", "0.999999999999999999999", "-0", ".5", "1e-30",
            "5.", "+2.5E+3", "0.1", "3.4028235e38", "1e-45", "123456789012345678", "0.000000000000000000000000001"]


def rounding_text(values=ROUNDING) -> bytes:
    return b"".join(b"chrR\t%d\t%d\t%s\n" % (10 * i, 10 * i + 5, v.encode()) for i, v in enumerate(values))


def strtod_float(text):
    return np.float32(float(text))


#: (file name, text, 1-based line, words in the message)
ERRORS = [
    ("fields.bedGraph", b"chr1\t0\t10\t1\nchr1\t10\t20\n", 2, "wrong number of fields"),
    ("coord.bedGraph", b"# c\nchr1\t0\t10\t1\nchr1\tx\t20\t1\n", 3, "bad number"),
    ("big.bedGraph", b"chr1\t0\t4294967296\t1\n", 1, "bad number"),
    ("value.bedGraph", b"chr1\t0\t10\t1\nchr1\t10\t20\tnan\n", 2, "bad number"),
    ("inf.bedGraph", b"chr1\t0\t10\tinf\n", 1, "bad number"),
    ("hex.bedGraph", b"chr1\t0\t10\t0x1p3\n", 1, "bad number"),
    ("range.bedGraph", b"chr1\t0\t10\t1\nchr1\t20\t20\t1\n", 2, "end is not greater than start"),
    ("nodecl.wig", b"track type=wiggle_0\n10 1\n", 2, "before any WIG declaration"),
    ("block.wig", b"variableStep chrom=chr1\n10 1\n5\n", 3, "WIG block"),
    ("decl.wig", b"fixedStep chrom=chr1 start=1\n1\n", 1, "declaration"),
    ("tracks.bedGraph", b"track type=bedGraph\ntrack name=x\nchr1\t0\t1\t1\n", 2, "more than one track"),
    ("late.bedGraph", b"chr1\t0\t1\t1\ntrack name=x\n", 2, "track line after the first data line"),
]


def truncated_gzip():
    data = golden_text()
    z = gzip.compress(data)
    return z[: len(z) // 2]
