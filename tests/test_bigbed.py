"""bigBed mappability tracks through the host reader (pymasc_amd.bigwig.BigWigReader, libpymasc_io.so pmx_bigwig_open with a bigBed
file): inputs.open_track's routing, the intervals of every input against its BED text twin read by
TextTrackReader, the keep rule at the chromosome's end, and the error text of each corrupt case (a cyclic R-tree included, which
must end).  The builders here are shared with tests/test_gpu_bigbed.py."""
import struct

import numpy as np
import pytest

from pymasc_amd import bigwig, inputs
from pymasc_amd import text_track as T
from pymasc_amd.bam import PmxIOError
from . import bigbed_writers as B
from . import text_track_cases as C

THRESHOLDS = (0, 1.0, 1.5)


def _text(records):
    """The BED text twin of {chrom: (starts, ends, rests as a list of bytes)}."""
    out = []
    for c, (s, e, r) in records.items():
        for b, x, rest in zip(np.asarray(s).tolist(), np.asarray(e).tolist(), r):
            out.append(b"%s\t%d\t%d%s\n" % (c.encode(), b, x, b"\t" + rest if rest else b""))
    return b"".join(out) or b"# no records\n"


def golden_records(rests=None):
    """{chr1: ...}: the golden track's mappable intervals, with text_track_cases.bed_text()'s name / score / strand."""
    mp = C.mappable()
    s = np.array([b for b, _ in mp], dtype=np.int64)
    e = np.array([x for _, x in mp], dtype=np.int64)
    if rests is None:
        rests = [b"name%d\t0\t+" % i for i in range(len(mp))]
    return {"chr1": (s, e, rests)}


GOLDEN_SIZES = {"chr1": 850000}     # the golden BigWig's


def write_golden_twin(path, compress=True, **kw):
    """The bigBed twin of the golden BigWig's mappable intervals (= text_track_cases.bed_text())."""
    B.write_bigbed(path, GOLDEN_SIZES, golden_records(), compress=compress, items_per_block=64, rtree_block=4, **kw)
    return path


def cases():
    """(name, chromsizes, records, writer options): every input of the reader tests.  Records as lists, so that _text can
    write their twins."""
    out = []
    g = golden_records()
    out.append(("twin_z", GOLDEN_SIZES, g, dict(compress=True, items_per_block=64, rtree_block=4)))
    out.append(("twin_raw", GOLDEN_SIZES, g, dict(compress=False, items_per_block=64, rtree_block=4)))
    n = len(g["chr1"][0])
    out.append(("bed3", GOLDEN_SIZES, golden_records([b""] * n), dict(items_per_block=100, field_count=3)))
    rl = [b"r" * (63, 64, 65, 300)[i % 4] for i in range(n)]
    out.append(("rest_lengths", GOLDEN_SIZES, golden_records(rl), dict(items_per_block=37)))
    out.append(("rest_lengths_raw", GOLDEN_SIZES, golden_records(rl), dict(items_per_block=37, compress=False)))
    zs = np.array([0, 256, 65536, 65536 * 256, 0x01000000 + 1], dtype=np.int64)
    ze = np.array([256, 512, 65536 + 256, 65536 * 256 + 65536, 0x01000000 + 0x100], dtype=np.int64)
    out.append(("zeros", {"a": 1 << 30, "b": 1 << 30}, {"a": (zs, ze, [b"", b"x", b"", b"\x01", b"n\t0\t-"]),
                                                         "b": (zs, ze, [b""] * 5)}, dict(items_per_block=2, field_count=3)))
    out.append(("deep_rtree", GOLDEN_SIZES, g, dict(items_per_block=3, rtree_block=2)))
    out.append(("no_records_chrom", {"chr1": 850000, "chr0": 1000, "chrZ": 5}, g, dict(items_per_block=50)))
    out.append(("empty", {"chr1": 1000, "chr2": 2000}, {}, dict(field_count=6)))
    ov_s = np.array([10, 15, 100, 100, 300], dtype=np.int64)
    ov_e = np.array([20, 30, 150, 200, 301], dtype=np.int64)
    out.append(("overlap", {"c": 10000}, {"c": (ov_s, ov_e, [b"a"] * 5)}, dict(items_per_block=2)))
    pe_s = np.array([5, 900, 990, 999, 1000, 5000], dtype=np.int64)
    pe_e = np.array([10, 1000, 1500, 2000, 1200, 6000], dtype=np.int64)
    out.append(("past_end", {"c": 1000}, {"c": (pe_s, pe_e, [b"p\t1\t+"] * 6)}, dict(items_per_block=4)))
    return out


def zero_length_case():
    """Records a text track refuses (end <= start is a malformed line there) but bigBed may hold: [0, 0) is dropped (end 0),
    [100, 100) kept, and the fetch is not sorted."""
    s = np.array([0, 10, 100, 100], dtype=np.int64)
    e = np.array([0, 20, 100, 120], dtype=np.int64)
    return ("zero_length", {"c": 10000}, {"c": (s, e, [b"z"] * 4)}, dict(items_per_block=3))


def write_case(tmp_path, name, sizes, records, opts):
    p = tmp_path / (name + ".bb")
    B.write_bigbed(p, sizes, records, **opts)
    t = tmp_path / (name + ".bed")
    t.write_bytes(_text(records))
    return p, t


def is_sorted(b, e):
    return bool((b < e).all() and (e[:-1] <= b[1:]).all())


def expected(text_path, sizes, chrom, th):
    """What a bigBed reader gives: the twin's lines (value 1) with start < size and end > 0."""
    with T.TextTrackReader(text_path) as t:
        if chrom not in t.chromsizes:
            z = np.empty(0, dtype=np.uint32)
            return z, z.copy(), np.empty(0, dtype=np.float32)
        b, e, v = t.fetch_arrays(th, chrom)
    keep = (b.astype(np.int64) < sizes[chrom]) & (e != 0)
    return b[keep], e[keep], v[keep]


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def corrupt_cases():
    """(name, writer(path), words of the message): one bad block (or index) in a file of one or two chromosomes."""
    g = golden_records()

    def plain(**kw):
        return lambda p: B.write_bigbed(p, GOLDEN_SIZES, g, items_per_block=64, rtree_block=4, **kw)

    def end_before_start(p):
        s, e, r = g["chr1"]
        e = e.copy()
        e[70] = s[70] - 1
        B.write_bigbed(p, GOLDEN_SIZES, {"chr1": (s, e, r)}, items_per_block=64)

    def mixed(p):
        s, e, r = g["chr1"]
        B.write_bigbed(p, {"chr1": 850000, "chr2": 850000}, {"chr1": (s[:100], e[:100], r[:100]), "chr2": (s[:100], e[:100], r[:100])},
                       items_per_block=64, split_chroms=False)

    def cyclic(p):
        lay = B.write_bigbed(p, GOLDEN_SIZES, g, items_per_block=8, rtree_block=2)
        assert lay["levels"] > 2
        root = lay["index_off"] + 48
        with open(p, "r+b") as fp:      # the root's first child: the root itself
            fp.seek(root + 4 + 16)
            fp.write(struct.pack("<Q", root))

    last = -(-len(g["chr1"][0]) // 64) - 1
    return [
        ("truncated", plain(raw_hook=lambda i, d: d + b"\x01" * 5 if i == 3 else d), "fewer than 13 bytes left"),
        ("truncated_raw", plain(compress=False, raw_hook=lambda i, d: d + b"\x01" * 12 if i == 0 else d), "fewer than 13 bytes left"),
        ("no_nul", plain(raw_hook=lambda i, d: d[:-1] if i == last else d), "no NUL before the block ends"),
        ("no_nul_raw", plain(compress=False, raw_hook=lambda i, d: d[:-1] if i == 2 else d), "no NUL before the block ends"),
        ("end_before_start", end_before_start, "bigBed record ends before it starts"),
        ("mixed", mixed, "more than one chromosome"),
        ("adler", plain(block_hook=lambda i, z: z[:-1] + bytes([z[-1] ^ 1]) if i == 5 else z), "Adler-32"),
        ("cyclic_rtree", cyclic, "R-tree child does not lie after its parent"),
    ]


def host_error(path):
    """The message of the first failing fetch of the host reader, chromosome by chromosome (None if every fetch works)."""
    with bigwig.BigWigReader(path) as r:
        for c in r.chromsizes:
            try:
                r.fetch_arrays(0, c)
            except PmxIOError as e:
                return e.msg
    return None


# ------------------------------------------------------------------------------------------------------------------
def test_open_track_routes_bigbed_files(tmp_path):
    bb = write_golden_twin(tmp_path / "twin.bb")
    data = bb.read_bytes()
    for name in ("twin.bb", "renamed.data", "upper.BB", "long.BIGBED", "mixed.BigBed"):
        p = tmp_path / name
        if not p.exists():
            p.write_bytes(data)
        assert T.is_bigbed(p), name
        assert not T.is_bigwig(p), name             # is_bigwig is the rule it was
        with inputs.open_track(p, False) as r:
            assert isinstance(r, bigwig.BigWigReader), name
            assert r.kind == "bigbed"
            assert r.chromsizes == GOLDEN_SIZES
    with inputs.open_track(C.BIGWIG, False) as r:
        assert isinstance(r, bigwig.BigWigReader) and r.kind == "bigwig"
    assert not T.is_bigbed(C.BIGWIG) and not T.is_bigbed(C.BEDGRAPH)
    zero = tmp_path / "zero.bb"                       # the suffix decides: a corrupt bigBed still says "magic"
    zero.write_bytes(b"\0" * 4096)
    with pytest.raises(PmxIOError, match="magic"):
        inputs.open_track(zero, False)
    text = tmp_path / "twin.bed"                      # a BED text track stays a text track
    text.write_bytes(C.bed_text())
    assert not T.is_bigbed(text)
    with inputs.open_track(text, False) as r:
        assert isinstance(r, T.TextTrackReader)


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_host_reader_equals_the_bed_twin(tmp_path, case):
    name, sizes, records, opts = case
    p, t = write_case(tmp_path, name, sizes, records, opts)
    with bigwig.BigWigReader(p) as r:
        assert r.kind == "bigbed"
        assert r.chromsizes == {c: sizes[c] for c in sorted(sizes)}
        assert list(r.chromsizes) == sorted(sizes)
        for th in THRESHOLDS:
            for c in r.chromsizes:
                got = r.fetch_arrays(th, c)
                want = expected(t, sizes, c, th)
                _same(got, want)
                assert r.sorted == is_sorted(want[0], want[1]), (c, th)
        with pytest.raises(KeyError):
            r.fetch_arrays(1.0, "no-such-chromosome")


def test_golden_twin_equals_the_golden_bigwig_at_one(tmp_path):
    for compress in (True, False):
        p = write_golden_twin(tmp_path / ("twin%d.bb" % compress), compress=compress)
        with bigwig.BigWigReader(p) as r, bigwig.BigWigReader(C.BIGWIG) as w, T.TextTrackReader(_bed(tmp_path)) as t:
            b, e, v = r.fetch_arrays(1.0, "chr1")
            wb, we, _ = w.fetch_arrays(1.0, "chr1")
            np.testing.assert_array_equal(b, wb)
            np.testing.assert_array_equal(e, we)
            assert (v == 1.0).all() and r.sorted
            _same((b, e, v), t.fetch_arrays(1.0, "chr1"))
            assert r.sorted == t.sorted


def _bed(tmp_path):
    p = tmp_path / "golden_twin.bed"
    p.write_bytes(C.bed_text())
    return p


def test_overlap_and_chromosome_end(tmp_path):
    c = dict((x[0], x) for x in cases())
    _n, sizes, records, opts = c["overlap"]
    p, _t = write_case(tmp_path, "overlap", sizes, records, opts)
    with bigwig.BigWigReader(p) as r:
        assert list(r.fetch(1.0, "c")) == [(10, 20, 1.0), (15, 30, 1.0), (100, 150, 1.0), (100, 200, 1.0), (300, 301, 1.0)]
        assert not r.sorted
    _n, sizes, records, opts = c["past_end"]
    p, _t = write_case(tmp_path, "past_end", sizes, records, opts)
    with bigwig.BigWigReader(p) as r:
        # start >= size or end == 0 is dropped; an interval that runs past the end is kept whole
        assert list(r.fetch(0, "c")) == [(5, 10, 1.0), (900, 1000, 1.0), (990, 1500, 1.0), (999, 2000, 1.0)]
        assert not r.sorted
    name, sizes, records, opts = zero_length_case()
    p = tmp_path / "zero_length.bb"
    B.write_bigbed(p, sizes, records, **opts)
    with bigwig.BigWigReader(p) as r:
        assert list(r.fetch(0, "c")) == [(10, 20, 1.0), (100, 100, 1.0), (100, 120, 1.0)]
        assert not r.sorted


def test_large_file_many_blocks(tmp_path):
    recs = B.random_records(0xB16B, 200_000, ["chr%d" % i for i in range(1, 25)])
    sizes = {n: int(v[1][-1]) + 1 for n, v in recs.items()}
    sizes["chr7"] = int(recs["chr7"][0][len(recs["chr7"][0]) // 2])      # half of chr7 lies past its end
    p = tmp_path / "big.bb"
    lay = B.write_bigbed(p, sizes, recs, items_per_block=512, rtree_block=16)
    assert len(lay["blocks"]) > 300 and lay["levels"] >= 3
    with bigwig.BigWigReader(p) as r:
        for c, (s, e, _r) in recs.items():
            b, x, v = r.fetch_arrays(1.0, c)
            keep = s < sizes[c]
            np.testing.assert_array_equal(b, s[keep].astype(np.uint32))
            np.testing.assert_array_equal(x, e[keep].astype(np.uint32))
            assert (v == 1.0).all() and r.sorted


@pytest.mark.parametrize("case", corrupt_cases(), ids=lambda c: c[0])
def test_corrupt_blocks_give_their_error(tmp_path, case):
    name, write, words = case
    p = tmp_path / (name + ".bb")
    write(p)
    with bigwig.BigWigReader(p) as r:
        assert r.kind == "bigbed"
    msg = host_error(p)
    assert msg is not None and words in msg, msg
    assert "BigWig" not in msg


def test_header_errors(tmp_path):
    p = write_golden_twin(tmp_path / "twin.bb")
    data = bytearray(p.read_bytes())
    fc = tmp_path / "fields.bb"
    struct.pack_into("<H", data, 32, 2)
    fc.write_bytes(bytes(data))
    with pytest.raises(PmxIOError, match="bigBed fieldCount below 3"):
        bigwig.BigWigReader(fc)
    sw = tmp_path / "swapped.bb"
    sw.write_bytes(struct.pack(">I", B.BIGBED_MAGIC) + p.read_bytes()[4:])
    with pytest.raises(PmxIOError, match="byte-swapped .* bigBed"):
        bigwig.BigWigReader(sw)
    cut = tmp_path / "cut.bb"
    cut.write_bytes(p.read_bytes()[:200])
    with pytest.raises(PmxIOError, match="bigBed structure points past the end"):
        bigwig.BigWigReader(cut)
