"""Text mappability tracks through the host reader (pymasc_amd.text_track.TextTrackReader, libpymasc_io.so pmx_ttrack_open): the
golden bedGraph in every compression and its BED / WIG twins give the golden BigWig's intervals; synthetic tracks agree with
their BigWig twins; interleaved and overlapping lines, comments, spaces and CRLF; extents as chromsizes; value rounding as
(float)strtod; the malformed cases and the line each names; and the reader inputs.open_track picks."""
import numpy as np
import pytest

from pymasc_amd import bigwig, inputs, kmer_track, native
from pymasc_amd import text_track as T
from pymasc_amd.bam import PmxIOError
from . import bigbed_writers as BB
from . import io_writers as W
from . import kmer_cases as K
from . import text_track_cases as C


def _same(a, b):
    for x, y in zip(a, b):
        assert x.dtype == y.dtype
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("how", ["plain", "gzip", "bgzf"])
def test_golden_bedgraph_equals_the_bigwig(tmp_path, how):
    path = C.golden_variants(tmp_path)[how]
    with T.TextTrackReader(path) as r, bigwig.BigWigReader(C.BIGWIG) as w:
        assert r.chromsizes_are_extents
        assert r.chromsizes == {"chr1": 850000}
        for th in (1.0, 0.5):
            _same(r.fetch_arrays(th, "chr1"), w.fetch_arrays(th, "chr1"))
            assert r.sorted
        assert list(r.fetch(1.0, "chr1")) == list(w.fetch(1.0, "chr1"))
        with pytest.raises(KeyError):
            r.fetch_arrays(1.0, "chr2")


@pytest.mark.parametrize("name,text", [("twin.bed", C.bed_text()), ("twin.wig", C.wig_variable_text()),
                                       ("fixed_gap.wig", C.wig_fixed_text(7)), ("fixed_eq.txt", C.wig_fixed_text(0))])
def test_bed_and_wig_twins_equal_the_bigwig_at_one(tmp_path, name, text):
    p = tmp_path / name
    p.write_bytes(text)
    with T.TextTrackReader(p) as r, bigwig.BigWigReader(C.BIGWIG) as w:
        b, e, v = r.fetch_arrays(1.0, "chr1")
        wb, we, _wv = w.fetch_arrays(1.0, "chr1")
        np.testing.assert_array_equal(b, wb)
        np.testing.assert_array_equal(e, we)
        assert (v == 1.0).all()


def test_fixedstep_blocks(tmp_path):
    text, want = C.FIXED_MULTI
    p = tmp_path / "multi.wig"
    p.write_bytes(text)
    with T.TextTrackReader(p) as r:
        b, e, v = r.fetch_arrays(0, "chrA")
        assert list(zip(b.tolist(), e.tolist(), v.tolist())) == want
        assert r.chromsizes == {"chrA": 104}


@pytest.mark.parametrize("compress", [False, True])
def test_synthetic_track_equals_its_bigwig_twin(tmp_path, compress):
    tracks = C.synthetic(0x7E57)
    p = tmp_path / "syn.bedGraph"
    p.write_bytes(C.bedgraph_of(tracks))
    sizes = {c: iv[-1][1] for c, iv in tracks.items()}
    W.write_bigwig(tmp_path / "syn.bw", sizes, tracks, compress=compress)
    with T.TextTrackReader(p) as r, bigwig.BigWigReader(tmp_path / "syn.bw") as w:
        assert r.chromsizes == sizes
        for c in tracks:
            for th in (0, 0.5, 1.0, 1.25):
                _same(r.fetch_arrays(th, c), w.fetch_arrays(th, c))


def test_interleaved_overlapping_and_unsorted(tmp_path):
    text = (b"chr2\t100\t200\t1\nchr1\t0\t50\t1\nchr2\t150\t300\t1\nchr1\t10\t20\t0\n"
            b"chr1\t500\t600\t1\nchr1\t400\t450\t1\nchr2\t1000\t1001\t0.5\n")
    p = tmp_path / "mixed.bedGraph"
    p.write_bytes(text)
    with T.TextTrackReader(p) as r:
        assert list(r.chromsizes) == ["chr2", "chr1"]
        assert r.chromsizes == {"chr2": 1001, "chr1": 600}
        assert list(r.fetch(1.0, "chr2")) == [(100, 200, 1.0), (150, 300, 1.0)]
        assert not r.sorted                                        # overlap
        assert list(r.fetch(1.0, "chr1")) == [(0, 50, 1.0), (500, 600, 1.0), (400, 450, 1.0)]
        assert not r.sorted                                        # out of order
        assert list(r.fetch(0, "chr1")) == [(0, 50, 1.0), (10, 20, 0.0), (500, 600, 1.0), (400, 450, 1.0)]
        assert list(r.fetch(0.5, "chr2"))[-1] == (1000, 1001, 0.5)


def test_comments_browser_spaces_and_crlf(tmp_path):
    text = (b"browser position chr1:1-100\r\n# a comment\r\ntrack type=bedGraph name=\"x y\"\r\n\r\n"
            b"chr1  0 \t 10   1\r\n   \r\n#chr1\t10\t20\t1\r\nbrowser hide all\r\nchr1\t20\t30\t0.5\r\nchr1\t30\t40\t2")
    p = tmp_path / "odd.txt"
    p.write_bytes(text)
    with T.TextTrackReader(p) as r:
        assert list(r.fetch(0, "chr1")) == [(0, 10, 1.0), (20, 30, 0.5), (30, 40, 2.0)]
        assert r.chromsizes == {"chr1": 40}


def test_extent_is_the_largest_end_whatever_its_value(tmp_path):
    p = tmp_path / "ext.bedGraph"
    p.write_bytes(b"chrX\t0\t10\t1\nchrX\t10\t5000\t0\nchrX\t20\t30\t1\n")
    with T.TextTrackReader(p) as r:
        assert r.chromsizes == {"chrX": 5000}


def test_value_rounding_is_strtod_then_float(tmp_path):
    p = tmp_path / "round.bedGraph"
    p.write_bytes(C.rounding_text())
    with T.TextTrackReader(p) as r:
        _b, _e, v = r.fetch_arrays(0, "chrR")
    want = np.array([C.strtod_float(x) for x in C.ROUNDING], dtype=np.float32)
    np.testing.assert_array_equal(v.view(np.uint32), want.view(np.uint32))   # bit for bit: -0 stays -0
    assert v[4] == np.float32(1.0) and v[3] == np.float32(0.99999994)        # the float midpoint rounds to even


@pytest.mark.parametrize("name,text,line,words", C.ERRORS)
def test_errors_name_their_line(tmp_path, name, text, line, words):
    p = tmp_path / name
    p.write_bytes(text)
    with pytest.raises(PmxIOError) as ei:
        T.TextTrackReader(p)
    assert "line {}: ".format(line) in str(ei.value) and words in str(ei.value)


def test_truncated_gzip_names_its_line(tmp_path):
    p = tmp_path / "cut.bedGraph.gz"
    p.write_bytes(C.truncated_gzip())
    with pytest.raises(PmxIOError, match=r"line \d+: truncated gzip stream"):
        T.TextTrackReader(p)


def test_kind_rules(tmp_path):
    # a track line decides; else a WIG declaration as the first data line; else the .bed suffix; else bedGraph
    p = tmp_path / "a.bed"
    p.write_bytes(b"track type=bedGraph\nchr1\t0\t10\t0.5\n")
    with T.TextTrackReader(p) as r:
        assert list(r.fetch(0, "chr1")) == [(0, 10, 0.5)]
    p = tmp_path / "b.bed.gz"
    p.write_bytes(C.compress(b"chr1\t0\t10\tx\t0.5\n", "gzip"))
    with T.TextTrackReader(p) as r:
        assert list(r.fetch(0, "chr1")) == [(0, 10, 1.0)]
    p = tmp_path / "c.bedGraph"
    p.write_bytes(b"# x\nvariableStep chrom=chr3 span=5\n11 0.25\n")
    with T.TextTrackReader(p) as r:
        assert list(r.fetch(0, "chr3")) == [(10, 15, 0.25)]


def test_open_track_picks_the_reader(tmp_path):
    v = C.golden_variants(tmp_path)
    for how in ("plain", "gzip", "bgzf"):
        with inputs.open_track(v[how], False) as r:
            assert isinstance(r, T.TextTrackReader)
    with inputs.open_track(C.BIGWIG, False) as r:
        assert isinstance(r, bigwig.BigWigReader)
    renamed = tmp_path / "track.data"                 # the bbi magic decides whatever the name
    renamed.write_bytes(open(C.BIGWIG, "rb").read())
    with inputs.open_track(renamed, False) as r:
        assert isinstance(r, bigwig.BigWigReader)
    zero = tmp_path / "zero.BW"                       # the suffix decides: a corrupt BigWig still says "magic"
    zero.write_bytes(b"\0" * 4096)
    with pytest.raises(PmxIOError, match="magic"):
        inputs.open_track(zero, False)
    assert T.is_bigwig(zero) and T.is_bigwig(renamed) and not T.is_bigwig(v["plain"])


def test_every_kind_of_host_track_through_the_one_base_class(tmp_path):
    """A BigWig, a bigBed, a bedGraph and a genome FASTA are one pmx_track behind ``native.HostTrackReader``: ``kind``,
    ``sorted`` before any fetch, KeyError for an unknown chromosome, ``fetch`` as the zip of ``fetch_arrays``, ValueError after
    ``close``."""
    bb = tmp_path / "twin.bb"
    BB.write_bigbed(str(bb), {"chr1": 1000, "chr2": 500}, {"chr1": ([10, 30], [20, 45], b"r\t0\t+"), "chr2": ([0], [7], b"r\t0\t-")})
    fasta, _recs = K.write_cases(str(tmp_path))[0]
    opened = [(bigwig.BigWigReader(C.BIGWIG), "bigwig"), (bigwig.BigWigReader(bb), "bigbed"),
              (T.TextTrackReader(C.BEDGRAPH), "bigwig"), (kmer_track.KmerTrackReader(fasta, 36), "kmer")]
    for r, kind in opened:
        assert isinstance(r, native.HostTrackReader) and type(r).fetch_arrays is native.HostTrackReader.fetch_arrays
        assert r.kind == kind
        assert r.sorted
        with pytest.raises(KeyError):
            r.fetch_arrays(1.0, "no-such-chromosome")
        with pytest.raises(KeyError):
            r.fetch(1.0, "no-such-chromosome")
        for chrom in r.chromsizes:
            b, e, v = r.fetch_arrays(0.5, chrom)
            assert list(r.fetch(0.5, chrom)) == list(zip(b.tolist(), e.tolist(), v.tolist()))
        assert sum(len(r.fetch_arrays(0.0, c)[0]) for c in r.chromsizes) > 0
        r.disable_progress_bar()
        r.close()
        assert r.closed and r.kind == kind
        with pytest.raises(ValueError, match="closed"):
            r.fetch_arrays(1.0, next(iter(r.chromsizes)))
        with pytest.raises(ValueError, match="closed"):
            r.fetch(1.0, next(iter(r.chromsizes)))
