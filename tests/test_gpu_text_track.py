"""Text mappability tracks on the device (pymasc_amd.text_track.DeviceTextTrackReader, pmx_dtt_open) against the host reader,
its checker: every input of tests/test_text_track.py, a 2 M-line 24-chromosome track, values the host re-parses, the error texts;
then the golden run with the bedGraph twin of the golden BigWig in three compressions and with its BED twin, the precalc cache,
and two gloo ranks (the host reader on each) against one."""
import shutil

import numpy as np
import pytest

from pymasc_amd import pipeline
from pymasc_amd import text_track as T
from pymasc_amd.bam import PmxIOError
from . import text_track_cases as C
from .test_gpu_cli import GOLDEN_JSON, STEM, _command, _tree
from .test_gpu_run_files import GOLD, TABLES, _check_tables

pytestmark = pytest.mark.gpu


def _agree(path):
    """The device reader equals the host reader: chromsizes, every chromosome's arrays at several thresholds, sorted."""
    with T.TextTrackReader(path) as h, T.DeviceTextTrackReader(path) as d:
        assert d.chromsizes_are_extents
        assert d.chromsizes == h.chromsizes
        assert list(d.chromsizes) == list(h.chromsizes)
        for th in (0, 0.5, 1.0):
            for c in h.chromsizes:
                a, b = h.fetch_arrays(th, c), d.fetch_arrays(th, c)
                for x, y in zip(a, b):
                    assert x.dtype == y.dtype
                    np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
                assert d.sorted == h.sorted, (c, th)
        with pytest.raises(KeyError):
            d.fetch_arrays(1.0, "no-such-chromosome")


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def test_golden_variants(tmp_path):
    for p in C.golden_variants(tmp_path).values():
        _agree(p)


def test_twins_and_synthetic_tracks(tmp_path):
    tracks = C.synthetic(0x7E57)
    order = list(tracks)
    mixed = C.bedgraph_of(tracks, order[::2]) + C.bedgraph_of(tracks, order[1::2]) + C.bedgraph_of(tracks, order[:2])
    cases = [("twin.bed", C.bed_text()), ("twin.wig", C.wig_variable_text()), ("fixed_gap.wig", C.wig_fixed_text(7)),
             ("fixed_eq.txt", C.wig_fixed_text(0)), ("multi.wig", C.FIXED_MULTI[0]), ("syn.bedGraph", C.bedgraph_of(tracks)),
             ("mixed.bedGraph", mixed), ("round.bedGraph", C.rounding_text()),
             ("odd.txt", b"browser position chr1:1-100\r\n# c\r\ntrack type=bedGraph name=\"x y\"\r\n\r\nchr1  0 \t 10   1\r\n"
                         b"   \r\nbrowser hide\r\nchr1\t20\t30\t0.5\r\nchr1\t30\t40\t2"),
             ("mixed.bed.gz", C.compress(b"chr2\t100\t200\nchr1\t0\t50\tx\nchr2\t150\t300\nchr1\t500\t600\nchr1\t400\t450\n", "bgzf")),
             ("empty.bedGraph", b"# nothing\n")]
    for name, data in cases:
        _agree(_write(tmp_path, name, data))


def test_two_million_lines_many_chunks(tmp_path):
    data = C.big_bedgraph(0x5EED, 2_000_000)
    assert data.count(b"\n") >= 2_000_000 and len(data) > 64 * 65536
    for how in ("plain", "bgzf"):
        _agree(_write(tmp_path, "big_%s.bedGraph" % how, C.compress(data, how)))


def test_values_the_host_reparses(tmp_path):
    vals = ["0.%s" % ("9" * (16 + i % 9)) for i in range(3000)] + ["%de-%d" % (i, 23 + i % 20) for i in range(1, 3000)]
    vals += ["1.%s" % ("0123456789" * 8) for _ in range(5)]     # tokens longer than 64 bytes
    p = _write(tmp_path, "slow.bedGraph", C.rounding_text(vals))
    _agree(p)
    with T.DeviceTextTrackReader(p) as d:
        _b, _e, v = d.fetch_arrays(0, "chrR")
    want = np.array([C.strtod_float(x) for x in vals], dtype=np.float32)
    np.testing.assert_array_equal(v.view(np.uint32), want.view(np.uint32))


def test_error_texts_equal_the_host_readers(tmp_path):
    cases = list(C.ERRORS) + [("cut.bedGraph.gz", C.truncated_gzip(), None, "truncated gzip stream")]
    for name, data, line, words in cases:
        p = _write(tmp_path, name, data)
        with pytest.raises(PmxIOError) as eh:
            T.TextTrackReader(p)
        with pytest.raises(PmxIOError) as ed:
            T.DeviceTextTrackReader(p)
        assert ed.value.msg == eh.value.msg, name
        assert words in ed.value.msg and (line is None or "line {}: ".format(line) in ed.value.msg)


def _golden_inputs(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    bam = d / (STEM + ".bam")
    shutil.copy(GOLD + ".bam", bam)
    shutil.copy(GOLD + ".bam.bai", str(bam) + ".bai")
    return bam


@pytest.mark.parametrize("how", ["plain", "gzip", "bgzf"])
def test_golden_run_with_the_bedgraph_twin(tmp_path, how):
    bam = _golden_inputs(tmp_path)
    track = C.golden_variants(tmp_path)[how]
    result, written = pipeline.run(bam, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10,
                                   mappability_path=track)
    assert [p.name for p in written] == [STEM + s for s in TABLES]
    _check_tables(written)


def test_golden_run_with_the_bed_twin(tmp_path):
    bam = _golden_inputs(tmp_path)
    track = _write(tmp_path, "hg19_36mer-test.bed", C.bed_text())
    _result, written = pipeline.run(bam, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10,
                                    mappability_path=track)
    _check_tables(written)


def test_precalc_writes_the_golden_cache(tmp_path):
    shutil.copy(C.BEDGRAPH, tmp_path / "hg19_36mer-test.bedGraph")
    rc, err = _command("pymasc_amd.precalc", ["-m", "hg19_36mer-test.bedGraph", "-d", "300", "-r", "36"], tmp_path)
    assert rc == 0, err
    assert (tmp_path / "hg19_36mer-test_mappability.json").read_bytes() == open(GOLDEN_JSON, "rb").read()


def test_two_gloo_ranks_equal_one_with_a_text_track(tmp_path):
    bam = tmp_path / (STEM + ".bam")
    shutil.copy(GOLD + ".bam", bam)
    shutil.copy(GOLD + ".bam.bai", str(bam) + ".bai")
    shutil.copy(C.BEDGRAPH, tmp_path / "x.bedGraph")
    common = [bam.name, "-m", "x.bedGraph", "-d", "300", "-q", "10", "-r", "36", "--skip-plots"]
    rc, err = _command("pymasc_amd", common + ["-o", "one"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", common + ["-o", "two", "-p", "2"], tmp_path, PMX_DIST_BACKEND="gloo")
    assert rc == 0, err
    assert _tree(tmp_path / "two") == _tree(tmp_path / "one")
    _check_tables([tmp_path / "one" / (STEM + s) for s in TABLES])
