"""Peaks called from the signal track without a GPU: the host path (``Signal.call``, ``Coverage.call``, ``Peaks``)
against the loop restatement of tests/call_cases -- rows, totals and text bytes, exactly --, on the planted tracks and on the golden
file's depth, cpm and log2 tracks; the refusals, the command line's exit codes, and the run: with a cutoff it writes the narrowPeak
file beside the track and ``peaks.open_peaks`` reads it, without one the bytes it has always written."""
import os

import numpy as np
import pytest

from pymasc_amd import cli, coverage, peaks, pipeline
from tests import call_cases as KC
from tests import fixtures as fx
from tests import sam_writers as SW
from tests.fake_context import FakeContext

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"


def _host(reads, refs, extend=0):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), extend)


def _rows(g):
    """The rows of a ``Signal`` as the restatement takes them."""
    return [(n, int(a), int(b), c) for n, (s, e, v) in g.runs.items() for a, b, c in zip(s, e, v)]


def _same(p, want):
    """A ``Peaks`` against the restatement: rows, totals, lines and text, whole and in chunks."""
    assert KC.peaks_got(p) == KC.peaks_of(want) and p.totals == KC.totals(want)
    assert (p.n_peaks, p.peak_bases) == (want["n_peaks"], want["peak_bases"]) and p.lines() == KC.lines_of(want)
    assert b"".join(p.text_chunks()) == b"".join(p.text_chunks(chunk=7)) == KC.text_of(want)
    return p


def test_the_edges():
    reads = KC.reads_of(KC.E_TRACK)
    rows = KC.track_rows(reads, KC.E_REFS)
    assert [(s, e, int(v)) for _n, s, e, v in rows] == [(s, e, d) for _r, s, e, d in KC.E_TRACK]     # the pileup is the planted track
    want = KC.restate(rows, *KC.E_ARGS)
    KC.check_edges(want)
    c = _host(reads, KC.E_REFS)
    p = _same(c.call(*KC.E_ARGS), want)
    assert p == c.signal(1, 1.0).call(*KC.E_ARGS) and (p.cutoff, p.max_gap, p.min_length) == KC.E_ARGS
    assert p != c.call(2.0, 10, 51) and p != c.call(2.0, 11, 50) and c.call(2.0, 10, 51).totals["peaks"] == 5
    # scaled by 0.25, with the cutoff an exact float32: the same peaks
    quarter = KC.restate(KC.track_rows(reads, KC.E_REFS, 1, 0.25), 0.5, 10, 50)
    assert [x[:4] for x in quarter["peaks"]] == [x[:4] for x in want["peaks"]]
    _same(c.signal(1, 0.25).call(0.5, 10, 50), quarter)
    # the defaults
    assert c.call(2.0) == c.call(2.0, 30, 200) and (coverage.CALL_GAP, coverage.CALL_LENGTH) == (30, 200)
    # at a bin: a reference shorter than the bin, one without a run
    for B in (7, 50):
        _same(c.signal(B, 1.0).call(1.5, 10, 50), KC.restate(KC.track_rows(reads, KC.E_REFS, B), 1.5, 10, 50))


def test_a_signed_track():
    rt, rc = KC.reads_of(KC.S_TREATMENT), KC.reads_of(KC.S_CONTROL)
    want = KC.restate(KC.compared_rows(rt, rc, KC.S_REFS, 1, "subtract"), *KC.S_ARGS)
    KC.check_signed(want)
    g = _host(rt, KC.S_REFS).compare(_host(rc, KC.S_REFS), 1, "subtract")
    _same(g.call(*KC.S_ARGS), want)
    # -0.0 equals 0.0: the first of the two is the summit, and its value's text is 0
    z = coverage.Signal({"z": ([0, 50, 100], [50, 100, 150], np.array([-0.0, 0.0, -1.0], dtype=np.float32))}, 1, 1.0)
    zw = KC.restate(_rows(z), -0.5, 0, 100)
    assert [x[:4] for x in zw["peaks"]] == [("z", 0, 100, 25)] and KC.text_of(zw) == b"z\t0\t100\tpeak_1\t0\t.\t0\t-1\t-1\t25\n"
    _same(z.call(-0.5, 0, 100), zw)
    assert z.call(-0.5, 0, 100).rows["z"][3].view(np.uint32)[0] == 0x80000000
    # the score is capped at 1000 and truncated
    big = coverage.Signal({"z": ([0, 10, 20], [10, 20, 30], np.array([100.5, 0.19, 99.99], dtype=np.float32))}, 1, 1.0)
    text = b"".join(big.call(0.0, 0, 1).text_chunks()).decode().split("\n")
    assert text[0].split("\t")[3:7] == ["peak_1", "1000", ".", "100.5"]
    assert [KC.score(np.float32(v)) for v in (100.5, 0.19, 99.99, -3.0)] == [1000, 1, 999, 0]
    _same(big.call(0.0, 0, 1), KC.restate(_rows(big), 0.0, 0, 1))


@pytest.mark.parametrize("args", KC.L_CASES)
def test_the_long_chain(args):
    rows = KC.track_rows(KC.L_READS, KC.L_REFS)
    want = KC.restate(rows, *args)
    KC.check_long(rows, want, args)
    _same(_host(KC.L_READS, KC.L_REFS).call(*args), want)


@pytest.mark.parametrize("at,twice", KC.SUMMITS)
def test_the_summit(at, twice):
    reads = KC.summit_reads(at, twice)
    want = KC.restate(KC.track_rows(reads, KC.L_REFS), 2.0, 1, 200)
    KC.check_summit(want, at)
    _same(_host(reads, KC.L_REFS).call(2.0, 1, 200), want)


@pytest.mark.parametrize("k,f", KC.BOUNDARIES)
def test_the_boundaries(k, f):
    reads = KC.reads_of(KC.boundary_track(k, f))
    rows = KC.track_rows(reads, KC.B_REFS)
    for args in KC.B_ARGS:
        want = KC.restate(rows, *args)
        KC.check_boundary(want, k, f, args)
        _same(_host(reads, KC.B_REFS).call(*args), want)


def test_nothing_and_everything():
    c = _host(KC.reads_of(KC.E_TRACK), KC.E_REFS)
    none = c.call(100.0)
    assert none.rows == {} and none.totals == dict.fromkeys(coverage.CALL_TOTALS, 0) and b"".join(none.text_chunks()) == b"" and none.lines() == {}
    rows = KC.track_rows(KC.reads_of(KC.E_TRACK), KC.E_REFS)
    every = _same(c.call(-1.0, 0, 1), KC.restate(rows, -1.0, 0, 1))
    assert every.totals["passing_runs"] == c.n_runs and every.totals["passing_bases"] == c.covered_bases
    empty = _host([], KC.E_REFS)
    assert empty.call(0.0).totals == dict.fromkeys(coverage.CALL_TOTALS, 0)      # a pileup with no kept read


def _golden(extend=200, mapq=10):
    from pymasc_amd.bam import BamReader
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(mapq))]
    return refs, cols


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    """The golden file's pileup at extend 200, and a control over its references: every third of its reads, moved 17 bases on."""
    refs, cols = _golden()
    names, lengths = [n for n, _l in refs], [l for _n, l in refs]
    t = coverage.count_host(*cols, names, lengths, [1] * len(refs), 200)
    rows = [(int(r), int(p) + 17, int(l), int(s)) for r, p, l, s in list(zip(*cols))[::3] if int(p) + 17 + int(l) <= refs[int(r)][1]]
    recs = [SW.rec("c%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(rows)]
    path = SW.write_twins(tmp_path_factory.mktemp("coverage_call"), "input", refs, recs)[1]
    return dict(t=t, c=_host(rows, refs, 200), control=path, refs=refs)


@pytest.mark.parametrize("B", [1, 50, 4096])
def test_the_golden_files_tracks(golden, B):
    t, c = golden["t"], golden["c"]
    cpm = 1e6 / t.reads
    tracks = [(t.signal(B, 1.0), 3.0), (t.signal(B, cpm, "cpm"), 2.5 * cpm), (t.compare(c, B, "log2", 1.0, t.reads / c.reads, 1.0), 1.0)]
    for g, cutoff in tracks:
        for gap, length in ((30, 200), (0, 1), (1000, 300)):
            want = KC.restate(_rows(g), cutoff, gap, length)
            _same(g.call(cutoff, gap, length), want)
        assert B == 4096 or want["n_peaks"] > 3
    assert t.call(3.0) == t.signal(1, 1.0).call(3.0)


def test_check_call():
    assert coverage.check_call(1, 0, 1) == (1.0, 0, 1) and coverage.check_call(-2.5, 2 ** 31 - 1, 2 ** 31 - 1) == (-2.5, 2 ** 31 - 1, 2 ** 31 - 1)
    assert coverage.check_call(np.float32(0.5)) == (0.5, 30, 200)
    assert coverage.CALL_TOTALS == ("passing_runs", "candidates", "peaks", "peak_bases", "passing_bases")
    for bad in (float("nan"), float("inf"), -float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="coverage_call "):
            coverage.check_call(bad)
    for bad in (-1, 2 ** 31, 1.5, "3", True, None):
        with pytest.raises(ValueError, match="coverage_call_gap"):
            coverage.check_call(1.0, bad, 200)
    for bad in (0, -5, 2 ** 31, 2.5, "3", False, None):
        with pytest.raises(ValueError, match="coverage_call_length"):
            coverage.check_call(1.0, 30, bad)
    g = coverage.Signal({"a": ([0], [10], [1.0])}, 1, 1.0)
    with pytest.raises(ValueError, match="coverage_call_length"):
        g.call(1.0, 0, 0)
    with pytest.raises(ValueError, match="five columns"):
        coverage.Peaks({"a": ([0], [10], [5], [1.0])}, 1.0, 0, 1, dict.fromkeys(coverage.CALL_TOTALS, 0))


def test_options(monkeypatch):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base + ["--coverage"])
    assert (a.coverage_call, a.coverage_call_gap, a.coverage_call_length) == (None, None, None)
    a = cli.parse_args(base + ["--coverage-call", "-1.5", "--coverage-extend", "200"])
    assert a.coverage and a.coverage_call == -1.5 and cli.parse_args(["-", "--coverage-call", "2", "--coverage-extend", "200"]).coverage
    a = cli.parse_args(base + ["--coverage-call", "2", "--coverage-call-gap", "0", "--coverage-call-length", "1"])
    assert (a.coverage_call, a.coverage_call_gap, a.coverage_call_length) == (2.0, 0, 1)
    for bad in (["--coverage-call-gap", "5"], ["--coverage-call-length", "100"], ["--coverage-call", "nan"], ["--coverage-call", "inf"],
                ["--coverage-call", "-inf"], ["--coverage-call", "x"], ["--coverage-call", "1", "--coverage-call-gap", "-1"],
                ["--coverage-call", "1", "--coverage-call-gap", "2147483648"], ["--coverage-call", "1", "--coverage-call-length", "0"],
                ["--coverage-call", "1", "--coverage-call-length", "2147483648"], ["--coverage-call", "1", "--coverage-call-gap", "1.5"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    text = " ".join(cli.get_parser().format_help().split())
    assert "--coverage-call X" in text and "--coverage-call-gap N" in text and "--coverage-call-length N" in text
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for more, want in ((["--coverage-call", "1"], dict(coverage=True, coverage_call=1.0)),
                       (["--coverage-call", "0.5", "--coverage-call-gap", "7", "--coverage-call-length", "90", "--coverage-bin", "50"],
                        dict(coverage=True, coverage_call=0.5, coverage_call_gap=7, coverage_call_length=90, coverage_bin=50))):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert {k: v for k, v in seen.items() if k.startswith("coverage")} == want


def test_the_run(tmp_path, golden, caplog):
    t, c, path = golden["t"], golden["c"], golden["control"]
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext(), coverage_extend=200)
    # no cutoff, given or not: the bytes the run has always written, and one coverage file
    want = coverage.write_coverage(tmp_path / "want", STEM, t).read_bytes()
    for n, more in enumerate((dict(), dict(coverage_call=None, coverage_call_gap=30, coverage_call_length=200))):
        _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / ("plain%d" % n)), 120, coverage=True, **more, **kw)
        assert written[-1].name == STEM + "_coverage.bedGraph" and written[-1].read_bytes() == want
        assert not [p for p in os.listdir(tmp_path / ("plain%d" % n)) if p.endswith(".narrowPeak")]
    # a cutoff implies coverage: the depth track, byte for byte as above, and the peaks of the depth beside it
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "depth"), 120, coverage_call=3, **kw)
    assert [p.name for p in written[-2:]] == [STEM + "_coverage.bedGraph", STEM + "_coverage_peaks.narrowPeak"]
    p = t.call(3.0)
    assert written[-2].read_bytes() == want and written[-1].read_bytes() == b"".join(p.text_chunks()) and p.n_peaks > 3
    assert written[-1].read_bytes() == KC.text_of(KC.restate(_rows(t.signal(1, 1.0)), 3.0))
    got, mine = peaks.open_peaks(str(written[-1])), peaks.open_peaks(p.lines())      # --peaks reads the file as it is
    assert list(got.lines) == list(mine.lines) == list(p.rows) and sum(len(v) for v in p.lines().values()) == p.n_peaks
    for name, (s, e, *_x) in p.rows.items():
        for k in (0, 1):
            assert got.lines[name][k].tolist() == mine.lines[name][k].tolist() == (s, e)[k].tolist()
    # the signal track and the compared track, through run_files: both files are in ``written``; bigWig beside narrowPeak
    out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "cpm"), 120, coverage_bin=50, coverage_normalize="cpm", coverage_call=100.0,
                             coverage_call_gap=100, coverage_call_length=150, coverage_format="bigwig", **kw)
    g = t.signal(50, 1e6 / t.reads, "cpm")
    assert out[0].error is None and [x.name for x in out[0].written[-2:]] == [STEM + "_coverage.bw", STEM + "_coverage_peaks.narrowPeak"]
    assert out[0].written[-2].read_bytes() == coverage.write_bigwig(tmp_path / "w", STEM, g).read_bytes()
    assert out[0].written[-1].read_bytes() == b"".join(g.call(100.0, 100, 150).text_chunks()) and g.call(100.0, 100, 150).n_peaks > 1
    assert sorted(os.listdir(tmp_path / "cpm")) == sorted(x.name for x in out[0].written)
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "log2"), 120, coverage_control=path, coverage_bin=50, coverage_call=1.0, **kw)
    g = t.compare(c, 50, "log2", 1.0, t.reads / c.reads, 1.0, "none", path)
    assert written[-2].read_bytes() == coverage.write_coverage(tmp_path / "w", STEM, g).read_bytes()
    assert written[-1].read_bytes() == b"".join(g.call(1.0).text_chunks()) and g.call(1.0).n_peaks > 1
    # "auto": called on the track of the run's own estimate; nothing passes: an empty file is written
    _r, w3 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage_call=1e6, mappability_path=None, **dict(kw, coverage_extend="auto"))
    assert w3[-1].name == STEM + "_coverage_peaks.narrowPeak" and w3[-1].read_bytes() == b"" and w3[-2].stat().st_size > 1000
    # an existing file of either suffix is warned about
    with caplog.at_level("WARNING"):
        pipeline.run_files([GOLDEN_BAM], str(tmp_path / "depth"), 120, coverage_call=3, **kw)
    assert sum("_coverage_peaks.narrowPeak' will be overwritten" in r.getMessage() for r in caplog.records) == 1
    assert sum("_coverage.bedGraph' will be overwritten" in r.getMessage() for r in caplog.records) == 1
    # the refusals, before any file is written
    for bad in (dict(coverage_call_gap=5), dict(coverage_call_length=100), dict(coverage_call=float("nan")), dict(coverage_call="1"),
                dict(coverage_call=1.0, coverage_call_gap=-1), dict(coverage_call=1.0, coverage_call_length=0),
                dict(coverage_call=1.0, coverage_call_gap=2 ** 31)):
        with pytest.raises(ValueError, match="coverage_call"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, **bad, **kw)
    assert not (tmp_path / "bad").exists()
