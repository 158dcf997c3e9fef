"""The fragment pileup without a GPU: the host checker against the loop restatement of tests/coverage_cases, the
file, the options, and the host path of the run."""
import os

import numpy as np
import pytest

from pymasc_amd import cli, coverage, pipeline, stats
from pymasc_amd.bam import BamReader
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests.fake_context import FakeContext

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
NAMES = [n for n, _l in CC.REFS]
LENGTHS = [l for _n, l in CC.REFS]


@pytest.fixture(scope="module")
def library():
    reads = FC.kept(CC.synthetic())
    assert 18_000 < len(reads) < 22_000 and {r[3] for r in reads} == {0, 1}
    return dict(reads=reads, less=FC.masked(reads, CC.REFS, CC.MASK), want={})


def _want(library, extend, masked=False):
    """The restatement, computed once per parameter set and left unchanged."""
    if (extend, masked) not in library["want"]:
        library["want"][extend, masked] = CC.restate(library["less" if masked else "reads"], CC.REFS, CC.USES["all"], extend)
    return library["want"][extend, masked]


def _host(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_count_host_equals_the_restatement(library, extend):
    want = _want(library, extend)
    CC.check_situations(library["reads"], want, extend)
    got = _host(library["reads"], CC.REFS, CC.USES["all"], extend)
    assert got.rows() == CC.rows_of(want) and got.totals == CC.totals(want) and got == CC.as_coverage(want, extend)
    assert want["n_runs"] > 1000 and want["fragment_bases"] == want["extents"]              # the identity of the totals
    part = CC.select(want, CC.REFS, library["reads"], CC.USES["no middle"], extend)
    assert list(part["runs"]) == ["f0", "f2"] and part["reads"] < want["reads"]
    got = _host(library["reads"], CC.REFS, CC.USES["no middle"], extend)
    assert got.rows() == CC.rows_of(part) and got.totals == CC.totals(part)
    less = _want(library, extend, True)
    assert less["reads"] < want["reads"]
    assert _host(library["less"], CC.REFS, CC.USES["all"], extend).rows() == CC.rows_of(less)
    # batches add up
    half = len(library["reads"]) // 2
    acc = coverage.HostCount(NAMES, LENGTHS, CC.USES["all"], extend)
    for chunk in (library["reads"][:half], library["reads"][half:]):
        acc.add(*[np.array(c) for c in zip(*chunk)])
    assert acc.result() == CC.as_coverage(want, extend)


def test_tile_edges_and_small_cases_by_hand():
    header = open(os.path.join(os.path.dirname(fx.GOLDEN), os.pardir, "include", "pymasc_amd_ingest.h")).read()
    assert "#define PMX_COVERAGE_TILE {}u\n".format(coverage.TILE) in header                # the module's tile is the library's
    refs, reads = CC.tile_case()
    assert [l % CC.T for _n, l in refs] == [CC.T - 1, 0, 1]
    for extend in (0, 200):
        want = CC.restate(reads, refs, [1, 1, 1], extend)
        assert want["fragment_bases"] == want["extents"] and _host(reads, refs, [1, 1, 1], extend).rows() == CC.rows_of(want)
    refs = [("a", 10), ("b", 3)]
    reads = [(0, 1, 2, 0), (0, 3, 2, 0), (0, 4, 3, 1), (0, 9, 5, 0), (1, 3, 4, 0), (0, 30, 4, 0), (1, 1, 1, 1)]
    # a: 1..2 and 3..4 abut at depth 1; 4..6 overlaps 3..4 in one base; 9..13 is clipped to 9..10; 30.. adds nothing
    want = CC.restate(reads, refs, [1, 1], 0)
    assert want["runs"] == {"a": [(0, 3, 1), (3, 4, 2), (4, 6, 1), (8, 10, 1)], "b": [(0, 1, 1), (2, 3, 1)]}
    assert CC.totals(want) == (6, 6, 10, 11, 2) and want["extents"] == 11
    assert _host(reads, refs, [1, 1], 0).rows() == CC.rows_of(want)
    want = CC.restate(reads, refs, [1, 1], 3)                                               # three bases from the 5' end
    assert want["runs"]["b"] == [(0, 1, 1), (2, 3, 1)] and _host(reads, refs, [1, 1], 3).rows() == CC.rows_of(want)
    empty = _host([], refs, [1, 0], 0)
    assert empty.rows() == [] and empty.totals == (0, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="no chosen reference"):
        _host(reads, refs, [0, 0], 0)


def test_file_round_trip(tmp_path, library):
    want = _want(library, 200)
    c = CC.as_coverage(want, 200)
    path = coverage.write_coverage(tmp_path / "x.y", "x.y", c)
    assert path.name == "x.y_coverage.bedGraph" and sorted(os.listdir(tmp_path)) == [path.name]
    blob = path.read_bytes()
    head, _nl, body = blob.partition(b"\n")
    assert head == b'track type=bedGraph name="x.y" description="pymasc_amd fragment pileup extend=200 reads=%d"' % want["reads"]
    assert body == CC.text_of(want) and b"".join(c.text_chunks(1000)) == body
    name, back = coverage.read_coverage(path)
    assert name == "x.y" and back == c and back.totals == CC.totals(want)
    own = coverage.Coverage({"b": ([0, 2], [1, 3], [1, 7])}, 2, 0)
    assert coverage.write_coverage(tmp_path / "o", "o", own).read_bytes().startswith(b'track type=bedGraph name="o" description="pymasc_amd '
                                                                                     b'fragment pileup extend=read reads=2"\nb\t0\t1\t1\n')
    assert coverage.read_coverage(tmp_path / "o_coverage.bedGraph")[1] == own != coverage.Coverage({"b": ([0, 2], [1, 3], [1, 7])}, 2, 5)
    none = coverage.Coverage({}, 0, 0)
    assert coverage.read_coverage(coverage.write_coverage(tmp_path / "n", "n", none))[1] == none
    with pytest.raises(ValueError):
        coverage.Coverage({"b": ([0], [1, 3], [1])}, 1, 0)


def test_options(tmp_path, capsys):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert (a.coverage, a.coverage_extend) == (False, None)
    assert cli.parse_args(base + ["--coverage"]).coverage_extend is None
    for text, value in (("150", 150), ("auto", "auto"), ("read", "read")):
        a = cli.parse_args(base + ["--coverage-extend", text])
        assert a.coverage and a.coverage_extend == value                                    # implies --coverage
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    for bad in (["--coverage-extend", "0"], ["--coverage-extend", "-3"], ["--coverage-extend", "x"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    assert "argument --coverage-extend must be > 0." in capsys.readouterr().err              # _NaturalNumber's message
    for reads, more in (("-", ["--coverage"]), ("-", ["--coverage-extend", "auto"]), (str(fifo), ["--coverage"])):
        args = [reads, "-d", "100", "-r", "36"] + more
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(args)
        assert ei.value.code == 2 and cli.main(args) == 2                                   # before anything runs
    assert "auto reads the file once more" in capsys.readouterr().err
    assert cli.parse_args(["-", "-d", "100", "-r", "36", "--coverage-extend", "200"]).coverage_extend == 200
    assert cli.parse_args(["-", "-d", "100", "-r", "36", "--coverage-extend", "read"]).coverage
    assert "_coverage.bedGraph" in cli.get_parser().format_help() and "12.4 GB" in cli.get_parser().format_help()


def test_options_reach_run_files(monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cli.main(["a.bam", "--skip-plots"]) == 0
    assert not any(k.startswith("coverage") for k in seen)
    for more, want in ((["--coverage"], dict(coverage=True)), (["--coverage-extend", "auto"], dict(coverage=True)),
                       (["--coverage-extend", "read"], dict(coverage=True, coverage_extend=0)),
                       (["--coverage-extend", "150"], dict(coverage=True, coverage_extend=150))):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert {k: v for k, v in seen.items() if k.startswith("coverage")} == want


def _golden_reads(mapq=10):
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, b.lengths))
        cols = [np.concatenate(x) for x in zip(*b.batches(mapq))]
    return refs, cols


def test_pipeline_writes_the_track_and_nothing_else_changes(tmp_path):
    refs, cols = _golden_reads()
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, stats=True, complexity=True)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 120, context=FakeContext(), **kw)
    r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 120, context=FakeContext(), coverage=True, coverage_extend=200, **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_coverage.bedGraph"] and len(w0) == 4
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c = coverage.read_coverage(w1[-1])
    want = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), 200)
    assert name == stem and c == want and c.extend == 200 and c.n_runs > 100 and c.reads == cols[0].size
    # "auto": the run's own estimate, with or without _stats.tab, on the chosen chromosomes
    est = stats.genome_wide_stats(r1, 36).est_lib_len
    chosen = [refs[0][0], refs[2][0]]
    use = [1 if n in chosen else 0 for n, _l in refs]
    for more in (dict(stats=True), dict(stats=False)):
        out = tmp_path / ("auto%d" % more["stats"])
        _r2, w2 = pipeline.run(GOLDEN_BAM, str(out), 120, context=FakeContext(), references=chosen, coverage=True,
                               **{**kw, **more, "complexity": False})
        assert [p.name.rsplit("_", 1)[-1] for p in w2] == ["cc.tab", "nreads.tab"] + ["stats.tab"] * more["stats"] + ["coverage.bedGraph"]
        _n, c2 = coverage.read_coverage(w2[-1])
        assert c2.extend == stats.genome_wide_stats(_r2, 36).est_lib_len == est > 36
        if more["stats"]:
            assert ["Estimated library length", str(c2.extend)] in [ln.rstrip("\n").split("\t") for ln in open(w2[-2])]
        assert c2 == coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, c2.extend)
        assert list(c2.runs) == [chosen[0]]             # (the file's reads are all on its first chromosome)
    with BamReader(GOLDEN_BAM) as b:
        assert b.coverage(10, chosen, c2.extend) == c2
    for bad in (-1, "read", 1.5, True):
        with pytest.raises(ValueError, match="coverage_extend"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, context=FakeContext(), coverage=True, coverage_extend=bad, **kw)
    assert not (tmp_path / "bad").exists()


def test_a_stream_with_auto_is_refused_before_it_is_read(tmp_path):
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)             # (nobody writes to it: a run that opened it would wait)
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext(), coverage=True)
    with pytest.raises(ValueError, match="is a stream and cannot be read twice"):
        pipeline.run(str(fifo), str(tmp_path / "out"), 120, **kw)
    out = pipeline.run_files([str(fifo), GOLDEN_BAM], str(tmp_path / "files"), 120, **kw)
    assert isinstance(out[0].error, ValueError) and "cannot be read twice" in str(out[0].error) and out[0].written == []
    assert out[1].error is None and out[1].written[-1].name == "ENCFF000RMB-test_coverage.bedGraph"
