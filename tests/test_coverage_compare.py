"""Treatment against control without a GPU: the host path (``Coverage.compare``, ``HostParts`` over its
``Signal``) against the loop restatement of tests/compare_cases -- runs, totals, text bytes and the bigWig file through the
independent reader of tests/bigwig_out_cases --, ``lg2`` against mpmath, ``factors_of``, the refusals, the command line's exit
codes, and the run: with a control it writes the compared track, without one the bytes it has always written."""
import os
import struct

import numpy as np
import pytest

from pymasc_amd import cli, coverage, pipeline
from tests import bigwig_out_cases as BC
from tests import compare_cases as PC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import sam_writers as SW
from tests import signal_cases as SC
from tests.fake_context import FakeContext

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"
ALL = CC.USES["all"]


def _host(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


@pytest.fixture(scope="module")
def pair():
    """coverage_cases' library as the treatment and a second draw of it as the control; pileups, depth lists and bin sums are
    computed once each and left unchanged."""
    return dict(t=FC.kept(CC.synthetic()), c=FC.kept(CC.synthetic(seed=23, n=9_000)), host={}, sums={})


def _pile(pair, which, extend):
    if (which, extend) not in pair["host"]:
        want = CC.restate(pair[which], BC.REFS, ALL, extend)
        pair["host"][which, extend] = _host(pair[which], BC.REFS, ALL, extend), BC.depth_lists(want, BC.REFS, ALL)
    return pair["host"][which, extend]


def _sums(pair, which, extend, B):
    if (which, extend, B) not in pair["sums"]:
        pair["sums"][which, extend, B] = SC.bin_sums(_pile(pair, which, extend)[1], B)
    return pair["sums"][which, extend, B]


def _factors(t, c, normalize):
    """The factors of ``factors_of``, which must be the restatement's."""
    got = coverage.factors_of(normalize, dict(zip(coverage.TOTALS, t.totals)), dict(zip(coverage.TOTALS, c.totals)), BC.LENGTHS)
    assert got == PC.factors(normalize, t.reads, c.reads, t.fragment_bases, c.fragment_bases, sum(BC.LENGTHS))
    return got


@pytest.mark.parametrize("B", PC.BINS)
@pytest.mark.parametrize("extend", [0, 200])
def test_the_pair_against_the_restatement(tmp_path, pair, extend, B):
    t, c = _pile(pair, "t", extend)[0], _pile(pair, "c", extend)[0]
    assert t.refs == c.refs == BC.REFS and t.reads != c.reads
    for k, (op, normalize) in enumerate(zip(PC.OPS, coverage.NORMALIZE)):
        for op in PC.OPS if k == 0 else (op,):              # every operation with "none", and one with each other normalisation
            a_t, a_c = _factors(t, c, normalize)
            want = PC.restate(_sums(pair, "t", extend, B), _sums(pair, "c", extend, B), op, a_t, a_c, 1.0)
            g = t.compare(c, B, op, a_t, a_c, 1.0, normalize, "dir/input.bam")
            assert PC.rows_got(g) == PC.rows_of(want) and g.totals == PC.totals(want) and (g.bin, g.scale, g.refs) == (B, a_t, BC.REFS)
            assert b"".join(g.text_chunks()) == b"".join(g.text_chunks(chunk=777)) == PC.text_of(want)
            assert g.tail == " bin={} normalize={} scale={!r} control=input.bam compare={} pseudocount=1.0".format(B, normalize, a_t, op)
            assert want["min"] < 0 or op == "ratio"
            if op == "log2":                                # the file, once per bin
                got = BC.read_file(coverage.write_bigwig(tmp_path / "f", "f", g))
                PC.check_file(got, want, BC.REFS, B)
                assert (B > 50 or len(got["zooms"]) >= 3) and got["sections"]
                assert struct.unpack_from("<Qdd", got["summary"]) == (want["covered_bases"], want["min"], want["max"])
    # another pseudocount, and the pileup against itself
    a_t, a_c = _factors(t, c, "cpm")
    want = PC.restate(_sums(pair, "t", extend, B), _sums(pair, "c", extend, B), "ratio", a_t, a_c, 0.25)
    assert PC.rows_got(t.compare(c, B, "ratio", a_t, a_c, 0.25)) == PC.rows_of(want)
    for op in PC.OPS:
        want = PC.restate(_sums(pair, "t", extend, B), _sums(pair, "t", extend, B), op, 0.5, 0.5, 1.0)
        PC.check_self(want, op)
        g = t.compare(t, B, op, 0.5, 0.5, 1.0)
        assert PC.rows_got(g) == PC.rows_of(want) and g.covered_bases == t.signal(B, 1.0).covered_bases


PLANTED = [("log2", 1.0, 1.0, 1.0), ("ratio", 1.0, 1.0, 1.0), ("subtract", 1.0, 1.0, 1.0), ("subtract", PC.TINY, PC.TINY, 1.0),
           ("subtract", 1 / 128, 1 / 128, 1.0), ("log2", 0.37, 1.9, 0.5), ("subtract", 16 / 15, 1.0, 1.0)]


def planted_pair(op, a_t, a_c, p, control=None):
    """(the treatment's pileup, the control's, the restatement at ``P_B``) of the planted pair, the situations asserted."""
    rt, rc = PC.planted_treatment(), PC.planted_control() if control is None else control
    use = [1] * 4
    sums = [SC.bin_sums(BC.depth_lists(CC.restate(r, PC.P_REFS, use, 0), PC.P_REFS, use), PC.P_B) for r in (rt, rc)]
    want = PC.restate(*sums, op, a_t, a_c, p)
    if control is None:
        PC.check_planted(want, op, a_t, a_c, p)
    return _host(rt, PC.P_REFS, use, 0), _host(rc, PC.P_REFS, use, 0), want


@pytest.mark.parametrize("op,a_t,a_c,p", PLANTED)
def test_the_planted_situations(tmp_path, op, a_t, a_c, p):
    t, c, want = planted_pair(op, a_t, a_c, p)
    g = t.compare(c, PC.P_B, op, a_t, a_c, p)
    assert PC.rows_got(g) == PC.rows_of(want) and g.totals == PC.totals(want) and b"".join(g.text_chunks()) == PC.text_of(want)
    assert b"-0\n" not in PC.text_of(want)
    got = BC.read_file(coverage.write_bigwig(tmp_path / "p", "p", g, items_per_section=2, index_block=2, zoom_base=PC.P_ZOOM), 2)
    PC.check_file(got, want, PC.P_REFS, PC.P_B, PC.P_ZOOM, 2)
    if op == "subtract":
        PC.check_planted_zoom(got, want)


def test_a_reference_with_reads_in_one_file_only():
    t, c, want = planted_pair("log2", 1.0, 1.0, 1.0, PC.planted_lonely())
    assert "p3" not in c.runs or list(c.runs) == ["p3"]
    assert list(want["runs"]) == ["p0", "p1", "p2", "p3"] and all(S[1] == 0 for n in ("p0", "p1", "p2") for _s, _e, _v, S in want["runs"][n])
    assert any(S == (0, 20) for _s, _e, _v, S in want["runs"]["p3"])                   # and a bin of p3 that only the control covers
    assert PC.rows_got(t.compare(c, PC.P_B, "log2")) == PC.rows_of(want)
    back = PC.restate(*[SC.bin_sums(BC.depth_lists(CC.restate(r, PC.P_REFS, [1] * 4, 0), PC.P_REFS, [1] * 4), PC.P_B)
                        for r in (PC.planted_lonely(), PC.planted_treatment())], "log2", 1.0, 1.0, 1.0)
    assert PC.rows_got(c.compare(t, PC.P_B, "log2")) == PC.rows_of(back)                # no treatment read on three references


def _mp_bits(x):
    import mpmath
    mpmath.mp.prec = 200
    return [np.float32(float(mpmath.log(mpmath.mpf(float(v)), 2))).tobytes() for v in x]


def test_lg2_against_mpmath():
    """float32(lg2(x)) is float32(log2(x)) for every x here, without exception (log2 by mpmath at 200 bits)."""
    rng = np.random.default_rng(20)
    n = 5_000
    a, b = rng.uniform(0.001, 3.0, 2), rng.integers(0, 3000, (2, n))
    x = np.concatenate([(b[0] * a[0] / 50.0 + 1.0) / (b[1] * a[1] / 50.0 + 1.0), np.exp(rng.uniform(-40, 40, n)), 1.0 + rng.uniform(-1e-3, 1e-3, n),
                        rng.uniform(0.5, 2.0, n)])
    planted = [2.0 ** k for k in (-140, -64, -1, 0, 1, 2, 41, 105)] + [0.7071067811865476, np.nextafter(0.7071067811865476, 0), 1.0 - 2.0 ** -53,
                                                                     1.0 + 2.0 ** -52, 3.0, 1 / 3, 4.0 / 2.0, 1e-300, 1e300]
    x = np.concatenate([x, planted])
    assert x.size == 4 * n + len(planted) and bool(np.all(x > 0))
    got = coverage.lg2(x)
    assert [v.tobytes() for v in got.astype(np.float32)] == _mp_bits(x)
    assert [PC.lg2(float(v)) for v in x] == got.tolist()   # the restatement's loop, to the bit
    for k in (-140, -64, -1, 0, 1, 2, 41, 105):             # powers of two come out exact
        assert coverage.lg2(2.0 ** k) == float(k)


def test_values_as_text():
    for v, text in ((-1.0, "-1"), (-0.5, "-0.5"), (-1 / 3, "-0.333333"), (-4.0e-7, "0"), (-5.0e-7, "0"), (-5.1e-7, "-0.000001"), (-1.5e-6, "-0.000002"),
                    (-1 / 128, "-0.007812"), (-3 / 128, "-0.023438"), (-123456.0, "-123456"), (-0.0, "0"), (0.0, "0"), (2.5, "2.5"), (-100.25, "-100.25")):
        assert coverage.format_value(np.float32(v)) == text == PC.text_value(np.float32(v)), v
        assert coverage.format_value(np.float32(abs(v))) == SC.text_value(np.float32(abs(v)))      # a value that is not negative: as ever


def test_factors_of_and_the_refusals():
    lengths = [1000, 500]
    t, c = dict(reads=30, fragment_bases=900), dict(reads=20, fragment_bases=360)
    assert coverage.COMPARE == ("log2", "ratio", "subtract")
    assert coverage.factors_of("none", t, c, lengths) == (1.0, 30.0 / 20.0) and coverage.factors_of("none", t, c, lengths, 2.0) == (2.0, 3.0)
    assert coverage.factors_of("cpm", t, c, lengths) == (1e6 / 30.0, 1e6 / 20.0)
    assert coverage.factors_of("cpm", t, c, lengths, 7.0) == ((1e6 / 30.0) * 7.0, (1e6 / 20.0) * 7.0)
    assert coverage.factors_of("rpgc", t, c, lengths) == (1500.0 / 900.0, 1500.0 / 360.0)
    assert coverage.factors_of("rpgc", t, c, lengths, 1.0, 2_000) == (2000.0 / 900.0, 2000.0 / 360.0)
    none = dict(reads=0, fragment_bases=0)
    for normalize in coverage.NORMALIZE:                    # no kept read in either file
        assert coverage.factors_of(normalize, none, none, lengths) == (1.0, 1.0)
    assert coverage.factors_of("none", t, none, lengths) == (1.0, 1.0) == coverage.factors_of("none", none, c, lengths)
    for bad in (dict(normalize="rpkm"), dict(genome_size=0), dict(scale=0.0), dict(scale="2"), dict(normalize="none", genome_size=100)):
        with pytest.raises(ValueError, match="coverage_"):
            coverage.factors_of(**dict(dict(normalize="rpgc", totals_t=t, totals_c=c, lengths=lengths), **bad))
    assert coverage.check_pseudocount(2.0 ** -64) == 2.0 ** -64 and coverage.check_pseudocount(-5, "subtract") == -5.0
    for op in ("log2", "ratio"):
        for bad in (2.0 ** -65, 0.0, -1.0, float("nan"), float("inf"), 2.0 ** 40, "1", True):
            with pytest.raises(ValueError, match="coverage_pseudocount"):
                coverage.check_pseudocount(bad, op)
    with pytest.raises(ValueError, match="coverage_compare"):
        coverage.check_pseudocount(1.0, "divide")
    deep = coverage.Coverage({"a": ([0, 10], [10, 20], [1, 1 << 20])}, 5, 0, [("a", 30)])
    flat = coverage.Coverage({"a": ([0], [10], [1])}, 1, 0, [("a", 30)])
    assert deep.compare(flat, 1, "subtract", 2.0 ** 19, 1.0, float("nan")).max == 2.0 ** 39      # subtract ignores the pseudocount
    for kw, text in ((dict(a_t=2.0 ** -65), "2\\^-64"), (dict(a_c=0.0), "2\\^-64"), (dict(a_t=float("nan")), "finite"), (dict(a_c=float("inf")), "finite"),
                     (dict(a_t=2.0 ** 20), "2\\^40"), (dict(pseudo=2.0 ** -65), "2\\^-64"), (dict(pseudo=2.0 ** 40), "2\\^40"),
                     (dict(op="ratio", a_t=1.0, pseudo=2.0 ** -21), "pseudocount\\) / pseudocount"), (dict(op="divide"), "coverage_compare"),
                     (dict(bin=0), "coverage_bin")):
        with pytest.raises(ValueError, match=text):
            deep.compare(flat, **dict(dict(bin=1, op="log2"), **kw))
    with pytest.raises(ValueError, match="2\\^40"):         # each factor against its own track's depth
        flat.compare(deep, 1, "log2", 1.0, 2.0 ** 20)
    assert flat.compare(deep, 1, "ratio", 2.0 ** 20, 1.0, 1.0).n_runs == 2 and deep.compare(flat, 1, "ratio", 1.0, 1.0, 2.0 ** -19).max < 2.0 ** 40
    with pytest.raises(ValueError, match="chosen references of the control"):
        deep.compare(coverage.Coverage({"a": ([0], [10], [1])}, 1, 0, [("a", 31)]))
    with pytest.raises(ValueError, match="lengths"):
        deep.compare(coverage.Coverage({"a": ([0], [10], [1])}, 1, 0))


def test_options(monkeypatch, tmp_path):
    control = str(tmp_path / "input.bam")
    open(control, "wb").close()
    os.mkfifo(tmp_path / "fifo")
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base + ["--coverage"])
    assert (a.coverage_control, a.coverage_compare, a.coverage_pseudocount) == (None, None, None)
    a = cli.parse_args(base + ["--coverage-control", control, "--coverage-extend", "200"])
    assert a.coverage and a.coverage_control == control and cli.parse_args(["-", "--coverage-control", control, "--coverage-extend", "200"]).coverage
    a = cli.parse_args(base + ["--coverage-control", control, "--coverage-compare", "subtract", "--coverage-pseudocount", "-3"])
    assert (a.coverage_compare, a.coverage_pseudocount) == ("subtract", -3.0)
    for bad in (["--coverage-compare", "ratio"], ["--coverage-pseudocount", "2"], ["--coverage-control", str(tmp_path / "missing.bam")],
                ["--coverage-control", "-"], ["--coverage-control", str(tmp_path / "fifo")], ["--coverage-control", str(tmp_path)],
                ["--coverage-control", control, "--coverage-compare", "divide"], ["--coverage-control", control, "--coverage-pseudocount", "0"],
                ["--coverage-control", control, "--coverage-pseudocount", "x"], ["--coverage-control", control, "--coverage-pseudocount", "nan"],
                ["--coverage-control", control, "--coverage-pseudocount", "inf"], ["--coverage-control", control, "--coverage-pseudocount", "1e13"],
                ["--coverage-control", control, "--coverage-compare", "ratio", "--coverage-pseudocount", "-1"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    text = " ".join(cli.get_parser().format_help().split())
    assert "--coverage-control FILE" in text and "--coverage-compare {log2,ratio,subtract}" in text and "--coverage-pseudocount X" in text
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for more, want in ((["--coverage-control", control], dict(coverage=True, coverage_control=control)),
                       (["--coverage-control", control, "--coverage-compare", "ratio", "--coverage-pseudocount", "0.5", "--coverage-bin", "50"],
                        dict(coverage=True, coverage_control=control, coverage_compare="ratio", coverage_pseudocount=0.5, coverage_bin=50))):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert {k: v for k, v in seen.items() if k.startswith("coverage")} == want


def _golden(extend, mapq=10):
    from pymasc_amd.bam import BamReader
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(mapq))]
    return refs, cols


@pytest.fixture(scope="module")
def control(tmp_path_factory):
    """(a control file over the golden file's references: every third of its reads, moved 17 bases on; its reads as columns)."""
    refs, cols = _golden(0)
    rows = [(int(r), int(p) + 17, int(l), int(s)) for r, p, l, s in list(zip(*cols))[::3] if int(p) + 17 + int(l) <= refs[int(r)][1]]
    recs = [SW.rec("c%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(rows)]
    d = tmp_path_factory.mktemp("coverage_compare")
    return SW.write_twins(d, "input", refs, recs)[1], rows


def test_the_run(tmp_path, control):
    path, rows = control
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext(), coverage_extend=200)
    refs, cols = _golden(200)
    names, lengths = [n for n, _l in refs], [l for _n, l in refs]
    t = coverage.count_host(*cols, names, lengths, [1] * len(refs), 200)
    c = _host(rows, refs, [1] * len(refs), 200)
    assert c.reads == len(rows) > 100
    # no control: the bytes the run has always written
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 120, coverage=True, coverage_control=None, coverage_compare="log2",
                               coverage_pseudocount=1.0, **kw)
    assert written[-1].read_bytes() == coverage.write_coverage(tmp_path / "want", STEM, t).read_bytes()
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain50"), 120, coverage=True, coverage_bin=50, coverage_normalize="cpm", **kw)
    assert written[-1].read_bytes() == coverage.write_coverage(tmp_path / "want", STEM, t.signal(50, 1e6 / t.reads, "cpm")).read_bytes()
    # a control implies coverage: log2 at the defaults, the control scaled to the treatment's reads
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "log2"), 120, coverage_control=path, coverage_bin=50, **kw)
    g = t.compare(c, 50, "log2", 1.0, t.reads / c.reads, 1.0, "none", path)
    head = ('track type=bedGraph name="{}" description="pymasc_amd fragment pileup extend=200 reads={}" bin=50 normalize=none scale=1.0 '
            'control=input.bam compare=log2 pseudocount=1.0\n').format(STEM, t.reads).encode()
    text = written[-1].read_bytes()
    assert written[-1].name == STEM + "_coverage.bedGraph" and text == head + b"".join(g.text_chunks()) and g.n_runs > 50 and g.min < 0 < g.max
    assert b"\t-" in text
    # the bigWig file through run_files, cpm, subtract
    out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "bw"), 120, coverage_control=path, coverage_bin=50, coverage_normalize="cpm",
                             coverage_scale=2.0, coverage_compare="subtract", coverage_format="bigwig", coverage_compress=True, **kw)
    g2 = t.compare(c, 50, "subtract", (1e6 / t.reads) * 2.0, (1e6 / c.reads) * 2.0, 1.0)
    got, want = BC.read_file(out[0].written[-1]), BC.read_file(coverage.write_bigwig(tmp_path / "w", STEM, g2))
    assert out[0].error is None and got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in want.items() if k != "compressed"}
    assert struct.unpack_from("<Qdd", got["summary"]) == (g2.covered_bases, g2.min, g2.max) and g2.min < 0
    assert sorted(os.listdir(tmp_path / "bw")) == sorted(p.name for p in out[0].written)
    # "auto": the control is piled up with the treatment's estimate
    _r, w3 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage_control=path, coverage_compare="ratio", coverage_pseudocount=0.5,
                          mappability_path=None, **dict(kw, coverage_extend="auto"))
    line = w3[-1].read_bytes().split(b"\n", 1)[0]
    assert line.endswith(b" control=input.bam compare=ratio pseudocount=0.5") and b"extend=200" not in line
    # the refusals, before any file is written
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    for bad in (dict(coverage_compare="ratio"), dict(coverage_pseudocount=2.0), dict(coverage_control=path, coverage_compare="divide"),
                dict(coverage_control=path, coverage_pseudocount=0.0), dict(coverage_control=path, coverage_pseudocount=2.0 ** 40),
                dict(coverage_control=str(fifo)), dict(coverage_control="-")):
        with pytest.raises(ValueError, match="coverage_"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, **bad, **kw)
    assert not (tmp_path / "bad").exists()
    # a control over other references: run raises, run_files skips the file as it does for the fingerprint's control
    other = SW.write_twins(tmp_path, "other", [(n, l + 1) for n, l in refs], [])[1]
    with pytest.raises(ValueError, match="the chosen references of the coverage control"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, coverage_control=other, **kw)
    out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "skipped"), 120, coverage_control=other, **kw)
    assert isinstance(out[0].error, ValueError) and out[0].written == []
