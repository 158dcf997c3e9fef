"""The p-score track without a GPU: ``lnfact`` and ``poisson_values`` against the loop restatement of
tests/poisson_cases to the bit and against mpmath, the host path (``Coverage.poisson``, ``HostParts`` over its ``Signal``) against
the restatement -- runs, totals, text bytes and the bigWig file through the independent reader of tests/bigwig_out_cases --, the
peaks of a p-score track with column 8 filled, the refusals, the command line's exit codes, and the run: with the option it writes
the p-score track, without it the bytes it has always written."""
import os
import struct

import numpy as np
import pytest

from pymasc_amd import cli, coverage, pipeline
from tests import bigwig_out_cases as BC
from tests import call_cases as LC
from tests import fixtures as fx
from tests import poisson_cases as PS
from tests import sam_writers as SW
from tests.fake_context import FakeContext

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"


def _host(reads, refs, extend=0):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), extend)


def test_lnfact():
    n = 70_001
    F = coverage.lnfact(n)
    assert F.dtype == np.float64 and F.tolist() == PS.lnfact(n) and F[0] == F[1] == 0.0 and F[2] == PS.ln(2.0)     # the loop, to the bit
    assert [coverage.lnfact(m).tolist() for m in (1, 2, 3)] == [[0.0], [0.0, 0.0], [0.0, 0.0, PS.ln(2.0)]]
    import mpmath
    mpmath.mp.dps = 60
    big = coverage.lnfact((1 << 20) + 1)
    assert big.size == (1 << 20) + 1 and big[:n].tolist() == F.tolist()        # an entry does not depend on the table's length
    worst = 0.0
    for i in list(range(2, 300)) + list(range(300, 1 << 20, 7919)) + [65_536, 1 << 20]:
        true = mpmath.loggamma(i + 1)
        worst = max(worst, float(abs(mpmath.mpf(float(big[i])) - true) / true))
    print("lnfact: the largest relative error against loggamma", worst)
    assert worst <= 1e-12
    for bad in (0, -1, (1 << 20) + 2, 2.5, "3", True):
        with pytest.raises(ValueError, match="ln\\(i!\\)"):
            coverage.lnfact(bad)


CORNERS = [(65_536, 1.0), (50_000, 49_999.9), (2, 1.9999999), (1, 1e-9)]


@pytest.fixture(scope="module")
def pairs():
    """2 x 10^4 pairs on a fixed seed: l log-uniform in [10^-3, 3000], k from floor(l) + 1 up to 2000 above it; the planted corners."""
    rng = np.random.default_rng(718_6)
    lam = 10.0 ** rng.uniform(-3.0, np.log10(3000.0), 20_000)
    k = np.floor(lam).astype(np.int64) + 1 + rng.integers(0, 2001, lam.size)
    k, lam = np.concatenate([k, [c[0] for c in CORNERS]]), np.concatenate([lam, [c[1] for c in CORNERS]])
    F = coverage.lnfact(int(k.max()) + 1)
    return k, lam, F, coverage.poisson_values(k, lam, F)


def test_poisson_values_against_the_restatement(pairs):
    k, lam, F, got = pairs
    assert got.dtype == np.float32 and bool(np.all(k > lam))
    assert [PS.value(int(a), float(b)).tobytes() for a, b in zip(k, lam)] == [v.tobytes() for v in got]
    S, steps = coverage.poisson_series(k[:500], lam[:500])
    assert [PS.series(int(a), float(b)) for a, b in zip(k[:500], lam[:500])] == list(zip(S.tolist(), steps.tolist()))
    # not enriched: k below l and k == l exactly, among enriched ones
    F = coverage.lnfact(10)
    v = coverage.poisson_values([3, 4, 5, 0, 0, 9], [4.0, 4.0, 4.0, 1e-3, 2.5, 9.0], F)
    assert v.tolist() == [0.0, 0.0, float(PS.value(5, 4.0)), 0.0, 0.0, 0.0] and v[2] > 0
    assert coverage.poisson_values([], [], F).size == 0


def test_poisson_values_against_mpmath(pairs):
    """Every float32 within 1 float32 ulp of the float32 of the true -log10 P(X >= k | l) (mpmath at 60 digits), and the share that
    differs at all at most 10^-3 (a condition, not a measurement).  Seen: 0 of 20 004 differ."""
    import mpmath
    mpmath.mp.dps = 60
    k, lam, F, got = pairs
    differ = 0
    for a, b, v in zip(k.tolist(), lam.tolist(), got):
        true = np.float32(float(-mpmath.log10(mpmath.gammainc(a, 0, mpmath.mpf(b), regularized=True))))
        if true.tobytes() != v.tobytes():
            differ += 1
            assert abs(int(true.view(np.int32)) - int(v.view(np.int32))) <= 1, (a, b, true, v)
    print("poisson_values: float32 values that differ from the truth's:", differ, "of", k.size)
    assert differ <= 1e-3 * k.size


@pytest.fixture(scope="module")
def planted():
    """(the treatment's pileup, the control's, {B: the two pileups' bin sums}) of the planted pair, computed once."""
    rt, rc = PS.planted_treatment(), PS.planted_control()
    return _host(rt, PS.P_REFS), _host(rc, PS.P_REFS), {B: PS.sums_of(rt, rc, PS.P_REFS, B) for B in PS.BINS}


@pytest.mark.parametrize("a_c,small,large", PS.P_SETS)
def test_the_planted_situations(tmp_path, planted, a_c, small, large):
    t, c, sums = planted
    for B in PS.BINS:
        want = PS.restate(*sums[B], B, a_c, small, large)
        if B == PS.P_B:
            PS.check_planted(want, a_c, small, large)
        g = t.poisson(c, B, a_c, small, large, "dir/input.bam")
        assert PS.rows_got(g) == PS.rows_of(want) and g.totals == PS.totals(want) and (g.bin, g.scale, g.refs, g.pscore) == (B, 1.0, PS.P_REFS, True)
        assert b"".join(g.text_chunks()) == b"".join(g.text_chunks(chunk=3)) == PS.text_of(want) and want["min"] >= 0.0
        assert g.tail == " bin={} normalize=none scale=1.0 control=input.bam poisson={},{}".format(B, small, large)
        if B in (1, PS.P_B):
            kw = dict(items_per_section=2, index_block=2, zoom_base=PS.P_ZOOM)
            got = BC.read_file(coverage.write_bigwig(tmp_path / "p", "p", g, **kw), 2)
            PS.check_file(got, want, PS.P_REFS, B, PS.P_ZOOM, 2)
            assert struct.unpack_from("<Qdd", got["summary"]) == (want["covered_bases"], want["min"], want["max"])


def test_the_series_and_the_scan_edges(planted):
    st, sc = PS.sums_of(PS.deep_treatment(), PS.deep_control(), PS.D_REFS, PS.D_B)
    want = PS.restate(st, sc, PS.D_B, 1.0, 0, 0)
    PS.check_deep(want)
    g = _host(PS.deep_treatment(), PS.D_REFS).poisson(_host(PS.deep_control(), PS.D_REFS), PS.D_B, 1.0, 0, 0)
    assert PS.rows_got(g) == PS.rows_of(want) and g.totals == PS.totals(want)
    for n in PS.SCAN_SMALL + PS.SCAN_LARGE[1:2]:
        rt, rc = PS.scan_reads(n)
        want = PS.restate(*PS.sums_of(rt, rc, [("s", n)], 1), 1, 1.0, *PS.SCAN_WINDOWS)
        g = _host(rt, [("s", n)]).poisson(_host(rc, [("s", n)]), 1, 1.0, *PS.SCAN_WINDOWS)
        assert PS.rows_got(g) == PS.rows_of(want) and g.totals == PS.totals(want) and want["n_runs"] >= 1
    # a reference with reads in one file only, either way round, and a pileup against itself
    t, c, _sums = planted
    lone = PS.planted_lonely()
    want = PS.restate(*PS.sums_of(PS.planted_treatment(), lone, PS.P_REFS, PS.P_B), PS.P_B, 1.0, *PS.P_WINDOWS)
    assert list(want["runs"]) == ["p0", "p1", "p2", "p3"] and PS.rows_got(t.poisson(_host(lone, PS.P_REFS), PS.P_B, 1.0, *PS.P_WINDOWS)) == PS.rows_of(want)
    back = PS.restate(*PS.sums_of(lone, PS.planted_treatment(), PS.P_REFS, PS.P_B), PS.P_B, 1.0, *PS.P_WINDOWS)
    assert list(back["runs"]) == ["p1"] and PS.rows_got(_host(lone, PS.P_REFS).poisson(t, PS.P_B, 1.0, *PS.P_WINDOWS)) == PS.rows_of(back)
    same = PS.restate(*PS.sums_of(PS.planted_treatment(), PS.planted_treatment(), PS.P_REFS, PS.P_B), PS.P_B, 1.0, 0, 0)
    assert all(float(v) == 0.0 for rows in same["runs"].values() for _s, _e, v, _S in rows)        # l >= c_0 = k: nothing is enriched
    assert PS.rows_got(t.poisson(t, PS.P_B, 1.0, 0, 0)) == PS.rows_of(same)


def _golden(mapq=10):
    from pymasc_amd.bam import BamReader
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(mapq))]
    return refs, cols


def _shifted(refs, cols):
    """Every third read of the golden file, moved 17 bases on."""
    return [(int(r), int(p) + 17, int(l), int(s)) for r, p, l, s in list(zip(*cols))[::3] if int(p) + 17 + int(l) <= refs[int(r)][1]]


def test_the_golden_file_against_itself_shifted():
    """The golden file's reads (all on chr1 within 150 000 bases) moved onto a reference of their own span, so that the restatement's
    loops can walk every base; the control is every third read 17 bases on."""
    refs, cols = _golden()
    assert set(cols[0].tolist()) == {0}
    first = int(cols[1].min()) - 1
    g_refs = [("g0", int(cols[1].max()) - first + 300), ("g1", 777)]
    rt = sorted((0, int(p) - first, int(l), int(s)) for p, l, s in zip(*cols[1:]))
    rc = [(0, p + 17, l, s) for _r, p, l, s in rt[::3]]
    t, c = _host(rt, g_refs, 200), _host(rc, g_refs, 200)
    a_c = coverage.factors_of("none", dict(reads=t.reads, fragment_bases=0), dict(reads=c.reads, fragment_bases=0), [])[1]
    assert a_c == t.reads / c.reads and t.max_depth > 3
    for B, windows in ((50, PS.WINDOWS), (7, (100, 1000))):
        want = PS.restate(*PS.sums_of(rt, rc, g_refs, B, 200), B, a_c, *windows)
        g = t.poisson(c, B, a_c, *windows)
        assert PS.rows_got(g) == PS.rows_of(want) and g.totals == PS.totals(want) and want["n_runs"] > 100 and want["max"] > 1.0 > want["min"] == 0.0


def test_the_peaks_of_a_p_score_track(planted):
    t, c, sums = planted
    g = t.poisson(c, PS.P_B, 1.0, *PS.P_WINDOWS)
    want = PS.restate(*sums[PS.P_B], PS.P_B, 1.0, *PS.P_WINDOWS)
    for args in ((0.5, 0, 50), (0.0, 100, 1), (2.0, 30, 50)):
        rules = LC.restate(LC.rows_of_want(want), *args)
        p = g.call(*args)
        assert p.pscore and LC.peaks_got(p) == LC.peaks_of(rules) and p.totals == LC.totals(rules)
        assert b"".join(p.text_chunks()) == b"".join(p.text_chunks(chunk=1)) == PS.narrowpeak_of(rules)
        plain = coverage.Signal(g.runs, g.bin, g.scale, g.refs).call(*args)                 # the same runs without the flag: -1, as ever
        assert not plain.pscore and b"".join(plain.text_chunks()) == LC.text_of(rules) and plain != p
    rules = LC.restate(LC.rows_of_want(want), 0.5, 0, 50)
    assert rules["n_peaks"] >= 2 and all(ln.split(b"\t")[6] == ln.split(b"\t")[7] != b"-1" for ln in PS.narrowpeak_of(rules).splitlines())


def test_the_refusals():
    deep = coverage.Coverage({"a": ([0, 10], [10, 20], [1, (1 << 20) + 1])}, 5, 0, [("a", 30)])
    edge = coverage.Coverage({"a": ([0, 10], [10, 20], [1, 1 << 20])}, 5, 0, [("a", 30)])
    flat = coverage.Coverage({"a": ([0], [10], [1])}, 1, 0, [("a", 30)])
    none = coverage.Coverage({}, 0, 0, [("a", 30)])
    assert coverage.LAMBDA_WINDOWS == (1000, 10000) and coverage.check_lambda_windows([0, (1 << 31) - 1]) == (0, (1 << 31) - 1)
    assert coverage.COMPARE == ("log2", "ratio", "subtract")                    # the score is no fourth operation
    assert edge.poisson(flat, 1).n_runs == 2 and flat.poisson(edge, 1, 2.0 ** 19).n_runs == 1 and none.poisson(flat, 1).n_runs == 0
    with pytest.raises(ValueError, match="max_depth is above 2\\^20"):
        deep.poisson(flat, 1)
    for kw, text in ((dict(small=-1), "coverage_lambda"), (dict(large=1 << 31), "coverage_lambda"), (dict(small=2.5), "coverage_lambda"),
                     (dict(small="1000"), "coverage_lambda"), (dict(large=True), "coverage_lambda"), (dict(a_c=2.0 ** -65), "2\\^-64"),
                     (dict(a_c=0.0), "2\\^-64"), (dict(a_c=float("nan")), "finite"), (dict(a_c=float("inf")), "finite"), (dict(a_c="1"), "number"),
                     (dict(bin=0), "coverage_bin"), (dict(bin=65537), "coverage_bin")):
        with pytest.raises(ValueError, match=text):
            flat.poisson(flat, **dict(dict(bin=1), **kw))
    with pytest.raises(ValueError, match="2\\^40"):         # the factor against the control's depth
        flat.poisson(edge, 1, 2.0 ** 20)
    with pytest.raises(ValueError, match="the control has no covered base"):
        flat.poisson(none, 1)
    with pytest.raises(ValueError, match="chosen references of the control"):
        flat.poisson(coverage.Coverage({"a": ([0], [10], [1])}, 1, 0, [("a", 31)]))
    with pytest.raises(ValueError, match="lengths"):
        flat.poisson(coverage.Coverage({"a": ([0], [10], [1])}, 1, 0))
    for bad in ((1000,), (1, 2, 3), None, 5, "ab"):
        with pytest.raises(ValueError, match="coverage_lambda"):
            coverage.check_lambda_windows(bad)
    assert coverage.poisson_tail("x/y/in.bam", 0, 7) == " control=in.bam poisson=0,7"


def test_options(monkeypatch, tmp_path):
    control = str(tmp_path / "input.bam")
    open(control, "wb").close()
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base + ["--coverage"])
    assert (a.coverage_poisson, a.coverage_lambda) == (False, None)
    a = cli.parse_args(base + ["--coverage-control", control, "--coverage-poisson", "--coverage-lambda", "0", "5000", "--coverage-extend", "200"])
    assert a.coverage and a.coverage_poisson and a.coverage_lambda == [0, 5000]
    assert cli.parse_args(base + ["--coverage-control", control, "--coverage-poisson", "--coverage-normalize", "none", "--coverage-scale", "1"]).coverage_poisson
    on = ["--coverage-control", control, "--coverage-poisson"]
    for bad in (["--coverage-poisson"], ["--coverage-lambda", "100", "1000"], ["--coverage-control", control, "--coverage-lambda", "100", "1000"],
                on + ["--coverage-compare", "log2"], on + ["--coverage-compare", "subtract"], on + ["--coverage-pseudocount", "1"],
                on + ["--coverage-normalize", "cpm"], on + ["--coverage-normalize", "rpgc", "--coverage-genome-size", "1000"],
                on + ["--coverage-scale", "2"], on + ["--coverage-lambda", "100"], on + ["--coverage-lambda", "-1", "100"],
                on + ["--coverage-lambda", "100", str(1 << 31)], on + ["--coverage-lambda", "x", "100"], on + ["--coverage-lambda", "1.5", "100"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    text = " ".join(cli.get_parser().format_help().split())
    assert "--coverage-poisson" in text and "--coverage-lambda S L" in text
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for more, want in ((on, dict(coverage=True, coverage_control=control, coverage_poisson=True)),
                       (on + ["--coverage-lambda", "0", "20000", "--coverage-bin", "50", "--coverage-call", "3"],
                        dict(coverage=True, coverage_control=control, coverage_poisson=True, coverage_lambda=(0, 20000), coverage_bin=50, coverage_call=3.0)),
                       (["--coverage-control", control], dict(coverage=True, coverage_control=control))):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert {k: v for k, v in seen.items() if k.startswith("coverage")} == want


@pytest.fixture(scope="module")
def control(tmp_path_factory):
    refs, cols = _golden()
    rows = _shifted(refs, cols)
    recs = [SW.rec("c%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(rows)]
    return SW.write_twins(tmp_path_factory.mktemp("coverage_poisson"), "input", refs, recs)[1], rows


def test_the_run(tmp_path, control):
    path, rows = control
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext(), coverage_extend=200)
    refs, cols = _golden()
    t = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), 200)
    c = _host(rows, refs, 200)
    a_c = t.reads / c.reads
    # without the option: the bytes of today's calls, the narrowPeak's column 8 at -1
    _r, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "log2"), 120, coverage_control=path, coverage_bin=50, coverage_call=0.5, coverage_poisson=False,
                          coverage_lambda=(1000, 10000), **kw)
    g0 = t.compare(c, 50, "log2", 1.0, a_c, 1.0, "none", path)
    assert [p.name for p in w0[-2:]] == [STEM + "_coverage.bedGraph", STEM + "_coverage_peaks.narrowPeak"]
    assert w0[-2].read_bytes() == coverage.write_coverage(tmp_path / "want", STEM, g0).read_bytes()
    lines = w0[-1].read_bytes()
    assert lines == b"".join(g0.call(0.5).text_chunks()) and lines.count(b"\n") > 3 and all(ln.split(b"\t")[7:9] == [b"-1", b"-1"] for ln in lines.splitlines())
    # with it: the p-score track, and the peaks with the score in column 8
    _r, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "ps"), 120, coverage_control=path, coverage_bin=50, coverage_poisson=True, coverage_call=1.0,
                          coverage_call_length=50, **kw)
    g = t.poisson(c, 50, a_c, 1000, 10000, path)
    head = ('track type=bedGraph name="{}" description="pymasc_amd fragment pileup extend=200 reads={}" bin=50 normalize=none scale=1.0 '
            'control=input.bam poisson=1000,10000\n').format(STEM, t.reads).encode()
    assert w1[-2].read_bytes() == head + b"".join(g.text_chunks()) and g.n_runs > 50 and g.min == 0.0 and g.max > 1.0
    peaks = g.call(1.0, 30, 50)
    lines = w1[-1].read_bytes()
    assert lines == b"".join(peaks.text_chunks()) and peaks.n_peaks >= 1
    assert all(ln.split(b"\t")[6] == ln.split(b"\t")[7] and ln.split(b"\t")[8] == b"-1" and float(ln.split(b"\t")[7]) >= 1.0 for ln in lines.splitlines())
    # the bigWig file through run_files, other windows
    out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "bw"), 120, coverage_control=path, coverage_bin=50, coverage_poisson=True,
                             coverage_lambda=(0, 5000), coverage_format="bigwig", coverage_compress=True, **kw)
    g2 = t.poisson(c, 50, a_c, 0, 5000)
    got, want = BC.read_file(out[0].written[-1]), BC.read_file(coverage.write_bigwig(tmp_path / "w", STEM, g2))
    assert out[0].error is None and got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in want.items() if k != "compressed"}
    assert g2 != g and sorted(os.listdir(tmp_path / "bw")) == sorted(p.name for p in out[0].written)
    # the refusals, before any file is written
    for bad in (dict(coverage_poisson=True), dict(coverage_lambda=(100, 1000)), dict(coverage_control=path, coverage_lambda=(100, 1000)),
                dict(coverage_control=path, coverage_poisson=True, coverage_compare="ratio"),
                dict(coverage_control=path, coverage_poisson=True, coverage_pseudocount=0.5),
                dict(coverage_control=path, coverage_poisson=True, coverage_normalize="cpm"),
                dict(coverage_control=path, coverage_poisson=True, coverage_scale=2.0),
                dict(coverage_control=path, coverage_poisson=True, coverage_lambda=(-1, 5)),
                dict(coverage_control=path, coverage_poisson=True, coverage_lambda=(5, 1 << 31)),
                dict(coverage_control=path, coverage_poisson=True, coverage_lambda=1000)):
        with pytest.raises(ValueError, match="coverage_"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, **bad, **kw)
    assert not (tmp_path / "bad").exists()
