"""The pileup as a signal track without a GPU: the host path (``Coverage.signal``, ``Signal``, ``HostParts`` over
it) against the loop restatement of tests/signal_cases -- runs, totals, text bytes and the bigWig file through the independent
reader of tests/bigwig_out_cases --, ``scale_of``, the refusals, the command line's exit codes, and the run: with the defaults it
writes the depth track's bytes, with a bin and a normalisation the signal's."""
import os
import struct

import numpy as np
import pytest

from pymasc_amd import cli, coverage, pipeline
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import signal_cases as SC
from tests.fake_context import FakeContext

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"


def _host(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


def _scales(c):
    """1.0, the cpm factor and an rpgc factor of the pileup ``c``."""
    lengths = [l for _n, l in c.refs]
    return (1.0, coverage.scale_of("cpm", c.reads, c.fragment_bases, lengths), coverage.scale_of("rpgc", c.reads, c.fragment_bases, lengths))


@pytest.fixture(scope="module")
def library():
    """coverage_cases' library under the renamed references; pileups, depth lists and bin sums are computed once each."""
    return dict(reads=FC.kept(CC.synthetic()), host={}, sums={})


def _pile(library, extend):
    if extend not in library["host"]:
        want = CC.restate(library["reads"], BC.REFS, CC.USES["all"], extend)
        library["host"][extend] = _host(library["reads"], BC.REFS, CC.USES["all"], extend), BC.depth_lists(want, BC.REFS, CC.USES["all"])
    return library["host"][extend]


def _sums(library, extend, B):
    if (extend, B) not in library["sums"]:
        library["sums"][extend, B] = SC.bin_sums(_pile(library, extend)[1], B)
    return library["sums"][extend, B]


@pytest.mark.parametrize("B", SC.BINS)
@pytest.mark.parametrize("extend", [0, 200])
def test_the_library_against_the_restatement(tmp_path, library, extend, B):
    c, _depths = _pile(library, extend)
    scales = _scales(c)
    assert scales[1] == 1e6 / c.reads and scales[2] == sum(BC.LENGTHS) / c.fragment_bases
    for k, scale in enumerate(scales):
        want = SC.restate(_sums(library, extend, B), scale)
        g = c.signal(B, scale)
        assert SC.rows_got(g) == SC.rows_of(want) and g.totals == SC.totals(want) and (g.bin, g.scale, g.refs) == (B, scale, BC.REFS)
        assert b"".join(g.text_chunks()) == b"".join(g.text_chunks(chunk=777)) == SC.text_of(want)
        if k == 1:                                          # the file, once per bin
            got = BC.read_file(coverage.write_bigwig(tmp_path / "f", "f", g))
            SC.check_file(got, want, BC.REFS, B)
            assert (B > 50 or len(got["zooms"]) >= 3) and got["sections"]
    if B == 1:                                              # the depth runs with another value column; at scale 1 the depth track's lines
        g = c.signal(1, 1.0)
        assert [(n, s, e) for n, s, e, _v in g.rows()] == [(n, s, e) for n, s, e, _d in c.rows()]
        assert b"".join(g.text_chunks()) == b"".join(c.text_chunks()) and g.n_runs > 3000
    else:
        assert c.signal(B, 1.0).n_runs < c.n_runs


@pytest.mark.parametrize("zoom", [None, 1, 2])              # z_0: its own choice, B itself, 2 B
@pytest.mark.parametrize("B", [1, 2, 7, 50])
def test_the_small_case(tmp_path, B, zoom):
    reads = BC.small_reads()
    want0 = CC.restate(reads, BC.SMALL_REFS, BC.SMALL_USE, 0)
    c = _host(reads, BC.SMALL_REFS, BC.SMALL_USE, 0)
    chosen = [r for r, u in zip(BC.SMALL_REFS, BC.SMALL_USE) if u]
    scale = coverage.scale_of("cpm", c.reads, c.fragment_bases, [l for _n, l in chosen], 3.0)
    assert scale == 1e6 / c.reads * 3.0
    want = SC.restate(SC.bin_sums(BC.depth_lists(want0, BC.SMALL_REFS, BC.SMALL_USE), B), scale)
    zoom_base = None if zoom is None else zoom * B
    g = c.signal(B, scale)
    path = coverage.write_bigwig(tmp_path / "s", "s", g, items_per_section=BC.SMALL_ITEMS, index_block=BC.SMALL_BLOCK, zoom_base=zoom_base)
    got = BC.read_file(path, BC.SMALL_BLOCK)
    SC.check_file(got, want, chosen, B, zoom_base, BC.SMALL_ITEMS)
    assert len(got["sections"]) > 8 and len(got["zooms"]) >= (1 if B == 50 else 2) and "z_empty" not in got["runs"]
    compressed = coverage.write_bigwig(tmp_path / "z", "z", g, compress=True, items_per_section=BC.SMALL_ITEMS, index_block=BC.SMALL_BLOCK,
                                       zoom_base=zoom_base)
    z = BC.read_file(compressed, BC.SMALL_BLOCK)
    assert z["compressed"] and {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in got.items() if k != "compressed"}


@pytest.mark.parametrize("scale", [1.0, 0.37, SC.TINY])
def test_the_planted_situations(tmp_path, scale):
    reads = SC.planted_reads()
    want0 = CC.restate(reads, SC.P_REFS, [1] * 4, 0)
    want = SC.restate(SC.bin_sums(BC.depth_lists(want0, SC.P_REFS, [1] * 4), SC.P_B), scale)
    SC.check_planted(want, scale)
    g = _host(reads, SC.P_REFS, [1] * 4, 0).signal(SC.P_B, scale)
    assert SC.rows_got(g) == SC.rows_of(want) and g.totals == SC.totals(want) and b"".join(g.text_chunks()) == SC.text_of(want)
    SC.check_file(BC.read_file(coverage.write_bigwig(tmp_path / "p", "p", g, items_per_section=2, index_block=2), 2), want, SC.P_REFS, SC.P_B, None, 2)


def test_two_sums_that_round_to_one_value_stay_two_runs():
    reads = SC.tie_reads()
    want0 = CC.restate(reads, SC.T_REFS, [1], SC.T_EXTEND)
    want = SC.restate(SC.bin_sums(BC.depth_lists(want0, SC.T_REFS, [1]), SC.T_B), 1.0)
    SC.check_tie(want)
    g = _host(reads, SC.T_REFS, [1], SC.T_EXTEND).signal(SC.T_B, 1.0)
    assert SC.rows_got(g) == SC.rows_of(want) and g.n_runs == 2 and g.min == g.max == 4097.0
    assert b"".join(g.text_chunks()) == b"t0\t0\t4096\t4097\nt0\t4096\t8192\t4097\n" == SC.text_of(want)


def test_values_as_text():
    for v, text in ((1.0, "1"), (0.5, "0.5"), (1 / 3, "0.333333"), (4.0e-7, "0"), (5.0e-7, "0"), (5.1e-7, "0.000001"), (1.5e-6, "0.000002"),
                    (1 / 128, "0.007812"), (3 / 128, "0.023438"), (5 / 128, "0.039062"), (123456.0, "123456"), (10.0, "10"), (100.25, "100.25"), (0.0000005 + 2 ** -40, "0.000001")):
        assert coverage.format_value(np.float32(v)) == text == SC.text_value(np.float32(v)), v
    assert coverage.format_value(np.float32(2.0 ** -21)) == "0" and coverage.format_value(np.float32(3 * 2.0 ** -21)) == "0.000001"
    # (an odd multiple of 1 / 128 is the only kind of float32 that is an exact tie at six decimals: it goes to the even digit)
    assert coverage.format_value(np.float32(0.5 + 2.0 ** -20)) == "0.500001"


def test_scale_of_and_the_refusals():
    lengths = [1000, 500]
    assert coverage.NORMALIZE == ("none", "cpm", "rpgc")
    assert coverage.scale_of("none", 10, 360, lengths) == 1.0 and coverage.scale_of("none", 10, 360, lengths, 2.5) == 2.5
    assert coverage.scale_of("cpm", 20_000_000, 360, lengths) == 1e6 / 20_000_000.0 == 0.05
    assert coverage.scale_of("cpm", 3, 360, lengths, 7.0) == (1e6 / 3.0) * 7.0
    assert coverage.scale_of("rpgc", 10, 360, lengths) == 1500.0 / 360.0
    assert coverage.scale_of("rpgc", 10, 360, lengths, 1.0, 2_000) == 2000.0 / 360.0
    assert coverage.scale_of("cpm", 0, 0, lengths, 4.0) == 4.0 == coverage.scale_of("rpgc", 0, 0, lengths, 4.0)    # no kept read
    for bad in (dict(normalize="rpkm"), dict(genome_size=0), dict(genome_size=1.5), dict(genome_size=True), dict(coverage_scale=0.0),
                dict(coverage_scale=float("inf")), dict(coverage_scale="2"), dict(normalize="cpm", genome_size=100)):
        kw = dict(dict(normalize="rpgc", reads=10, fragment_bases=360, lengths=lengths), **bad)
        with pytest.raises(ValueError, match="coverage_"):
            coverage.scale_of(**kw)
    assert [coverage.check_bin(b) for b in (1, 50, 65536, np.int64(7), 2.0)] == [1, 50, 65536, 7, 2]
    for bad in (0, -1, 65537, 1.5, "50", True, None, float("nan")):
        with pytest.raises(ValueError, match="coverage_bin"):
            coverage.check_bin(bad)
    c = coverage.Coverage({"a": ([0, 10], [10, 20], [1, 1 << 20])}, 5, 0, [("a", 30)])
    assert coverage.check_scale(2.0 ** -64) == 2.0 ** -64 and c.signal(1, 2.0 ** 19).max == 2.0 ** 39
    for scale, text in ((2.0 ** -65, "2\\^-64"), (0.0, "2\\^-64"), (-1.0, "2\\^-64"), (float("nan"), "finite"), (float("inf"), "finite"),
                        (2.0 ** 20, "2\\^40")):
        with pytest.raises(ValueError, match=text):
            c.signal(1, scale)
    with pytest.raises(ValueError, match="lengths"):
        coverage.Coverage({"a": ([0], [10], [1])}, 1, 0).signal(2, 1.0)          # a bin needs the references' lengths
    g = c.signal(10, 1.0)
    for zoom_base in (15, 5, 1):
        with pytest.raises(ValueError, match="multiple of the signal's bin"):
            coverage.zoom_plan([30], g.covered_bases, g.n_runs, zoom_base, g.bin)
    assert coverage.zoom_plan([3000], 20, 2, None, 10) == (160, 2) and coverage.zoom_plan([3000], 20, 2, 20, 10) == (20, 4)
    assert coverage.zoom_plan([3000], 2000, 2, None, 50) == (12_800, 0) and coverage.zoom_plan([3000], 20, 2, None, 1) == (128, 2)
    assert c.signal(1, 1.0) == c.signal(1, 1.0) and c.signal(1, 1.0) != c.signal(1, 2.0) and c.signal(1, 1.0) != c.signal(10, 1.0)


def test_options(monkeypatch):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base + ["--coverage"])
    assert (a.coverage_bin, a.coverage_normalize, a.coverage_scale, a.coverage_genome_size) == (None, None, None, None)
    for more, key, value in ((["--coverage-bin", "50"], "coverage_bin", 50), (["--coverage-normalize", "cpm"], "coverage_normalize", "cpm"),
                             (["--coverage-scale", "2.5"], "coverage_scale", 2.5),
                             (["--coverage-normalize", "rpgc", "--coverage-genome-size", "2913022398"], "coverage_genome_size", 2913022398)):
        a = cli.parse_args(base + more + ["--coverage-extend", "200"])
        assert a.coverage and getattr(a, key) == value
        assert cli.parse_args(["-"] + more + ["--coverage-extend", "200"]).coverage        # (each implies --coverage)
    for bad in (["--coverage-bin", "0"], ["--coverage-bin", "65537"], ["--coverage-bin", "x"], ["--coverage-bin", "1.5"],
                ["--coverage-normalize", "rpkm"], ["--coverage-scale", "0"], ["--coverage-scale", "-1"], ["--coverage-scale", "inf"],
                ["--coverage-scale", "nan"], ["--coverage-scale", "x"], ["--coverage-genome-size", "0"], ["--coverage-genome-size", "1000"],
                ["--coverage-normalize", "cpm", "--coverage-genome-size", "1000"], ["--coverage-normalize", "rpgc", "--coverage-genome-size", "x"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    text = " ".join(cli.get_parser().format_help().split())
    assert "--coverage-bin N" in text and "--coverage-normalize {none,cpm,rpgc}" in text and "--coverage-genome-size N" in text
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for more, want in ((["--coverage-bin", "50", "--coverage-normalize", "cpm"], dict(coverage=True, coverage_bin=50, coverage_normalize="cpm")),
                       (["--coverage-normalize", "rpgc", "--coverage-genome-size", "5000", "--coverage-scale", "0.5", "--coverage-format", "bigwig"],
                        dict(coverage=True, coverage_normalize="rpgc", coverage_genome_size=5000, coverage_scale=0.5, coverage_format="bigwig")),
                       (["--coverage"], dict(coverage=True))):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert {k: v for k, v in seen.items() if k.startswith("coverage")} == want


def _golden_pile(extend):
    from pymasc_amd.bam import BamReader
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(10))]
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), extend)


def test_the_run(tmp_path):
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext(), coverage=True, coverage_extend=200)
    c = _golden_pile(200)
    # the defaults, given or not: the depth track through the calls the run has always made, byte for byte
    for fmt, write in (("bedgraph", coverage.write_coverage), ("bigwig", coverage.write_bigwig)):
        want = write(tmp_path / "want", STEM, c).read_bytes()
        for n, more in enumerate((dict(), dict(coverage_bin=1, coverage_normalize="none", coverage_scale=1.0, coverage_genome_size=None))):
            _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / (fmt + str(n))), 120, coverage_format=fmt, **more, **kw)
            assert written[-1].name == STEM + coverage.SUFFIXES[fmt] and written[-1].read_bytes() == want
    assert b" bin=" not in want[:300]
    # a bin and cpm: the signal of the same pileup, in both formats
    scale = 1e6 / c.reads
    g = c.signal(50, scale, "cpm")
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "sig"), 120, coverage_bin=50, coverage_normalize="cpm", **kw)
    text = written[-1].read_bytes()
    head = 'track type=bedGraph name="{}" description="pymasc_amd fragment pileup extend=200 reads={}" bin=50 normalize=cpm scale={!r}\n'.format(
        STEM, c.reads, scale).encode()
    assert text == head + b"".join(g.text_chunks()) == coverage.write_coverage(tmp_path / "w", STEM, g).read_bytes() and g.n_runs > 50
    out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "sigbw"), 120, coverage_bin=50, coverage_normalize="rpgc", coverage_scale=2.0,
                             coverage_genome_size=3_000_000, coverage_format="bigwig", **kw)
    g2 = c.signal(50, (3_000_000 / c.fragment_bases) * 2.0)
    assert out[0].error is None and out[0].written[-1].read_bytes() == coverage.write_bigwig(tmp_path / "w", STEM, g2).read_bytes()
    got = BC.read_file(out[0].written[-1])
    assert struct.unpack_from("<Qdd", got["summary"]) == (g2.covered_bases, g2.min, g2.max)
    assert sorted(os.listdir(tmp_path / "sigbw")) == sorted(p.name for p in out[0].written)
    # "auto" counts on one more read of the file, with the run's own estimate, and scales there
    _r, w3 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage_normalize="cpm", mappability_path=None,
                          **dict(kw, coverage_extend="auto"))
    line = w3[-1].read_bytes().split(b"\n", 1)[0]
    assert b" bin=1 normalize=cpm scale=" in line and b"extend=200" not in line
    for bad in (dict(coverage_bin=0), dict(coverage_bin=65537), dict(coverage_bin="50"), dict(coverage_normalize="rpkm"), dict(coverage_scale=0),
                dict(coverage_scale="x"), dict(coverage_genome_size=1000), dict(coverage_normalize="cpm", coverage_genome_size=1000),
                dict(coverage_normalize="rpgc", coverage_genome_size=0)):
        with pytest.raises(ValueError, match="coverage_"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, **bad, **kw)
    with pytest.raises(ValueError, match="2\\^-64"):           # the final factor is refused where it is known
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad2"), 120, coverage_scale=1e-30, **kw)
    assert not (tmp_path / "bad").exists()
