"""The pileup as a bigWig file without a GPU: the host path (numpy sections and zoom records, the shared
assembler) read back by the independent reader of tests/bigwig_out_cases and set against its loop restatement, by the project's
own reader, compressed, through the options and through the run."""
import os
import struct

import numpy as np
import pytest

from pymasc_amd import cli, coverage, pipeline
from pymasc_amd.bigwig import BigWigReader
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests.fake_context import FakeContext

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")


def _host(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


@pytest.fixture(scope="module")
def library():
    """coverage_cases' library under the renamed references; the restatements are computed once each and left unchanged."""
    reads = FC.kept(CC.synthetic())
    return dict(reads=reads, less=FC.masked(reads, BC.REFS, BC.MASK), want={})


def _want(library, extend, masked=False):
    if (extend, masked) not in library["want"]:
        want = CC.restate(library["less" if masked else "reads"], BC.REFS, CC.USES["all"], extend)
        library["want"][extend, masked] = want, BC.depth_lists(want, BC.REFS, CC.USES["all"])
    return library["want"][extend, masked]


@pytest.fixture(scope="module")
def small():
    reads = BC.small_reads()
    want = CC.restate(reads, BC.SMALL_REFS, BC.SMALL_USE, 0)
    BC.check_small(want)
    return dict(reads=reads, want=want, depths=BC.depth_lists(want, BC.SMALL_REFS, BC.SMALL_USE))


@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_the_library_as_a_file(tmp_path, library, extend):
    want, depths = _want(library, extend)
    c = _host(library["reads"], BC.REFS, CC.USES["all"], extend)
    assert c.rows() == CC.rows_of(want) and c.refs == BC.REFS and want["max_depth"] == CC.PILE[2]
    path = coverage.write_bigwig(tmp_path / "lib", "lib", c)
    assert path.name == "lib_coverage.bw" and os.listdir(tmp_path) == [path.name]
    got = BC.read_file(path)
    BC.check_file(got, want, BC.REFS, CC.USES["all"], depths)
    assert not got["compressed"] and len(got["zooms"]) >= 4 and "c" not in got["runs"] and ("c", 0, 8191) in got["chroms"]
    # the project's own reader gives the same intervals, and read_bigwig the same runs
    ids = BC.chrom_ids(BC.NAMES)
    with BigWigReader(path) as r:
        assert list(r.chromsizes.items()) == sorted(BC.REFS, key=lambda x: ids[x[0]])
        for name, rows in want["runs"].items():
            s, e, v = r.fetch_arrays(0.0, name)
            assert list(zip(s.tolist(), e.tolist(), v.tolist())) == [(a, b, float(d)) for a, b, d in rows]
        assert r.fetch_arrays(0.0, "c")[0].size == 0
    back = coverage.read_bigwig(path)
    assert back.rows() == sorted(c.rows(), key=lambda x: ids[x[0]]) and back.refs == sorted(BC.REFS, key=lambda x: ids[x[0]])
    assert back.totals[1:] == c.totals[1:] and (back.reads, back.extend) == (0, 0)
    assert back == coverage.Coverage({n: c.runs[n] for n in back.runs}, 0, 0)
    # compressed: the same file after inflation
    packed = coverage.write_bigwig(tmp_path / "z", "z", c, compress=True)
    z = BC.read_file(packed)
    assert z["compressed"] and packed.stat().st_size < path.stat().st_size // 2
    assert {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in got.items() if k != "compressed"}
    assert coverage.read_bigwig(packed) == back


def test_masked_reads_and_a_selection(tmp_path, library):
    want, depths = _want(library, 200, True)
    c = _host(library["less"], BC.REFS, CC.USES["all"], 200)
    BC.check_file(BC.read_file(coverage.write_bigwig(tmp_path / "m", "m", c)), want, BC.REFS, CC.USES["all"], depths)
    use = CC.USES["no middle"]
    whole, _d = _want(library, 200)
    part = CC.select(whole, BC.REFS, library["reads"], use, 200)
    c = _host(library["reads"], BC.REFS, use, 200)
    got = BC.read_file(coverage.write_bigwig(tmp_path / "p", "p", c))
    BC.check_file(got, part, BC.REFS, use, BC.depth_lists(part, BC.REFS, use))
    assert [n for n, _i, _l in got["chroms"]] == ["c", "chr2", "chrX_alt"]                  # the reference left out is not in the tree


@pytest.mark.parametrize("zoom_base", [2, 32, None])
def test_the_small_case(tmp_path, small, zoom_base):
    c = _host(small["reads"], BC.SMALL_REFS, BC.SMALL_USE, 0)
    path = coverage.write_bigwig(tmp_path / "s", "s", c, items_per_section=BC.SMALL_ITEMS, index_block=BC.SMALL_BLOCK, zoom_base=zoom_base)
    got = BC.read_file(path, BC.SMALL_BLOCK)
    BC.check_file(got, small["want"], BC.SMALL_REFS, BC.SMALL_USE, small["depths"], zoom_base, BC.SMALL_ITEMS)
    assert "left_out" not in [n for n, _i, _l in got["chroms"]] and ("z_empty", 6, 700) in got["chroms"]
    assert [n for n, _i, _l in got["chroms"]] == ["B13long", "a3", "m12", "s4", "s5x", "tiny", "z_empty"]
    assert got["sections"].count(1) >= 2 and len(got["sections"]) > BC.SMALL_BLOCK ** 2     # three tiers of index nodes
    zs = [z for z, _r in got["zooms"]]
    assert zs[0] == (zoom_base or 256) and zs[-1] <= 2500 < 4 * zs[-1]                     # (automatic: 10 * 2648 bases / 110 runs = 240.7)
    if zoom_base == 32:
        tiny = [r for r in got["zooms"][0][1] if struct.unpack_from("<I", r)[0] == 5]
        assert [struct.unpack_from("<IIII", r) for r in tiny] == [(5, 0, 20, 10)]           # one bin, clipped to the length
    packed = coverage.write_bigwig(tmp_path / "sz", "sz", c, None, True, BC.SMALL_ITEMS, BC.SMALL_BLOCK, zoom_base)
    z = BC.read_file(packed, BC.SMALL_BLOCK)
    assert z["compressed"] and z["largest"] == got["largest"] and z["zooms"] == got["zooms"] and z["runs"] == got["runs"]


def test_no_kept_read_gives_a_valid_empty_file(tmp_path, small):
    use = [0, 0, 0, 0, 0, 0, 1, 0]                                                          # the one reference without a read
    c = _host(small["reads"], BC.SMALL_REFS, use, 0)
    assert c.totals == (0, 0, 0, 0, 0)
    path = coverage.write_bigwig(tmp_path / "e", "e", c)
    got = BC.read_file(path)
    assert got["chroms"] == [("z_empty", 0, 700)] and got["runs"] == {} and got["zooms"] == [] and got["sections"] == []
    assert got["summary"] == struct.pack("<Qdddd", 0, 0, 0, 0, 0)
    with BigWigReader(path) as r:
        assert r.chromsizes == {"z_empty": 700} and r.fetch_arrays(0.0, "z_empty")[0].size == 0
    assert coverage.read_bigwig(path).rows() == []
    assert BC.read_file(coverage.write_bigwig(tmp_path / "ez", "ez", c, compress=True))["runs"] == {}


def test_argument_errors_and_the_bound(tmp_path, small):
    c = _host(small["reads"], BC.SMALL_REFS, BC.SMALL_USE, 0)
    for kw in (dict(items_per_section=0), dict(items_per_section=65536), dict(index_block=1), dict(zoom_base=0), dict(zoom_base=1.5),
               dict(zoom_base=True)):
        with pytest.raises(ValueError):
            coverage.write_bigwig(tmp_path / "bad", "bad", c, **kw)
    with pytest.raises(ValueError, match="chosen references"):
        coverage.write_bigwig(tmp_path / "bad", "bad", coverage.Coverage(c.runs, c.reads, 0))   # (as read from a bedGraph file)
    assert os.listdir(tmp_path) == []
    assert coverage.check_format("bigwig", True) == "bigwig" and coverage.check_format("bedgraph") == "bedgraph"
    for bad in (("bw", False), ("bedgraph", True), (None, False)):
        with pytest.raises(ValueError, match="coverage_"):
            coverage.check_format(*bad)
    # the overflow bound, on the two totals finish leaves: exact while max_depth * fragment_bases < 2^64
    assert coverage.sumsq_fits(0, 0) and coverage.sumsq_fits(5000, 10 ** 12) and coverage.sumsq_fits(2 ** 31 - 1, 2 ** 33)
    assert coverage.sumsq_fits(2 ** 32, 2 ** 32 - 1) and not coverage.sumsq_fits(2 ** 32, 2 ** 32)
    assert coverage.sumsq_fits(1, 2 ** 64 - 1) and not coverage.sumsq_fits(1, 2 ** 64) and not coverage.sumsq_fits(2 ** 31, 2 ** 34)
    assert coverage.zoom_plan([1000], 0, 0) == (0, 0) and coverage.zoom_plan([100_000], 320, 100) == (32, 6)
    assert coverage.zoom_plan([100_000], 321, 100) == (64, 5) and coverage.zoom_plan([63], 10, 1, 32) == (32, 0)
    assert coverage.zoom_plan([64], 10, 1, 32) == (32, 1) and coverage.zoom_plan([2 ** 31], 1, 1, 2)[1] == 10


def test_read_bigwig_refuses_a_fractional_value(tmp_path, small):
    c = _host(small["reads"], BC.SMALL_REFS, BC.SMALL_USE, 0)
    path = coverage.write_bigwig(tmp_path / "f", "f", c)
    blob = bytearray(path.read_bytes())
    at = struct.unpack_from("<Q", blob, 16)[0] + 8 + 24 + 8                                 # the first item's value
    assert struct.unpack_from("<f", blob, at)[0] == 2.0
    struct.pack_into("<f", blob, at, 2.5)
    path.write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="not a whole number"):
        coverage.read_bigwig(path)
    struct.pack_into("<f", blob, at, float(2 ** 24))
    path.write_bytes(bytes(blob))
    with pytest.raises(ValueError, match="not a whole number"):
        coverage.read_bigwig(path)


def test_options(monkeypatch):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert not a.coverage and a.coverage_format is None and not a.coverage_compress
    a = cli.parse_args(base + ["--coverage-format", "bigwig", "--coverage-compress"])
    assert a.coverage and a.coverage_format == "bigwig" and a.coverage_compress
    assert cli.parse_args(base + ["--coverage-format", "bedgraph"]).coverage
    for bad in (["--coverage-compress"], ["--coverage", "--coverage-compress"], ["--coverage-format", "bedgraph", "--coverage-compress"],
                ["--coverage-format", "wig"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    text = cli.get_parser().format_help()
    assert "_coverage.bw" in text and "2^24" in text and "--coverage-compress" in text
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for more, want in ((["--coverage-format", "bigwig"], dict(coverage=True, coverage_format="bigwig")),
                       (["--coverage-format", "bigwig", "--coverage-compress", "--coverage-extend", "150"],
                        dict(coverage=True, coverage_format="bigwig", coverage_compress=True, coverage_extend=150)),
                       (["--coverage-format", "bedgraph"], dict(coverage=True, coverage_format="bedgraph"))):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert {k: v for k, v in seen.items() if k.startswith("coverage")} == want


def _golden_reads(mapq=10):
    """The golden file's references and its kept reads as four columns."""
    from pymasc_amd.bam import BamReader
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(mapq))]
    return refs, cols


def test_the_run_writes_the_file_and_no_bedgraph(tmp_path, caplog):
    refs, cols = _golden_reads()
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext())
    _r, written = pipeline.run(GOLDEN_BAM, str(tmp_path / "bw"), 120, coverage=True, coverage_extend=200, coverage_format="bigwig", **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in written][-1] == stem + "_coverage.bw"
    assert sorted(os.listdir(tmp_path / "bw")) == sorted(p.name for p in written) and not any(n.endswith(".bedGraph") for n in os.listdir(tmp_path / "bw"))
    want = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), 200)
    back = coverage.read_bigwig(written[-1])
    assert back.runs.keys() == want.runs.keys() and all(np.array_equal(a, b) for n in want.runs for a, b in zip(back.runs[n], want.runs[n]))
    assert sorted(back.refs) == sorted(refs) and back.n_runs > 100
    got = BC.read_file(written[-1])
    assert not got["compressed"] and struct.unpack_from("<Q", got["summary"])[0] == want.covered_bases
    # "auto" counts on one more read of the file; compressed; through run_files, which warns about the file it replaces
    import logging
    with caplog.at_level(logging.WARNING):
        out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "bw"), 120, coverage=True, coverage_format="bigwig", coverage_compress=True, **kw)
    w2 = out[0].written
    assert out[0].error is None and w2[-1] == written[-1] and BC.read_file(w2[-1])["compressed"] and coverage.read_bigwig(w2[-1]).n_runs > 100
    assert sorted(os.listdir(tmp_path / "bw")) == sorted(p.name for p in w2)
    assert any("_coverage.bw' will be overwritten" in r.getMessage() for r in caplog.records)
    for bad in (dict(coverage_format="bw"), dict(coverage_compress=True), dict(coverage_format="bedgraph", coverage_compress=True)):
        with pytest.raises(ValueError, match="coverage_"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, coverage=True, coverage_extend=200, **bad, **kw)
    assert not (tmp_path / "bad").exists()
