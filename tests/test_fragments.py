"""Paired-end fragment sizes without a GPU: the host readers' mate columns and ``fragments.rows_host`` /
``count_host`` against the loop restatement of tests/fragments_cases, for BAM and SAM; the statistics against the expanded list of
sizes in exact arithmetic; the table file; the options; the host path of the run; the host pair pileup."""
import functools
import math
import os
import random
from fractions import Fraction

import numpy as np
import pytest

from pymasc_amd import cli, coverage, fragments, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bed_reads import BedReadsReader
from pymasc_amd.fragments import FragmentSizes
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import SamReader
from tests import coverage_cases as CC
from tests import fragments_cases as FC
from tests import io_writers as W
from tests.fake_context import FakeContext

NAMES = [n for n, _l in FC.REFS]


@functools.lru_cache(maxsize=None)
def lib():
    return FC.library()


@functools.lru_cache(maxsize=None)
def want(max_size, use, masked):
    return FC.restate(lib(), FC.REFS, FC.USES[use], max_size, FC.MASK if masked else None)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("fragments")
    bam, sam, gz = str(d / "pe.bam"), str(d / "pe.sam"), str(d / "pe.sam.gz")
    FC.write_bam(bam, lib())
    text = FC.sam_text(lib())
    with open(sam, "wb") as fh:
        fh.write(text)
    with open(gz, "wb") as fh:
        fh.write(W.bgzf_compress(text))
    return dict(dir=d, bam=bam, sam=sam, gz=gz)


def _chosen(use):
    return [n for n, u in zip(NAMES, FC.USES[use]) if u]


def _open(path):
    return BamReader(path) if path.endswith(".bam") else SamReader(path)


def _masked(r):
    r.set_exclude(region_mask.open_mask(FC.MASK).resolve(r.references, r.lengths))


def test_the_library_holds_the_cases():
    recs = lib()
    assert 90_000 < len(recs) < 120_000
    rows, c, hist = want(65536, "all", False)
    c = dict(zip(FC.COUNTERS, c))
    assert all(c[k] > 0 for k in FC.COUNTERS if k != "masked") and c["reads"] > c["paired"]
    assert hist[FC.FR][FC.PILE_SIZE - 1] >= FC.PILE > 65535             # one cell above 16 bits
    for m in FC.MAX_SIZES:
        h = want(m, "all", False)[2]
        assert all(h[o][m - 1] > 0 for o in (FC.FR, FC.RF)) and (m == 1 or h[FC.FR][m - 2] > 0)
        over = dict(zip(FC.COUNTERS, want(m, "all", False)[1]))
        assert over["over_fr"] > 0 and over["over_rf"] > 0
    assert all(want(2000, "all", False)[2][o][299] >= 2 for o in range(3))      # all three orientations at one size
    assert want(2000, "all", True)[1][9] >= 3 and want(2000, "not_chrC", False)[1][0] < c["reads"]
    assert FC.straddles(recs, 16384) > 100 and FC.straddles(recs, 0xff00 - 0) > 20      # 16-KB pieces; (header aside) BGZF members
    assert any(r.long for r in recs)
    labels = dict(FC.planted())
    one = lambda label, m=2000, mask=None: FC.restate([labels[label]], FC.REFS, FC.USES["all"], m, mask)
    assert dict(zip(FC.COUNTERS, one("mate unmapped and elsewhere")[1]))["mate_unmapped"] == 1
    assert dict(zip(FC.COUNTERS, one("mate elsewhere with a size")[1]))["mate_elsewhere"] == 1
    for label in ("tlen 0", "tlen -2^31", "next_pos -1", "PNEXT 0 with ="):
        assert dict(zip(FC.COUNTERS, one(label)[1]))["no_size"] == 1
    assert one("tlen 2^31 - 1", 65536)[1][5] == 1 and one("tlen -(2^31 - 1)", 65536)[1][5] == 1
    assert one("forward read, negative tlen: RF")[0][0][3] == FC.RF and one("reverse read, positive tlen: RF")[0][0][3] == FC.RF
    assert one("read1 outside, the fragment reaches in", 2000, FC.MASK)[1][9] == 1
    assert one("the fragment abuts on the left", 2000, FC.MASK)[1][9] == 0 and one("the fragment abuts on the right", 2000, FC.MASK)[1][9] == 0
    assert one("over size spans the region", 65536, FC.MASK)[1][8:] == [0, 0]
    assert one("past the end of chrB")[0] == [(1, 49901, 300, FC.FR)]


@pytest.mark.parametrize("kind", ["bam", "sam", "gz"])
def test_mate_columns(case, kind):
    """The four raw columns, record for record, beside the columns of ``batches``."""
    kept = [r for r in lib() if not r.flag & FC.EXCLUDE and r.mapq >= FC.MAPQ and r.ref >= 0 and sum(n for op, n in r.cigar if op in "MIS=X")]
    with _open(case[kind]) as r:
        cols = [np.concatenate(x) for x in zip(*r.mate_batches(FC.MAPQ, batch=40_000))]
        plain = [np.concatenate(x) for x in zip(*r.batches(FC.MAPQ))]
    assert all(np.array_equal(a, b) for a, b in zip(cols[:4], plain))
    assert cols[4].dtype == np.uint16 and cols[0].size == len(kept)
    assert cols[4].tolist() == [r.flag for r in kept]
    assert cols[6].tolist() == [r.mpos0 + 1 for r in kept] and cols[7].tolist() == [r.tlen for r in kept]
    assert cols[5].tolist() == [r.mref for r in kept]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("use", sorted(FC.USES))
@pytest.mark.parametrize("max_size", FC.MAX_SIZES)
@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_host_equals_the_restatement(case, kind, max_size, use, masked):
    rows, counters, hist = want(max_size, use, masked)
    with _open(case[kind]) as r:
        if masked:
            _masked(r)
        got = list(fragments.rows_host(r, FC.MAPQ, _chosen(use), max_size))
        c = r.fragment_sizes(FC.MAPQ, _chosen(use), max_size)
    got_rows = [np.concatenate([g[k] for g in got]) for k in range(4)]
    assert list(zip(*(x.tolist() for x in got_rows))) == rows
    assert sum(g[4] for g in got).tolist() == counters
    assert [c.counters[k] for k in FC.COUNTERS] == counters and c.hist.tolist() == hist and c.max_size == max_size
    assert c.per_reference == {n: l for (n, l), u in zip(FC.REFS, FC.USES[use]) if u}
    k = c.counters
    assert k["paired"] == k["mate_unmapped"] + k["mate_elsewhere"] + k["no_size"] + sum(c.over) + k["rows"]
    assert k["rows"] - k["masked"] == int(c.hist.sum()) == len(rows)


def test_the_gzip_twin_and_the_golden_twins(case):
    with SamReader(case["gz"]) as a, BamReader(case["bam"]) as b:
        assert a.fragment_sizes(FC.MAPQ) == b.fragment_sizes(FC.MAPQ)
    gold = os.path.join(os.path.dirname(__file__), "golden", "ENCFF000RMB-test")
    with BamReader(gold + ".bam") as a, SamReader(gold + ".sam.gz") as b:
        x, y = a.fragment_sizes(1), b.fragment_sizes(1)
    assert x == y and x.counters["reads"] > 1000


@pytest.mark.parametrize("n", [0, 1, 256, 257])
def test_edge_libraries(tmp_path, n):
    path = str(tmp_path / "edge.bam")
    FC.write_bam(path, FC.edge_library(n))
    with BamReader(path) as r:
        c = r.fragment_sizes(FC.MAPQ, None, 2000)
    assert c.counters["rows"] == n == c.n and c.counters["reads"] == n + 1
    st = c.stats(fragments.FR)
    assert (st is None) == (n == 0) and c.stats(fragments.RF) is None
    if n == 1:
        assert math.isnan(st["sd"]) and st["mean"] == st["median"] == 100.0 and st["mad"] == 0.0


def _expanded_stats(sizes):
    """The statistics of a list of sizes, element by element, in exact arithmetic with one float operation at the end."""
    v = sorted(sizes)
    n = len(v)

    def median(xs):
        return Fraction(xs[(len(xs) - 1) // 2] + xs[len(xs) // 2], 2)

    def quantile(num, den):
        need = -((-num * n) // den)
        return v[need - 1]
    med = median(v)
    s1, s2 = sum(v), sum(x * x for x in v)
    counts = {}
    for x in v:
        counts[x] = counts.get(x, 0) + 1
    var = Fraction(n * s2 - s1 * s1, n * (n - 1)) if n > 1 else None
    return {"n": n, "mean": s1 / n, "sd": math.sqrt(var.numerator / var.denominator) if var is not None else float("nan"),
            "median": med.numerator / med.denominator, "q25": quantile(1, 4), "q75": quantile(3, 4),
            "mad": (lambda m: m.numerator / m.denominator)(median(sorted(abs(x - med) for x in v))),
            "mode": min(x for x, c in counts.items() if c == max(counts.values())), "min": v[0], "max": v[-1]}


def test_statistics_are_those_of_the_expanded_list():
    rng = random.Random(5)
    lists = [[7], [3, 4], [1, 1, 2, 9], [5, 5, 5, 6, 6, 6, 2], [65536, 1, 65535], [10 ** 4] * 3 + [1] * 3,
             [max(1, int(rng.gauss(200, 40))) for _ in range(5001)], [rng.randrange(1, 65537) for _ in range(4000)],
             [rng.choice((150, 151, 400)) for _ in range(1000)]]
    rows = want(65536, "all", False)[0]
    lists += [[s for _r, _p, s, o in rows if o == k] for k in range(3)]
    for sizes in lists:
        h = np.bincount(np.array(sizes) - 1, minlength=65536)
        got, ref = fragments.size_stats(h), _expanded_stats(sizes)
        for k in fragments.STATS:
            assert got[k] == ref[k] or (k == "sd" and len(sizes) == 1 and math.isnan(got[k])), (k, got[k], ref[k], len(sizes))
        assert isinstance(got["mean"], float) and isinstance(got["q25"], int)
    assert fragments.size_stats(np.zeros(10)) is None
    c = FragmentSizes(65536, {}, np.stack([np.bincount(np.array(lists[6]) - 1, minlength=65536)] + [np.zeros(65536, dtype=np.int64)] * 2),
                      [0] * 10)
    assert (c.median, c.mode, c.mad) == tuple(_expanded_stats(lists[6])[k] for k in ("median", "mode", "mad"))
    assert c.stats(fragments.RF) is None


def test_the_table_reads_back(case, tmp_path):
    with BamReader(case["bam"]) as r:
        _masked(r)
        c = r.fragment_sizes(FC.MAPQ, _chosen("not_chrC"), 4097)
    path = fragments.write_fragments(tmp_path / "x", "x", c)
    assert path.name == "x_fragments.tab"
    name, back, stats = fragments.read_fragments(path)
    assert name == "x" and back == c and back.counters == c.counters
    assert list(stats) == ["FR", "RF", "TANDEM"]
    for o, label in enumerate(fragments.ORIENTATIONS):
        assert stats[label] == c.stats(o)
    text = path.read_text()
    assert "Max size\t4097\n" in text and "Masked\t{}\n".format(c.counters["masked"]) in text
    assert "{}\t{}\t".format(FC.PILE_SIZE, int(c.hist[0][FC.PILE_SIZE - 1])) in text
    one = FragmentSizes(10, {"a": 5}, [[0] * 9 + [1], [0] * 10, [0] * 10], [1, 1, 0, 0, 0, 0, 0, 0, 1, 0])
    name, back, stats = fragments.read_fragments(fragments.write_fragments(tmp_path / "one", "one", one))
    assert back == one and list(stats) == ["FR"] and math.isnan(stats["FR"]["sd"])
    assert FragmentSizes(10, {"a": 5}, one.hist, [2, 1, 0, 0, 0, 0, 0, 0, 1, 0]) != one


def test_bad_arguments(case):
    with BamReader(case["bam"]) as r:
        for bad in (0, 65537, -1, 2.5, "9"):
            with pytest.raises(ValueError, match="max_size is"):
                r.fragment_sizes(FC.MAPQ, None, bad)
    with pytest.raises(ValueError):
        FragmentSizes(10, {}, np.zeros((3, 9)), [0] * 10)


def test_a_malformed_tlen_names_its_line(tmp_path):
    recs = [r for r in lib() if r.flag & 0x40][:50]
    lines = FC.sam_text(recs).split(b"\n")
    n_head = sum(1 for ln in lines if ln[:1] == b"@")
    bad_at = n_head + 30
    f = lines[bad_at].split(b"\t")
    f[8] = b"12x"
    lines[bad_at] = b"\t".join(f)
    path = tmp_path / "bad.sam"
    path.write_bytes(b"\n".join(lines))
    with SamReader(str(path)) as r:
        assert sum(b[0].size for b in r.batches(0)) > 0                # (the fields the run reads are well formed)
        with pytest.raises(PmxIOError, match="line {}: TLEN is not a decimal".format(bad_at + 1)):
            list(r.mate_batches(0, 0))
    f[8], f[7] = b"-12", b"-3"
    lines[bad_at] = b"\t".join(f)
    path.write_bytes(b"\n".join(lines))
    with SamReader(str(path)) as r:
        with pytest.raises(PmxIOError, match="line {}: PNEXT is not a decimal".format(bad_at + 1)):
            r.fragment_sizes(0)


def _tagalign(tmp_path):
    bed = tmp_path / "reads.tagAlign"
    bed.write_text("chrA\t100\t136\tr\t30\t+\nchrA\t200\t236\tr\t30\t-\n")
    return str(bed)


def test_a_bed_read_file_has_no_mates(tmp_path):
    with BedReadsReader(_tagalign(tmp_path), NAMES, [l for _n, l in FC.REFS]) as r:
        with pytest.raises(ValueError, match="the input has no mate fields"):
            r.fragment_sizes(0)
        flag = np.zeros(2, dtype=np.uint16)
        r.decode(0)
        assert r._L.pmx_sam_fetch_mates(r._h, 0, 1, flag.ctypes.data, None, None, None) == -3


def test_options(capsys):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert (a.fragments, a.fragments_max) == (False, None)
    assert cli.parse_args(base + ["--fragments"]).fragments is True
    a = cli.parse_args(base + ["--fragments-max", "500"])
    assert (a.fragments, a.fragments_max) == (True, 500)
    assert cli.parse_args(base + ["--fragments-max", "65536"]).fragments_max == 65536
    for bad in (["--fragments-max", "0"], ["--fragments-max", "65537"], ["--fragments-max", "x"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2
        assert cli.main(base + bad) == 2
    capsys.readouterr()
    a = cli.parse_args(base + ["--coverage-extend", "pair"])
    assert (a.coverage, a.coverage_extend) == (True, "pair")
    a = cli.parse_args(["-", "-d", "100", "-r", "36", "--coverage-extend", "pair"])         # known before the feed: a stream takes it
    assert a.coverage_extend == "pair"
    assert "_fragments.tab" in cli.get_parser().format_help()


def test_options_reach_run_files(monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert cli.main(["a.bam", "--skip-plots"]) == 0
    assert not any(k.startswith("fragments") for k in seen)
    seen.clear()
    assert cli.main(["a.bam", "--skip-plots", "--fragments-max", "300", "--coverage-extend", "pair"]) == 0
    assert {k: seen.get(k) for k in ("fragments", "fragments_max", "coverage", "coverage_extend")} == dict(
        fragments=True, fragments_max=300, coverage=True, coverage_extend="pair")


@functools.lru_cache(maxsize=None)
def small_lib():
    recs = [r for _l, r in FC.planted()] + FC.random_pairs(random.Random(3), 3000)
    return [r for _i, r in sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))]


def _pileup_want(recs, use, max_size, mask):
    rows = FC.restate(recs, FC.REFS, use, max_size, mask)[0]
    return CC.restate([(r, p, s, 0) for r, p, s, o in rows if o == FC.FR], FC.REFS, use, 0)


def test_host_pair_pileup(tmp_path):
    recs = small_lib()
    bam, sam = str(tmp_path / "s.bam"), str(tmp_path / "s.sam")
    FC.write_bam(bam, recs)
    with open(sam, "wb") as fh:
        fh.write(FC.sam_text(recs))
    for path in (bam, sam):
        for use, masked in (("all", False), ("not_chrC", True)):
            ref = _pileup_want(recs, FC.USES[use], 2000, FC.MASK if masked else None)
            with _open(path) as r:
                if masked:
                    _masked(r)
                c = coverage.from_reader(r, FC.MAPQ, _chosen(use), "pair", 2000)
            assert c.extend == "pair" and c == CC.as_coverage(ref, "pair") and c.totals == CC.totals(ref)
            assert c.fragment_bases == ref["extents"] and c.reads > 1000
    # past the end of chrB: a row, clipped by the pileup
    assert ref["runs"]["chrB"][-1][1] == 50000
    path = coverage.write_coverage(tmp_path / "s", "s", c)
    assert path.read_bytes().startswith(b'track type=bedGraph name="s" description="pymasc_amd fragment pileup extend=pair reads=%d"\n' % c.reads)
    name, back = coverage.read_coverage(path)
    assert name == "s" and back == c and back.extend == "pair"
    with BamReader(bam) as r:
        assert coverage.from_reader(r, FC.MAPQ, None, "pair", 300).reads < coverage.from_reader(r, FC.MAPQ, None, "pair", 2000).reads
        assert coverage.from_reader(r, FC.MAPQ, None, 0).extend == 0


def test_pipeline_writes_the_table_and_nothing_else_changes(tmp_path):
    recs = small_lib()
    bam = str(tmp_path / "pe.bam")
    FC.write_bam(bam, recs)
    kw = dict(read_len=36, mapq_criteria=FC.MAPQ, device_ingest=False, stats=True, complexity=True)
    _r0, w0 = pipeline.run(bam, str(tmp_path / "plain"), 120, context=FakeContext(), **kw)
    _r1, w1 = pipeline.run(bam, str(tmp_path / "with"), 120, context=FakeContext(), fragments=True, **kw)
    assert [p.name for p in w1] == [p.name for p in w0] + ["pe_fragments.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, _stats = fragments.read_fragments(w1[-1])
    rows, counters, hist = FC.restate(recs, FC.REFS, FC.USES["all"], 2000)
    assert name == "pe" and [c.counters[k] for k in FC.COUNTERS] == counters and c.hist.tolist() == hist
    # the chosen chromosomes with the excluded regions and another bound; the pair pileup beside it
    _r2, w2 = pipeline.run(bam, str(tmp_path / "two"), 120, context=FakeContext(), references=_chosen("not_chrC"), fragments=True,
                           fragments_max=4097, exclude_regions=FC.MASK, coverage=True, coverage_extend="pair", **kw)
    assert [p.name for p in w2][-2:] == ["pe_coverage.bedGraph", "pe_fragments.tab"]
    c2 = fragments.read_fragments(w2[-1])[1]
    rows, counters, hist = FC.restate(recs, FC.REFS, FC.USES["not_chrC"], 4097, FC.MASK)
    assert [c2.counters[k] for k in FC.COUNTERS] == counters and c2.hist.tolist() == hist and c2.counters["masked"] > 0
    cov = coverage.read_coverage(w2[-2])[1]
    assert cov == CC.as_coverage(_pileup_want(recs, FC.USES["not_chrC"], 4097, FC.MASK), "pair")
    for bad in (0, 65537):
        with pytest.raises(ValueError, match="max_size is {}".format(bad)):
            pipeline.run(bam, str(tmp_path / "bad"), 120, context=FakeContext(), fragments=True, fragments_max=bad, **kw)
    with pytest.raises(ValueError, match="coverage_extend is"):
        pipeline.run(bam, str(tmp_path / "bad"), 120, context=FakeContext(), coverage=True, coverage_extend="pairs", **kw)
    # a tagAlign input: refused before it is read, skipped among several files
    bed = _tagalign(tmp_path)
    sizes = dict(FC.REFS)
    for extra in (dict(fragments=True), dict(coverage=True, coverage_extend="pair")):
        with pytest.raises(ValueError, match="the input has no mate fields"):
            pipeline.run(bed, str(tmp_path / "bad"), 120, context=FakeContext(), chrom_sizes=sizes, **extra, **kw)
    assert not os.path.exists(tmp_path / "bad") or not os.listdir(tmp_path / "bad")
    res = pipeline.run_files([bed, bam], str(tmp_path / "files"), 120, context=FakeContext(), chrom_sizes=sizes, fragments=True, **kw)
    assert res[0].error is not None and "the input has no mate fields" in str(res[0].error) and res[0].written == []
    assert res[1].error is None and res[1].written[-1].name == "pe_fragments.tab"
    assert fragments.read_fragments(res[1].written[-1])[1] == fragments.read_fragments(w1[-1])[1]
