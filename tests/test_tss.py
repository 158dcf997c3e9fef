"""The read profile around anchor sites without a GPU: the host path through the host readers against the
restatement of tests/tss_cases, the statistics against the formula on plain ints, the table file, the refusals and the options."""
import gzip
import math
import os

import numpy as np
import pytest

from pymasc_amd import cli, pipeline, tss
from pymasc_amd.bam import BamReader
from pymasc_amd.bed_reads import BedReadsReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.tss import TssProfile
from tests import fixtures as fx
from tests import sam_writers as SW
from tests import tss_cases as TC
from tests.fake_context import FakeContext

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
NAMES = [n for n, _l in TC.REFS]
LENGTHS = [l for _n, l in TC.REFS]
FC = TC.FC


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    d = tmp_path_factory.mktemp("tss")
    rows = TC.synthetic()
    reads = FC.kept(rows)
    assert 15_000 < len(reads) < 21_000 and {r[3] for r in reads} == {0, 1}
    _sam, bam = SW.write_twins(d, "ts", TC.REFS, FC.alignment_records(rows, TC.REFS))
    tag = str(d / "ts.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, TC.REFS)))
    sites = TC.anchor_sites()
    bed = d / "sites.bed"
    bed.write_text("".join(TC.bed_text(sites)))
    return dict(dir=d, rows=rows, reads=reads, bam=bam, tag=tag, sites=sites, bed=str(bed), parts={})


def want_of(library, flank, extend, use="all"):
    """The restatement, computed once per (flank, extend) and left unchanged."""
    if (flank, extend) not in library["parts"]:
        library["parts"][flank, extend] = TC.restate_by_reference(library["reads"], TC.REFS, library["sites"], flank, extend)
    return TC.combine(library["parts"][flank, extend], TC.USES[use])


def expected(want, flank, extend):
    """The restatement as the TssProfile the package must return."""
    return TssProfile(want["same"], want["opposite"], want["N"], want["n_near"], want["anchors"], want["pairs"], flank, extend)


def chosen(use):
    return [n for n, u in zip(NAMES, TC.USES[use]) if u]


def check_statistics(c, want, flank):
    """The statistics of ``c`` equal the formula applied to the restated ints, float for float."""
    background, normalized, best, at_tss, offset = TC.statistics(want, flank)
    assert c.total.tolist() == [s + o for s, o in zip(want["same"], want["opposite"])] and c.background == background
    if normalized is None:
        assert all(math.isnan(x) for x in (c.enrichment, c.at_tss, c.peak_offset)) and np.isnan(c.normalized).all()
    else:
        assert c.normalized.tolist() == normalized and (c.enrichment, c.at_tss, c.peak_offset) == (best, at_tss, offset)


@pytest.mark.parametrize("extend", TC.EXTENDS)
@pytest.mark.parametrize("flank", TC.FLANKS)
def test_the_host_path_equals_the_restatement(library, flank, extend):
    TC.check_situations(library["reads"], TC.REFS, library["sites"], want_of(library, flank, extend), flank, extend)
    with BamReader(library["bam"]) as bam, BedReadsReader(library["tag"], NAMES, LENGTHS) as tag:
        for use in sorted(TC.USES):
            want = want_of(library, flank, extend, use)
            c = bam.tss_profile(library["sites"], FC.MAPQ, chosen(use), flank, extend)
            assert c == expected(want, flank, extend) and c.same.dtype == np.int64
            assert tag.tss_profile(library["bed"], FC.MAPQ, chosen(use), flank, extend) == c     # a BED6 file gives what the dict gives
            check_statistics(c, want, flank)
    assert want_of(library, flank, extend, "no middle")["anchors"] == want_of(library, flank, extend)["anchors"] - len(TC.ON_F1)


def test_the_two_restatements_agree(library):
    reads = FC.kept(TC.few(library["rows"], 100))
    sites = {"f0": library["sites"]["f0"]}
    for flank, extend in ((1, 0), (50, 0), (50, 1), (2000, 1)):
        assert TC.restate_literal(reads, TC.REFS, [1, 1, 1], sites, flank, extend) == TC.restate(reads, TC.REFS, [1, 1, 1], sites, flank, extend)


def test_small_cases_by_hand():
    refs = [("a", 20), ("b", 5)]
    sites = {"a": [(10, "+"), (10, "-"), (20, "+")], "b": [(1, "-")]}
    reads = [(0, 9, 3, 0), (0, 17, 6, 1), (1, 2, 2, 0), (0, 1, 2, 0)]
    # F = 2.  a: the forward read 9..11 lies at the offsets -1..1 of (10, +): same, and at 1..-1 of (10, -): opposite.  The reverse
    # read 17..22 is clipped to 17..20: the offsets -2..0 of (20, +), opposite (17 is out of reach).  The read 1..2 is near nothing.
    # b: the forward read 2..3 lies at the offsets -1, -2 of (1, -): opposite.
    want = TC.restate(reads, refs, [1, 1], sites, 2, 0)
    assert want == TC.restate_literal(reads, refs, [1, 1], sites, 2, 0)
    assert (want["same"], want["opposite"]) == ([0, 1, 1, 1, 0], [2, 3, 2, 1, 0])
    assert (want["N"], want["n_near"], want["pairs"], want["anchors"]) == (4, 3, 4, 4)
    cols = [np.array(c) for c in zip(*reads)]
    bound = tss.open_anchors(sites, ["a", "b"], [20, 5])
    table, n, n_near, pairs = tss.count_host(*cols, bound, [1, 1], 2, 0)
    assert (table.tolist(), n, n_near, pairs) == ([want["same"], want["opposite"]], 4, 3, 4)
    # the 5' base only: 9 (forward) and 22 -> clipped away (reverse: its extent lies past the end)
    want = TC.restate_literal(reads, refs, [1, 1], sites, 2, 1)
    assert (want["same"], want["opposite"], want["n_near"]) == ([0, 1, 0, 0, 0], [0, 1, 0, 1, 0], 2)
    table, n, n_near, pairs = tss.count_host(*cols, bound, [1, 1], 2, 1)
    assert (table.tolist(), n, n_near, pairs) == ([want["same"], want["opposite"]], 4, 2, want["pairs"])


def test_statistics_on_hand_made_tables():
    same, opposite = [1, 0, 5, 2, 1], [1, 2, 5, 0, 1]
    c = TssProfile(same, opposite, 50, 9, 3, 11, 2, 0)
    check_statistics(c, dict(same=same, opposite=opposite), 2)
    assert (c.background, c.enrichment, c.at_tss, c.peak_offset) == (2.0, 5.0, 5.0, 0)
    flat = TssProfile([0, 3, 0, 3, 0], [0] * 5, 5, 2, 1, 2, 2, 1)      # nothing at the edges: no background
    check_statistics(flat, dict(same=[0, 3, 0, 3, 0], opposite=[0] * 5), 2)
    assert flat.background == 0 and math.isnan(flat.enrichment) and math.isnan(flat.at_tss) and math.isnan(flat.peak_offset)
    first = TssProfile([1, 4, 0, 4, 1], [0] * 5, 5, 2, 1, 2, 2, 1)     # the first of two equal maxima
    assert first.peak_offset == -1
    assert c == TssProfile(same, opposite, 50, 9, 3, 11, 2, 0) and c != TssProfile(same, opposite, 50, 9, 3, 12, 2, 0) and c != flat
    with pytest.raises(ValueError):
        TssProfile([1, 2, 3], [1, 2, 3], 1, 1, 1, 1, 2, 0)


def test_table_round_trip(tmp_path, library):
    want = want_of(library, 50, 1)
    c = expected(want, 50, 1)
    path = tss.write_tss(tmp_path / "x.y", "x.y", c, "sites.bed")
    assert path.name == "x.y_tss.tab" and sorted(os.listdir(tmp_path)) == ["x.y_tss.tab"]
    name, back, block = tss.read_tss(path)
    assert name == "x.y" and back == c and block["Anchor file"] == "sites.bed"
    assert (block["Background"], block["TSS enrichment"], block["At TSS"], block["Peak offset"]) == (c.background, c.enrichment, c.at_tss,
                                                                                                  c.peak_offset)
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert [r[0] for r in rows[:12]] == ["Name", "Anchor file", "Flank", "Extend", "Anchors", "Reads", "Reads near anchors",
                                         "Read-anchor pairs", "Background", "TSS enrichment", "At TSS", "Peak offset"]
    assert rows[12] == ["offset", "same", "opposite", "total", "normalized"] and len(rows) == 13 + 101
    assert [int(r[0]) for r in rows[13:]] == list(range(-50, 51)) and [float(r[4]) for r in rows[13:]] == c.normalized.tolist()
    empty = TssProfile([0] * 3, [0] * 3, 7, 0, 0, 0, 1, 0)
    _n, back, block = tss.read_tss(tss.write_tss(tmp_path / "e", "e", empty))
    assert back == empty and all(math.isnan(block[k]) for k in ("TSS enrichment", "At TSS", "Peak offset")) and block["Background"] == 0


def test_refusals(tmp_path, library):
    with BamReader(library["bam"]) as r:
        for flank in (0, 4096):
            with pytest.raises(ValueError, match="the flank is {}".format(flank)):
                r.tss_profile(library["sites"], FC.MAPQ, None, flank)
        with pytest.raises(ValueError, match="extend is not negative"):
            r.tss_profile(library["sites"], FC.MAPQ, None, 50, -1)
        for a in (0, LENGTHS[1] + 1):
            with pytest.raises(ValueError, match="position {} is outside f1".format(a)):
                r.tss_profile({"f1": [(5, "+"), (a, "-")]}, FC.MAPQ)
        with pytest.raises(ValueError, match="not among the alignment's references"):
            r.tss_profile({"f0": [(5, "+")], TC.MISSING: [(5, "+")]}, FC.MAPQ)
        with pytest.raises(ValueError, match="strand"):
            r.tss_profile({"f0": [(5, ".")]}, FC.MAPQ)
        for name, text, message in (("dot.bed", "f0\t5\t9\tn\t0\t.\n", "strand is neither"), ("three.bed", "f0\t5\t9\n", "fewer than 6 fields"),
                                    ("other.bed", "f0\t5\t9\tn\t0\t+\nzz\t5\t9\tn\t0\t+\n", "line 2: chrom is not a chromosome"),
                                    ("past.bed", "f1\t490\t500\tn\t0\t-\n", "position 500 is outside f1")):
            (tmp_path / name).write_text(text)
            with pytest.raises((PmxIOError, ValueError), match=message):
                r.tss_profile(str(tmp_path / name), FC.MAPQ)
    with pytest.raises(ValueError, match="more than 2\\^20"):
        tss.Anchors(NAMES, LENGTHS, np.zeros((1 << 20) + 1, dtype=np.int32), np.ones((1 << 20) + 1), np.zeros((1 << 20) + 1))


def test_anchor_files(tmp_path, library):
    sites = library["sites"]
    packed = tmp_path / "sites.bed.gz"
    with gzip.open(packed, "wt") as fp:
        fp.write("#a comment\n" + "".join(TC.bed_text(sites)))
    for path in (library["bed"], str(packed)):
        got = tss.open_anchors(path, NAMES, LENGTHS)
        assert got.source == path and len(got) == sum(len(v) for v in sites.values())
        have = sorted(zip(got.ref.tolist(), got.pos1.tolist(), got.reverse.tolist()))
        assert have == sorted((NAMES.index(n), a, int(s == "-")) for n, v in sites.items() for a, s in v)
    source = tss.AnchorSource(library["bed"])
    assert source.resolve(NAMES, LENGTHS) is source.resolve(NAMES, LENGTHS)                 # read once per header
    assert tss.open_anchors(got, NAMES, LENGTHS) is got
    with pytest.raises(ValueError):
        tss.open_anchors(got, NAMES, [l + 1 for l in LENGTHS])


def test_options(tmp_path, capsys):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert (a.tss, a.tss_flank, a.tss_extend) == (None, None, None)
    bed = tmp_path / "sites.bed"
    bed.write_text("chr1\t5\t10\tn\t0\t+\n")
    a = cli.parse_args(base + ["--tss", str(bed), "--tss-flank", "500", "--tss-extend", "1"])
    assert (a.tss, a.tss_flank, a.tss_extend) == (bed, 500, 1)
    for bad in (["--tss-flank", "500"], ["--tss-extend", "1"], ["--tss", str(tmp_path / "none.bed")], ["--tss", str(bed), "--tss-flank", "0"],
                ["--tss", str(bed), "--tss-flank", "4096"], ["--tss", str(bed), "--tss-extend", "x"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2
        assert cli.main(base + bad) == 2
    err = capsys.readouterr().err
    assert "--tss-flank: needs an anchor file (--tss)" in err and "--tss-extend: needs an anchor file (--tss)" in err
    assert "no such file" in err and "it must lie in [1, 4095]" in err
    assert "_tss.tab" in cli.get_parser().format_help()


def test_options_reach_run_files(tmp_path, monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bed = tmp_path / "sites.bed"
    bed.write_text("chr1\t5\t10\tn\t0\t+\n")
    assert cli.main(["a.bam", "--skip-plots"]) == 0
    assert not any(k.startswith("tss") for k in seen)
    seen.clear()
    assert cli.main(["a.bam", "--skip-plots", "--tss", str(bed), "--tss-flank", "300", "--tss-extend", "1"]) == 0
    assert {k: v for k, v in seen.items() if k.startswith("tss")} == dict(tss=str(bed), tss_flank=300, tss_extend=1)


def golden_case(mapq=10):
    """(refs, reads, sites) of the golden BAM: anchors on about every 40th read start of the first reference, on both strands, some
    twice, and one on the last base of the second reference."""
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, b.lengths))
        cols = [np.concatenate(x).tolist() for x in zip(*b.batches(mapq))]
    reads = list(zip(cols[0], cols[1], cols[2], [int(x) for x in cols[3]]))
    at = sorted({r[1] for r in reads if r[0] == 0})[::40][:30]
    first = [(p + 20, "+-"[k % 2]) for k, p in enumerate(at)]
    return refs, reads, {refs[0][0]: first[::-1] + first[:3], refs[1][0]: [(refs[1][1], "-")]}


def test_pipeline_writes_the_table_and_nothing_else_changes(tmp_path):
    refs, reads, sites = golden_case()
    bed = tmp_path / "golden.bed"
    bed.write_text("".join(TC.bed_text(sites)))
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, complexity=True)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 40, context=FakeContext(), **kw)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 40, context=FakeContext(), tss=str(bed), tss_flank=300, **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_tss.tab"] and len(w0) == 3
    assert [p.name.rsplit("_", 1)[-1] for p in w1[-2:]] == ["complexity.tab", "tss.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, block = tss.read_tss(w1[-1])
    want = TC.restate(reads, refs, [1] * len(refs), sites, 300, 0)
    assert name == stem and block["Anchor file"] == str(bed) and c == expected(want, 300, 0) and 0 < c.n_near < c.N
    assert block["TSS enrichment"] == TC.statistics(want, 300)[2] > 1
    # the chosen chromosomes, the 5' base, a dict: the host reader, as the run reads it
    chosen_refs = [refs[0][0], refs[2][0]]
    part = TC.restate(reads, refs, [1 if n in chosen_refs else 0 for n, _l in refs], sites, 2000, 1)
    with BamReader(GOLDEN_BAM) as b:
        c2 = b.tss_profile(sites, 10, chosen_refs, 2000, 1)
    assert c2 == expected(part, 2000, 1) and c2.anchors == len(sites[refs[0][0]])
    for bad in (dict(tss_flank=5), dict(tss_extend=1)):
        with pytest.raises(ValueError, match="need tss"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 40, context=FakeContext(), **bad, **kw)
    with pytest.raises(ValueError, match="not among the alignment's references"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 40, context=FakeContext(), tss={"not_there": [(1, "+")]}, **kw)
    assert not (tmp_path / "bad").exists()      # before any table is written


def test_anchors_that_do_not_match_skip_the_sample(tmp_path):
    refs, _reads, sites = golden_case()
    bed = tmp_path / "golden.bed"
    bed.write_text("".join(TC.bed_text(sites)))
    other = [("x" + n, l) for n, l in refs]
    (tmp_path / "in").mkdir()
    _sam, renamed = SW.write_twins(tmp_path / "in", "renamed", other, [SW.rec("q0", 0, other[0][0], 100, 40, (("M", 36),))])
    out = pipeline.run_files([renamed, GOLDEN_BAM], str(tmp_path / "out"), 40, read_len=36, mapq_criteria=10, device_ingest=False,
                             context=FakeContext(), tss=str(bed), tss_flank=300)
    assert isinstance(out[0].error, ValueError) and "anchor file" in str(out[0].error) and out[0].written == []
    assert out[1].error is None and out[1].written[-1].name == "ENCFF000RMB-test_tss.tab"
    assert sorted(os.listdir(tmp_path / "out")) == sorted(p.name for p in out[1].written)       # the skipped file gets no table
