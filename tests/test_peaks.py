"""Reads in peaks and reads per peak line without a GPU: the host checker against the loop restatement of
tests/peaks_cases, the metrics on hand-made counts, the table file, the options, and the host path of the run."""
import gzip
import math
import os

import numpy as np
import pytest

from pymasc_amd import cli, peaks, pipeline
from pymasc_amd.bam import BamReader
from pymasc_amd.peaks import PeakCounts
from tests import fixtures as fx
from tests import peaks_cases as PC
from tests.fake_context import FakeContext

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
NAMES = [n for n, _l in PC.REFS]
LENGTHS = [l for _n, l in PC.REFS]


@pytest.fixture(scope="module")
def library():
    rows = PC.synthetic()
    reads = PC.FC.kept(rows)
    assert 15_000 < len(reads) < 21_000 and {r[3] for r in reads} == {0, 1}
    return dict(rows=rows, reads=reads, lines=PC.peak_lines(), want={})


def _want(library, extend, use="all"):
    """The restatement, computed once per parameter set and left unchanged."""
    if (extend, use) not in library["want"]:
        library["want"][extend, use] = PC.restate(library["reads"], PC.REFS, PC.USES[use], library["lines"], extend)
    return library["want"][extend, use]


def _host(reads, refs, use, lines, extend):
    """``count_host`` as the dict of ``restate`` (without ``hits``)."""
    resolved = peaks.open_peaks(lines).resolve([n for n, _l in refs], [l for _n, l in refs])
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    counts, per_ref = peaks.count_host(*cols, resolved, use, extend)
    offsets, _b, _e = resolved.csr(use)
    chosen = [r for r, u in enumerate(use) if u]
    return dict(counts={refs[r][0]: counts[offsets[r]:offsets[r + 1]].tolist() for r in chosen},
                per_ref={refs[r][0]: tuple(per_ref[r].tolist()) for r in chosen}, N=int(per_ref[:, 0].sum()),
                n_in=int(per_ref[:, 1].sum()))


def _same(have, want):
    return all(have[k] == want[k] for k in ("counts", "per_ref", "N", "n_in"))


@pytest.mark.parametrize("extend", PC.EXTENDS)
def test_count_host_equals_the_restatement(library, extend):
    lines = library["lines"]
    assert 250 < sum(len(v) for v in lines.values()) < 350
    want = _want(library, extend)
    PC.check_situations(library["reads"], PC.REFS, lines, want, extend)
    assert _same(_host(library["reads"], PC.REFS, PC.USES["all"], lines, extend), want)
    part = _want(library, extend, "no middle")
    assert list(part["counts"]) == ["f0", "f2"] and part["N"] < want["N"] and part["union_bases"] < want["union_bases"]
    assert _same(_host(library["reads"], PC.REFS, PC.USES["no middle"], lines, extend), part)
    # batches add up
    half = len(library["reads"]) // 2
    a, b = (_host(x, PC.REFS, PC.USES["all"], lines, extend) for x in (library["reads"][:half], library["reads"][half:]))
    assert all([x + y for x, y in zip(a["counts"][n], b["counts"][n])] == want["counts"][n] for n in want["counts"])
    assert a["n_in"] + b["n_in"] == want["n_in"]


def test_count_host_many_lines(library):
    lines = PC.many_lines()
    reads = PC.FC.kept(PC.few(library["rows"]))
    assert len(lines["f0"]) == 3000 and len(reads) > 400
    for extend in (0, 200):
        want = PC.restate(reads, PC.REFS, [1, 1, 1], lines, extend)
        assert max(want["hits"]) > 3 and min(want["counts"]["f0"]) == 0 < max(want["counts"]["f0"])
        assert _same(_host(reads, PC.REFS, [1, 1, 1], lines, extend), want)


def test_small_cases_by_hand():
    refs = [("a", 10), ("b", 3)]
    lines = {"a": [(2, 5), (4, 12), (20, 30), (2, 5)], "b": [(0, 3)]}
    reads = [(0, 1, 2, 0), (0, 2, 2, 0), (0, 5, 1, 1), (0, 9, 5, 0), (1, 3, 4, 0), (0, 30, 4, 0)]
    # a: (2, 5) covers 3..5, (4, 12) is clipped to 5..10, (20, 30) is empty.  Reads: 1..2 in none; 2..3 in (2, 5) twice; 5..5 in all
    # three full lines; 9..10 (clipped) in (4, 12); 30.. is past the end: counted in N, in no line.  b: 3..3 (clipped) in (0, 3).
    want = PC.restate(reads, refs, [1, 1], lines, 0)
    assert want["counts"] == {"a": [2, 2, 0, 2], "b": [1]} and want["per_ref"] == {"a": (5, 3), "b": (1, 1)}
    assert (want["N"], want["n_in"], want["union_bases"], want["genome_bases"]) == (6, 4, 8 + 3, 13)
    assert _same(_host(reads, refs, [1, 1], lines, 0), want)
    # three bases from the 5' end: the reverse read at 5 covers 3..5, the forward read at 1 covers 1..3
    want = PC.restate(reads, refs, [1, 1], lines, 3)
    assert want["counts"]["a"] == [3, 2, 0, 3]
    assert _same(_host(reads, refs, [1, 1], lines, 3), want)
    assert _same(_host([], refs, [1, 1], lines, 0), PC.restate([], refs, [1, 1], lines, 0))


def _counts(per=(("c1", 1000, 40), ("c2", 500, 10)), union=150, genome=3000, extend=0):
    lines = {n: ([0, 100][:k], [50, 200][:k]) for k, (n, _r, _i) in zip((2, 1), per)}
    return PeakCounts(lines, {n: [7, 9][:len(lines[n][0])] for n in lines}, {n: (r, i) for n, r, i in per}, union, genome, extend)


def test_metrics_on_hand_made_counts():
    c = _counts()
    assert (c.N, c.n_in, c.n_lines) == (1500, 50, 3)
    assert c.frip == 50 / 1500 and c.enrichment == (50 / 1500) / (150 / 3000)
    empty = _counts(per=(("c1", 0, 0), ("c2", 0, 0)))
    assert math.isnan(empty.frip) and math.isnan(empty.enrichment)
    assert math.isnan(_counts(per=(("c1", 5, 0), ("c2", 0, 0)), union=0).enrichment)       # no base in a line: 0 / 0
    assert c == _counts() and c != _counts(extend=5) and c != _counts(union=151) and c != _counts(per=(("c1", 1000, 41), ("c2", 500, 10)))
    with pytest.raises(ValueError):
        PeakCounts({"c": ([0], [5])}, {"c": [1, 2]}, {"c": (3, 1)}, 5, 10, 0)


def test_table_round_trip(tmp_path):
    c = PeakCounts({"f0": ([500, 10, 500], [900, 20, 900]), "f1": ([], []), "f2": ([7], [70_500])},
                   {"f0": [12, 0, 12], "f1": [], "f2": [3]}, {"f0": (100, 12), "f1": (4, 0), "f2": (9, 3)}, 70_404, 170_503, 200)
    path = peaks.write_peaks(tmp_path / "x.y", "x.y", c, "some.narrowPeak")
    assert path.name == "x.y_peaks.tab" and sorted(os.listdir(tmp_path)) == ["x.y_peaks.tab"]
    name, back, block = peaks.read_peaks(path)
    assert name == "x.y" and back == c and block["Peak file"] == "some.narrowPeak"
    assert (block["FRiP"], block["Enrichment"]) == (c.frip, c.enrichment)                   # repr: they read back exactly
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert [r[0] for r in rows[:10]] == ["Name", "Peak file", "Extend", "Lines", "Peak bases", "Genome bases", "Reads", "Reads in peaks",
                                         "FRiP", "Enrichment"]
    assert rows[2:8] == [["Extend", "200"], ["Lines", "4"], ["Peak bases", "70404"], ["Genome bases", "170503"], ["Reads", "113"],
                         ["Reads in peaks", "15"]]
    assert rows[10:14] == [["chrom", "lines", "reads", "reads_in_peaks"], ["f0", "3", "100", "12"], ["f1", "0", "4", "0"], ["f2", "1", "9", "3"]]
    assert rows[14:] == [["#chrom", "start", "end", "reads"], ["f0", "500", "900", "12"], ["f0", "10", "20", "0"], ["f0", "500", "900", "12"],
                         ["f2", "7", "70500", "3"]]
    empty = PeakCounts({"f0": ([], [])}, {"f0": []}, {"f0": (0, 0)}, 0, 100, 0)
    _n, back, block = peaks.read_peaks(peaks.write_peaks(tmp_path / "e", "e", empty))
    assert back == empty and math.isnan(block["FRiP"]) and math.isnan(block["Enrichment"])


def test_peak_files_keep_every_line_in_file_order(tmp_path, library, caplog):
    lines = library["lines"]
    plain, packed = tmp_path / "p.bed", tmp_path / "p.narrowPeak.gz"
    plain.write_text("".join(PC.bed_text(lines)))
    with gzip.open(packed, "wt") as fp:
        fp.write("".join(PC.bed_text(lines, wide=True)))
    for path in (plain, packed):
        got = peaks.open_peaks(str(path))
        assert got.source == str(path) and set(got.lines) == set(lines)
        for n, ivs in lines.items():            # unsorted, repeated and nested lines: every one, in the file's order
            assert list(zip(got.lines[n][0].tolist(), got.lines[n][1].tolist())) == ivs
    with caplog.at_level("WARNING"):
        resolved = got.resolve(NAMES, LENGTHS)
    assert "Peak file: 1 chromosome name(s) are not among the alignment's references" in caplog.text
    offsets, b, e = resolved.csr([1, 0, 1])
    assert offsets.tolist() == [0, len(lines["f0"]), len(lines["f0"]), len(lines["f0"]) + len(lines["f2"])]
    assert list(zip(b.tolist(), e.tolist())) == lines["f0"] + lines["f2"]                   # unmerged and unclipped
    assert max(resolved.lines(0, clip=True)[1].tolist()) == LENGTHS[0] < max(e.tolist())
    with pytest.raises(ValueError, match="no chromosome of the peak file .* is among the alignment's references"):
        got.resolve(["chr1", "chr2"], [1000, 1000])
    with pytest.raises(FileNotFoundError, match="peak file: no such file"):
        peaks.open_peaks(str(tmp_path / "none.bed"))


def test_options(tmp_path, capsys):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert (a.peaks, a.peaks_extend) == (None, None)
    bed = tmp_path / "p.narrowPeak"
    bed.write_text("chr1\t5\t10\n")
    a = cli.parse_args(base + ["--peaks", str(bed), "--peaks-extend", "200"])
    assert a.peaks == bed and a.peaks_extend == 200
    for bad in (["--peaks-extend", "200"], ["--peaks", str(tmp_path / "none.bed")], ["--peaks", str(bed), "--peaks-extend", "0"],
                ["--peaks", str(bed), "--peaks-extend", "x"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2
        assert cli.main(base + bad) == 2
    err = capsys.readouterr().err
    assert "needs a peak file" in err and "no such file" in err
    assert "_peaks.tab" in cli.get_parser().format_help()


def test_options_reach_run_files(tmp_path, monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bed = tmp_path / "p.bed"
    bed.write_text("chr1\t5\t10\n")
    assert cli.main(["a.bam", "--skip-plots"]) == 0
    assert not any(k.startswith("peaks") for k in seen)
    seen.clear()
    assert cli.main(["a.bam", "--skip-plots", "--peaks", str(bed), "--peaks-extend", "150"]) == 0
    assert {k: v for k, v in seen.items() if k.startswith("peaks")} == dict(peaks=str(bed), peaks_extend=150)


def golden_case(mapq=10):
    """(refs, reads, lines) of the golden BAM: lines about every 40th read of chr1, some twice, one nesting others, a line past
    the end of the second reference, and a name the header lacks."""
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, b.lengths))
        cols = [np.concatenate(x).tolist() for x in zip(*b.batches(mapq))]
    reads = list(zip(cols[0], cols[1], cols[2], [int(x) for x in cols[3]]))
    at = sorted({r[1] for r in reads if r[0] == 0})[::40][:30]
    first = [(max(p - 120, 0), p + 80) for p in at]
    lines = {refs[0][0]: first[::-1] + first[:3] + [(first[0][0], first[10][1])], refs[1][0]: [(refs[1][1] - 10, refs[1][1] + 500)],
             "not_there": [(1, 2)]}
    return refs, reads, lines


def test_pipeline_writes_the_table_and_nothing_else_changes(tmp_path):
    refs, reads, lines = golden_case()
    bed = tmp_path / "golden.narrowPeak"
    bed.write_text("".join(PC.bed_text(lines, wide=True)))
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, stats=True, complexity=True)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 120, context=FakeContext(), **kw)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 120, context=FakeContext(), peaks=str(bed), **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_peaks.tab"] and len(w0) == 4
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, block = peaks.read_peaks(w1[-1])
    want = PC.restate(reads, refs, [1] * len(refs), lines, 0)
    assert name == stem and block["Peak file"] == str(bed) and c.extend == 0 and list(c.lines) == [n for n, _l in refs]
    assert {n: v.tolist() for n, v in c.counts.items()} == want["counts"] and c.per_reference == want["per_ref"]
    assert (c.N, c.n_in, c.union_bases, c.genome_bases) == (want["N"], want["n_in"], want["union_bases"], want["genome_bases"])
    assert 0 < c.n_in < c.N and block["FRiP"] == c.n_in / c.N and block["Enrichment"] > 1
    assert [list(zip(b.tolist(), e.tolist())) for b, e in list(c.lines.values())[:2]] == [lines[refs[0][0]], lines[refs[1][0]]]
    # the chosen chromosomes, an extension, a dict, beside a fingerprint
    chosen = [refs[0][0], refs[2][0]]
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 120, context=FakeContext(), references=chosen, peaks=lines, peaks_extend=200,
                           fingerprint=True, **kw)
    assert [p.name.rsplit("_", 1)[-1] for p in w2[-2:]] == ["fingerprint.tab", "peaks.tab"]
    _n, c2, block2 = peaks.read_peaks(w2[-1])
    part = PC.restate(reads, refs, [1 if n in chosen else 0 for n, _l in refs], lines, 200)
    assert list(c2.lines) == chosen and {n: v.tolist() for n, v in c2.counts.items()} == part["counts"] and c2.extend == 200
    assert (c2.per_reference, c2.union_bases, c2.genome_bases, block2["Peak file"]) == (part["per_ref"], part["union_bases"],
                                                                                        part["genome_bases"], "")
    with BamReader(GOLDEN_BAM) as b:
        assert b.peak_counts(lines, 10, chosen, 200) == c2
    with pytest.raises(ValueError, match="peaks_extend"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, context=FakeContext(), peaks_extend=5, **kw)
    with pytest.raises(ValueError, match="no chromosome of the peak file"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, context=FakeContext(), peaks={"not_there": [(1, 2)]}, **kw)
    assert not (tmp_path / "bad").exists()      # before any table is written


def test_a_peak_file_without_a_matching_name_skips_the_sample(tmp_path):
    refs, _reads, lines = golden_case()
    from tests import sam_writers as SW
    other = [("x" + n, l) for n, l in refs]
    (tmp_path / "in").mkdir()
    _sam, renamed = SW.write_twins(tmp_path / "in", "renamed", other, [SW.rec("q0", 0, other[0][0], 100, 40, (("M", 36),))])
    out = pipeline.run_files([renamed, GOLDEN_BAM], str(tmp_path / "out"), 120, read_len=36, mapq_criteria=10, device_ingest=False,
                             context=FakeContext(), peaks=lines)
    assert isinstance(out[0].error, ValueError) and "peak file" in str(out[0].error) and out[0].written == []
    assert out[1].error is None and out[1].written[-1].name == "ENCFF000RMB-test_peaks.tab"
    assert sorted(os.listdir(tmp_path / "out")) == sorted(p.name for p in out[1].written)       # the skipped file gets no table
