"""GC bias without a GPU: the host checker against the loop restatement of tests/gcbias_cases through the host
BamReader, the metrics against their formulas, the table file, the header checks, the options, and the host path of the run."""
import gzip
import math
import os

import pytest

from pymasc_amd import cli, gcbias, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.gcbias import GcBias
from tests import gcbias_cases as GC
from tests import io_writers as W
from tests import sam_writers as SW
from tests.fake_context import FakeContext

NAMES = [n for n, _l in GC.REFS]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gcbias")
    fasta = d / "genome.fa"
    fasta.write_bytes(GC.fasta_text())
    rows = GC.synthetic()
    recs = GC.alignment_records(rows)
    assert any(r["flag"] & 0x400 for r in recs) and any(r["flag"] & 0x80 for r in recs) and any(r["flag"] & 0x4 for r in recs)
    _sam, bam = SW.write_twins(d, "gc", GC.REFS, recs)[:2]
    reads = GC.kept(rows)
    assert len(reads) > 80_000 and {r[3] for r in reads} == {0, 1} and {r[2] for r in reads} == set(GC.READ_LENS)
    return dict(dir=d, fasta=str(fasta), bam=bam, reads=reads, less=GC.masked(reads), genome=gcbias.HostGenome(str(fasta)))


def _chosen(use):
    return [n for n, u in zip(NAMES, GC.USES[use]) if u]


def test_the_fasta_reads_back(case):
    g = GC.genome()
    records = gcbias.read_fasta(case["fasta"])
    assert list(records) == list(GC.FASTA_ORDER)
    assert all(records[n].tobytes().decode() == g[n] for n in g)
    text = GC.fasta_text()
    assert b"\r\n" in text and any(ln.islower() for ln in text.split(b"\n") if ln and ln[:1] != b">")
    gz = case["dir"] / "genome.fa.gz"
    gz.write_bytes(gzip.compress(text))
    bgz = case["dir"] / "genome.bgz.fa.gz"
    bgz.write_bytes(W.bgzf_compress(text))
    for twin in (gz, bgz):
        h = gcbias.HostGenome(str(twin))
        assert (h.names, h.lengths) == (case["genome"].names, case["genome"].lengths)
    assert case["genome"].lengths == tuple(len(g[n]) for n in GC.FASTA_ORDER)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("use", sorted(GC.USES))
@pytest.mark.parametrize("window", GC.PARAMS)
def test_count_host_equals_the_restatement(case, window, use, masked):
    reads = case["less" if masked else "reads"]
    flags = GC.USES[use]
    assert GC.wanted_situations(flags, window, masked) <= GC.situations(reads, flags, window, masked)
    N, F, off_end, blocked = GC.restate(reads, flags, window, masked)
    assert sum(N) + GC.blocked_windows(flags, window, masked) == sum(max(0, l - window + 1) for (_n, l), u in zip(GC.REFS, flags) if u)
    if window == 1:                 # the unblocked bases of the chosen references
        g = GC.blocked_genome(GC.MASK if masked else None)
        assert N[0] + N[1] == sum(sum(g[n].count(c) for c in "ACGT") for (n, _l), u in zip(GC.REFS, flags) if u)
    assert N[0] > 0 and N[window] > 0 and sum(F) > 70_000 and off_end > 0 and blocked > 0
    with BamReader(case["bam"]) as r:
        if masked:
            r.set_exclude(region_mask.open_mask(GC.MASK).resolve(r.references, r.lengths))
        c = r.gc_bias(case["genome"], GC.MAPQ, _chosen(use), window)
    assert (c.N.tolist(), c.F.tolist(), c.off_end, c.blocked) == (N, F, off_end, blocked)
    assert (c.windows, c.reads, c.window) == (sum(N), sum(F), window)
    assert c.per_reference == {n: max(0, l - window + 1) for (n, l), u in zip(GC.REFS, flags) if u}


def _formulas(N, F, w):
    windows, reads = sum(N), sum(F)
    n, f = [x / windows for x in N], [x / reads for x in F]
    return dict(normalized=[f[g] / n[g] if N[g] else float("nan") for g in range(w + 1)],
                at_dropout=100 * sum(max(0.0, n[g] - f[g]) for g in range(w + 1) if 2 * g <= w),
                gc_dropout=100 * sum(max(0.0, n[g] - f[g]) for g in range(w + 1) if 2 * g > w),
                window_gc=sum(g * N[g] for g in range(w + 1)) / (w * windows), read_gc=sum(g * F[g] for g in range(w + 1)) / (w * reads),
                distance=0.5 * sum(abs(n[g] - f[g]) for g in range(w + 1)))


def test_metrics_against_their_formulas(case):
    tables = [(4, [10, 0, 50, 30, 10], [1, 0, 70, 20, 9]), (5, [1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1]), (1, [7, 3], [0, 5])]
    with BamReader(case["bam"]) as r:
        c = r.gc_bias(case["genome"], GC.MAPQ, None, 100)
    tables.append((100, c.N.tolist(), c.F.tolist()))
    for w, N, F in tables:
        c = GcBias(w, {"a": 1}, N, F, 3, 4)
        want = _formulas(N, F, w)
        for k in ("at_dropout", "gc_dropout", "window_gc", "read_gc", "distance"):
            assert math.isclose(getattr(c, k), want[k], rel_tol=1e-12), k
        for have, x in zip(c.normalized.tolist(), want["normalized"]):
            assert (math.isnan(have) and math.isnan(x)) or math.isclose(have, x, rel_tol=1e-12)
    c = GcBias(4, {"a": 1}, *tables[0][1:], 0, 0)
    assert math.isnan(c.normalized[1]) and not math.isnan(c.normalized[0])        # a g with N[g] == 0
    assert 0 <= c.distance <= 1 and c.at_dropout >= 0 and c.gc_dropout >= 0
    for empty in (GcBias(4, {"a": 1}, [1, 2, 3, 4, 5], [0] * 5, 7, 0), GcBias(4, {"a": 0}, [0] * 5, [0] * 5, 7, 0)):
        assert empty.reads == 0                                                   # reads == 0 (and windows == 0): nan everywhere
        assert all(math.isnan(x) for x in (empty.at_dropout, empty.gc_dropout, empty.window_gc, empty.read_gc, empty.distance))
        assert all(math.isnan(x) for x in empty.normalized)


def test_equality_and_checks():
    a = GcBias(2, {"a": 5}, [1, 2, 3], [3, 2, 1], 1, 2)
    assert a == GcBias(2, {"a": 5}, [1, 2, 3], [3, 2, 1], 1, 2, "other.fa")
    assert a != GcBias(2, {"a": 5}, [1, 2, 3], [3, 2, 1], 1, 3) and a != GcBias(2, {"b": 5}, [1, 2, 3], [3, 2, 1], 1, 2)
    assert a != GcBias(2, {"a": 5}, [1, 2, 4], [3, 2, 1], 1, 2)
    with pytest.raises(ValueError):
        GcBias(2, {}, [1, 2], [1, 2, 3], 0, 0)
    for bad in (0, 1025, -1, 2.5, True):
        with pytest.raises(ValueError, match="it must lie in \\[1, 1024\\]"):
            gcbias.check_window(bad)


def test_table_round_trip(case, tmp_path):
    with BamReader(case["bam"]) as r:
        c = r.gc_bias(case["fasta"], GC.MAPQ, _chosen("no middle"), 64)
    path = gcbias.write_gcbias(tmp_path / "s.1", "s.1", c)
    assert path.name == "s.1_gcbias.tab" and sorted(os.listdir(tmp_path)) == ["s.1_gcbias.tab"]
    rows = [ln.split("\t") for ln in path.read_text().splitlines()]
    assert [r[0] for r in rows[:12]] == ["Name", "Genome", "Window", "Windows", "Reads", "Off end", "Blocked", "Window GC", "Read GC",
                                         "AT dropout", "GC dropout", "Distance"]
    assert rows[12] == ["chrom", "windows"] and [r[0] for r in rows[13:15]] == _chosen("no middle")
    assert rows[15] == ["gc", "windows", "reads", "normalized"] and len(rows) == 16 + 65 and [int(r[0]) for r in rows[16:]] == list(range(65))
    name, back, block = gcbias.read_gcbias(path)
    assert name == "s.1" and back == c and back.genome == case["fasta"]                       # the integers exactly
    for label, have in (("Window GC", c.window_gc), ("Read GC", c.read_gc), ("AT dropout", c.at_dropout), ("GC dropout", c.gc_dropout),
                        ("Distance", c.distance)):
        assert repr(block[label]) == repr(have) == dict((r[0], r[1]) for r in rows[:12])[label]   # the floats by repr
    assert [repr(x) for x in block["normalized"]] == [repr(float(x)) for x in c.normalized.tolist()]
    empty = GcBias(2, {"a": 0}, [0, 0, 0], [0, 0, 0], 5, 0)
    _n, back, block = gcbias.read_gcbias(gcbias.write_gcbias(tmp_path / "e", "e", empty))
    assert back == empty and math.isnan(block["Distance"])


def test_header_mismatch_names_the_reference(case, tmp_path):
    g = GC.genome()

    def fasta(name, records):
        p = tmp_path / name
        p.write_text("".join(">{}\n{}\n".format(n, s) for n, s in records))
        return str(p)
    with BamReader(case["bam"]) as r:
        shuffled = fasta("shuffled.fa", [(n, g[n]) for n in ("g1", "g2", "g0")])
        assert r.gc_bias(shuffled, GC.MAPQ, None, 33) == r.gc_bias(case["genome"], GC.MAPQ, None, 33)     # the order is free
        renamed = fasta("renamed.fa", [("g0", g["g0"]), ("g1", g["g1"]), ("chr2", g["g2"])])
        with pytest.raises(ValueError, match="reference 'g2' has no record in the genome"):
            r.gc_bias(renamed, GC.MAPQ, None, 33)
        shorter = fasta("shorter.fa", [("g0", g["g0"]), ("g1", g["g1"][:-1]), ("g2", g["g2"])])
        with pytest.raises(ValueError, match="reference 'g1' is 499 long in the alignment header and 498 in the genome"):
            r.gc_bias(shorter, GC.MAPQ, None, 33)
        assert r.gc_bias(shorter, GC.MAPQ, _chosen("no middle"), 33) == r.gc_bias(case["genome"], GC.MAPQ, _chosen("no middle"), 33)
        with pytest.raises(ValueError, match="no chosen reference"):
            r.gc_bias(case["genome"], GC.MAPQ, [], 33)
        for bad in (0, 1025):
            with pytest.raises(ValueError, match="the window is {}".format(bad)):
                r.gc_bias(case["genome"], GC.MAPQ, None, bad)
    bad = tmp_path / "bad.fa"
    bad.write_text(">a\nACGT\nAC-T\n")
    with pytest.raises(ValueError, match="line 3: sequence byte that is not a letter"):
        gcbias.HostGenome(str(bad))


def test_options(tmp_path, capsys):
    base = ["a.bam", "-d", "100"]
    genome = tmp_path / "genome.fa"
    genome.write_text(">a\nACGT\n")
    a = cli.parse_args(base)
    assert (a.gc_bias, a.gc_window) == (None, None)
    a = cli.parse_args(base + ["--gc-bias", str(genome), "--gc-window", "64"])
    assert (a.gc_bias, a.gc_window) == (genome, 64)
    for bad in (["--gc-window", "64"], ["--gc-bias", str(genome), "--gc-window", "0"], ["--gc-bias", str(genome), "--gc-window", "1025"],
                ["--gc-bias", str(tmp_path / "none.fa")]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2
        assert cli.main(base + bad) == 2
    assert "needs a genome" in capsys.readouterr().err
    assert "_gcbias.tab" in cli.get_parser().format_help()


def test_options_reach_run_files(tmp_path, monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    genome = tmp_path / "genome.fa"
    genome.write_text(">a\nACGT\n")
    assert cli.main(["a.bam", "--skip-plots"]) == 0
    assert not any(k.startswith("gc_") for k in seen)
    seen.clear()
    assert cli.main(["a.bam", "--skip-plots", "--gc-bias", str(genome), "--gc-window", "33"]) == 0
    assert {k: v for k, v in seen.items() if k.startswith("gc_")} == dict(gc_bias=str(genome), gc_window=33)


def test_pipeline_writes_the_table_and_nothing_else_changes(case, tmp_path):
    genome, bam = case["fasta"], case["bam"]
    kw = dict(read_len=36, mapq_criteria=GC.MAPQ, device_ingest=False, stats=True, complexity=True)
    _r0, w0 = pipeline.run(bam, str(tmp_path / "plain"), 120, context=FakeContext(), **kw)
    _r1, w1 = pipeline.run(bam, str(tmp_path / "with"), 120, context=FakeContext(), gc_bias=genome, gc_window=64, **kw)
    assert [p.name for p in w1] == [p.name for p in w0] + ["gc_gcbias.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, block = gcbias.read_gcbias(w1[-1])
    N, F, off_end, blocked = GC.restate(case["reads"], GC.USES["all"], 64, False)
    assert name == "gc" and (c.N.tolist(), c.F.tolist(), c.off_end, c.blocked) == (N, F, off_end, blocked)
    assert block["Genome"] == genome and c.window == 64 and c.per_reference == {n: max(0, l - 63) for n, l in GC.REFS}
    # the chosen chromosomes with the excluded regions; a genome of another assembly; an option without its genome; a FASTA that
    # cannot be parsed
    _r2, w2 = pipeline.run(bam, str(tmp_path / "two"), 120, context=FakeContext(), references=_chosen("no middle"), gc_bias=genome,
                           exclude_regions=GC.MASK, **kw)
    c2 = gcbias.read_gcbias(w2[-1])[1]
    N, F, off_end, blocked = GC.restate(case["less"], GC.USES["no middle"], 100, True)
    assert list(c2.per_reference) == _chosen("no middle") and (c2.N.tolist(), c2.F.tolist(), c2.off_end, c2.blocked) == (N, F, off_end, blocked)
    other = tmp_path / "other.fa"
    other.write_text(">g0\nACGT\n")
    with pytest.raises(ValueError, match="reference 'g0' is 100003 long in the alignment header and 4 in the genome"):
        pipeline.run(bam, str(tmp_path / "bad"), 120, context=FakeContext(), gc_bias=str(other), **kw)
    with pytest.raises(ValueError, match="gc_window needs gc_bias"):
        pipeline.run(bam, str(tmp_path / "bad"), 120, context=FakeContext(), gc_window=64, **kw)
    broken = tmp_path / "broken.fa"
    broken.write_text("ACGT\n")
    with pytest.raises(pipeline.GenomeError, match="line 1: sequence before the first header"):
        pipeline.run(bam, str(tmp_path / "bad"), 120, context=FakeContext(), gc_bias=str(broken), **kw)
    assert not os.path.exists(tmp_path / "bad") or not os.listdir(tmp_path / "bad")
    # run_files: the file whose references the genome does not have is skipped, the call goes on
    short = tmp_path / "short.fa"
    g = GC.genome()
    short.write_text("".join(">{}\n{}\n".format(n, g[n]) for n in ("g0", "g2")))
    small = SW.write_twins(tmp_path, "small", [GC.REFS[0], GC.REFS[2]], [r for r in GC.alignment_records(GC.synthetic()[::40])
                                                                          if r["rname"] != "g1"])[1]
    res = pipeline.run_files([bam, small], str(tmp_path / "files"), 120, context=FakeContext(), gc_bias=str(short), **kw)
    assert res[0].error is not None and "reference 'g1' has no record in the genome" in str(res[0].error) and res[0].written == []
    assert res[1].error is None and res[1].written[-1].name == "small_gcbias.tab"
    assert gcbias.read_gcbias(res[1].written[-1])[1].reads > 1000
