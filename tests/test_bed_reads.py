"""BED read files (tagAlign) through the host reader (pymasc_amd.bed_reads.BedReadsReader, libpymasc_io.so pmx_bed_open): the
golden reads written as tagAlign give what the golden BAM gives, plain / gzip / BGZF and shuffled; the line rules with their
line numbers; run_files with chrom_sizes; the command line's --chrom-sizes."""
import csv
import logging
import os
import shutil

import numpy as np
import pytest

from pymasc_amd import bed_reads, cli, inputs, pipeline
from pymasc_amd import bam as B
from . import bed_reads_cases as BC
from . import fixtures as fx
from .fake_context import FakeContext


def arrays(reader, mapq):
    parts = list(reader.batches(mapq))
    if not parts:
        return [np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, bool)]
    return [np.concatenate(x) for x in zip(*parts)]


def assert_same(a, b, mapqs=(0, 10), keys=True):
    assert a.references == b.references and a.lengths == b.lengths
    for q in mapqs:
        for x, y in zip(arrays(a, q), arrays(b, q)):
            np.testing.assert_array_equal(x, y)
        ha, hb = a.read_length_histogram(q), b.read_length_histogram(q)
        np.testing.assert_array_equal(ha.lengths, hb.lengths)
        np.testing.assert_array_equal(ha.counts, hb.counts)
        assert ha.counters == hb.counters
        if keys:
            np.testing.assert_array_equal(ha.first, hb.first)


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    d = tmp_path_factory.mktemp("bed")
    sizes = BC.golden_sizes()
    names = [n for n, _ in sizes]
    lines = BC.golden_lines()
    sh = BC.shuffled(lines)
    return dict(dir=d, sizes=sizes, names=names, lens=[v for _, v in sizes], sizes_path=BC.write_sizes(d / "g.chrom.sizes", sizes),
                copies=BC.write_copies(d, BC.STEM, "".join(lines).encode()),
                shuffled=BC.write_copies(d, "shuf", "".join(sh).encode()),
                resorted=BC.write_copies(d, "resorted", "".join(BC.stable_sorted(sh, names)).encode()))


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
@pytest.mark.parametrize("mapq", [0, 10])
def test_golden_twin_equals_golden_bam(golden, kind, mapq):
    with bed_reads.BedReadsReader(golden["copies"][kind], golden["names"], golden["lens"]) as r, \
            B.BamReader(BC.GOLD + ".bam", index=False) as b:
        assert_same(r, b, (mapq,), keys=False)
        assert list(r.read_length_histogram(mapq).as_counter()) == list(b.read_length_histogram(mapq).as_counter())
        c = r.counters()
        assert c["records"] == 2501 and c["members"] == 0 and r.header_text == ""
        assert c["bytes_in"] == os.path.getsize(golden["copies"][kind])


@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_shuffled_equals_stably_sorted(golden, kind):
    """Arrays, histogram and counters of the shuffled file are those of its lines stably sorted; the first-occurrence keys are
    offsets of lines in each file, so only the resorted file's ORDER of lengths is the same, not the keys."""
    with bed_reads.BedReadsReader(golden["shuffled"][kind], golden["names"], golden["lens"], threads=3) as r, \
            bed_reads.BedReadsReader(golden["resorted"][kind], golden["names"], golden["lens"]) as s:
        assert_same(r, s, keys=False)


def test_ties_keep_file_order(tmp_path):
    lines = BC.tie_lines()
    names = [n for n, _ in BC.TIE_SIZES]
    lens = [v for _, v in BC.TIE_SIZES]
    (tmp_path / "t.bed").write_text("".join(lines))
    (tmp_path / "s.bed").write_text("".join(BC.stable_sorted(lines, names)))
    with bed_reads.BedReadsReader(tmp_path / "t.bed", names, lens) as r, bed_reads.BedReadsReader(tmp_path / "s.bed", names, lens) as s:
        assert_same(r, s, (0, 20), keys=False)
        ref, pos, rlen, rev = arrays(r, 0)
        assert ref.tolist() == [0, 0, 0, 0, 0, 0, 1, 1, 1]
        assert pos.tolist() == [51, 101, 101, 101, 101, 101, 501, 501, 501]
        assert rlen.tolist() == [36, 36, 30, 40, 36, 1, 36, 20, 36]
        assert rev.tolist() == [True, False, False, True, True, False, True, False, False]
        # MAPQ: '.' and 1000 give 255, so a -q 255 filter keeps exactly them and the 255
        assert arrays(r, 255)[2].tolist() == [40, 1, 20]
        h = r.read_length_histogram(0)
        # the first-occurrence key of a length is the offset of the first line of that length in the file, whatever the sort did
        text = "".join(lines)
        first = {}
        off = 0
        for line in lines:
            f = line.split()
            first.setdefault(int(f[2]) - int(f[1]), off)
            off += len(line)
        assert dict(zip(h.lengths.tolist(), h.first.tolist())) == first
        assert len(text) == off


def test_accepted_lines(tmp_path):
    p = tmp_path / "a.tagAlign"
    p.write_bytes(BC.ACCEPTED_TEXT.encode())
    with bed_reads.BedReadsReader(p, [n for n, _ in BC.TIE_SIZES], [v for _, v in BC.TIE_SIZES]) as r:
        ref, pos, rlen, rev = arrays(r, 0)
        assert ref.tolist() == [0, 0, 1] and pos.tolist() == [6, 11, 1] and rlen.tolist() == [36, 36, 36]
        assert rev.tolist() == [True, False, False]
        assert r.counters()["records"] == 3


@pytest.mark.parametrize("name,text,line,word", BC.ERROR_CASES, ids=[c[0] for c in BC.ERROR_CASES])
def test_line_errors(tmp_path, name, text, line, word):
    p = tmp_path / (name + ".bed")
    p.write_text(text)
    with pytest.raises(B.PmxIOError) as e:
        bed_reads.BedReadsReader(p, [n for n, _ in BC.TIE_SIZES], [v for _, v in BC.TIE_SIZES])
    msg = str(e.value)
    assert "line {}: ".format(line) in msg and word in msg, msg


def test_sizes_are_checked(tmp_path):
    p = tmp_path / "x.bed"
    p.write_text("chr1\t1\t5\tn\t0\t+\n")
    with pytest.raises(B.PmxIOError, match="named twice"):
        bed_reads.BedReadsReader(p, ["chr1", "chr1"], [10, 10])
    with pytest.raises(B.PmxIOError, match="length"):
        bed_reads.BedReadsReader(p, ["chr1"], [0])
    with pytest.raises(ValueError, match="chromosome sizes"):
        inputs.open_alignments(p, False)
    with pytest.raises(ValueError, match="chromosome sizes"):
        bed_reads.chrom_sizes_of(tmp_path / "missing.sizes")
    # the sizes' order is the reference order
    with inputs.open_alignments(p, False, chrom_sizes={"chrZ": 5, "chr1": 10}) as r:
        assert r.references == ("chrZ", "chr1") and arrays(r, 0)[0].tolist() == [1]


def test_name_rule_and_header():
    for n in ("x.tagAlign", "x.TAGALIGN.gz", "x.bed", "X.Bed.bgz", "/a/b.tagalign.GZ"):
        assert bed_reads.is_bed_reads(n), n
    for n in ("notes.txt", "plain.sam.gz", "-", "x.bam", "x.bed.txt", "x.bedgraph", BC.GOLD + ".bam"):
        assert not bed_reads.is_bed_reads(n), n


def test_open_header_reads_nothing(tmp_path):
    p = tmp_path / "x.tagAlign.gz"
    p.write_bytes(b"not gzip at all")           # (the header step does not read it)
    with inputs.open_header(p, {"chr1": 10, "chr2": 20}) as h:
        assert h.references == ("chr1", "chr2") and h.lengths == (10, 20)
    with pytest.raises(OSError):
        inputs.open_header(tmp_path / "missing.bed", {"chr1": 10})


def _rows(path):
    with open(path, newline="") as fp:
        return list(csv.reader(fp, dialect="excel-tab"))


def check_golden_tables(paths, stem):
    """_cc / _mscc equal the golden tables; _nreads equals the golden chr1 column (as tests/test_pipeline.py checks them)."""
    for p in paths:
        gold = os.path.join(fx.GOLDEN, p.name.replace(stem, BC.STEM))
        got, exp = _rows(p), _rows(gold)
        if p.name.endswith("_nreads.tab"):
            col = exp[0].index("chr1")
            assert got[0] == ["shift", "whole", "chr1"]
            assert [r[:3] for r in got[1:]] == [[r[0], r[1], r[col]] for r in exp[1:]]
        else:
            assert got[0] == exp[0] and len(got) == len(exp)
            np.testing.assert_almost_equal(np.array([r[1:] for r in got[1:]], dtype=float),
                                           np.array([r[1:] for r in exp[1:]], dtype=float), decimal=15)


def _run_files(tmp_path, tag, path, **kw):
    d = tmp_path / tag
    d.mkdir()
    bw = d / "hg19_36mer-test.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    return pipeline.run_files([path], d / "out", 300, read_len=36, mapq_criteria=10, mappability_path=str(bw),
                              device_ingest=False, context=FakeContext(), **kw)[0]


@pytest.mark.parametrize("which", ["copies", "shuffled"])
def test_run_files_writes_golden_tables(golden, tmp_path, which):
    """The twin, plain and shuffled, writes the golden tables, and byte for byte what the golden BAM writes in the same call."""
    path = golden[which]["plain"]
    res = _run_files(tmp_path, "bed", path, chrom_sizes=golden["sizes_path"])
    assert res.error is None
    stem = os.path.basename(path)[:-len(".tagAlign")]
    assert sorted(p.name for p in res.written) == sorted(stem + s for s in ("_cc.tab", "_mscc.tab", "_nreads.tab"))
    check_golden_tables(res.written, stem)
    ref = _run_files(tmp_path, "bam", BC.GOLD + ".bam")
    assert [open(p, "rb").read() for p in sorted(res.written)] == [open(p, "rb").read() for p in sorted(ref.written)]


def test_run_files_skips_bed_without_sizes(golden, tmp_path, caplog):
    bam = tmp_path / "g.bam"
    shutil.copy(BC.GOLD + ".bam", bam)
    with caplog.at_level(logging.ERROR):
        res = pipeline.run_files([golden["copies"]["plain"], str(bam)], tmp_path / "out", 300, read_len=36, mapq_criteria=10,
                                 device_ingest=False, context=FakeContext())
    assert isinstance(res[0].error, ValueError) and "chromosome sizes" in str(res[0].error)
    assert res[1].error is None and res[1].written
    with pytest.raises(ValueError, match="chromosome sizes"):
        pipeline.run(golden["copies"]["plain"], tmp_path / "o2", 300, read_len=36, device_ingest=False, context=FakeContext())


def test_run_estimates_read_length_from_bed(golden, tmp_path):
    res, written = pipeline.run(golden["shuffled"]["gzip"], tmp_path / "out", 300, mapq_criteria=10, device_ingest=False,
                                context=FakeContext(), chrom_sizes=dict(golden["sizes"]))
    assert res.read_len == 36 and written


def test_cli_chrom_sizes(golden, tmp_path, monkeypatch):
    calls = []

    def fake_run_files(paths, outdir, max_shift, **kw):
        calls.append((paths, kw.get("chrom_sizes")))
        return [pipeline.FileResult(p, "x", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", fake_run_files)
    rc = cli.main([golden["copies"]["gzip"], "--chrom-sizes", golden["sizes_path"], "-d", "300", "-r", "36", "--skip-plots"])
    assert rc == 0 and calls == [([golden["copies"]["gzip"]], golden["sizes_path"])]
    assert cli.main([golden["copies"]["gzip"], "-d", "300"]) == 2
    assert cli.main([golden["copies"]["gzip"], "--chrom-sizes", str(tmp_path / "missing"), "-d", "300"]) == 2
    assert len(calls) == 1


def test_cli_help_lists_chrom_sizes(capsys):
    assert cli.main(["--help"]) == 0
    assert "--chrom-sizes" in capsys.readouterr().out
