"""SAM input through the host reader (pymasc_amd.sam.SamReader, libpymasc_io.so pmx_sam_*): for a SAM file, plain or BGZF, the
same records, references, read-length histogram, counters and estimates as the BAM reader gives for the BAM twin; the parsing
rules' errors with their line numbers; format detection; and the golden run and pipeline.run from the SAM file."""
import csv
import gzip
import os

import numpy as np
import pytest

from pymasc_amd import pipeline, readlen, sam
from pymasc_amd import bam as B
from pymasc_amd import tables as T
from pymasc_amd.bigwig import BigWigReader
from pymasc_amd.calculator import CCHipCalculator
from . import fixtures as fx
from . import io_writers as W
from . import sam_cases as SC
from . import sam_writers as SW
from .fake_context import FakeContext

GOLD = os.path.join(fx.GOLDEN, "ENCFF000RMB-test")


@pytest.fixture(scope="module")
def gold_sam(tmp_path_factory):
    """The golden SAM as plain text."""
    p = tmp_path_factory.mktemp("golden") / "ENCFF000RMB-test.sam"
    p.write_bytes(SC.golden_sam_text())
    return str(p)


def arrays(reader, mapq):
    parts = list(reader.batches(mapq))
    if not parts:
        return [np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, bool)]
    return [np.concatenate(x) for x in zip(*parts)]


def assert_same_reads(a, b, mapqs=(0, 1, 10, 20, 30)):
    assert a.references == b.references and a.lengths == b.lengths
    for q in mapqs:
        for x, y in zip(arrays(a, q), arrays(b, q)):
            np.testing.assert_array_equal(x, y)


def assert_same_histogram(a, b, mapq):
    ha, hb = a.read_length_histogram(mapq), b.read_length_histogram(mapq)
    np.testing.assert_array_equal(ha.lengths, hb.lengths)
    np.testing.assert_array_equal(ha.counts, hb.counts)
    assert ha.counters == hb.counters
    assert list(ha.as_counter()) == list(hb.as_counter())           # first-occurrence ORDER (the keys are offsets of each format)
    if ha.counts.size:
        for e in readlen.ESTIMATORS:
            assert ha.estimate(e) == hb.estimate(e), e
    return ha


@pytest.mark.parametrize("mapq", [0, 1, 10, 20, 30])
def test_golden_sam_equals_golden_bam(mapq, gold_sam):
    with sam.SamReader(gold_sam) as s, B.BamReader(GOLD + ".bam", index=False) as b:
        assert_same_reads(s, b, (mapq,))
        h = assert_same_histogram(s, b, mapq)
        assert h.counters["nreads"] == 2501
        c = s.counters()
        assert c["records"] == 2501 and c["bytes_out"] == c["bytes_in"] == os.path.getsize(gold_sam) and c["members"] == 0


def test_golden_sam_mode_tie_and_header(gold_sam):
    with sam.SamReader(gold_sam, threads=3) as s:
        h = s.read_length_histogram(10)
        assert (h.estimate("MIN"), h.estimate("MAX"), h.estimate("MEDIAN"), h.estimate("MODE")) == (20, 36, 36, 36)
        assert s.header_text.startswith("@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:chr1\tLN:249250621\n")
        assert not s.has_index()
        with pytest.raises(ValueError):
            s.fetch("chr1")
    assert readlen.estimate_readlen(gold_sam, "MODE", 10) == 36


@pytest.mark.parametrize("name", sorted(SC.twin_cases()))
def test_synthetic_twins(tmp_path, name):
    refs, recs, kw = SC.twin_cases()[name]
    paths = SW.write_twins(tmp_path, name, refs, recs, **kw)
    with B.BamReader(paths[1], index=False) as b:
        for p in [paths[0]] + list(paths[2:]):
            with sam.SamReader(p, threads=4) as s:
                assert_same_reads(s, b, (0, 10))
                for q in (0, 10):
                    assert_same_histogram(s, b, q)
                assert s.counters()["records"] == len(recs)
    if len(paths) == 3:
        assert sam.detect_format(paths[2]) == "sam.bgzf"
        with sam.SamReader(paths[2]) as s:
            c = s.counters()
            assert c["members"] > 2 and c["bytes_out"] == os.path.getsize(paths[0])


@pytest.mark.parametrize("name", sorted(SC.malformed_cases()))
def test_malformed_lines_name_their_line(tmp_path, name):
    text, line, word = SC.malformed_cases()[name]
    p = tmp_path / (name + ".sam")
    p.write_bytes(text.encode())
    with pytest.raises(B.PmxIOError) as ei:
        sam.SamReader(p, threads=4)
    msg = str(ei.value)
    assert word in msg, msg
    if line is not None:
        assert "line {}:".format(line) in msg, msg


def test_detect_format(tmp_path, gold_sam):
    assert sam.detect_format(gold_sam) == "sam"
    assert sam.detect_format(GOLD + ".bam") == "bam"
    assert sam.detect_format(SC.GOLDEN_SAM_GZ) == "sam.bgzf"
    # a text file that is not SAM, and BGZF that is not SAM text: still BAM, with today's errors
    txt = tmp_path / "notes.txt"
    txt.write_bytes(b"hello\tworld\n")
    assert sam.detect_format(txt) == "bam"
    with pytest.raises(B.PmxIOError, match="not BGZF|BGZF"):
        B.BamReader(txt)
    bad = tmp_path / "bad.bam"
    bad.write_bytes(W.bgzf_compress(b"SAM\1" + b"\0" * 64))
    assert sam.detect_format(bad) == "bam"
    assert sam.detect_format(tmp_path / "missing.bam") == "bam"
    # plain gzip: refused with a pointer to bgzip
    pg = tmp_path / "plain.sam.gz"
    pg.write_bytes(gzip.compress(open(gold_sam, "rb").read()))
    with pytest.raises(B.PmxIOError, match="bgzip"):
        sam.detect_format(pg)
    with pytest.raises(B.PmxIOError, match="bgzip"):
        sam.SamReader(pg)


def _check_tables(paths, stem):
    for p in paths:
        gold = os.path.join(fx.GOLDEN, p.name.replace(stem, "ENCFF000RMB-test"))
        if p.name.endswith("_nreads.tab"):
            assert open(p, "rb").read() == open(gold, "rb").read()
        else:
            g = list(csv.reader(open(gold, newline=""), dialect="excel-tab"))
            o = list(csv.reader(open(p, newline=""), dialect="excel-tab"))
            assert g[0] == o[0] and len(g) == len(o)
            np.testing.assert_almost_equal(np.array([r[1:] for r in o[1:]], dtype=float),
                                           np.array([r[1:] for r in g[1:]], dtype=float), decimal=15)


@pytest.mark.parametrize("kind", ["sam", "sam.bgzf"])
def test_golden_run_from_sam(kind, gold_sam, tmp_path):
    path = gold_sam if kind == "sam" else SC.GOLDEN_SAM_GZ
    with sam.SamReader(path) as s, BigWigReader(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig")) as bw:
        calc = CCHipCalculator(300, 36, s.references, s.lengths, bwfeeder=bw, context=FakeContext())
        assert B.feed_bam(calc, s, mapq_criteria=10) == 1292
        whole = calc.get_whole_result()
        names = s.references
    _check_tables(T.write_tables(tmp_path / "ENCFF000RMB-test.bam", whole, references=names), "ENCFF000RMB-test")


def test_pipeline_run_sam_equals_bam(tmp_path):
    rng = np.random.default_rng(3)
    recs = SW.synth_records(rng, SC.REFS, 400)
    sam_p, bam_p, gz_p = SW.write_twins(tmp_path, "twin", SC.REFS, recs, bgzf_block=3000)
    out = {}
    for p in (bam_p, sam_p, gz_p):
        res, written = pipeline.run(p, tmp_path / "out", 60, read_len=36, mapq_criteria=10, device_ingest=False,
                                    context=FakeContext())
        out[p] = [open(w, "rb").read() for w in written]
        names = sorted(w.name for w in written)
        assert names[0].startswith({bam_p: "twin_", sam_p: "twin_", gz_p: "twin.sam_"}[p]), names
    assert out[sam_p] == out[bam_p] and out[gz_p] == out[bam_p]
    # read_len None: the same estimate from the SAM and its BAM twin, and the same tables
    est = {}
    for p in (bam_p, sam_p):
        res, written = pipeline.run(p, tmp_path / ("est_" + os.path.basename(p)), 60, mapq_criteria=10, device_ingest=False,
                                    context=FakeContext(), chromfilter=[(False, ["c2"])])
        est[p] = (res.read_len, [open(w, "rb").read() for w in written])
    assert est[sam_p] == est[bam_p]
