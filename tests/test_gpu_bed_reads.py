"""BED read files on the device (pymasc_amd.bed_reads.DeviceBedReadsReader, libpymasc_ingest.so pmx_dbed_open): the device
reader equals the host reader (its checker) on the golden twin, plain / gzip / BGZF and shuffled, on a 2 M-line synthetic file
over 400 chromosomes with starts near 2^31, and on every malformed line; pipeline.run and ``python -m pymasc_amd`` from the
shuffled twin write what the golden BAM run writes; ``-p 2`` over gloo equals ``-p 1``."""
import os
import shutil

import numpy as np
import pytest

from pymasc_amd import bed_reads, pipeline
from pymasc_amd import bam as B
from . import bed_reads_cases as BC
from . import fixtures as fx
from .test_bed_reads import arrays, check_golden_tables
from .test_gpu_cli import _command, _tree

pytestmark = pytest.mark.gpu

GOLD_BW = os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig")


def _runs(ref, pos):
    """(ref_id, start, count, first pos, last pos) of the runs of one reference in host arrays (DeviceBamReader.device_runs)."""
    out = []
    i = 0
    while i < len(ref):
        j = i
        while j < len(ref) and ref[j] == ref[i]:
            j += 1
        out.append((int(ref[i]), i, j - i, int(pos[i]), int(pos[j - 1])))
        i = j
    return out


def check_device(path, names, lens, mapqs=(0, 10)):
    with bed_reads.DeviceBedReadsReader(path, names, lens) as d, bed_reads.BedReadsReader(path, names, lens) as h:
        assert d.references == h.references and d.lengths == h.lengths and d.header_text == ""
        for q in mapqs:
            got, want = arrays(d, q), arrays(h, q)
            for x, y in zip(got, want):
                np.testing.assert_array_equal(x, y)
            assert d.device_runs() == _runs(want[0], want[1])
            dc, hc = d.counters(), h.counters()
            assert dc == hc, (dc, hc)
            hd, hh = d.read_length_histogram(q), h.read_length_histogram(q)
            np.testing.assert_array_equal(hd.lengths, hh.lengths)
            np.testing.assert_array_equal(hd.counts, hh.counts)
            np.testing.assert_array_equal(hd.first, hh.first)
            assert hd.counters == hh.counters
        return hc


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    d = tmp_path_factory.mktemp("dbed")
    sizes = BC.golden_sizes()
    lines = BC.golden_lines()
    return dict(dir=d, sizes=sizes, names=[n for n, _ in sizes], lens=[v for _, v in sizes],
                sizes_path=BC.write_sizes(d / "g.chrom.sizes", sizes),
                copies=BC.write_copies(d, BC.STEM, "".join(lines).encode()),
                shuffled=BC.write_copies(d, "shuf", "".join(BC.shuffled(lines)).encode()))


@pytest.mark.parametrize("which", ["copies", "shuffled"])
@pytest.mark.parametrize("kind", ["plain", "gzip", "bgzf"])
def test_golden_device_equals_host(golden, which, kind):
    c = check_device(golden[which][kind], golden["names"], golden["lens"])
    assert c["records"] == 2501


def test_ties_and_accepted_lines(tmp_path):
    names, lens = [n for n, _ in BC.TIE_SIZES], [v for _, v in BC.TIE_SIZES]
    (tmp_path / "t.bed").write_text("".join(BC.tie_lines()))
    check_device(tmp_path / "t.bed", names, lens, (0, 20, 255))
    (tmp_path / "a.tagAlign").write_bytes(BC.ACCEPTED_TEXT.encode())
    check_device(tmp_path / "a.tagAlign", names, lens)
    (tmp_path / "c.tagAlign").write_bytes(b"# only a comment\n\n")
    assert check_device(tmp_path / "c.tagAlign", names, lens)["records"] == 0
    (tmp_path / "e.tagAlign").write_bytes(b"")
    with pytest.raises(B.PmxIOError) as eh:
        bed_reads.BedReadsReader(tmp_path / "e.tagAlign", names, lens)
    with pytest.raises(B.PmxIOError) as ed:
        bed_reads.DeviceBedReadsReader(tmp_path / "e.tagAlign", names, lens)
    assert str(ed.value) == str(eh.value) and "empty file" in str(ed.value)


@pytest.mark.parametrize("name,text,line,word", BC.ERROR_CASES, ids=[c[0] for c in BC.ERROR_CASES])
def test_device_errors_equal_host(tmp_path, name, text, line, word):
    p = tmp_path / (name + ".bed")
    p.write_text(text)
    names, lens = [n for n, _ in BC.TIE_SIZES], [v for _, v in BC.TIE_SIZES]
    with pytest.raises(B.PmxIOError) as eh:
        bed_reads.BedReadsReader(p, names, lens)
    with pytest.raises(B.PmxIOError) as ed:
        bed_reads.DeviceBedReadsReader(p, names, lens)
    assert str(ed.value) == str(eh.value) and "line {}: ".format(line) in str(ed.value)


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["plain", "bgzf"])
def test_synthetic_two_million_lines(tmp_path, kind):
    """2 M reads over 400 chromosomes (the reference index spans two 8-bit digits of the key), starts near 2^31, shuffled,
    with exact ties: the device sort gives the host's stable_sort."""
    sizes, lines = BC.synthetic_lines(np.random.default_rng(7), 2_000_000, 400)
    paths = BC.write_copies(tmp_path, "syn", "".join(BC.shuffled(lines, 3)).encode(), bgzf_block=0xff00)
    c = check_device(paths[kind], [n for n, _ in sizes], [v for _, v in sizes], (0, 30))
    assert c["records"] == 2_000_000


def _track(d):
    bw = d / "hg19_36mer-test.bigwig"
    shutil.copy(GOLD_BW, bw)
    return bw


@pytest.mark.parametrize("read_len", [36, None])
def test_pipeline_run_from_shuffled_gzip(golden, tmp_path, read_len):
    bed = tmp_path / (BC.STEM + ".tagAlign.gz")
    shutil.copy(golden["shuffled"]["gzip"], bed)
    bw = _track(tmp_path)
    res, written = pipeline.run(bed, tmp_path / "out", 300, read_len=read_len, mapq_criteria=10, mappability_path=bw,
                                chrom_sizes=golden["sizes_path"])
    assert res.read_len == 36
    stem = BC.STEM + ".tagAlign"
    assert sorted(p.name for p in written) == sorted(stem + s for s in ("_cc.tab", "_mscc.tab", "_nreads.tab"))
    check_golden_tables(written, stem)
    bam = tmp_path / (BC.STEM + ".bam")
    shutil.copy(BC.GOLD + ".bam", bam)
    _r, ref = pipeline.run(bam, tmp_path / "bam", 300, read_len=read_len, mapq_criteria=10, mappability_path=bw)
    assert [open(p, "rb").read() for p in sorted(written)] == [open(p, "rb").read() for p in sorted(ref)]


@pytest.mark.timeout(1200)
def test_command_line_equals_golden_bam_run_and_two_ranks(golden, tmp_path):
    bed = tmp_path / "x.tagAlign.gz"
    shutil.copy(golden["shuffled"]["gzip"], bed)
    shutil.copy(golden["sizes_path"], tmp_path / "g.chrom.sizes")
    bam = tmp_path / "x.bam"
    shutil.copy(BC.GOLD + ".bam", bam)
    bw = _track(tmp_path)
    common = ["-m", bw.name, "-d", "300", "-q", "10", "--skip-plots"]
    rc, err = _command("pymasc_amd", [bam.name] + common + ["-o", "bam"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", [bed.name, "--chrom-sizes", "g.chrom.sizes"] + common + ["-o", "bed", "-n", "x"], tmp_path)
    assert rc == 0, err
    want = _tree(tmp_path / "bam")
    assert sorted(want) == ["x_cc.tab", "x_mscc.tab", "x_nreads.tab", "x_stats.tab"]
    assert _tree(tmp_path / "bed") == want
    rc, err = _command("pymasc_amd", [bed.name, "--chrom-sizes", "g.chrom.sizes"] + common + ["-r", "36", "-o", "one", "-n", "x"],
                       tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", [bed.name, "--chrom-sizes", "g.chrom.sizes"] + common + ["-r", "36", "-o", "two", "-n", "x",
                                                                                              "-p", "2"],
                       tmp_path, PMX_DIST_BACKEND="gloo")
    assert rc == 0, err
    assert _tree(tmp_path / "two") == _tree(tmp_path / "one") == want
