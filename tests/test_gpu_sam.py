"""SAM input on the GPU (pymasc_amd.sam.DeviceSamReader, libpymasc_ingest.so pmx_dsam_open): the device reader equals the host
SAM reader (its checker) and the device BAM reader on the BAM twin -- arrays, runs, read-length histogram, counters -- on the
golden file, the synthetic corner cases and 2 M-record files; malformed text gives the host reader's error and line; the golden
run from SAM and BGZF SAM; run_sharded with a chromosome filter and on two gloo ranks on one GPU."""
import csv
import multiprocessing as mp
import os
import shutil

import numpy as np
import pytest

from pymasc_amd import bam as B
from pymasc_amd import bam_device as D
from pymasc_amd import sam
from . import fixtures as fx
from . import io_writers as W
from . import sam_cases as SC
from . import sam_writers as SW
from . import test_gpu_ingest_indexed as IX

pytestmark = pytest.mark.gpu

GOLD = os.path.join(fx.GOLDEN, "ENCFF000RMB-test")


@pytest.fixture(scope="module")
def gold_sam(tmp_path_factory):
    """The golden SAM as plain text."""
    p = tmp_path_factory.mktemp("golden") / "ENCFF000RMB-test.sam"
    p.write_bytes(SC.golden_sam_text())
    return str(p)


def _arrays(reader, mapq):
    parts = list(reader.batches(mapq))
    if not parts:
        return [np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, np.int32), np.empty(0, bool)]
    return [np.concatenate(x) for x in zip(*parts)]


def _hist(reader, mapq):
    h = reader.read_length_histogram(mapq)
    return h.lengths.tolist(), h.counts.tolist(), h.first.tolist(), h.counters


def _check_device(dev, host, bam_dev=None, mapqs=(0, 10)):
    """dev (DeviceSamReader) == host (SamReader) in everything, == bam_dev (DeviceBamReader of the twin) but for the keys."""
    assert dev.references == host.references and dev.lengths == host.lengths
    for q in mapqs:
        got = _arrays(dev, q)
        for x, y in zip(got, _arrays(host, q)):
            np.testing.assert_array_equal(x, y)
        dc, hc = dev.counters(), host.counters()
        assert (dc["records"], dc["kept"], dc["bytes_out"], dc["members"], dc["rewalked"]) == \
            (hc["records"], hc["kept"], hc["bytes_out"], hc["members"], 0)
        runs = dev.device_runs()
        hd = _hist(dev, q)
        assert hd == _hist(host, q)
        if bam_dev is not None:
            for x, y in zip(got, _arrays(bam_dev, q)):
                np.testing.assert_array_equal(x, y)
            assert runs == bam_dev.device_runs()
            assert dc["records"] == bam_dev.counters()["records"]
            hb = _hist(bam_dev, q)
            assert hd[0] == hb[0] and hd[1] == hb[1] and hd[3] == hb[3]
            assert np.argsort(hd[2], kind="stable").tolist() == np.argsort(hb[2], kind="stable").tolist()


@pytest.mark.parametrize("mapq", [0, 1, 10, 20, 30])
def test_golden_device_sam(mapq, gold_sam):
    with D.DeviceBamReader(GOLD + ".bam") as b:
        for p in (gold_sam, SC.GOLDEN_SAM_GZ):
            with sam.DeviceSamReader(p) as d, sam.SamReader(p) as h:
                _check_device(d, h, b, (mapq,))
                t = d.timings()
                assert t["upload_s"] > 0 and t["chain_s"] > 0


@pytest.mark.parametrize("name", sorted(SC.twin_cases()))
def test_synthetic_twins_device(tmp_path, name):
    refs, recs, kw = SC.twin_cases()[name]
    paths = SW.write_twins(tmp_path, name, refs, recs, **kw)
    with D.DeviceBamReader(paths[1]) as b:
        for p in [paths[0]] + list(paths[2:]):
            with sam.DeviceSamReader(p) as d, sam.SamReader(p) as h:
                _check_device(d, h, b)


def _big_text(n, seed, crlf=False):
    rng = np.random.default_rng(seed)
    refs = [("chr%d" % i, 50_000_000) for i in range(1, 9)]
    per = n // len(refs)
    eol = "\r\n" if crlf else "\n"
    lines = [SW.sam_header(refs, eol)]
    k = 0
    for name, ln in refs:
        pos = np.sort(rng.integers(1, ln - 200, size=per))
        fl = rng.choice([0, 16, 1040, 0x81, 4], size=per, p=[0.45, 0.45, 0.04, 0.04, 0.02])
        mq = rng.integers(0, 61, size=per)
        ql = np.where(rng.random(per) < 0.2, rng.integers(20, 2000, size=per), 36)
        for p, f, q, l in zip(pos.tolist(), fl.tolist(), mq.tolist(), ql.tolist()):
            lines.append("q%d\t%d\t%s\t%d\t%d\t%dM\t*\t0\t0\t*\t*%s" % (k, f, name, p, q, l, eol))
            k += 1
    return "".join(lines).encode()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("kind", ["sam", "sam.bgzf"])
def test_two_million_records(tmp_path, kind):
    text = _big_text(2_000_000, 5, crlf=(kind == "sam.bgzf"))
    p = tmp_path / ("big." + kind.replace(".bgzf", ".gz"))
    p.write_bytes(W.bgzf_compress(text, level=1) if kind == "sam.bgzf" else text)
    with sam.DeviceSamReader(p) as d, sam.SamReader(p) as h:
        _check_device(d, h, None, (0, 20))
        assert d.counters()["records"] == 2_000_000


@pytest.mark.parametrize("name", sorted(SC.malformed_cases()))
def test_malformed_same_error_as_host(tmp_path, name):
    text, line, word = SC.malformed_cases()[name]
    p = tmp_path / (name + ".sam")
    p.write_bytes(text.encode())
    with pytest.raises(B.PmxIOError) as eh:
        sam.SamReader(p)
    with pytest.raises(B.PmxIOError) as ed:
        sam.DeviceSamReader(p)
    msg = str(eh.value).split("] ", 1)[1]
    assert str(ed.value).split("] ", 1)[1] == msg
    if line is not None:
        assert "line {}:".format(line) in msg


def test_decode_after_histogram_and_select(tmp_path):
    refs, recs, _kw = SC.twin_cases()["synthetic"]
    sam_p, bam_p = SW.write_twins(tmp_path, "s", refs, recs)
    with sam.DeviceSamReader(sam_p) as d, sam.SamReader(sam_p) as h:
        n = d.decode(10)
        before = d._fetch(0, n)
        d.read_length_histogram(0)
        for x, y in zip(before, d._fetch(0, n)):
            np.testing.assert_array_equal(x, y)
        assert d.decode(10) == n
        d.select(["c2"])
        got = _arrays(d, 10)
        want = [x[_arrays(h, 10)[0] == 1] for x in _arrays(h, 10)]
        for x, y in zip(got, want):
            np.testing.assert_array_equal(x, y)
        L = D.load_ingest_library()
        ids = (__import__("ctypes").c_int32 * 1)(0)
        assert L.pmx_dbam_select(d._h, ids, 1) == -3            # no index behind a SAM handle
    with sam.DeviceSamReader(sam_p, references=["c1", "c3"]) as d:
        assert set(np.unique(_arrays(d, 0)[0]).tolist()) == {0, 2}


def _rows(path):
    with open(path, newline="") as fp:
        return list(csv.reader(fp, dialect="excel-tab"))


@pytest.mark.parametrize("kind", ["sam", "sam.gz"])
def test_pipeline_golden_from_sam(tmp_path, kind):
    from pymasc_amd import pipeline
    src = tmp_path / ("ENCFF000RMB-test." + kind)
    data = SC.golden_sam_text()
    src.write_bytes(W.bgzf_compress(data, 7000) if kind == "sam.gz" else data)
    bw = tmp_path / "hg19_36mer-test.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    result, written = pipeline.run(src, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10, mappability_path=bw)
    stem = src.stem
    assert [p.name for p in written] == [stem + "_cc.tab", stem + "_mscc.tab", stem + "_nreads.tab"]
    for p in written[:2]:                          # as tests/test_pipeline.py checks the BAM run
        got, want = _rows(p), _rows(os.path.join(fx.GOLDEN, p.name.replace(stem, "ENCFF000RMB-test")))
        assert got[0] == want[0] and len(got) == len(want)
        np.testing.assert_almost_equal(np.array([r[1:] for r in got[1:]], dtype=float),
                                       np.array([r[1:] for r in want[1:]], dtype=float), decimal=15)
    got, exp = _rows(written[2]), _rows(os.path.join(fx.GOLDEN, "ENCFF000RMB-test_nreads.tab"))
    col = exp[0].index("chr1")
    assert got[0] == ["shift", "whole", "chr1"]
    assert [r[:3] for r in got[1:]] == [[r[0], r[1], r[col]] for r in exp[1:]]
    assert (result.forward_sum, result.reverse_sum) == (622, 670)
    # and byte for byte what the BAM twin gives
    bam = tmp_path / "ENCFF000RMB-test.bam"
    shutil.copy(GOLD + ".bam", bam)
    _r, wb = pipeline.run(bam, tmp_path / "out_bam", max_shift=300, read_len=36, mapq_criteria=10, mappability_path=bw)
    assert [open(p, "rb").read() for p in written] == [open(p, "rb").read() for p in wb]
    # without read_len: estimated on the device SAM reader, the same tables
    r2, w2 = pipeline.run(src, tmp_path / "out2", max_shift=300, mapq_criteria=10, mappability_path=bw)
    assert r2.read_len == 36 and [open(p, "rb").read() for p in w2] == [open(p, "rb").read() for p in written]


def _twin_files(tmp_path):
    rng = np.random.default_rng(21)
    refs = [("c%d" % i, 20000 + 3000 * i) for i in range(1, 7)]
    recs = SW.synth_records(rng, refs, 250)
    return SW.write_twins(tmp_path, "t", refs, recs, bgzf_block=4000)


def test_run_sharded_chromfilter_sam_equals_bam(tmp_path):
    from pymasc_amd import sharding
    sam_p, bam_p, gz_p = _twin_files(tmp_path)
    flt = [(False, ["c2", "c5"])]
    want = IX._table_bytes(sharding.run_sharded(bam_p, 120, 36, 10, device=0, chromfilter=flt), tmp_path, "bam")
    for k, p in enumerate((sam_p, gz_p)):
        got = IX._table_bytes(sharding.run_sharded(p, 120, 36, 10, device=0, chromfilter=flt), tmp_path, "sam%d" % k)
        assert got == want, p


@pytest.mark.timeout(900)
def test_two_ranks_on_one_gpu_sam(tmp_path):
    """Two gloo ranks on one GPU (the worker of tests/test_gpu_ingest_indexed.py): each reads the whole SAM file and feeds its
    share; both hold the tables of the BAM twin's one-rank run."""
    from pymasc_amd import sharding
    sam_p, bam_p, _gz = _twin_files(tmp_path)
    expect = IX._table_bytes(sharding.run_sharded(bam_p, 120, 36, 10, device=0), tmp_path, "single")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = IX._free_port()
    procs = [ctx.Process(target=IX._rank_worker, args=(r, 2, port, q, sam_p, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = [q.get(timeout=600) for _ in range(2)]
    finally:
        for p in procs:
            p.join(120)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs)
    for rank, tabs, seen, err in got:
        assert err is None, (rank, err)
        assert tabs == expect and seen == [], rank          # (no index behind a SAM file: nothing selected)
