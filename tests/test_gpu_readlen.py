"""Read-length histogram on the device (pmx_dbam_readlen_hist: one more walk over the record chain in HBM) against the host
reader's (pmx_bam_readlen_hist), and pipeline.run without read_len through the device reader."""
import csv
import os
import shutil

import numpy as np
import pytest

from pymasc_amd import bam as B
from pymasc_amd import bam_device as D
from pymasc_amd import readlen
from tests import io_writers as W
from tests import readlen_cases as RC

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLD = os.path.join(GOLDEN, "ENCFF000RMB-test.bam")
BIGWIG = os.path.join(GOLDEN, "hg19_36mer-test.bigwig")


def _same(path, mapqs=(0, 10), threads=8):
    for mapq in mapqs:
        with B.BamReader(path, threads=threads) as h:
            exp = h.read_length_histogram(mapq)
        with D.DeviceBamReader(path) as d:
            got = d.read_length_histogram(mapq)
        assert got.counters == exp.counters
        assert got.lengths.tolist() == exp.lengths.tolist()
        assert got.counts.tolist() == exp.counts.tolist()
        # first occurrences: the same file order (both keys are offsets in the inflated stream)
        assert np.argsort(got.first, kind="stable").tolist() == np.argsort(exp.first, kind="stable").tolist()
        assert got.first.tolist() == exp.first.tolist()
        for e in RC.ESTIMATORS:
            if exp.counts.size:
                assert got.estimate(e) == exp.estimate(e)
    return got


@pytest.mark.parametrize("name", sorted(RC.synthetic_cases()))
def test_synthetic_cases_device_equals_host(tmp_path, name):
    path = str(tmp_path / (name + ".bam"))
    descs = RC.write_case(path, RC.synthetic_cases()[name], block=3000)
    got = _same(path)
    counter, counters = RC.restate_counter(descs, 0)
    assert got.counters == RC.restate_counter(descs, 10)[1]
    with D.DeviceBamReader(path) as d:
        h = d.read_length_histogram(0)
    assert h.counters == counters and h.as_counter() == counter


@pytest.mark.parametrize("mapq", [0, 1, 10, 20, 30])
def test_golden_bam(mapq):
    _same(GOLD, (mapq,))


def test_empty_and_filtered_files(tmp_path):
    for name, recs in (("empty", []), ("filtered", [(0, 0x4, 30, [("M", 36)], None), (-1, 0, 30, [("M", 36)], None)])):
        p = str(tmp_path / (name + ".bam"))
        RC.write_case(p, recs)
        got = _same(p)
        assert got.counts.size == 0
        with pytest.raises(ValueError, match="no reads"):
            readlen.estimate_readlen(p, "MEDIAN", 0)


def test_records_straddling_members_and_pieces(tmp_path):
    """Records of very different sizes over many 16-KB pieces and BGZF members (as test_many_pieces_and_long_records)."""
    rng = np.random.default_rng(12)
    recs, pos = [], 0
    for i in range(6000):
        pos += int(rng.integers(0, 50))
        n = int(rng.choice([20, 36, 101, 250, 2000, 40000], p=[0.3, 0.3, 0.2, 0.15, 0.045, 0.005]))
        cig = [("S", 2), ("M", n - 2)] if i % 3 else [("M", n)]
        flag = int(rng.choice([0, 16, 0x400, 4, 0x1 | 0x80, 0x100]))
        recs.append(W.bam_record(int(rng.integers(-1, 1)) if flag == 4 else 0, pos, int(rng.integers(0, 61)), flag, cig,
                                 b"r%d" % i, tags=b"XAZ" + bytes(rng.integers(65, 91, int(rng.integers(0, 40)), dtype=np.uint8))
                                 + b"\0"))
    path = str(tmp_path / "l.bam")
    W.write_bam(path, [("c1", 5_000_000)], recs, level=1)
    _same(path, (0, 5, 30))


@pytest.mark.timeout(900)
def test_two_million_records_trimmed_mix(tmp_path):
    rng = np.random.default_rng(7)
    n = 2_100_000
    lens = RC.trimmed_mix(rng, n)
    flags = rng.choice(np.array([0, 16, 0x400, 4], dtype=np.uint16), size=n, p=[0.45, 0.45, 0.05, 0.05])
    mapq = rng.integers(0, 61, size=n).astype(np.uint8)
    path = str(tmp_path / "mix.bam")
    RC.write_big(path, lens, flags, mapq)
    got = _same(path, (0, 10), threads=16)
    keep = ((flags & 0x404) == 0) & (mapq >= 10)
    exp = np.bincount(lens[keep], minlength=37)
    assert got.lengths.tolist() == np.flatnonzero(exp).tolist()
    assert got.counts.tolist() == exp[exp > 0].tolist()


@pytest.mark.timeout(900)
def test_two_million_records_one_length(tmp_path):
    """The contention case: every record 36."""
    n = 2_000_000
    path = str(tmp_path / "one.bam")
    RC.write_big(path, np.full(n, 36, dtype=np.uint32))
    got = _same(path, (0,), threads=16)
    assert got.lengths.tolist() == [36] and got.counts.tolist() == [n]
    assert got.counters["nreads"] == n and got.counters["ncounted"] == n


def test_histogram_leaves_the_decode_alone(tmp_path):
    rng = np.random.default_rng(4)
    refs = [("c1", 300000), ("c2", 200000)]
    recs, _m = W.synth_bam_records(rng, refs, 20000)
    path = str(tmp_path / "d.bam")
    W.write_bam(path, refs, recs, block=5000)
    with D.DeviceBamReader(path) as fresh:
        n = fresh.decode(10)
        expect = fresh._fetch(0, n)
    with D.DeviceBamReader(path) as d:              # histogram first, then decode
        h0 = d.read_length_histogram(0)
        assert d.decode(10) == n
        got = d._fetch(0, n)
        assert all((x == y).all() for x, y in zip(got, expect))
        addrs, runs, cnt = d.device_arrays(), d.device_runs(), d.counters()
        h1 = d.read_length_histogram(10)            # decode, then histogram: the decode's arrays unchanged
        h2 = d.read_length_histogram(0)
        assert d.device_arrays() == addrs and d.device_runs() == runs and d.counters() == cnt
        got = d._fetch(0, n)
        assert all((x == y).all() for x, y in zip(got, expect))
        assert h2.counters == h0.counters and h2.counts.tolist() == h0.counts.tolist()
        assert h1.counters["ncounted"] <= h0.counters["ncounted"]


def _compare_tables(outdir, result):
    """The golden tables, written in the BAM header's chromosome order (as tests/test_gpu_ingest.py compares them)."""
    from pymasc_amd import tables as T
    with B.BamReader(GOLD) as b:
        names = b.references
    os.makedirs(outdir, exist_ok=True)
    by = {p.name: p for p in T.write_tables(outdir / "ENCFF000RMB-test.bam", result, references=names)}
    for name in ("ENCFF000RMB-test_cc.tab", "ENCFF000RMB-test_mscc.tab", "ENCFF000RMB-test_nreads.tab"):
        p, gold = by[name], os.path.join(GOLDEN, name)
        if name.endswith("_nreads.tab"):
            assert open(p, "rb").read() == open(gold, "rb").read()
            continue
        g = list(csv.reader(open(gold, newline=""), dialect="excel-tab"))
        o = list(csv.reader(open(p, newline=""), dialect="excel-tab"))
        assert g[0] == o[0] and len(g) == len(o)
        np.testing.assert_almost_equal(np.array([r[1:] for r in o[1:]], dtype=float),
                                       np.array([r[1:] for r in g[1:]], dtype=float), decimal=15)


def test_pipeline_without_read_len_on_the_device_inflates_once(tmp_path, monkeypatch):
    """-d 300 -q 10 -m bigwig with no -r: the estimate (36) is made on the device reader the run then feeds from."""
    from pymasc_amd import pipeline
    opened = []

    class Counting(D.DeviceBamReader):
        def __init__(self, *a, **k):
            opened.append(a[0] if a else k.get("path"))
            super().__init__(*a, **k)

    monkeypatch.setattr(D, "DeviceBamReader", Counting)
    results = {}
    for tag, rl in (("est", None), ("r36", 36)):
        d = tmp_path / tag
        d.mkdir()
        shutil.copy(BIGWIG, d / "hg19_36mer-test.bigwig")
        opened.clear()
        res, written = pipeline.run(GOLD, d / "out", 300, read_len=rl, mapq_criteria=10,
                                    mappability_path=str(d / "hg19_36mer-test.bigwig"))
        assert len(opened) == 1
        _compare_tables(d / "gold_order", res)
        results[tag] = [open(p, "rb").read() for p in written]
        assert res.read_len == 36
    assert results["est"] == results["r36"]


def test_estimate_readlen_reference_signature():
    assert readlen.estimate_readlen(GOLD, "median", 10) == 36
    assert readlen.estimate_readlen(path=GOLD, esttype="MODE", mapq_criteria=10) == 36
