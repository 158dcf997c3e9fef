"""pipeline.run_files on the GPU: the reference's golden run (`-d 300 -q 10 -r 36 -m bigwig`) of the BAM file, its BGZF SAM twin and a
renamed copy in one call through the device readers -- every file's tables equal the golden ones, the track is decoded once, and
the context's device memory does not grow from one file to the next; the same with the read length estimated, two synthetic
files with different read lengths against per-file pipeline.run, and two gloo ranks on one GPU."""
import csv
import multiprocessing as mp
import os
import shutil
from pathlib import Path

import numpy as np
import pytest

from pymasc_amd import bam_device as D
from pymasc_amd import bigwig_device as BD
from pymasc_amd import ffi, pipeline
from pymasc_amd import sam as S
from pymasc_amd.calculator import CCHipCalculator
from . import fixtures as fx
from . import io_writers as W
from . import sam_cases as SC
from . import test_gpu_ingest_indexed as IX
from .test_gpu_stats import _check_golden

pytestmark = pytest.mark.gpu

GOLD = os.path.join(fx.GOLDEN, "ENCFF000RMB-test")
TABLES = ["_cc.tab", "_mscc.tab", "_nreads.tab"]


def _rows(path):
    with open(path, newline="") as fp:
        return list(csv.reader(fp, dialect="excel-tab"))


def _check_tables(written):
    """The golden _cc / _mscc to decimal=15 and the golden _nreads.tab's columns (as tests/test_pipeline.py checks run)."""
    by = {p.name[p.name.rindex("_"):]: p for p in written}
    for suffix in ("_cc.tab", "_mscc.tab"):
        got, exp = _rows(by[suffix]), _rows(GOLD + suffix)
        assert got[0] == exp[0] and len(got) == len(exp)
        np.testing.assert_almost_equal(np.array([r[1:] for r in got[1:]], dtype=float),
                                       np.array([r[1:] for r in exp[1:]], dtype=float), decimal=15)
    got, exp = _rows(by["_nreads.tab"]), _rows(GOLD + "_nreads.tab")
    col = exp[0].index("chr1")
    assert got[0] == ["shift", "whole", "chr1"]
    assert got[1:] == [[r[0], r[1], r[col]] for r in exp[1:]]


def _inputs(tmp_path):
    """The golden BAM (with its index), its BGZF SAM twin and a renamed copy of the BAM, and the track."""
    d = tmp_path / "in"
    d.mkdir()
    bam = d / "ENCFF000RMB-test.bam"
    shutil.copy(GOLD + ".bam", bam)
    shutil.copy(GOLD + ".bam.bai", str(bam) + ".bai")
    sam = d / "twin.sam.gz"
    shutil.copy(SC.GOLDEN_SAM_GZ, sam)
    renamed = d / "renamed.bam"
    shutil.copy(GOLD + ".bam", renamed)
    bw = tmp_path / "hg19_36mer-test.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    return [str(bam), str(sam), str(renamed)], str(bw)


@pytest.mark.parametrize("read_len", [36, None])
def test_golden_files_in_one_call(tmp_path, monkeypatch, read_len):
    paths, bw = _inputs(tmp_path)
    tracks, contexts, after = [], [], []

    class CountingTrack(BD.DeviceBigWigReader):
        def __init__(self, *a, **k):
            tracks.append(a[0] if a else k.get("path"))
            super().__init__(*a, **k)

    class CountingContext(ffi.Context):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.live = 0
            contexts.append(self)

        def bits_alloc(self, nbits):
            p = super().bits_alloc(nbits)
            self.live += 1
            return p

        def bits_free(self, d_words):
            super().bits_free(d_words)
            self.live -= 1

    real_run = pipeline.run_sharded

    def run_sharded(*a, **k):
        out = real_run(*a, **k)
        after.append(k["context"].live)
        return out

    host_sam = []

    class CountingSam(S.SamReader):
        def __init__(self, *a, **k):
            host_sam.append(bool(k.get("header_only")))
            super().__init__(*a, **k)

    monkeypatch.setattr(BD, "DeviceBigWigReader", CountingTrack)
    monkeypatch.setattr(ffi, "Context", CountingContext)
    monkeypatch.setattr(pipeline, "run_sharded", run_sharded)
    monkeypatch.setattr(S, "SamReader", CountingSam)
    # without the garbage collector's help: run_sharded must close each calculator itself
    monkeypatch.setattr(CCHipCalculator, "__del__", lambda self: None)
    got = pipeline.run_files(paths, tmp_path / "out", max_shift=300, read_len=read_len, mapq_criteria=10,
                             mappability_path=bw, stats=True)
    assert [g.error for g in got] == [None] * 3
    assert [g.basename for g in got] == ["ENCFF000RMB-test", "twin.sam", "renamed"]
    assert len(tracks) == 1 and len(contexts) == 1
    assert len(after) == 3 and after[2] == after[0]
    assert host_sam == [True]           # the SAM twin's header on the host; its text is read on the device alone
    assert open(tmp_path / "hg19_36mer-test_mappability.json", "rb").read() == \
        open(os.path.join(fx.GOLDEN, "hg19_36mer-test_mappability.json"), "rb").read()
    for g in got:
        assert g.result.read_len == 36
        assert (g.result.forward_sum, g.result.reverse_sum) == (622, 670)
        assert [p.name for p in g.written] == [g.basename + s for s in TABLES + ["_stats.tab"]]
        _check_tables(g.written)
        _check_golden(g.written[3], g.basename)


def _synthetic(d):
    refs = [("c1", 400000), ("c2", 250000)]
    paths = []
    for name, rl, seed in (("r36", 36, 1), ("r50", 50, 2)):
        recs, _m = W.synth_bam_records(np.random.default_rng(seed), refs, 20000, readlen=rl, mapq_lo=5)
        paths.append(str(d / (name + ".bam")))
        W.write_bam(paths[-1], refs, recs)
    tracks = {"c1": [(1000, 90000, 1.0), (120000, 390000, 1.0)], "c2": [(0, 180000, 1.0), (200000, 249000, 1.0)]}
    bw = d / "m.bw"
    W.write_bigwig(str(bw), dict(refs), tracks)
    return paths, str(bw)


def _tables(paths):
    return {os.path.basename(str(p)): open(p, "rb").read() for p in paths}


def test_different_read_lengths_equal_per_file_runs(tmp_path, monkeypatch):
    d = tmp_path / "in"
    d.mkdir()
    paths, bw = _synthetic(d)
    got = pipeline.run_files(paths, tmp_path / "out", max_shift=200, mapq_criteria=10, mappability_path=bw)
    assert [g.error for g in got] == [None, None] and [g.result.read_len for g in got] == [50, 50]
    for g, p in zip(got, paths):
        s = tmp_path / ("single_" + g.basename)
        s.mkdir()
        shutil.copy(bw, s / "m.bw")
        _r, written = pipeline.run(p, s / "out", max_shift=200, read_len=50, mapq_criteria=10, mappability_path=s / "m.bw")
        assert _tables(g.written) == _tables(written)
    # one file without read_len: the estimate's device reader feeds the run (the file is inflated once), as run does it
    opened = []

    class Counting(D.DeviceBamReader):
        def __init__(self, *a, **k):
            opened.append(a[0] if a else k.get("path"))
            super().__init__(*a, **k)

    monkeypatch.setattr(D, "DeviceBamReader", Counting)
    one, = pipeline.run_files([paths[0]], tmp_path / "one", max_shift=200, mapq_criteria=10, mappability_path=bw)
    assert opened == [paths[0]] and one.result.read_len == 36
    _r, written = pipeline.run(paths[0], tmp_path / "one_run", max_shift=200, mapq_criteria=10, mappability_path=bw)
    assert _tables(one.written) == _tables(written)


def _rank_worker(rank, world, port, q, paths, bw, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        got = pipeline.run_files(paths, os.path.join(out, "rank%d" % rank), max_shift=300, read_len=36, mapq_criteria=10,
                                 mappability_path=bw, device=0, stats=True)
        q.put((rank, [(g.basename, [str(p) for p in g.written], None if g.error is None else repr(g.error)) for g in got],
               None))
    except Exception as e:       # reported, not hung on
        q.put((rank, None, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_on_one_gpu(tmp_path):
    paths, bw = _inputs(tmp_path)
    paths = [paths[0], paths[2]]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = IX._free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, paths, bw, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=600) for _ in range(2))
    finally:
        for p in procs:
            p.join(120)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs)
    (_r0, w0, e0), (_r1, w1, e1) = got
    assert e0 is None and e1 is None, (e0, e1)
    assert [x[0] for x in w0] == [x[0] for x in w1] == ["ENCFF000RMB-test", "renamed"]
    assert all(x[2] is None for x in w0 + w1)
    assert all(x[1] == [] for x in w1) and not os.path.exists(tmp_path / "rank1")
    for name, written, _e in w0:
        written = [Path(p) for p in written]
        assert [p.name for p in written] == [name + s for s in TABLES + ["_stats.tab"]]
        _check_tables(written)
        _check_golden(written[3], name)
