"""pipeline.run(stats=True) on the GPU: the _stats.tab of the reference's golden run (`-d 300 -q 10 -r 36 -m bigwig`), made from
what the device ingest, the device BigWig reader and the kernels produced, equals the reference's golden ENCFF000RMB-test_stats.tab
(integers and strings exactly, floats to decimal=10) from the BAM file, from SAM, with the read length estimated, and from rank 0
of two gloo ranks on one GPU; stats=False writes the three tables it always wrote; bad options fail before a context exists."""
import multiprocessing as mp
import os
import shutil

import pytest

from pymasc_amd import pipeline
from pymasc_amd import stats as S
from . import fixtures as fx
from . import sam_cases as SC
from . import test_gpu_ingest_indexed as IX
from .test_stats import _assert_rows

pytestmark = pytest.mark.gpu

GOLD = os.path.join(fx.GOLDEN, "ENCFF000RMB-test")
TABLES = ["_cc.tab", "_mscc.tab", "_nreads.tab"]


def _inputs(tmp_path, kind="bam"):
    src = tmp_path / ("ENCFF000RMB-test." + kind)
    if kind == "bam":
        shutil.copy(GOLD + ".bam", src)
        shutil.copy(GOLD + ".bam.bai", str(src) + ".bai")
    elif kind == "sam":
        src.write_bytes(SC.golden_sam_text())
    else:
        shutil.copy(SC.GOLDEN_SAM_GZ, src)
    bw = tmp_path / "hg19_36mer-test.bigwig"
    if not bw.exists():
        shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    return src, bw


def _check_golden(path, name="ENCFF000RMB-test"):
    got = S.load_stats(path)
    want = S.load_stats(GOLD + "_stats.tab")
    assert got["Name"] == name
    want["Name"] = name
    _assert_rows(got, want)


@pytest.mark.parametrize("kind", ["bam", "sam", "sam.gz"])
def test_golden_stats_from_device_run(tmp_path, kind):
    src, bw = _inputs(tmp_path, kind)
    result, written = pipeline.run(src, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10,
                                   mappability_path=bw, stats=True)
    stem = src.stem
    assert [p.name for p in written] == [stem + s for s in TABLES] + [stem + "_stats.tab"]
    _check_golden(written[3], stem)
    assert (result.forward_sum, result.reverse_sum) == (622, 670)


def test_golden_stats_with_estimated_read_len(tmp_path):
    src, bw = _inputs(tmp_path)
    result, written = pipeline.run(src, tmp_path / "out", max_shift=300, mapq_criteria=10, mappability_path=bw,
                                   stats=True)
    assert result.read_len == 36                                            # the MEDIAN estimate
    _check_golden(written[3])


def test_stats_off_writes_the_three_tables(tmp_path):
    src, bw = _inputs(tmp_path)
    _r, written = pipeline.run(src, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10, mappability_path=bw)
    assert [p.name for p in written] == ["ENCFF000RMB-test" + s for s in TABLES]
    assert sorted(os.listdir(tmp_path / "out")) == sorted("ENCFF000RMB-test" + s for s in TABLES)


def test_library_length_and_options_on_device_result(tmp_path):
    """The options reach the statistics: the same file as genome_wide_stats gives for the returned result."""
    src, bw = _inputs(tmp_path)
    opts = dict(library_length=150, smooth_window=7, bg_avr_width=30, mask_size=2, chi2_pval=0.01)
    result, written = pipeline.run(src, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10,
                                   mappability_path=bw, stats=True, **opts)
    got = S.load_stats(written[3])
    assert got == dict(S.stats_rows("ENCFF000RMB-test", S.genome_wide_stats(result, 36, **opts)))
    assert got["Expected library length"] == "150" and got["FWHM"] not in ("nan", "False")


@pytest.mark.parametrize("kw", [dict(library_length=301), dict(library_length=0), dict(smooth_window=0)])
def test_bad_options_fail_before_a_context(tmp_path, monkeypatch, kw):
    from pymasc_amd import ffi

    def no_context(*a, **k):
        raise AssertionError("a GPU context was created")
    monkeypatch.setattr(ffi, "Context", no_context)
    src, bw = _inputs(tmp_path)
    with pytest.raises(ValueError):
        pipeline.run(src, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10, mappability_path=bw,
                     stats=True, **kw)
    assert not (tmp_path / "out").exists()


def _rank_worker(rank, world, port, q, src, bw, out):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        _r, written = pipeline.run(src, os.path.join(out, "rank%d" % rank), max_shift=300, read_len=36, mapq_criteria=10,
                                   mappability_path=bw, device=0, stats=True)
        q.put((rank, [str(p) for p in written], None))
    except Exception as e:       # reported, not hung on
        q.put((rank, None, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_on_one_gpu(tmp_path):
    """Two gloo ranks on one GPU: rank 0 writes the golden _stats.tab, rank 1 writes nothing."""
    src, bw = _inputs(tmp_path)
    pipeline.run(src, tmp_path / "warm", max_shift=300, read_len=36, mapq_criteria=10, mappability_path=bw)  # the cache
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = IX._free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, str(src), str(bw), str(tmp_path))) for r in range(2)]
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
    (r0, w0, e0), (r1, w1, e1) = got
    assert e0 is None and e1 is None, (e0, e1)
    assert [os.path.basename(p) for p in w0] == ["ENCFF000RMB-test" + s for s in TABLES + ["_stats.tab"]]
    assert w1 == [] and not os.path.exists(tmp_path / "rank1")
    _check_golden(w0[3])
