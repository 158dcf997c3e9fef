"""Read-length estimation through the host reader (pmx_bam_readlen_hist + pymasc_amd.readlen): histogram, counters and all five
estimators against a restatement of the reference's rules (tests/readlen_cases.py), and pipeline.run without read_len."""
import os
import shutil

import numpy as np
import pytest

from pymasc_amd import readlen
from pymasc_amd.bam import BamReader
from tests import readlen_cases as RC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ENCFF000RMB-test.bam")


def _check(hist, counter, counters):
    assert list(hist.lengths) == sorted(counter)
    assert [int(x) for x in hist.counts] == [counter[k] for k in sorted(counter)]
    assert hist.counters == counters
    # first occurrences: the file order of the lengths is the counter's insertion order
    assert list(hist.as_counter()) == list(counter)
    for e in RC.ESTIMATORS:
        assert hist.estimate(e) == RC.restate_estimate(counter, e), e
        assert hist.estimate(e.lower()) == hist.estimate(e)


@pytest.mark.parametrize("mapq", [0, 1, 10, 20, 30])
def test_golden_bam_every_estimator(mapq):
    counter, counters = RC.restate_counter(RC.golden_descs(), mapq)
    with BamReader(GOLD) as b:
        _check(b.read_length_histogram(mapq), counter, counters)
    for e in RC.ESTIMATORS:
        assert readlen.estimate_readlen(GOLD, e, mapq) == RC.restate_estimate(counter, e)


def test_golden_bam_expected_values():
    with BamReader(GOLD) as b:
        h = b.read_length_histogram(10)
    assert (h.estimate("MIN"), h.estimate("MAX"), h.estimate("MEDIAN"), h.estimate("MODE")) == (20, 36, 36, 36)
    assert readlen.estimate_readlen(GOLD, "median", 10) == 36


@pytest.mark.parametrize("name", sorted(RC.synthetic_cases()))
@pytest.mark.parametrize("mapq", [0, 10])
def test_synthetic_cases(tmp_path, name, mapq):
    path = str(tmp_path / (name + ".bam"))
    descs = RC.write_case(path, RC.synthetic_cases()[name], block=3000)
    counter, counters = RC.restate_counter(descs, mapq)
    with BamReader(path, threads=4) as b:
        h = b.read_length_histogram(mapq)
        _check(h, counter, counters)
        assert b.read_length_histogram(mapq).counters == counters      # (the kept result)


def test_corner_values(tmp_path):
    cases = RC.synthetic_cases()
    got = {}
    for name in ("flags", "even_35_36", "even_36_37", "mode_tie_a", "mode_tie_b", "long_reads"):
        path = str(tmp_path / (name + ".bam"))
        RC.write_case(path, cases[name])
        with BamReader(path) as b:
            got[name] = b.read_length_histogram(10)
    f = got["flags"]
    assert f.counters == {"nreads": 16, "nunmapped": 2, "ncounted": 10, "npaired": 4, "nread2": 3, "nnoqlen": 2}
    assert {50, 51, 52, 53, 32, 70030} <= set(f.lengths.tolist()) and 99 not in f.lengths and 94 not in f.lengths
    assert got["even_35_36"].estimate("MEDIAN") == 36 and got["even_35_36"].estimate("MEAN") == 36   # 35.5 -> 36
    assert got["even_36_37"].estimate("MEDIAN") == 36 and got["even_36_37"].estimate("MEAN") == 36   # 36.5 -> 36
    assert got["mode_tie_a"].estimate("MODE") == 35 and got["mode_tie_b"].estimate("MODE") == 36
    assert got["long_reads"].estimate("MAX") == 200000 and 65536 in got["long_reads"].lengths


def test_reading_between_batches_does_not_disturb_the_iteration(tmp_path):
    rng = np.random.default_rng(3)
    from tests import io_writers as W
    recs, _m = W.synth_bam_records(rng, [("c1", 200000), ("c2", 100000)], 3000)
    path = str(tmp_path / "b.bam")
    W.write_bam(path, [("c1", 200000), ("c2", 100000)], recs, block=4000)
    with BamReader(path) as b:
        whole = [np.concatenate(x) for x in zip(*b.batches(10, batch=500))]
        parts = []
        for i, batch in enumerate(b.batches(10, batch=500)):
            if i in (0, 3):
                b.read_length_histogram(i)
            parts.append(batch)
        again = [np.concatenate(x) for x in zip(*parts)]
    assert all((x == y).all() for x, y in zip(whole, again))


def test_errors(tmp_path):
    cases = RC.synthetic_cases()
    empty = str(tmp_path / "empty.bam")
    RC.write_case(empty, [])
    filtered = str(tmp_path / "filtered.bam")
    RC.write_case(filtered, [(0, 0x4, 30, [("M", 36)], None), (0, 0x400, 30, [("M", 36)], None), (-1, 0, 30, [("M", 36)], None),
                             (0, 0, 30, [], None)])
    for p in (empty, filtered):
        with pytest.raises(ValueError, match="no reads"):
            readlen.estimate_readlen(p, "MEDIAN", 0)
        with BamReader(p) as b:
            h = b.read_length_histogram(0)
            for e in RC.ESTIMATORS:
                with pytest.raises(ValueError):
                    h.estimate(e)
    big = str(tmp_path / "long.bam")
    RC.write_case(big, cases["long_reads"])
    with pytest.raises(ValueError, match="longer than shift size"):
        readlen.estimate_readlen(big, "MAX", 10, max_shift=199999)
    assert readlen.estimate_readlen(big, "MAX", 10, max_shift=200000) == 200000
    with pytest.raises(ValueError, match="estimator"):
        readlen.estimate_readlen(GOLD, "AVERAGE", 10)
    with BamReader(GOLD) as b:
        with pytest.raises(ValueError):
            b.read_length_histogram(10).estimate("mid")


def test_truncated_file_is_a_format_error(tmp_path):
    from pymasc_amd.bam import PmxIOError
    from tests import io_writers as W
    path = str(tmp_path / "t.bam")
    recs = [W.bam_record(0, 10 * i, 30, 0, [("M", 36)], b"r%d" % i) for i in range(50)]
    data = W.bam_header(RC.REFS) + b"".join(recs)
    with open(path, "wb") as fp:
        fp.write(W.bgzf_compress(data[:-10]))
    with BamReader(path) as b:
        with pytest.raises(PmxIOError) as ei:
            b.read_length_histogram(0)
    assert ei.value.code == -2


# ---- pipeline.run without read_len ----------------------------------------------------------------------------------
def _inputs(tmp):
    """A coordinate-sorted BAM with mixed read lengths (20..40, some soft-clipped) + a track, as tests/test_sharding.py's."""
    from tests import io_writers as W
    rng = np.random.default_rng(11)
    refs = [("c1", 30000), ("c2", 20000)]
    recs, descs, rec_refs = [], [], []
    for rid, (_n, ln) in enumerate(refs):
        for pos in np.sort(rng.integers(0, ln - 60, size=800)).tolist():
            n = int(rng.choice([20, 27, 33, 38, 40], p=[0.1, 0.15, 0.2, 0.25, 0.3]))
            cig = [("S", 2), ("M", n - 2)] if pos % 3 == 0 else [("M", n)]
            flag = int(rng.choice([0, 16, 0x400, 0x1 | 0x80, 4]))
            mq = int(rng.integers(0, 61))
            recs.append(W.bam_record(rid, pos, mq, flag, cig, b"r%d" % len(recs)))
            descs.append((rid, flag, mq, cig))
            rec_refs.append(rid)
    bam = os.path.join(tmp, "s.bam")
    W.write_bam_indexed(bam, refs, recs, rec_refs, block=3000)
    tracks = {"c1": [(100, 9000, 1.0), (12000, 29000, 1.0)], "c2": [(0, 18000, 1.0)]}
    bw = os.path.join(tmp, "m.bw")
    W.write_bigwig(bw, {"c1": 30000, "c2": 20000}, tracks, items_per_block=40)
    return bam, bw, descs


def test_pipeline_without_read_len_equals_the_explicit_estimate(tmp_path):
    from pymasc_amd import pipeline
    from tests.fake_context import FakeContext
    tmp = str(tmp_path)
    bam, bw, descs = _inputs(tmp)
    counter, _c = RC.restate_counter(descs, 10)
    expect = RC.restate_estimate(counter, "MEDIAN")
    runs = {}
    for tag, rl in (("est", None), ("explicit", expect)):
        d = os.path.join(tmp, tag)
        os.makedirs(d)
        shutil.copy(bw, os.path.join(d, "m.bw"))
        res, written = pipeline.run(bam, os.path.join(d, "out"), 120, read_len=rl, mapq_criteria=10,
                                    mappability_path=os.path.join(d, "m.bw"), device_ingest=False, context=FakeContext())
        runs[tag] = (res.read_len, [open(p, "rb").read() for p in written], open(os.path.join(d, "m_mappability.json")).read())
    assert runs["est"][0] == expect
    assert runs["est"] == runs["explicit"]
    with pytest.raises(ValueError, match="longer than shift size"):
        pipeline.run(bam, os.path.join(tmp, "x"), expect - 1, mapq_criteria=10, device_ingest=False, context=FakeContext())
    mean = RC.restate_estimate(counter, "MEAN")
    res, _w = pipeline.run(bam, os.path.join(tmp, "mean"), 120, mapq_criteria=10, device_ingest=False, context=FakeContext(),
                           readlen_estimator="mean")
    assert res.read_len == mean


def _rank_worker(rank, world, port, q, bam, bw, tmp):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pymasc_amd import pipeline
        from tests.fake_context import FakeContext
        res, written = pipeline.run(bam, os.path.join(tmp, "out_%d" % rank), 120, mapq_criteria=10, mappability_path=bw,
                                    context=FakeContext())
        tabs = [open(p, "rb").read() for p in written]
        try:
            pipeline.run(bam, os.path.join(tmp, "bad_%d" % rank), 5, mapq_criteria=10, context=FakeContext())
            err = "no error"
        except Exception as e:
            err = type(e).__name__
        q.put((rank, res.read_len, tabs, err))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_share_the_estimate(tmp_path):
    import socket
    import torch.multiprocessing as mp
    from pymasc_amd import pipeline
    from tests.fake_context import FakeContext
    tmp = str(tmp_path)
    bam, bw, _descs = _inputs(tmp)
    single, written = pipeline.run(bam, os.path.join(tmp, "single"), 120, mapq_criteria=10, mappability_path=bw,
                                   device_ingest=False, context=FakeContext())
    expect = [open(p, "rb").read() for p in written]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, bam, bw, tmp)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted(q.get(timeout=600) for _ in range(2))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert [g[1] for g in got] == [single.read_len] * 2
    assert got[0][2] == expect and got[1][2] == []
    assert [g[3] for g in got] == ["ValueError", "RuntimeError"]      # every rank raises; rank 0 its own ValueError
