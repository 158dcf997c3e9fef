"""pmx_dbam_coverage_* on the GPU: the device against the loop restatement of tests/coverage_cases, run for run, in
all five totals and in the bytes of the track, through every device reader, with and without excluded regions, a stream window by
window, beside the other counts, and up to the run's file.  Everything is an integer or a byte and exact."""
import os
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, fingerprint, pipeline, region_mask, stats
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import io_writers as W
from tests import sam_writers as SW

pytestmark = pytest.mark.gpu

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
GOLDEN_TRACK = os.path.join(fx.GOLDEN, "hg19_36mer-test.bedGraph")
NAMES = [n for n, _l in CC.REFS]
LENGTHS = [l for _n, l in CC.REFS]
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_coverage")
    rows = CC.synthetic()
    recs = FC.alignment_records(rows, CC.REFS)
    _sam, bam, gz = SW.write_twins(d, "cv", CC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, CC.REFS, SW.bam_bytes(CC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "cv.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, CC.REFS)))
    reads = FC.kept(rows)
    less = FC.masked(reads, CC.REFS, CC.MASK)
    assert 18_000 < len(less) < len(reads) < 22_000
    return dict(dir=d, bam=bam, gz=gz, indexed=indexed, tag=tag, reads=reads, less=less, want={})


def _want(case, extend, use="all", masked=False):
    """The restatement, computed once per parameter set and left unchanged."""
    if (extend, masked) not in case["want"]:
        case["want"][extend, masked] = CC.restate(case["less" if masked else "reads"], CC.REFS, CC.USES["all"], extend)
    whole = case["want"][extend, masked]
    return whole if use == "all" else CC.select(whole, CC.REFS, case["less" if masked else "reads"], CC.USES[use], extend)


def _chosen(use):
    return [n for n, u in zip(NAMES, CC.USES[use]) if u]


def _check(acc, reader, want, extend):
    """The finished count against the restatement: the five totals, every run, the Coverage."""
    assert tuple(acc.finish(reader)[k] for k in coverage.TOTALS) == CC.totals(want)
    ref, start, end, depth = acc.runs(reader)
    assert (ref.dtype, start.dtype, end.dtype, depth.dtype) == (np.int32, np.uint32, np.uint32, np.uint32)
    got = list(zip([NAMES[r] for r in ref.tolist()], start.tolist(), end.tolist(), depth.tolist()))
    assert got == CC.rows_of(want) and len(got) > 1000
    assert acc.result(reader) == CC.as_coverage(want, extend)


@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_runs_totals_and_text(case, extend):
    CC.check_situations(case["reads"], _want(case, extend), extend)
    with DeviceBamReader(case["bam"]) as r:
        assert r._L.pmx_dbam_version() >= 13
        for use in sorted(CC.USES):
            want = _want(case, extend, use)
            acc = coverage.DeviceCount(r, FC.MAPQ, _chosen(use), extend)
            assert acc.add(r) == want["reads"]
            _check(acc, r, want, extend)
            text = CC.text_of(want)
            assert b"".join(acc.text_chunks(r, 1000)) == text and acc.text(r) == text and want["n_runs"] > 3000
            assert acc.text(r, 5, 0) == b"" and acc.text(r, want["n_runs"] - 2, 2) == b"".join(text.splitlines(True)[-2:])
            assert r.coverage(FC.MAPQ, _chosen(use), extend) == CC.as_coverage(want, extend)


def _fifo_count(case, tmp_path, mask, extend, more=False):
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = open(case["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    t = threading.Thread(target=writer)
    t.start()
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r:
            assert not r.seekable
            if mask is not None:
                r.set_exclude(mask.resolve(r.references, r.lengths))
            acc = r.arm_coverage(FC.MAPQ, None, extend)
            others = (r.arm_fingerprint(FC.MAPQ, None, 500, extend), r.arm_complexity(FC.MAPQ, None),
                      r.arm_peaks({"f0": [(100, 30_000)], "f2": [(5, 900)]}, FC.MAPQ, None, extend)) if more else None
            for _ in r._windows():
                pass
            got = acc.result(r)
            got.device_totals = tuple(acc.finish(r)[k] for k in coverage.TOTALS)
            if more:
                others = (others[0].result(r), others[1].result(), others[2].result(r))
            info = r.stream_info()
    finally:
        t.join(60)
    os.unlink(fifo)
    return got, others, info


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_every_reader_gives_the_whole_file_runs(case, tmp_path, extend, masked):
    mask = region_mask.open_mask(CC.MASK) if masked else None
    want = _want(case, extend, "all", masked)
    whole = CC.as_coverage(want, extend)
    if masked:
        assert whole.reads < _want(case, extend)["reads"]

    def count(reader, want=want):
        """The reader's Coverage, its five totals of ``finish`` set against the restatement's first."""
        if mask is not None:
            reader.set_exclude(mask.resolve(reader.references, reader.lengths))
        acc = coverage.device_count_of(reader, FC.MAPQ, None, extend)
        assert tuple(acc.finish(reader)[k] for k in coverage.TOTALS) == CC.totals(want)
        return acc.result(reader)
    with DeviceBamReader(case["bam"]) as r:
        assert count(r) == whole
    with DeviceSamReader(case["gz"]) as r:
        assert count(r) == whole
    with DeviceBedReadsReader(case["tag"], NAMES, LENGTHS) as r:
        assert count(r) == whole
    less = _want(case, extend, "no middle", masked)
    part = CC.as_coverage(less, extend)
    with DeviceBamReader(case["indexed"], references=_chosen("no middle")) as r:
        assert r.indexed
        c = count(r, less)
        assert c == part and list(c.runs) == ["f0", "f2"]
        with pytest.raises(ValueError):
            r.coverage(FC.MAPQ, [NAMES[1]], extend)                                         # (not selected)
    got, _others, info = _fifo_count(case, tmp_path, mask, extend)
    assert got == whole and got.device_totals == CC.totals(want) and info["windows"] >= 10 and info["peak_device_bytes"] > 4 * sum(LENGTHS)


def test_beside_the_other_counts(case, tmp_path):
    extend = 200
    want = _want(case, extend)
    lines = {"f0": [(100, 30_000)], "f2": [(5, 900)]}
    with DeviceBamReader(case["bam"]) as r:
        bins_alone = r.bin_counts(FC.MAPQ, None, 500, extend)
        nrf_alone = r.library_complexity(FC.MAPQ)
        peaks_alone = r.peak_counts(lines, FC.MAPQ, None, extend)
        n = r.decode(30)
        before, counters, runs = r._fetch(0, n), r.counters(), r.device_runs()
        fp = fingerprint.DeviceCount(r, FC.MAPQ, None, 500, extend)                         # the tables on one handle
        cv = coverage.DeviceCount(r, FC.MAPQ, None, extend)
        fp.add(r)
        cv.add(r)
        assert r.library_complexity(FC.MAPQ) == nrf_alone and r.peak_counts(lines, FC.MAPQ, None, extend) == peaks_alone
        _check(cv, r, want, extend)
        assert fp.result(r) == bins_alone
        # the arrays, counters and runs of the last decode are as they were
        assert all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n)))
        assert r.counters() == counters and r.device_runs() == runs
    got, others, info = _fifo_count(case, tmp_path, None, extend, more=True)
    assert info["windows"] >= 10 and got == CC.as_coverage(want, extend)
    assert others == (bins_alone, nrf_alone, peaks_alone)


def test_tile_multiples(case):
    refs, reads = CC.tile_case()
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    _sam, bam = SW.write_twins(case["dir"], "tiles", refs, recs)
    for extend in (0, 200):
        want = CC.restate(reads, refs, [1, 1, 1], extend)
        with DeviceBamReader(bam) as r:
            acc = coverage.DeviceCount(r, FC.MAPQ, None, extend)
            assert acc.add(r) == want["reads"] == len(reads)
            assert tuple(acc.finish(r)[k] for k in coverage.TOTALS) == CC.totals(want)
            assert acc.text(r) == CC.text_of(want)


def test_add_twice_doubles_and_begin_replaces(case):
    want = _want(case, 200)
    with DeviceBamReader(case["bam"]) as r:
        acc = coverage.DeviceCount(r, FC.MAPQ, None, 200)
        assert acc.add(r) == acc.add(r) == want["reads"]
        twice = acc.result(r)
        assert twice.rows() == [(n, s, e, 2 * d) for n, s, e, d in CC.rows_of(want)] and twice.reads == 2 * want["reads"]
        acc.begin(r)                                                                        # in the runs state: a new table
        assert acc.finish(r) == dict(zip(coverage.TOTALS, (0, 0, 0, 0, 0))) and acc.text(r) == b""
        acc.begin(r)
        acc.add(r)
        acc.begin(r)                                                                        # in the table state: the marks are gone
        assert acc.add(r) == want["reads"]
        _check(acc, r, want, 200)


def test_error_paths(case):
    with DeviceBamReader(case["bam"]) as r:
        L, h = r._L, r._h
        added, totals = np.zeros(1, dtype=np.uint64), np.zeros(5, dtype=np.uint64)
        a = [np.zeros(4, dtype=t) for t in (np.int32, np.uint32, np.uint32, np.uint32)]
        buf = np.zeros(64, dtype=np.uint8)
        ptr = [x.ctypes.data for x in a]
        import ctypes
        out = ctypes.cast(added.ctypes.data, ctypes.POINTER(ctypes.c_uint64))

        def fails(rc, text):
            assert rc == -3
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc)
        no_table, no_runs = "no table: call pmx_dbam_coverage_begin first", "no runs: call pmx_dbam_coverage_finish first"
        fails(L.pmx_dbam_coverage_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out), "pmx_dbam_coverage_add: " + no_table)
        fails(L.pmx_dbam_coverage_finish(h, totals.ctypes.data), "pmx_dbam_coverage_finish: " + no_table)
        fails(L.pmx_dbam_coverage_runs(h, 0, 0, *ptr), "pmx_dbam_coverage_runs: " + no_runs)
        fails(L.pmx_dbam_coverage_text(h, 0, 0, None, 0), "pmx_dbam_coverage_text: " + no_runs)
        none = np.zeros(len(NAMES), dtype=np.uint8)
        fails(L.pmx_dbam_coverage_begin(h, 0, none.ctypes.data), "pmx_dbam_coverage_begin: no chosen reference")
        fails(L.pmx_dbam_coverage_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out), no_table)       # a failed begin leaves no table
        acc = coverage.DeviceCount(r, FC.MAPQ, None, 0)
        fails(L.pmx_dbam_coverage_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, None), "pmx_dbam_coverage_add: null output")
        fails(L.pmx_dbam_coverage_finish(h, None), "pmx_dbam_coverage_finish: null output")
        fails(L.pmx_dbam_coverage_runs(h, 0, 0, *ptr), no_runs)                             # a table, no runs yet
        fails(L.pmx_dbam_coverage_text(h, 0, 0, None, 0), no_runs)
        acc.add(r)
        n = acc.finish(r)["runs"]
        fails(L.pmx_dbam_coverage_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out), no_table)       # the table has become runs
        fails(L.pmx_dbam_coverage_finish(h, totals.ctypes.data), no_table)
        fails(L.pmx_dbam_coverage_runs(h, 0, 4, ptr[0], None, ptr[2], ptr[3]), "pmx_dbam_coverage_runs: null output")
        for first, count in ((n - 3, 4), (-1, 2), (0, -1), (n + 1, 0)):
            fails(L.pmx_dbam_coverage_runs(h, first, count, *ptr), "pmx_dbam_coverage_runs: range outside the runs")
            fails(L.pmx_dbam_coverage_text(h, first, count, None, 0), "pmx_dbam_coverage_text: range outside the runs")
        size = L.pmx_dbam_coverage_text(h, 0, 4, None, 0)
        assert 4 * 8 <= size <= 64
        fails(L.pmx_dbam_coverage_text(h, 0, 4, buf.ctypes.data, size - 1), "pmx_dbam_coverage_text: the buffer is too small")
        assert L.pmx_dbam_coverage_text(h, 0, 4, buf.ctypes.data, size) == size and buf[:size].tobytes() == acc.text(r, 0, 4)


def test_the_run_writes_the_track_at_its_own_estimate(tmp_path):
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=GOLDEN_TRACK, save_mappability_stats=False, stats=True)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 300, **kw)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 300, coverage=True, **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_coverage.bedGraph"] and len(w0) == 4
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c = coverage.read_coverage(w1[-1])
    rows = dict(ln.rstrip("\n").split("\t") for ln in open(w1[-2]))
    assert name == stem and str(c.extend) == rows["Estimated library length"] and 36 < c.extend <= 301
    assert c.extend == stats.genome_wide_stats(_r1, 36).est_lib_len
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, b.lengths))
        cols = [np.concatenate(x) for x in zip(*b.batches(10))]
    assert c == coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), c.extend) and c.n_runs > 100
    # an integer is counted on the reader that feeds the run, beside the other counts, in the order they are asked for
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 300, references=[refs[0][0]], coverage=True, coverage_extend=0,
                           complexity=True, fingerprint=True, **kw)
    assert [p.name.rsplit("_", 1)[-1] for p in w2[-3:]] == ["complexity.tab", "fingerprint.tab", "coverage.bedGraph"]
    assert sorted(os.listdir(tmp_path / "two")) == sorted(p.name for p in w2)               # (the temporary file is gone)
    assert coverage.read_coverage(w2[-1])[1] == coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs],
                                                                    [1] + [0] * (len(refs) - 1), 0)
