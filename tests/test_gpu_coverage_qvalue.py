"""The q-score table on the GPU: pmx_dbam_coverage_qvalue* against the loop restatement of tests/qvalue_cases
and against the host path (``Signal.qvalues``), bit for bit -- every planted situation, the rows in ranges, the four totals and the
cutoffs --, pmx_dbam_coverage_call_text with the table against ``Peaks.text_chunks`` byte for byte, the treatment through every device
reader and a stream window by window, qvalue twice, the table's lifetime, the refusals, the stream's peak to the byte and up to the
run's files."""
import os
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, pipeline
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bigwig_out_cases as BC
from tests import call_cases as LC
from tests import coverage_cases as CC
from tests import poisson_cases as PS
from tests import qvalue_cases as QV
from tests import sam_writers as SW

pytestmark = pytest.mark.gpu

FC = CC.FC
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows


def _bam_of(d, name, refs, reads):
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], int(p), 40, (("M", int(l)),)) for i, (r, p, l, s) in enumerate(reads)]
    return SW.write_twins(d, name, refs, recs)[1]


def _tag_of(d, name, refs, cols):
    """A tagAlign file of four columns (ref, pos1, read_len, reverse)."""
    path = str(d / (name + ".tagAlign"))
    names = [n for n, _l in refs]
    with open(path, "w") as fp:
        fp.write("".join("%s\t%d\t%d\tN\t1000\t%s\n" % (names[r], p - 1, p - 1 + l, "-" if s else "+")
                         for r, p, l, s in zip(*(np.asarray(c).tolist() for c in cols))))
    return path


def _cols(reads):
    return [np.array(c, dtype=np.int64) for c in zip(*reads)]


def _check(acc, r, refs, want=None, cutoffs=()):
    """The table on the handle of ``acc``'s p-score track against the host path over the same runs and the restatement: the totals,
    the rows whole and in ranges, the cutoffs.  Returns (the track, its QTable, the restated table)."""
    g = acc.signal_result(r)
    assert g.pscore and g.refs == [(n, l) for n, l in refs]
    want = QV.restate(QV.rows_of_runs(g.runs), refs) if want is None else want
    host = g.qvalues()
    tot = acc.qvalue(r)
    assert tuple(tot[k] for k in coverage.QVALUE_TOTALS) == QV.totals(want) == host.totals
    dev = acc.qvalue_result(r)
    m = len(want["table"])
    assert dev == host and QV.table_got(dev.p, dev.bases, dev.q) == QV.table_of(want)
    for first, n in ((0, 0), (m, 0), (0, min(m, 1)), (m // 2, m - m // 2), (max(m - 1, 0), min(m, 1)), (min(255, m), min(3, m - min(255, m)))):
        got = acc.qvalue_rows(r, first, n)
        assert QV.table_got(*got) == QV.table_of(want)[first:first + n]
    for bad in ((-1, 1), (0, m + 1), (m + 1, 0), (1, m), (0, -1)):
        with pytest.raises(PmxIOError, match="pmx_dbam_coverage_qvalue_rows: range outside the rows"):
            acc.qvalue_rows(r, *bad)
    for X in (0.0, -1.0, 1e30, 0.25, 2.0) + tuple(float(q) for _u, _W, q in want["table"][:2] + want["table"][m // 2:m // 2 + 1]) + tuple(x for x, _c in cutoffs):
        assert acc.qvalue_cutoff(r, X) == QV.pcut(want, X) == host.cutoff(X)
    for X, cut in cutoffs:
        assert acc.qvalue_cutoff(r, X) == cut
    return g, host, want


def _peaks(acc, r, g, host, want, args, chunk=1):
    """call with the table on the handle: the lines against ``Peaks.text_chunks`` and the restatement, byte for byte."""
    rules = LC.restate(QV.rows_of_runs(g.runs), *args)
    assert acc.call(r, *args) == LC.totals(rules)
    text = acc.call_text(r)
    assert text == QV.narrowpeak_of(rules, want) == b"".join(g.call(*args, qtable=host).text_chunks()) == b"".join(acc.call_text_chunks(r, chunk))
    p = acc.call_result(r)
    assert p == g.call(*args, qtable=host) and p.qtable == host and b"".join(p.text_chunks()) == text
    return rules, text


@pytest.mark.parametrize("name", QV.SMALL)
def test_the_planted_situations(tmp_path, name):
    refs, t, c, B, a_c, small, large = QV.small_case(name)
    loops = PS.restate(*PS.sums_of(t, c, refs, B), B, a_c, small, large)
    want = QV.restate(LC.rows_of_want(loops), refs)
    QV.check_small(name, want)
    with DeviceBamReader(_bam_of(tmp_path, "t", refs, t)) as r, DeviceBamReader(_bam_of(tmp_path, "c", refs, c)) as rc:
        assert r._L.pmx_dbam_version() >= 23
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        acc.poisson(r, cacc, rc, B, a_c, small, large)
        g, host, _w = _check(acc, r, refs, want, QV.cutoffs(want) if name == "bites" else ())
        assert PS.rows_got(g) == PS.rows_of(loops)
        rules, _text = _peaks(acc, r, g, host, want, (0.0, 0, 1))
        assert rules["n_peaks"] >= 1
        # qvalue twice in a row: the same table, and the peaks are gone until call is made again
        again = acc.qvalue(r)
        assert tuple(again[k] for k in coverage.QVALUE_TOTALS) == QV.totals(want) and acc.qvalue_result(r) == host
        out = np.zeros(8, dtype=np.uint8)
        assert r._L.pmx_dbam_coverage_call_text(r._h, 0, 0, out.ctypes.data, 8) == -3
        _peaks(acc, r, g, host, want, (0.0, 0, 1))


@pytest.mark.parametrize("B", (1, 50))
def test_the_p_score_tracks_planted_pair(tmp_path, B):
    rt, rc_rows = PS.planted_treatment(), PS.planted_control()
    with DeviceBamReader(_bam_of(tmp_path, "t", PS.P_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PS.P_REFS, rc_rows)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        for a_c, small, large in PS.P_SETS[:2] + PS.P_SETS[6:7]:
            loops = PS.restate(*PS.sums_of(rt, rc_rows, PS.P_REFS, B), B, a_c, small, large)
            acc.poisson(r, cacc, rc, B, a_c, small, large)
            g, host, want = _check(acc, r, PS.P_REFS, QV.restate(LC.rows_of_want(loops), PS.P_REFS))
            _peaks(acc, r, g, host, want, (0.5, 0, 50))
        # the lifetime: poisson, qvalue, call: column 9 filled; then compare, call: -1, and the table is gone
        assert all(ln.split(b"\t")[8] != b"-1" for ln in acc.call_text(r).splitlines()) and acc.called["totals"]["peaks"] >= 1
        acc.compare(r, cacc, rc, B)
        acc.call(r, 0.0, 0, 1)
        lines = acc.call_text(r).splitlines()
        assert lines and all(ln.split(b"\t")[7:9] == [b"-1", b"-1"] for ln in lines) and acc.call_result(r).qtable is None
        for fails in (lambda: acc.qvalue_rows(r, 0, 0), lambda: acc.qvalue_cutoff(r, 1.0)):
            with pytest.raises(PmxIOError, match="no table: call pmx_dbam_coverage_qvalue first"):
                fails()


@pytest.mark.parametrize("n", QV.RUN_COUNTS)
def test_the_run_counts_at_the_edges(tmp_path, n):
    refs, t, c, B, a_c, small, large = QV.run_count_case(n)
    names, lengths = [x for x, _l in refs], [l for _x, l in refs]
    with DeviceBedReadsReader(_tag_of(tmp_path, "t", refs, _cols(t)), names, lengths) as r, DeviceBamReader(_bam_of(tmp_path, "c", refs, c)) as rc:
        acc, cacc = coverage.device_count_of(r, 0, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        acc.poisson(r, cacc, rc, B, a_c, small, large)
        g, host, want = _check(acc, r, refs)
        QV.check_run_count(n, want)
        _peaks(acc, r, g, host, want, (0.0, 1, 2), 1000)


@pytest.mark.parametrize("m", QV.DISTINCT_SMALL + QV.DISTINCT_LARGE)
def test_the_distinct_counts_at_the_edges(tmp_path, m):
    refs, t, c, B, a_c, small, large = QV.sawtooth_case(QV.sawtooth_length(m))
    names, lengths = [x for x, _l in refs], [l for _x, l in refs]
    with DeviceBedReadsReader(_tag_of(tmp_path, "t", refs, t), names, lengths) as r, DeviceBedReadsReader(_tag_of(tmp_path, "c", refs, c), names, lengths) as rc:
        acc, cacc = coverage.device_count_of(r, 0, None, 0), coverage.device_count_of(rc, 0, None, 0)
        acc.poisson(r, cacc, rc, B, a_c, small, large)
        g, host, want = _check(acc, r, refs)
        QV.check_distinct(m, want)
        cut = QV.pcut(want, float(want["table"][m // 2][2]))
        rules, _text = _peaks(acc, r, g, host, want, (cut, 0, 1), 100)
        assert rules["n_peaks"] >= 1


def test_more_than_2_32_tests(tmp_path):
    """Three references near 2^31 bases at bin 65536 with reads on one of them: N is above 2^32."""
    top = (1 << 31) - 1
    refs = [("g%d" % i, top) for i in range(3)]
    # k = 36 in bins 0 and 2 (one value, two runs), k = 17 and the spill's k = 0 in bins 1068 and 1069, k = 0 in the control's bin 15258 and
    # in the spill behind it (another l: a run of its own), k = 2 in the short last bin; the control's two places give a tiny l_bg
    t = [(1, 1, 60_000, 0)] * 40 + [(1, 2 * 65536 + 1, 60_000, 0)] * 40 + [(1, 70_000_001, 60_000, 0)] * 20 + [(1, 1_000_000_000, 60_000, 0)] \
        + [(1, top - 60_000, 60_000, 0)] * 3
    c = [(1, 500_000_000, 50, 0)] * 2 + [(1, 1_000_000_000, 50, 0)] * 4
    with DeviceBamReader(_bam_of(tmp_path, "t", refs, sorted(t))) as r, DeviceBamReader(_bam_of(tmp_path, "c", refs, sorted(c))) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        acc.poisson(r, cacc, rc, 65536, 1.0, 0, 0)
        g, host, want = _check(acc, r, refs)
        assert want["tests"] == 3 * top > 1 << 32 and want["n_runs"] == 7 and len(want["table"]) == 4 and list(g.runs) == ["g1"]
        assert want["table"][0][1] == 2 * 65536 and want["table"][-1][1] == 3 * 65536 and QV.bits32(want["table"][-1][0]) == 0
        assert 0 < want["positive"] < want["covered"] == 6 * 65536 + 65535 and want["r"][-1] > 3 * 65536
        _peaks(acc, r, g, host, want, (0.0, 0, 1))


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """coverage_cases' library as every kind of input (the treatment) and a second draw of it as a BAM file (the control)."""
    d = tmp_path_factory.mktemp("gpu_coverage_qvalue")
    rows = CC.synthetic()
    recs = FC.alignment_records(rows, BC.REFS)
    _sam, bam, gz = SW.write_twins(d, "cv", BC.REFS, recs, bgzf_block=60_000)
    tag = str(d / "cv.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, BC.REFS)))
    control = SW.write_twins(d, "input", BC.REFS, FC.alignment_records(CC.synthetic(seed=23, n=9_000), BC.REFS))[1]
    return dict(dir=d, bam=bam, gz=gz, tag=tag, control=control)


def _table_and_lines(acc, reader, case, B=7):
    with DeviceBamReader(case["control"]) as rc:
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 200)
        a_c = coverage.factors_of("none", acc.finish(reader), cacc.finish(rc), [l for _n, l in acc.refs])[1]
        acc.poisson(reader, cacc, rc, B, a_c, 1000, 10000, case["control"])
    g, host, want = _check(acc, reader, BC.REFS)
    X = sorted({float(q) for q in host.q if q > 0})
    assert len(X) >= 3
    cut = acc.qvalue_cutoff(reader, X[len(X) // 2])
    _rules, text = _peaks(acc, reader, g, host, want, (cut, 30, 50))
    assert text.count(b"\n") >= 1
    return host, text


def test_every_reader_makes_the_same_table(case, tmp_path):
    with DeviceBamReader(case["bam"]) as r:
        whole = _table_and_lines(coverage.device_count_of(r, FC.MAPQ, None, 200), r, case)
    with DeviceSamReader(case["gz"]) as r:
        got = _table_and_lines(coverage.device_count_of(r, FC.MAPQ, None, 200), r, case)
        assert got[0] == whole[0] and got[1] == whole[1]
    with DeviceBedReadsReader(case["tag"], BC.NAMES, BC.LENGTHS) as r:
        got = _table_and_lines(coverage.device_count_of(r, FC.MAPQ, None, 200), r, case)
        assert got[0] == whole[0] and got[1] == whole[1]
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = open(case["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    th = threading.Thread(target=writer)
    th.start()
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r:
            acc = r.arm_coverage(FC.MAPQ, None, 200)
            for _ in r._windows():
                pass
            got = _table_and_lines(acc, r, case)
            assert r.stream_info()["windows"] >= 10
    finally:
        th.join(60)
    assert got[0] == whole[0] and got[1] == whole[1]


def test_the_refusals(tmp_path):
    rt, rc_rows = PS.planted_treatment(), PS.planted_control()
    with DeviceBamReader(_bam_of(tmp_path, "t", PS.P_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PS.P_REFS, rc_rows)) as rc:
        L, h, tot = r._L, r._h, np.zeros(4, dtype=np.uint64)
        stem = "pmx_dbam_coverage_qvalue: "

        def fails(rc_, text, code=-3):
            assert rc_ == code
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc_)
        fails(L.pmx_dbam_coverage_qvalue(None, tot.ctypes.data), "null handle")
        fails(L.pmx_dbam_coverage_qvalue(h, tot.ctypes.data), stem + "no signal")              # nothing begun
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        fails(L.pmx_dbam_coverage_qvalue(h, tot.ctypes.data), stem + "no signal")              # runs, no signal
        fails(L.pmx_dbam_coverage_qvalue(h, None), stem + "null output")
        acc.signal(r, 50, 1.0)
        fails(L.pmx_dbam_coverage_qvalue(h, tot.ctypes.data), stem + "the signal is not a p-score track")
        acc.compare(r, cacc, rc, 50)
        fails(L.pmx_dbam_coverage_qvalue(h, tot.ctypes.data), stem + "the signal is not a p-score track")
        with pytest.raises(PmxIOError, match="not a p-score track"):
            acc.qvalue(r)
        three = [np.zeros(4, dtype=t) for t in (np.float32, np.uint64, np.float32)]
        fails(L.pmx_dbam_coverage_qvalue_rows(h, 0, 0, *(x.ctypes.data for x in three)), "pmx_dbam_coverage_qvalue_rows: no table")
        out = np.zeros(1, dtype=np.float64)
        fails(L.pmx_dbam_coverage_qvalue_cutoff(h, 1.0, out.ctypes.data), "pmx_dbam_coverage_qvalue_cutoff: no table")
        acc.poisson(r, cacc, rc, 50)
        assert acc.qvalue(r)["rows"] >= 2
        fails(L.pmx_dbam_coverage_qvalue_rows(h, 0, 1, None, three[1].ctypes.data, three[2].ctypes.data), "pmx_dbam_coverage_qvalue_rows: null output")
        fails(L.pmx_dbam_coverage_qvalue_cutoff(h, 1.0, None), "pmx_dbam_coverage_qvalue_cutoff: null output")
        for bad in (float("nan"), float("inf"), -float("inf")):
            fails(L.pmx_dbam_coverage_qvalue_cutoff(h, bad, out.ctypes.data), "pmx_dbam_coverage_qvalue_cutoff: X is a finite number")
            with pytest.raises(ValueError, match="finite"):
                acc.qvalue_cutoff(r, bad)
        # a treatment without a kept read: an empty p-score track gives an empty table
        none = coverage.device_count_of(rc, 255, None, 0)
        none.poisson(rc, acc, r, 50)
        assert none.qvalue(rc) == dict(rows=0, tests=2660, covered_bases=0, positive_bases=0) and none.qvalue_result(rc) == none.signal_result(rc).qvalues()
        assert none.qvalue_cutoff(rc, 0.0) == 2.0 ** 40 == none.qvalue_cutoff(rc, -1.0) and none.call(rc, 0.0, 0, 1)["peaks"] == 0
        acc.begin(r)                                                                            # a new table: runs, track and q-scores are gone
        fails(L.pmx_dbam_coverage_qvalue(h, tot.ctypes.data), stem + "no signal")
        fails(L.pmx_dbam_coverage_qvalue_cutoff(h, 1.0, out.ctypes.data), "pmx_dbam_coverage_qvalue_cutoff: no table")


def _held(n, m):
    """The bytes qvalue holds at its peak beside the depth runs, for a track of n runs with m distinct values: the signal runs, 40 per
    run, 3072 per tile of 8192 runs, 64, and the table with as much again for the ranks and the raw scores."""
    return 16 * n + 40 * n + 3072 * (-(-n // 8192)) + 64 + 32 * m


def test_the_stream_peak_counts_the_buffers_to_the_byte(tmp_path):
    """A sawtooth pair in which nearly every base is a run of its own value (the control's sawtooth stands on 2048 reads and the
    reference is half as long again, so that l is the control's own depth everywhere): qvalue's buffers outgrow what finish and
    poisson hold, so both peaks are qvalue's, and they differ by exactly what the two calls hold."""
    L = 20_000
    refs = [("s", 30_000)]
    t, c = QV.sawtooth_columns(L, QV.SAW_P), QV.sawtooth_columns(L, QV.SAW_Q, 2048)
    with DeviceStreamReader(_bam_of(tmp_path, "t", refs, list(zip(*(x.tolist() for x in t)))), window_bytes=WINDOW) as r, \
            DeviceBedReadsReader(_tag_of(tmp_path, "c", refs, c), ["s"], [30_000]) as rc:
        acc = r.arm_coverage(FC.MAPQ, None, 0)
        for _ in r._windows():
            pass
        assert acc.finish(r)["runs"] >= L - 30
        cacc = coverage.device_count_of(rc, 0, None, 0)
        peaks, held = [], []
        for B in (2, 1):
            acc.poisson(r, cacc, rc, B, 2.0 ** -8, 0, 0)
            before = r.stream_info()["peak_device_bytes"]
            _g, host, want = _check(acc, r, refs)
            n, m = want["n_runs"], len(want["table"])
            assert n >= L // B - 30 and m >= n * 3 // 4
            peaks.append(r.stream_info()["peak_device_bytes"])
            held.append(_held(n, m))
            assert before < peaks[-1]
        assert peaks[1] - peaks[0] == held[1] - held[0] > 0
        acc.poisson(r, cacc, rc, 50, 2.0 ** -8, 0, 0)       # (fewer runs: the peak stays)
        acc.qvalue(r)
        assert r.stream_info()["peak_device_bytes"] == peaks[1]


def test_the_run_with_the_options(tmp_path):
    from tests.test_coverage_qvalue import R_REFS, _library
    files = []
    for name, rows in (("chip", _library(1, [(0, 5_000, 60), (0, 12_000, 25), (1, 2_000, 12)])), ("input", _library(2, []))):
        files.append(_bam_of(tmp_path, name, R_REFS, rows))
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=None, save_mappability_stats=False, coverage_extend=100, coverage_bin=50,
              coverage_control=files[1], coverage_poisson=True, coverage_call_length=50)
    for i, more in enumerate((dict(coverage_call_q=1.0), dict(coverage_call=2.0, coverage_qvalue=True),
                              dict(coverage_call_q=1.0, coverage_format="bigwig", coverage_compress="device"))):
        _r1, w1 = pipeline.run(files[0], str(tmp_path / ("dev%d" % i)), 120, **more, **kw)
        _r0, w0 = pipeline.run(files[0], str(tmp_path / ("host%d" % i)), 120, device_ingest=False, **dict(more, coverage_compress=bool(more.get("coverage_compress"))), **kw)
        assert [p.name for p in w1[-2:]] == [p.name for p in w0[-2:]] and w1[-1].name == "chip_coverage_peaks.narrowPeak"
        lines = w1[-1].read_bytes()
        assert lines == w0[-1].read_bytes() and lines.count(b"\n") >= 1 and all(ln.split(b"\t")[8] != b"-1" for ln in lines.splitlines())
        if "coverage_call_q" in more:
            assert all(float(ln.split(b"\t")[8]) >= 1.0 - 1e-6 for ln in lines.splitlines())
        if "coverage_format" in more:
            got, want = BC.read_file(w1[-2]), BC.read_file(w0[-2])
            assert got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in want.items() if k != "compressed"}
        else:
            assert w1[-2].read_bytes() == w0[-2].read_bytes()
        assert sorted(os.listdir(tmp_path / ("dev%d" % i))) == sorted(p.name for p in w1)          # (the temporary files are gone)
