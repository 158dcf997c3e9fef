"""Peaks called on the GPU: pmx_dbam_coverage_call, _call_rows and _call_text against the loop restatement of
tests/call_cases and against the host path (``Signal.call``) -- rows, totals and text bytes, exactly: everything is an integer, a
maximum or a first-argmax.  The shapes are the smallest at which the kernels can go wrong: a chain longer than a scan tile, the
maximum either side of a wave's and a workgroup's end, chains across the boundaries of the three lists, the link and length edges,
references side by side, signed tracks, nothing and everything passing, the text in chunks, the table's life on the handle, every
reader, and the run's two files."""
import os
import random
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, peaks, pipeline
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import call_cases as KC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import fragments_cases as FR
from tests import io_writers as W
from tests import sam_writers as SW

pytestmark = pytest.mark.gpu

MAPQ = 10
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"
WINDOW = 512                        # compressed bytes per stream window: the golden file's reads, in small members, make tens of windows


def _bam_of(d, name, refs, reads):
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    return SW.write_twins(d, name, refs, recs)[1]


def _host(reads, refs, extend=0):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), extend)


def _same(acc, r, want, host, args):
    """``call`` on the handle against the restatement ``want`` and the host path's ``Peaks``: totals, rows, text whole and in chunks."""
    assert acc.call(r, *args) == KC.totals(want) == host.totals
    p = acc.call_result(r)
    assert KC.peaks_got(p) == KC.peaks_of(want) and p == host
    assert acc.call_text(r) == KC.text_of(want) == b"".join(acc.call_text_chunks(r, 100)) == b"".join(host.text_chunks())
    return p


@pytest.fixture(scope="module")
def long_chain(tmp_path_factory):
    """The long chain as a file, its restated rows and its host pileup, made once."""
    d = tmp_path_factory.mktemp("gpu_coverage_call")
    return dict(dir=d, bam=_bam_of(d, "long", KC.L_REFS, KC.L_READS), rows=KC.track_rows(KC.L_READS, KC.L_REFS), host=_host(KC.L_READS, KC.L_REFS))


def test_the_edges(tmp_path):
    reads = KC.reads_of(KC.E_TRACK)
    want = KC.restate(KC.track_rows(reads, KC.E_REFS), *KC.E_ARGS)
    KC.check_edges(want)
    c = _host(reads, KC.E_REFS)
    with DeviceBamReader(_bam_of(tmp_path, "edges", KC.E_REFS, reads)) as r:
        assert r._L.pmx_dbam_version() >= 21
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        _same(acc, r, want, c.call(*KC.E_ARGS), KC.E_ARGS)              # no signal yet: the depth through signal(1, 1.0)
        assert acc.sig["bin"] == 1 and acc.sig["scale"] == 1.0
        for args in ((2.0, 10, 51), (2.0, 11, 50), (2.0, 9, 49), (4.0, 0, 1), (2.0, 2 ** 31 - 1, 2 ** 31 - 1), (2.0, 2 ** 31 - 1, 1)):
            _same(acc, r, KC.restate(KC.track_rows(reads, KC.E_REFS), *args), c.call(*args), args)
        acc.signal(r, 1, 0.25)                                          # v == cutoff with the cutoff an exact float32
        quarter = KC.restate(KC.track_rows(reads, KC.E_REFS, 1, 0.25), 0.5, 10, 50)
        assert [x[:4] for x in quarter["peaks"]] == [x[:4] for x in want["peaks"]]
        _same(acc, r, quarter, c.signal(1, 0.25).call(0.5, 10, 50), (0.5, 10, 50))
        for B in (7, 50):                                               # a reference shorter than the bin, one without a run
            acc.signal(r, B, 1.0)
            _same(acc, r, KC.restate(KC.track_rows(reads, KC.E_REFS, B), 1.5, 10, 50), c.signal(B, 1.0).call(1.5, 10, 50), (1.5, 10, 50))


def test_signed_tracks(tmp_path):
    rt, rc_reads = KC.reads_of(KC.S_TREATMENT), KC.reads_of(KC.S_CONTROL)
    want = KC.restate(KC.compared_rows(rt, rc_reads, KC.S_REFS, 1, "subtract"), *KC.S_ARGS)
    KC.check_signed(want)
    t, c = _host(rt, KC.S_REFS), _host(rc_reads, KC.S_REFS)
    with DeviceBamReader(_bam_of(tmp_path, "t", KC.S_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", KC.S_REFS, rc_reads)) as rc:
        acc, cacc = coverage.device_count_of(r, MAPQ, None, 0), coverage.device_count_of(rc, MAPQ, None, 0)
        acc.compare(r, cacc, rc, 1, "subtract")
        _same(acc, r, want, t.compare(c, 1, "subtract").call(*KC.S_ARGS), KC.S_ARGS)
        assert acc.call_text(r).startswith(b"s0\t0\t100\tpeak_1\t0\t.\t-1\t-1\t-1\t25\n")
        # a log2 track at B = 50 with the cutoff 1.0
        acc.compare(r, cacc, rc, 50, "log2", 4.0, 1.0, 1.0)
        rows = KC.compared_rows(rt, rc_reads, KC.S_REFS, 50, "log2", 4.0, 1.0, 1.0)
        w2 = KC.restate(rows, 1.0, 100, 50)
        assert 0 < w2["n_peaks"] and 0 < w2["passing_runs"] < len(rows)
        _same(acc, r, w2, t.compare(c, 50, "log2", 4.0, 1.0, 1.0).call(1.0, 100, 50), (1.0, 100, 50))


@pytest.mark.parametrize("args", KC.L_CASES)
def test_the_long_chain(long_chain, args):
    want = KC.restate(long_chain["rows"], *args)
    KC.check_long(long_chain["rows"], want, args)
    with DeviceBamReader(long_chain["bam"]) as r:
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        _same(acc, r, want, long_chain["host"].call(*args), args)


@pytest.mark.parametrize("at,twice", KC.SUMMITS)
def test_the_summit(tmp_path, at, twice):
    reads = KC.summit_reads(at, twice)
    rows = KC.track_rows(reads, KC.L_REFS)
    want = KC.restate(rows, 2.0, 1, 200)
    KC.check_summit(want, at)
    host = _host(reads, KC.L_REFS)
    with DeviceBamReader(_bam_of(tmp_path, "summit", KC.L_REFS, reads)) as r:
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        _same(acc, r, want, host.call(2.0, 1, 200), (2.0, 1, 200))
        _same(acc, r, KC.restate(rows, 1.0, 0, 200), host.call(1.0, 0, 200), (1.0, 0, 200))     # the same maximum among all the runs


@pytest.mark.parametrize("k,f", KC.BOUNDARIES)
def test_the_boundaries(tmp_path, k, f):
    reads = KC.reads_of(KC.boundary_track(k, f))
    rows = KC.track_rows(reads, KC.B_REFS)
    host = _host(reads, KC.B_REFS)
    with DeviceBamReader(_bam_of(tmp_path, "b", KC.B_REFS, reads)) as r:
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        for args in KC.B_ARGS:
            want = KC.restate(rows, *args)
            KC.check_boundary(want, k, f, args)
            _same(acc, r, want, host.call(*args), args)
        _same(acc, r, KC.restate(rows, 1.0, 1, 1), host.call(1.0, 1, 1), (1.0, 1, 1))       # everything one chain


def test_nothing_everything_and_no_read(tmp_path):
    reads = KC.reads_of(KC.E_TRACK)
    rows = KC.track_rows(reads, KC.E_REFS)
    c = _host(reads, KC.E_REFS)
    zero = dict.fromkeys(coverage.CALL_TOTALS, 0)
    with DeviceBamReader(_bam_of(tmp_path, "edges", KC.E_REFS, reads)) as r:
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        assert acc.call(r, 100.0) == zero and acc.call_result(r) == c.call(100.0) and acc.call_text(r) == b""
        assert list(acc.call_text_chunks(r)) == [] and tuple(x.size for x in acc.call_rows(r)) == (0,) * 6
        out = coverage.write_called(tmp_path / "none", acc.call_text_chunks(r))
        assert out.name == "none_coverage_peaks.narrowPeak" and out.read_bytes() == b""      # an empty file is written
        every = _same(acc, r, KC.restate(rows, -1.0, 0, 1), c.call(-1.0, 0, 1), (-1.0, 0, 1))
        assert every.totals["passing_runs"] == c.n_runs and every.totals["passing_bases"] == c.covered_bases
        none = coverage.device_count_of(r, 255, None, 0)                # a pileup with no kept read
        assert none.finish(r)["reads"] == 0 and none.call(r, 0.0) == zero and none.call_text(r) == b""
        assert none.call_result(r) == _host([], KC.E_REFS).call(0.0)


def test_the_text_in_chunks(tmp_path):
    reads = KC.L_READS[:700]
    rows = KC.track_rows(reads, KC.L_REFS)
    args = (2.0, 0, 1)
    want = KC.restate(rows, *args)
    assert want["n_peaks"] == 699
    with DeviceBamReader(_bam_of(tmp_path, "chunks", KC.L_REFS, reads)) as r:
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        _same(acc, r, want, _host(reads, KC.L_REFS).call(*args), args)
        whole = KC.text_of(want)
        for chunk in (1, 7, 300):
            parts = list(acc.call_text_chunks(r, chunk))
            assert len(parts) == -(-699 // chunk) and b"".join(parts) == whole              # the peak numbers go on across chunks
        assert acc.call_text(r, 698, 1) == KC.text_of(want, 698, 1) and b"\tpeak_699\t" in acc.call_text(r, 698, 1)
        assert acc.call_text(r, 699, 0) == b"" and acc.call_text(r, 10, 0) == b""
        ref, start, end, summit, value, runs = acc.call_rows(r, 5, 3)
        assert [(KC.L_REFS[int(a)][0], int(b), int(c), int(d), int(e), int(f)) for a, b, c, d, e, f
                in zip(ref, start, end, summit, value.view(np.uint32), runs)] == KC.peaks_of(want)[5:8]
        L, h = r._L, r._h
        size = L.pmx_dbam_coverage_call_text(h, 0, 699, None, 0)
        assert size == len(whole)
        buf = np.zeros(size, dtype=np.uint8)
        text, rows = L.pmx_dbam_coverage_call_text, L.pmx_dbam_coverage_call_rows
        for bad, what in ((lambda: text(h, 0, 699, buf.ctypes.data, size - 1), "the buffer is too small: %d bytes are needed" % size),
                          (lambda: text(h, 0, 699, buf.ctypes.data, -1), "a negative capacity"),
                          (lambda: text(h, 0, 700, None, 0), "range outside the peaks"),
                          (lambda: text(h, 700, 0, None, 0), "range outside the peaks"),
                          (lambda: text(h, -1, 1, None, 0), "range outside the peaks"),
                          (lambda: rows(h, 698, 2, *([buf.ctypes.data] * 6)), "range outside the peaks"),
                          (lambda: rows(h, 0, 1, None, *([buf.ctypes.data] * 5)), "null output")):
            rc_ = bad()                                     # (the message is the last failure's: one call at a time)
            assert rc_ == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_coverage_call_(text|rows): " + what):
                r._raise(rc_)
        assert L.pmx_dbam_coverage_call_text(h, 0, 699, buf.ctypes.data, size) == size and buf.tobytes() == whole


@pytest.mark.parametrize("kind", ["depth", "signal", "peaks", "p-score peaks", "p- and q-score peaks"])
def test_pulls_of_lines_from_the_fourth_on(tmp_path, kind):
    """Every kind of line through the one line writer: pulls that end on lane 63, on a workgroup's edge and in the third workgroup,
    over two references whose names have 1 and 12 characters, against the same lines of the host path's text."""
    c = _host(CC.OUT_READS, CC.OUT_REFS)
    with DeviceBamReader(_bam_of(tmp_path, "t", CC.OUT_REFS, CC.OUT_READS)) as r, \
            DeviceBamReader(_bam_of(tmp_path, "c", CC.OUT_REFS, [(1, 2301, 40, 0)])) as rc:
        acc = coverage.device_count_of(r, MAPQ, None, 0)
        if kind == "depth":
            assert acc.finish(r)["runs"] == CC.OUT_SHORT + CC.OUT_LONG
            return CC.check_line_pulls(lambda first, n: acc.text(r, first, n), b"".join(c.text_chunks()))
        if kind == "signal":
            acc.signal(r, 1, 0.37)
            return CC.check_line_pulls(lambda first, n: acc.text(r, first, n, signal=True), b"".join(c.signal(1, 0.37).text_chunks()))
        if kind == "peaks":                                 # every run a peak: peak_9 / peak_10 and peak_99 / peak_100 inside the pulls
            acc.signal(r, 1, 0.37)
            acc.call(r, 0.3, 0, 1)
            whole = b"".join(c.signal(1, 0.37).call(0.3, 0, 1).text_chunks())
            assert all(ln.split(b"\t")[7:9] == [b"-1", b"-1"] for ln in whole.splitlines())
        else:                                               # column 8, and with the table column 9, are a value's text as well
            acc.poisson(r, coverage.device_count_of(rc, MAPQ, None, 0), rc, 1, 1.0, 0, 0)
            g = acc.signal_result(r)
            table = g.qvalues() if kind == "p- and q-score peaks" else None
            if table is not None:
                acc.qvalue(r)
            acc.call(r, 0.0, 0, 1)
            whole = b"".join(g.call(0.0, 0, 1, qtable=table).text_chunks())
            assert all((ln.split(b"\t")[7] != b"-1") and (ln.split(b"\t")[8] == b"-1") == (table is None) for ln in whole.splitlines())
        assert whole.splitlines()[8].split(b"\t")[3] == b"peak_9" and whole.splitlines()[99].split(b"\t")[3] == b"peak_100"
        CC.check_line_pulls(lambda first, n: acc.call_text(r, first, n), whole)


def test_the_tables_life_on_the_handle(tmp_path):
    reads = KC.reads_of(KC.E_TRACK)
    c = _host(reads, KC.E_REFS)
    with DeviceBamReader(_bam_of(tmp_path, "edges", KC.E_REFS, reads)) as r:
        L, h, tot = r._L, r._h, np.zeros(5, dtype=np.uint64)
        six = [np.zeros(8, dtype=np.uint32) for _ in range(6)]

        def fails(rc_, text):
            assert rc_ == -3
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc_)

        def call(cutoff=2.0, gap=10, length=50, out=tot):
            return L.pmx_dbam_coverage_call(h, cutoff, gap, length, None if out is None else out.ctypes.data)

        def pull():
            return L.pmx_dbam_coverage_call_rows(h, 0, 0, *(x.ctypes.data for x in six))
        no_signal = "pmx_dbam_coverage_call: no signal: call pmx_dbam_coverage_signal or pmx_dbam_coverage_compare first"
        fails(call(), no_signal)                                        # nothing begun
        acc = coverage.DeviceCount(r, MAPQ, None, 0)
        acc.add(r)
        fails(call(), no_signal)                                        # a table
        acc.finish(r)
        fails(call(), no_signal)                                        # runs, but no signal
        fails(pull(), "pmx_dbam_coverage_call_rows: no peaks: call pmx_dbam_coverage_call first")
        fails(L.pmx_dbam_coverage_call(None, 2.0, 10, 50, tot.ctypes.data), "null handle")
        depth_text = acc.text(r)
        acc.signal(r, 1, 0.5)
        signal_text = acc.text(r, signal=True)
        fails(call(out=None), "pmx_dbam_coverage_call: null output")
        for bad in (float("nan"), float("inf"), -float("inf")):
            fails(call(cutoff=bad), "pmx_dbam_coverage_call: the cutoff is a finite number")
        fails(call(gap=2 ** 31), "pmx_dbam_coverage_call: max_gap is 0 to 2\\^31 - 1")
        for bad in (0, 2 ** 31):
            fails(call(length=bad), "pmx_dbam_coverage_call: min_length is 1 to 2\\^31 - 1")
        fails(pull(), "no peaks")                                       # a refused call leaves no table ...
        assert acc.text(r, signal=True) == signal_text                  # ... and the signal usable
        assert call(1.0) == 0 and tot.tolist() == list(c.signal(1, 0.5).call(1.0, 10, 50).totals.values()) and pull() == 0
        first = acc.call(r, 1.0, 10, 50)
        fails(call(length=0), "min_length")                             # refused after a call: the table is dropped by the next call only
        assert pull() == 0 and acc.call_result(r) == c.signal(1, 0.5).call(1.0, 10, 50)
        second = acc.call(r, 1.5, 0, 1)                                 # call twice: the table is replaced
        assert second != first and acc.call_result(r) == c.signal(1, 0.5).call(1.5, 0, 1)
        assert acc.text(r) == depth_text and acc.text(r, signal=True) == signal_text and acc.result(r) == c     # nothing else changed
        acc.signal(r, 1, 0.5)                                           # a new signal: the peaks are gone
        fails(pull(), "no peaks")
        fails(L.pmx_dbam_coverage_call_text(h, 0, 0, None, 0), "pmx_dbam_coverage_call_text: no peaks")
        with pytest.raises(ValueError, match="no peaks"):
            acc.call_rows(r)
        acc.call(r, 1.0, 10, 50)
        acc.compare(r, acc, r, 1, "subtract")                           # a compared track: gone as well
        fails(pull(), "no peaks")
        acc.call(r, -1.0, 10, 50)
        acc.begin(r)                                                    # a new table: runs, track and peaks are gone
        fails(pull(), "no peaks")
        fails(call(), no_signal)


def test_the_stream_peak_counts_the_table(tmp_path):
    """One reference of 4000 bases with every second base a peak: the signal's runs outweigh what finish held, so the stream's peak
    is set by the handle's bytes from there on, and call raises it by exactly what it holds at its fullest: 64 bytes, 12 per 256
    signal runs, 4 per passing run, candidate and peak, and the table of 24 bytes per peak."""
    refs = [("tiny", 4000)]
    dense = [(0, 1 + 2 * k, 3, 0) for k in range(1998)]
    with DeviceStreamReader(_bam_of(tmp_path, "dense", refs, dense), window_bytes=WINDOW) as r:
        acc = r.arm_coverage(MAPQ, None, 0)
        for _ in r._windows():
            pass
        runs = acc.finish(r)["runs"]
        before = r.stream_info()["peak_device_bytes"]
        acc.signal(r, 1, 1.0)
        mid = r.stream_info()["peak_device_bytes"]
        assert runs == 3995 and mid > before
        tot = acc.call(r, 2.0, 0, 1)
        after = r.stream_info()["peak_device_bytes"]
        assert (tot["passing_runs"], tot["candidates"], tot["peaks"]) == (1997, 1997, 1997)
        assert after - mid == 64 + 12 * -(-runs // 256) + 4 * 3 * 1997 + 24 * 1997
        assert acc.call_result(r) == _host(dense, refs).call(2.0, 0, 1)
        acc.call(r, 2.0, 0, 1)                              # again: the first table is dropped before the second is made
        assert r.stream_info()["peak_device_bytes"] == after


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    """The golden file's kept reads as SAM.gz and tagAlign beside the file itself, and the host path's peaks of its log2 track
    against every third read moved 17 bases on."""
    d = tmp_path_factory.mktemp("gpu_coverage_call_golden")
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(MAPQ))]
    rows = [(int(r), int(p), int(l), int(s)) for r, p, l, s in zip(*cols)]
    recs = [SW.rec("t%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(rows)]
    gz = SW.write_twins(d, "golden", refs, recs, bgzf_block=20_000)[2]
    small = str(d / "golden_small.bam")                     # BGZF members of 2000 bytes: the stream reader's windows hold a few each
    W.write_bam(small, refs, SW.bam_bytes(refs, recs), block=2000, text=SW.sam_header(refs))
    tag = str(d / "golden.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join("{}\t{}\t{}\tN\t40\t{}\n".format(refs[r][0], p - 1, p - 1 + l, "-" if s else "+") for r, p, l, s in rows))
    crow = [(r, p + 17, l, s) for r, p, l, s in rows[::3] if p + 17 + l <= refs[r][1]]
    crec = [SW.rec("c%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(crow)]
    control = SW.write_twins(d, "input", refs, crec)[1]
    names, lengths = [n for n, _l in refs], [l for _n, l in refs]
    t = coverage.count_host(*cols, names, lengths, [1] * len(refs), 200)
    return dict(dir=d, refs=refs, names=names, lengths=lengths, gz=gz, tag=tag, small=small, control=control, t=t, c=_host(crow, refs, 200), rows=rows, crow=crow)


def _golden_peaks(reader, golden, references=None):
    """(the depth's peaks, the cpm track's at bin 50, the log2 track's at bin 50) of a device reader, with their texts."""
    out = []
    with DeviceBamReader(golden["control"]) as rc:
        acc = coverage.device_count_of(reader, MAPQ, references, 200)
        cacc = coverage.device_count_of(rc, MAPQ, references, 200)
        acc.call(reader, 3.0)
        out.append((acc.call_result(reader), acc.call_text(reader)))
        acc.signal(reader, 50, 1e6 / acc.finish(reader)["reads"], "cpm")
        acc.call(reader, 100.0, 100, 150)
        out.append((acc.call_result(reader), acc.call_text(reader)))
        acc.compare(reader, cacc, rc, 50, "log2", 1.0, acc.finish(reader)["reads"] / cacc.finish(rc)["reads"], 1.0)
        acc.call(reader, 1.0)
        out.append((acc.call_result(reader), acc.call_text(reader)))
    return out


def test_every_reader_makes_the_host_paths_peaks(golden, tmp_path):
    t, c = golden["t"], golden["c"]
    host = [t.call(3.0), t.signal(50, 1e6 / t.reads, "cpm").call(100.0, 100, 150), t.compare(c, 50, "log2", 1.0, t.reads / c.reads, 1.0).call(1.0)]
    want = [(p, b"".join(p.text_chunks())) for p in host]
    assert all(p.n_peaks > 1 for p in host)
    with DeviceBamReader(GOLDEN_BAM) as r:
        assert _golden_peaks(r, golden) == want
    with DeviceBamReader(GOLDEN_BAM, references=["chr1", "chr3"]) as r:
        assert r.indexed
        assert _golden_peaks(r, golden, ["chr1", "chr3"]) == want       # (every read of the file is on chr1)
    with DeviceSamReader(golden["gz"]) as r:
        assert _golden_peaks(r, golden) == want
    with DeviceBedReadsReader(golden["tag"], golden["names"], golden["lengths"]) as r:
        assert _golden_peaks(r, golden) == want
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = open(golden["small"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    th = threading.Thread(target=writer)
    th.start()
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r:
            acc = r.arm_coverage(MAPQ, None, 200)
            for _ in r._windows():
                pass
            acc.call(r, 3.0)
            streamed = acc.call_result(r), acc.call_text(r)
            assert r.stream_info()["windows"] >= 10
    finally:
        th.join(60)
    assert streamed == want[0]


def test_the_run_writes_both_files(golden, tmp_path):
    t, c, control = golden["t"], golden["c"], golden["control"]
    kw = dict(read_len=36, mapq_criteria=MAPQ, mappability_path=None, save_mappability_stats=False, coverage_extend=200)
    names = [STEM + "_coverage.bedGraph", STEM + "_coverage_peaks.narrowPeak"]
    # the depth: the coverage file as ever, the peaks through signal(1, 1.0); equal to the host run's two files
    _r, w = pipeline.run(GOLDEN_BAM, str(tmp_path / "depth"), 300, coverage_call=3, **kw)
    _r, wh = pipeline.run(GOLDEN_BAM, str(tmp_path / "depth_host"), 300, coverage_call=3, device_ingest=False, **kw)
    assert [p.name for p in w[-2:]] == names == [p.name for p in wh[-2:]] and [p.read_bytes() for p in w[-2:]] == [p.read_bytes() for p in wh[-2:]]
    assert w[-2].read_bytes() == coverage.write_coverage(tmp_path / "host", STEM, t).read_bytes()
    assert w[-1].read_bytes() == b"".join(t.call(3.0).text_chunks()) and sorted(os.listdir(tmp_path / "depth")) == sorted(p.name for p in w)
    got = peaks.open_peaks(str(w[-1]), True)                            # --peaks takes the file, on the device too
    assert {n: [x.tolist() for x in v] for n, v in got.lines.items()} == {n: [list(x) for x in zip(*v)] for n, v in t.call(3.0).lines().items()}
    # the signal track as a bigWig file, plain and compressed on the device
    g = t.signal(50, 1e6 / t.reads, "cpm")
    more = dict(coverage_bin=50, coverage_normalize="cpm", coverage_call=100.0, coverage_call_gap=100, coverage_call_length=150, coverage_format="bigwig")
    _r, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "bw"), 300, **more, **kw)
    assert [p.name for p in w2[-2:]] == [STEM + "_coverage.bw", names[1]]
    assert w2[-2].read_bytes() == coverage.write_bigwig(tmp_path / "host", STEM, g).read_bytes()
    assert w2[-1].read_bytes() == b"".join(g.call(100.0, 100, 150).text_chunks())
    _r, w3 = pipeline.run(GOLDEN_BAM, str(tmp_path / "z"), 300, coverage_compress="device", **more, **kw)
    assert w3[-1].read_bytes() == w2[-1].read_bytes() and 0 < w3[-2].stat().st_size < w2[-2].stat().st_size
    assert sorted(os.listdir(tmp_path / "z")) == sorted(p.name for p in w3)                 # (the temporary files are gone)
    # against a control, through run_files
    out = pipeline.run_files([GOLDEN_BAM], str(tmp_path / "log2"), 300, coverage_control=control, coverage_bin=50, coverage_call=1.0, **kw)
    g3 = t.compare(c, 50, "log2", 1.0, t.reads / c.reads, 1.0, "none", control)
    assert out[0].error is None and [p.name for p in out[0].written[-2:]] == names
    assert out[0].written[-2].read_bytes() == coverage.write_coverage(tmp_path / "host", STEM, g3).read_bytes()
    assert out[0].written[-1].read_bytes() == b"".join(g3.call(1.0).text_chunks())
    # "auto": on one more read of the file, with the run's own estimate
    _r, w4 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage_call=3, stats=True, **dict(kw, coverage_extend="auto"))
    table = dict(ln.rstrip("\n").split("\t") for ln in open(w4[-3]))
    extend = int(table["Estimated library length"])
    cols = [np.array(x, dtype=np.int64) for x in zip(*golden["rows"])]
    t4 = coverage.count_host(*cols, golden["names"], golden["lengths"], [1] * len(golden["refs"]), extend)
    assert [p.name for p in w4[-2:]] == names and w4[-2].read_bytes() == coverage.write_coverage(tmp_path / "host4", STEM, t4).read_bytes()
    assert w4[-1].read_bytes() == b"".join(t4.call(3.0).text_chunks())


def test_the_run_on_the_pair_pileup(tmp_path):
    recs = [r for _l, r in FR.planted()] + FR.random_pairs(random.Random(3), 3000)
    recs = [r for _i, r in sorted(enumerate(recs), key=lambda x: (x[1].ref < 0, x[1].ref, x[1].pos0, x[0]))]
    bam = str(tmp_path / "pe.bam")
    FR.write_bam(bam, recs)
    with BamReader(bam) as h:
        t = coverage.from_reader(h, FR.MAPQ, None, "pair", 2000)
    p = t.call(2.0, 50, 100)
    assert p.n_peaks > 3
    kw = dict(read_len=36, mapq_criteria=FR.MAPQ, mappability_path=None, save_mappability_stats=False)
    _r, w = pipeline.run(bam, str(tmp_path / "pair"), 300, coverage_extend="pair", coverage_call=2.0, coverage_call_gap=50, coverage_call_length=100, **kw)
    assert w[-2].read_bytes() == coverage.write_coverage(tmp_path / "host", "pe", t).read_bytes()
    assert w[-1].name == "pe_coverage_peaks.narrowPeak" and w[-1].read_bytes() == b"".join(p.text_chunks())
