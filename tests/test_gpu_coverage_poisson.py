"""The p-score track on the GPU: pmx_dbam_coverage_poisson and the signal consumers over its runs against the loop
restatement of tests/poisson_cases and against the host path -- runs, totals, text bytes and the whole bigWig file with compression
off, byte for byte: everything is an integer or has one stated order.  The treatment through every device reader, a stream window
by window, poisson, signal and compare in turn on one pileup with the p-score flag following, the peaks with column 8 filled, a
pileup against itself, the compressed doors, the long series beside short ones in one wave, the new scan's edges, the error paths,
the stream's peak to the byte and up to the run's files."""
import os
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, pipeline
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bigwig_out_cases as BC
from tests import call_cases as LC
from tests import compare_cases as PC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import io_writers as W
from tests import poisson_cases as PS
from tests import sam_writers as SW
from tests import signal_cases as SC

pytestmark = pytest.mark.gpu

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """coverage_cases' library under the renamed references of bigwig_out_cases as every kind of input (the treatment), and a second
    draw of it as a BAM file (the control)."""
    d = tmp_path_factory.mktemp("gpu_coverage_poisson")
    rows = CC.synthetic()
    recs = FC.alignment_records(rows, BC.REFS)
    _sam, bam, gz = SW.write_twins(d, "cv", BC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(BC.NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, BC.REFS, SW.bam_bytes(BC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "cv.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, BC.REFS)))
    crows = CC.synthetic(seed=23, n=9_000)
    control = SW.write_twins(d, "input", BC.REFS, FC.alignment_records(crows, BC.REFS))[1]
    return dict(dir=d, bam=bam, gz=gz, indexed=indexed, tag=tag, control=control, t=FC.kept(rows), c=FC.kept(crows), pile={}, sums={})


def _host_count(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


def _pile(case, which, extend, use="all"):
    """(the host pileup, the per-base depth lists of the restated runs), computed once per parameter set and left unchanged."""
    key = which, extend, use
    if key not in case["pile"]:
        want = CC.restate(case[which], BC.REFS, CC.USES[use], extend)
        case["pile"][key] = _host_count(case[which], BC.REFS, CC.USES[use], extend), BC.depth_lists(want, BC.REFS, CC.USES[use])
    return case["pile"][key]


def _sums(case, which, extend, B):
    if (which, extend, B) not in case["sums"]:
        case["sums"][which, extend, B] = SC.bin_sums(_pile(case, which, extend)[1], B)
    return case["sums"][which, extend, B]


def _a_c(t, c):
    return coverage.factors_of("none", dict(zip(coverage.TOTALS, t.totals)), dict(zip(coverage.TOTALS, c.totals)), [l for _n, l in t.refs])[1]


def _totals(tot):
    return tuple(tot[k] for k in coverage.SIGNAL_TOTALS)


@pytest.mark.parametrize("B", PS.BINS)
@pytest.mark.parametrize("extend", [0, 200])
def test_the_device_against_the_restatement(case, tmp_path, extend, B):
    t, c = _pile(case, "t", extend)[0], _pile(case, "c", extend)[0]
    a_c = _a_c(t, c)
    assert a_c == t.reads / c.reads != 1.0
    with DeviceBamReader(case["bam"]) as r, DeviceBamReader(case["control"]) as rc:
        assert r._L.pmx_dbam_version() >= 22
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, extend), coverage.device_count_of(rc, FC.MAPQ, None, extend)
        for small, large in (PS.WINDOWS, (120, 0)):
            want = PS.restate(_sums(case, "t", extend, B), _sums(case, "c", extend, B), B, a_c, small, large)
            assert _totals(acc.poisson(r, cacc, rc, B, a_c, small, large, case["control"])) == PS.totals(want)
            g = acc.signal_result(r)
            host = t.poisson(c, B, a_c, small, large, case["control"])
            assert PS.rows_got(g) == PS.rows_of(want) and g == host and g.tail == host.tail and g.pscore
            assert acc.text(r, signal=True) == PS.text_of(want) == b"".join(acc.text_chunks(r, 1000, signal=True))
            assert want["max"] > 0.5 and want["min"] == 0.0
            assert coverage.write_coverage(tmp_path / "dev", "dev", acc, r, signal=True).read_bytes() == \
                coverage.write_coverage(tmp_path / "host", "dev", host).read_bytes()
        dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r, signal=True)       # the whole file, once per bin
        assert dev.read_bytes() == coverage.write_bigwig(tmp_path / "host", "host", host).read_bytes()
        PS.check_file(BC.read_file(dev), want, BC.REFS, B)
        assert acc.result(r) == t and cacc.result(rc) == c  # the depth runs of both stay as they are


def _pull(acc, reader, cacc, rc, case, base, B, windows):
    a_c = coverage.factors_of("none", acc.finish(reader), cacc.finish(rc), [l for _n, l in acc.refs])[1]
    tot = acc.poisson(reader, cacc, rc, B, a_c, *windows, case["control"])
    track = coverage.write_coverage(base, "dev", acc, reader, signal=True).read_bytes()
    return track, coverage.write_bigwig(base, "dev", acc, reader, signal=True).read_bytes(), _totals(tot)


def _poisson_files(reader, case, base, extend, B, windows, references=None):
    """(text, file bytes, totals) of the device's p-score track of ``reader`` against the control file."""
    with DeviceBamReader(case["control"]) as rc:
        acc, cacc = coverage.device_count_of(reader, FC.MAPQ, references, extend), coverage.device_count_of(rc, FC.MAPQ, references, extend)
        return _pull(acc, reader, cacc, rc, case, base, B, windows)


def _host_files(t, c, case, base, B, windows):
    g = t.poisson(c, B, _a_c(t, c), *windows, case["control"])
    return coverage.write_coverage(base, "dev", g).read_bytes(), coverage.write_bigwig(base, "dev", g).read_bytes(), g.totals


@pytest.mark.parametrize("extend,B,windows", [(0, 50, PS.WINDOWS), (200, 7, (0, 3000))])
def test_every_reader_makes_the_host_paths_track(case, tmp_path, extend, B, windows):
    whole = _host_files(_pile(case, "t", extend)[0], _pile(case, "c", extend)[0], case, tmp_path / "host", B, windows)
    assert b" control=input.bam poisson=%d,%d\n" % windows in whole[0][:400] and whole[2][0] > 500 and whole[2][3] > 0.5
    with DeviceBamReader(case["bam"]) as r:
        assert _poisson_files(r, case, tmp_path / "bam", extend, B, windows) == whole
    with DeviceSamReader(case["gz"]) as r:
        assert _poisson_files(r, case, tmp_path / "gz", extend, B, windows) == whole
    with DeviceBedReadsReader(case["tag"], BC.NAMES, BC.LENGTHS) as r:
        assert _poisson_files(r, case, tmp_path / "tag", extend, B, windows) == whole
    chosen = [n for n, u in zip(BC.NAMES, CC.USES["no middle"]) if u]
    with DeviceBamReader(case["indexed"], references=chosen) as r:
        assert r.indexed
        part = _poisson_files(r, case, tmp_path / "indexed", extend, B, windows, chosen)
    assert part == _host_files(_pile(case, "t", extend, "no middle")[0], _pile(case, "c", extend, "no middle")[0], case, tmp_path / "host2", B, windows)
    assert part != whole                                    # (other chosen lengths: another background)
    # a FIFO cut into windows
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = open(case["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    th = threading.Thread(target=writer)
    th.start()
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r, DeviceBamReader(case["control"]) as rc:
            acc = r.arm_coverage(FC.MAPQ, None, extend)
            for _ in r._windows():
                pass
            streamed = _pull(acc, r, coverage.device_count_of(rc, FC.MAPQ, None, extend), rc, case, tmp_path / "fifo_out", B, windows)
            assert r.stream_info()["windows"] >= 10
    finally:
        th.join(60)
    assert streamed == whole


def _bam_of(d, name, refs, reads):
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    return SW.write_twins(d, name, refs, recs)[1]


def _want(rt, rc, refs, B, a_c, small, large):
    return PS.restate(*PS.sums_of(rt, rc, refs, B), B, a_c, small, large)


@pytest.mark.parametrize("a_c,small,large", PS.P_SETS)
def test_the_planted_situations(tmp_path, a_c, small, large):
    rt, rc_rows = PS.planted_treatment(), PS.planted_control()
    want = _want(rt, rc_rows, PS.P_REFS, PS.P_B, a_c, small, large)
    PS.check_planted(want, a_c, small, large)
    kw = dict(items_per_section=2, index_block=2, zoom_base=PS.P_ZOOM)
    with DeviceBamReader(_bam_of(tmp_path, "t", PS.P_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PS.P_REFS, rc_rows)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert _totals(acc.poisson(r, cacc, rc, PS.P_B, a_c, small, large)) == PS.totals(want)
        assert PS.rows_got(acc.signal_result(r)) == PS.rows_of(want) and acc.text(r, signal=True) == PS.text_of(want)
        got = BC.read_file(coverage.write_bigwig(tmp_path / "p", "p", acc, r, signal=True, **kw), 2)
        PS.check_file(got, want, PS.P_REFS, PS.P_B, PS.P_ZOOM, 2)
        # the compressed doors: the file decodes to the same sections
        z = BC.read_file(coverage.write_bigwig(tmp_path / "z", "p", acc, r, compress="device", signal=True, **kw), 2)
        assert z["compressed"] and {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in got.items() if k != "compressed"}
        # the peaks of the p-score track: column 8 holds the value
        args = (0.5, 0, 50)
        rules = LC.restate(LC.rows_of_want(want), *args)
        assert acc.call(r, *args) == LC.totals(rules) and acc.call_text(r) == PS.narrowpeak_of(rules) == b"".join(acc.call_text_chunks(r, 1))
        p = acc.call_result(r)
        assert p.pscore and LC.peaks_got(p) == LC.peaks_of(rules) and b"".join(p.text_chunks()) == acc.call_text(r)
        assert rules["n_peaks"] >= 1
        # poisson, then signal, then poisson, then compare on one pileup: each replaces the one before, and the flag follows
        depths = BC.depth_lists(CC.restate(rt, PS.P_REFS, [1] * 4, 0), PS.P_REFS, [1] * 4)
        plain = SC.restate(SC.bin_sums(depths, 7), 0.37)
        assert _totals(acc.signal(r, 7, 0.37)) == SC.totals(plain) and acc.text(r, signal=True) == SC.text_of(plain)
        flat = LC.restate(LC.rows_of_want(plain), 0.0, 0, 1)
        assert acc.call(r, 0.0, 0, 1) == LC.totals(flat) and acc.call_text(r) == LC.text_of(flat) and flat["n_peaks"] >= 4      # -1 again
        for B in (1, 7, 65536):
            other = _want(rt, rc_rows, PS.P_REFS, B, a_c, small, large)
            assert _totals(acc.poisson(r, cacc, rc, B, a_c, small, large)) == PS.totals(other)
            assert PS.rows_got(acc.signal_result(r)) == PS.rows_of(other) and acc.text(r, signal=True) == PS.text_of(other)
        rules = LC.restate(LC.rows_of_want(other), 0.0, 0, 1)
        assert acc.call(r, 0.0, 0, 1) == LC.totals(rules) and acc.call_text(r) == PS.narrowpeak_of(rules)
        log2 = PC.restate(*PS.sums_of(rt, rc_rows, PS.P_REFS, PS.P_B), "log2", 1.0, 1.0, 1.0)
        assert _totals(acc.compare(r, cacc, rc, PS.P_B)) == PC.totals(log2) and acc.text(r, signal=True) == PC.text_of(log2)
        rules = LC.restate(LC.rows_of_want(log2), 0.0, 0, 1)
        assert acc.call(r, 0.0, 0, 1) == LC.totals(rules) and acc.call_text(r) == LC.text_of(rules) and not acc.call_result(r).pscore   # after compare: -1
        # the other way round: the control's handle takes the track, the treatment's keeps its own
        back = _want(rc_rows, rt, PS.P_REFS, PS.P_B, a_c, small, large)
        assert _totals(cacc.poisson(rc, acc, r, PS.P_B, a_c, small, large)) == PS.totals(back) and cacc.text(rc, signal=True) == PS.text_of(back)
        assert acc.text(r, signal=True) == PC.text_of(log2)
        # a pileup against itself: c == b
        mine = _want(rt, rt, PS.P_REFS, PS.P_B, a_c, small, large)
        assert _totals(acc.poisson(r, acc, r, PS.P_B, a_c, small, large)) == PS.totals(mine) and acc.text(r, signal=True) == PS.text_of(mine)
        assert acc.text(r) == CC.text_of(CC.restate(rt, PS.P_REFS, [1] * 4, 0))


def test_a_reference_with_reads_in_one_file_only(tmp_path):
    rt, lone = PS.planted_treatment(), PS.planted_lonely()
    want, back = _want(rt, lone, PS.P_REFS, PS.P_B, 1.0, *PS.P_WINDOWS), _want(lone, rt, PS.P_REFS, PS.P_B, 1.0, *PS.P_WINDOWS)
    assert list(want["runs"]) == ["p0", "p1", "p2", "p3"] and list(back["runs"]) == ["p1"]
    with DeviceBamReader(_bam_of(tmp_path, "t", PS.P_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PS.P_REFS, lone)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert _totals(acc.poisson(r, cacc, rc, PS.P_B, 1.0, *PS.P_WINDOWS)) == PS.totals(want) and PS.rows_got(acc.signal_result(r)) == PS.rows_of(want)
        assert _totals(cacc.poisson(rc, acc, r, PS.P_B, 1.0, *PS.P_WINDOWS)) == PS.totals(back) and PS.rows_got(cacc.signal_result(rc)) == PS.rows_of(back)
        # a treatment without a kept read: an empty track, which is still a p-score track
        none = coverage.device_count_of(rc, 255, None, 0)
        assert none.finish(rc)["reads"] == 0
        assert _totals(none.poisson(rc, acc, r, PS.P_B)) == (0, 0, 0.0, 0.0) and none.text(rc, signal=True) == b"" and none.signal_result(rc).pscore
        assert none.ranges(rc, signal=True).tolist() == [0] * 5


def test_a_long_series_beside_short_ones_in_one_wave(tmp_path):
    rt, rc_rows = PS.deep_treatment(), PS.deep_control()
    want = _want(rt, rc_rows, PS.D_REFS, PS.D_B, 1.0, 0, 0)
    PS.check_deep(want)
    with DeviceBamReader(_bam_of(tmp_path, "t", PS.D_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PS.D_REFS, rc_rows)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert acc.finish(r)["max_depth"] == PS.D_DEPTH + 1         # k = max_depth_t: the last entry of F
        assert _totals(acc.poisson(r, cacc, rc, PS.D_B, 1.0, 0, 0)) == PS.totals(want)
        assert PS.rows_got(acc.signal_result(r)) == PS.rows_of(want) and acc.text(r, signal=True) == PS.text_of(want)


@pytest.mark.parametrize("n", PS.SCAN_SMALL + PS.SCAN_LARGE)
def test_the_edges_of_the_scan(tmp_path, n):
    rt, rc_rows = PS.scan_reads(n)
    refs = [("s", n)]
    want = _want(rt, rc_rows, refs, 1, 1.0, *PS.SCAN_WINDOWS)
    with DeviceBamReader(_bam_of(tmp_path, "t", refs, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", refs, rc_rows)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert _totals(acc.poisson(r, cacc, rc, 1, 1.0, *PS.SCAN_WINDOWS)) == PS.totals(want)
        assert PS.rows_got(acc.signal_result(r)) == PS.rows_of(want) and want["n_runs"] >= 1
        if n > 1000:                                        # the table behind a first reference, too: every base of the prefix moves
            host = _host_count(rt, refs, [1], 0).poisson(_host_count(rc_rows, refs, [1], 0), 3, 0.7, 9, 0)
            assert _totals(acc.poisson(r, cacc, rc, 3, 0.7, 9, 0)) == host.totals and acc.signal_result(r) == host


def test_the_error_paths(tmp_path):
    rt = PS.planted_treatment()
    bam = _bam_of(tmp_path, "t", PS.P_REFS, rt)
    other = _bam_of(tmp_path, "o", [(n, l + 1) for n, l in PS.P_REFS], rt)
    fewer = _bam_of(tmp_path, "f", PS.P_REFS[:3], [x for x in rt if x[0] < 3])
    deep = _bam_of(tmp_path, "d", PS.P_REFS, [(0, 1, 36, 0)] * 1024)
    tag = str(tmp_path / "pile.tagAlign")
    with open(tag, "w") as fp:
        fp.write("p0\t0\t36\tN\t1000\t+\n" * ((1 << 20) + 1))
    F = np.ascontiguousarray(coverage.lnfact(64))
    with DeviceBamReader(bam) as r, DeviceBamReader(bam) as rc, DeviceBamReader(other) as ro, DeviceBamReader(fewer) as rf, DeviceBamReader(deep) as rd:
        L, h, tot = r._L, r._h, np.zeros(4, dtype=np.float64)
        stem = "pmx_dbam_coverage_poisson: "

        def fails(rc_, text, code=-3):
            assert rc_ == code
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc_)

        def call(hc, B=50, a_c=1.0, small=1000, large=10000, n=F.size, hb=None, out=tot, table=F):
            return L.pmx_dbam_coverage_poisson(hb or h, hc, B, a_c, small, large, None if table is None else table.ctypes.data, n,
                                               None if out is None else out.ctypes.data)
        fails(call(rc._h), stem + "no runs: call pmx_dbam_coverage_finish first")          # nothing begun
        acc = coverage.DeviceCount(r, FC.MAPQ, None, 0)
        acc.add(r)
        fails(call(rc._h), stem + "no runs: call pmx_dbam_coverage_finish first")          # a table, no runs yet
        acc.finish(r)
        fails(call(rc._h), stem + "the control has no runs")                               # the control: nothing begun
        cacc = coverage.DeviceCount(rc, FC.MAPQ, None, 0)
        cacc.add(rc)
        fails(call(rc._h), stem + "the control has no runs")                               # the control: a table
        cacc.finish(rc)
        fails(L.pmx_dbam_coverage_poisson(None, rc._h, 50, 1.0, 0, 0, F.ctypes.data, F.size, tot.ctypes.data), "null handle")
        fails(L.pmx_dbam_coverage_poisson(h, None, 50, 1.0, 0, 0, F.ctypes.data, F.size, tot.ctypes.data), "null handle")
        fails(call(rc._h, out=None), stem + "null output")
        coverage.device_count_of(ro, FC.MAPQ, None, 0)
        coverage.device_count_of(rf, FC.MAPQ, None, 0)
        fails(call(ro._h), stem + "the chosen references of the control differ")            # other lengths
        fails(call(rf._h), stem + "the chosen references of the control differ")            # fewer references
        part = coverage.device_count_of(rc, FC.MAPQ, ["p0", "p2"], 0)
        fails(call(rc._h), stem + "the chosen references of the control differ")            # another choice of the same header
        with pytest.raises(ValueError, match="the chosen references of the control differ"):
            acc.poisson(r, part, rc, 50)
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 0)
        for bad in (0, 65537):
            fails(call(rc._h, B=bad), stem + "a bin of 1 to 65536 bases")
        fails(call(rc._h, small=1 << 31), stem + "a window is 0 \\(off\\) to 2\\^31 - 1 bases")
        fails(call(rc._h, large=(1 << 32) - 1), stem + "a window is 0 \\(off\\) to 2\\^31 - 1 bases")
        assert call(rc._h, small=(1 << 31) - 1, large=(1 << 31) - 1) == 0
        assert acc.finish(r)["max_depth"] == 25
        for n in (0, 25):
            fails(call(rc._h, n=n), stem + "the table of ln\\(i!\\) has %d entries, the treatment's max_depth \\+ 1 = 26 are needed" % n)
        fails(call(rc._h, table=None), stem + "the table of ln\\(i!\\) has 0 entries")
        assert call(rc._h, n=26) == 0
        for bad in (2.0 ** -65, 0.0, -1.0, float("nan"), float("inf")):
            fails(call(rc._h, a_c=bad), stem + "the factor is a finite number of at least 2\\^-64")
        fails(call(rc._h, a_c=2.0 ** 37), stem + "factor \\* max_depth is 2\\^40 or more")  # (the control here is the treatment's file: its depth is 25)
        dacc = coverage.device_count_of(rd, FC.MAPQ, None, 0)                               # the factor against the control's depth only
        assert dacc.finish(rd)["max_depth"] == 1024
        fails(call(rd._h, a_c=2.0 ** 30), stem + "factor \\* max_depth is 2\\^40 or more")
        big = np.ascontiguousarray(coverage.lnfact(1025))
        assert L.pmx_dbam_coverage_poisson(rd._h, h, 50, 2.0 ** 30, 0, 0, big.ctypes.data, big.size, tot.ctypes.data) == 0
        none = coverage.device_count_of(rc, 255, None, 0)                                   # a control without a covered base
        assert none.finish(rc)["fragment_bases"] == 0
        fails(call(rc._h), stem + "the control has no covered base")
        # the host's checks say the same before the call
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 0)
        for kw, text in ((dict(a_c=2.0 ** 37), "2\\^40"), (dict(a_c=0.0), "2\\^-64"), (dict(small=-1), "coverage_lambda"), (dict(large=1 << 31), "coverage_lambda"),
                         (dict(bin=0), "coverage_bin"), (dict(a_c=float("nan")), "finite")):
            with pytest.raises(ValueError, match=text):
                acc.poisson(r, cacc, rc, **dict(dict(bin=50), **kw))
        with pytest.raises(ValueError, match="the control has no covered base"):
            acc.poisson(r, coverage.device_count_of(rc, 255, None, 0), rc, 50)
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert acc.poisson(r, cacc, rc, 50)["runs"] > 0
        acc.begin(r)                                                                        # a new table: runs and track are gone
        fails(call(rc._h), stem + "no runs: call pmx_dbam_coverage_finish first")
    # a treatment deeper than 2^20
    with DeviceBedReadsReader(tag, [n for n, _l in PS.P_REFS], [l for _n, l in PS.P_REFS]) as rp, DeviceBamReader(bam) as rc:
        pile, cacc = coverage.device_count_of(rp, 0, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert pile.finish(rp)["max_depth"] == (1 << 20) + 1
        big = np.zeros((1 << 20) + 2, dtype=np.float64)
        tot = np.zeros(4, dtype=np.float64)
        rc_ = rp._L.pmx_dbam_coverage_poisson(rp._h, rc._h, 50, 1.0, 0, 0, big.ctypes.data, big.size, tot.ctypes.data)
        assert rc_ == -3
        with pytest.raises(PmxIOError, match="the treatment's max_depth is above 2\\^20"):
            rp._raise(rc_)
        with pytest.raises(ValueError, match="max_depth is above 2\\^20"):
            pile.poisson(rp, cacc, rc, 50)
        assert cacc.poisson(rc, pile, rp, 50, 2.0 ** -10)["runs"] > 0                       # as a control it is fine


def _held(refs, B, rows, max_depth):
    """The bytes poisson holds at its peak on ``refs`` at bin ``B`` when its track is ``rows`` (name, start0, end0, bits): 24 per bin,
    12 per workgroup of 256 bins, 8 per entry of F, 20 per boundary, 16 per run, and the geometry."""
    nb = sum(-(-l // B) for _n, l in refs)
    ne = 0
    for name, length in refs:
        at = 0
        for _n, s, e, _v in (x for x in rows if x[0] == name):
            ne += (s > at) + 1
            at = e
        ne += at < length
    return 8 * (len(refs) + 1) + 8 * len(refs) * 2 + 8 * len(refs) + 24 * nb + 12 * (-(-nb // 256)) + 8 * (max_depth + 1) + 20 * ne + 16 * len(rows)


def test_the_stream_peak_counts_the_tables_to_the_byte(case):
    """Few reads on long references: finish holds 4 bytes per base; poisson at B = 2 holds 24 bytes per bin of 2 bases, three times
    as much, and at B = 1 twice that: both peaks are poisson's, and they differ by exactly what the two calls hold."""
    refs = [("long0", 3_000_000), ("long1", 1_000_001)]
    reads = [(0, 1000 * i + 1, 36, 0) for i in range(40)] + [(1, 999_990, 36, 0)]
    bam, control = _bam_of(case["dir"], "long", refs, reads), _bam_of(case["dir"], "long_input", refs, reads[::2])
    t, c = _host_count(reads, refs, [1, 1], 0), _host_count(reads[::2], refs, [1, 1], 0)
    with DeviceStreamReader(bam, window_bytes=WINDOW) as r, DeviceBamReader(control) as rc:
        acc = r.arm_coverage(FC.MAPQ, None, 0)
        for _ in r._windows():
            pass
        assert acc.finish(r)["runs"] == 41
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 0)
        before = r.stream_info()["peak_device_bytes"]
        peaks, held = [], []
        for B in (2, 1):
            host = t.poisson(c, B, 2.0, 100, 1000)
            assert _totals(acc.poisson(r, cacc, rc, B, 2.0, 100, 1000)) == host.totals and acc.signal_result(r) == host
            peaks.append(r.stream_info()["peak_device_bytes"])
            held.append(_held(refs, B, PS.rows_got(host), 1))
        assert before < peaks[0] < peaks[1] and peaks[1] - peaks[0] == held[1] - held[0] and held[0] > 24 * 2_000_000
        acc.poisson(r, cacc, rc, 4, 2.0, 100, 1000)         # (smaller tables: the peak stays)
        assert r.stream_info()["peak_device_bytes"] == peaks[1]


def test_the_run_with_the_option(tmp_path):
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(10))]
    rows = [(int(r), int(p) + 17, int(l), int(s)) for r, p, l, s in list(zip(*cols))[::3] if int(p) + 17 + int(l) <= refs[int(r)][1]]
    recs = [SW.rec("c%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(rows)]
    control = SW.write_twins(tmp_path, "input", refs, recs)[1]
    use = [1] * len(refs)
    t = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, 200)
    c = _host_count(rows, refs, use, 200)
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=None, save_mappability_stats=False, coverage_extend=200, coverage_bin=50,
              coverage_control=control, coverage_poisson=True)
    g = t.poisson(c, 50, t.reads / c.reads, 1000, 10000, control)
    # the text track and the peaks: the device run, the host run and the host path write the same bytes
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "text"), 300, coverage_call=1.0, coverage_call_length=50, **kw)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "host"), 300, coverage_call=1.0, coverage_call_length=50, device_ingest=False, **kw)
    assert [p.name for p in w1[-2:]] == [STEM + "_coverage.bedGraph", STEM + "_coverage_peaks.narrowPeak"] == [p.name for p in w0[-2:]]
    assert w1[-2].read_bytes() == w0[-2].read_bytes() == coverage.write_coverage(tmp_path / "want", STEM, g).read_bytes()
    lines = w1[-1].read_bytes()
    assert lines == w0[-1].read_bytes() == b"".join(g.call(1.0, 30, 50).text_chunks()) and lines.count(b"\n") >= 1
    assert all(ln.split(b"\t")[6] == ln.split(b"\t")[7] and ln.split(b"\t")[8] == b"-1" for ln in lines.splitlines())
    assert g.n_runs > 50 and g.min == 0.0 and g.max > 1.0 and sorted(os.listdir(tmp_path / "text")) == sorted(p.name for p in w1)
    # the bigWig file, other windows; then compressed on the device
    more = dict(coverage_lambda=(0, 5000), coverage_format="bigwig")
    g2 = t.poisson(c, 50, t.reads / c.reads, 0, 5000, control)
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "bw"), 300, **more, **kw)
    assert w2[-1].name == STEM + "_coverage.bw" and w2[-1].read_bytes() == coverage.write_bigwig(tmp_path / "want", STEM, g2).read_bytes() and g2 != g
    _r3, w3 = pipeline.run(GOLDEN_BAM, str(tmp_path / "z"), 300, coverage_compress="device", **more, **kw)
    got, want = BC.read_file(w3[-1]), BC.read_file(w2[-1])
    assert got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in want.items() if k != "compressed"}
    assert sorted(os.listdir(tmp_path / "z")) == sorted(p.name for p in w3)                # (the temporary file is gone)
    # "auto": the control is piled up with the treatment's estimate, on one more read of both files
    _r4, w4 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, stats=True, **dict(kw, coverage_extend="auto"))
    rows4 = dict(ln.rstrip("\n").split("\t") for ln in open(w4[-2]))
    extend = int(rows4["Estimated library length"])
    t4 = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)
    c4 = _host_count(rows, refs, use, extend)
    g4 = t4.poisson(c4, 50, t4.reads / c4.reads, 1000, 10000, control)
    assert w4[-1].read_bytes() == coverage.write_coverage(tmp_path / "host4", STEM, g4).read_bytes()
