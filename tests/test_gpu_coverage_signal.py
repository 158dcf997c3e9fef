"""The signal track on the GPU: pmx_dbam_coverage_signal and its consumers against the loop restatement of
tests/signal_cases and against the host path -- runs, totals, text bytes (chunked and in one call) and the whole bigWig file with
compression off, byte for byte: everything is an integer or has one stated order.  Through every device reader, with a mask, a stream
window by window, the pair pileup, two signals on one pileup, the compressed doors, the error paths and up to the run's file."""
import os
import random
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import fragments_cases as FR
from tests import io_writers as W
from tests import sam_writers as SW
from tests import signal_cases as SC

pytestmark = pytest.mark.gpu

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """coverage_cases' library under the renamed references of bigwig_out_cases, as every kind of input."""
    d = tmp_path_factory.mktemp("gpu_coverage_signal")
    rows = CC.synthetic()
    recs = FC.alignment_records(rows, BC.REFS)
    _sam, bam, gz = SW.write_twins(d, "cv", BC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(BC.NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, BC.REFS, SW.bam_bytes(BC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "cv.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, BC.REFS)))
    reads = FC.kept(rows)
    return dict(dir=d, bam=bam, gz=gz, indexed=indexed, tag=tag, reads=reads, less=FC.masked(reads, BC.REFS, BC.MASK), pile={}, sums={})


def _host_count(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


def _pile(case, extend, masked=False, use="all"):
    """(the host pileup, the per-base depth lists of the restated runs), computed once per parameter set and left unchanged."""
    key = extend, masked, use
    if key not in case["pile"]:
        reads = case["less" if masked else "reads"]
        want = CC.restate(reads, BC.REFS, CC.USES[use], extend)
        case["pile"][key] = _host_count(reads, BC.REFS, CC.USES[use], extend), BC.depth_lists(want, BC.REFS, CC.USES[use])
    return case["pile"][key]


def _sums(case, extend, B):
    if (extend, B) not in case["sums"]:
        case["sums"][extend, B] = SC.bin_sums(_pile(case, extend)[1], B)
    return case["sums"][extend, B]


def _scales(c):
    lengths = [l for _n, l in c.refs]
    return (1.0, coverage.scale_of("cpm", c.reads, c.fragment_bases, lengths), coverage.scale_of("rpgc", c.reads, c.fragment_bases, lengths))


def _totals(tot):
    return tuple(tot[k] for k in coverage.SIGNAL_TOTALS)


@pytest.mark.parametrize("B", SC.BINS)
@pytest.mark.parametrize("extend", [0, 200])
def test_the_device_against_the_restatement(case, tmp_path, extend, B):
    c, _depths = _pile(case, extend)
    with DeviceBamReader(case["bam"]) as r:
        assert r._L.pmx_dbam_version() >= 19
        acc = coverage.device_count_of(r, FC.MAPQ, None, extend)
        for k, scale in enumerate(_scales(c)):
            want = SC.restate(_sums(case, extend, B), scale)
            assert _totals(acc.signal(r, B, scale)) == SC.totals(want)
            g = acc.signal_result(r)
            assert SC.rows_got(g) == SC.rows_of(want) and g == c.signal(B, scale)
            assert acc.text(r, signal=True) == SC.text_of(want) == b"".join(acc.text_chunks(r, 1000, signal=True))
            if k == 1:                                      # the whole file, once per bin
                dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r, signal=True)
                assert dev.read_bytes() == coverage.write_bigwig(tmp_path / "host", "host", c.signal(B, scale)).read_bytes()
                SC.check_file(BC.read_file(dev), want, BC.REFS, B)
        assert acc.result(r) == c                           # the depth runs stay as they are
        if B == 1:
            acc.signal(r, 1, 1.0)
            assert acc.text(r, signal=True) == acc.text(r)  # scale 1, B = 1: the depth track's lines


def _signal_files(reader, base, mask, extend, B, normalize, references=None):
    """(text, file bytes, totals) of the device's signal on ``reader``."""
    if mask is not None:
        reader.set_exclude(mask.resolve(reader.references, reader.lengths))
    acc = coverage.device_count_of(reader, FC.MAPQ, references, extend)
    t = acc.finish(reader)
    scale = coverage.scale_of(normalize, t["reads"], t["fragment_bases"], [l for _n, l in acc.refs])
    tot = acc.signal(reader, B, scale, normalize)
    track = coverage.write_coverage(base, "dev", acc, reader, signal=True).read_bytes()
    return track, coverage.write_bigwig(base, "dev", acc, reader, signal=True).read_bytes(), _totals(tot)


def _host_files(c, base, B, normalize):
    g = c.signal(B, coverage.scale_of(normalize, c.reads, c.fragment_bases, [l for _n, l in c.refs]), normalize)
    return coverage.write_coverage(base, "dev", g).read_bytes(), coverage.write_bigwig(base, "dev", g).read_bytes(), g.totals


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("extend,B,normalize", [(0, 50, "cpm"), (200, 7, "rpgc")])
def test_every_reader_makes_the_host_paths_signal(case, tmp_path, extend, B, normalize, masked):
    mask = region_mask.open_mask(BC.MASK) if masked else None
    whole = _host_files(_pile(case, extend, masked)[0], tmp_path / "host", B, normalize)
    assert b" bin=%d normalize=%s scale=" % (B, normalize.encode()) in whole[0][:300] and whole[2][0] > 500
    with DeviceBamReader(case["bam"]) as r:
        assert _signal_files(r, tmp_path / "bam", mask, extend, B, normalize) == whole
    with DeviceSamReader(case["gz"]) as r:
        assert _signal_files(r, tmp_path / "gz", mask, extend, B, normalize) == whole
    with DeviceBedReadsReader(case["tag"], BC.NAMES, BC.LENGTHS) as r:
        assert _signal_files(r, tmp_path / "tag", mask, extend, B, normalize) == whole
    chosen = [n for n, u in zip(BC.NAMES, CC.USES["no middle"]) if u]
    with DeviceBamReader(case["indexed"], references=chosen) as r:
        assert r.indexed
        part = _signal_files(r, tmp_path / "indexed", mask, extend, B, normalize)
    assert part == _host_files(_pile(case, extend, masked, "no middle")[0], tmp_path / "host2", B, normalize)
    # a FIFO cut into windows
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
            if mask is not None:
                r.set_exclude(mask.resolve(r.references, r.lengths))
            acc = r.arm_coverage(FC.MAPQ, None, extend)
            for _ in r._windows():
                pass
            tot = acc.finish(r)
            acc.signal(r, B, coverage.scale_of(normalize, tot["reads"], tot["fragment_bases"], BC.LENGTHS), normalize)
            streamed = (coverage.write_coverage(tmp_path / "fifo_out", "dev", acc, r, signal=True).read_bytes(),
                        coverage.write_bigwig(tmp_path / "fifo_out", "dev", acc, r, signal=True).read_bytes(), _totals(acc.sig["totals"]))
            assert r.stream_info()["windows"] >= 10
    finally:
        t.join(60)
    assert streamed == whole


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_coverage_signal_small")
    reads = BC.small_reads()
    recs = [SW.rec("q%d" % i, 16 if s else 0, BC.SMALL_REFS[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    _sam, bam = SW.write_twins(d, "small", BC.SMALL_REFS, recs)
    want = CC.restate(reads, BC.SMALL_REFS, BC.SMALL_USE, 0)
    return dict(dir=d, bam=bam, reads=reads, depths=BC.depth_lists(want, BC.SMALL_REFS, BC.SMALL_USE),
                chosen=[x for x, u in zip(BC.SMALL_REFS, BC.SMALL_USE) if u])


@pytest.mark.parametrize("zoom", [None, 1, 2])              # z_0: its own choice, B itself, 2 B
@pytest.mark.parametrize("B", [1, 2, 7, 50])
def test_the_small_case(small, tmp_path, B, zoom):
    kw = dict(items_per_section=BC.SMALL_ITEMS, index_block=BC.SMALL_BLOCK, zoom_base=None if zoom is None else zoom * B)
    c = _host_count(small["reads"], BC.SMALL_REFS, BC.SMALL_USE, 0)
    scale = coverage.scale_of("cpm", c.reads, c.fragment_bases, [l for _n, l in small["chosen"]], 3.0)
    want = SC.restate(SC.bin_sums(small["depths"], B), scale)
    with DeviceBamReader(small["bam"]) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, [n for n, _l in small["chosen"]], 0)
        assert _totals(acc.signal(r, B, scale)) == SC.totals(want)
        dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r, signal=True, **kw)
        assert dev.read_bytes() == coverage.write_bigwig(tmp_path / "host", "host", c.signal(B, scale), **kw).read_bytes()
        again = coverage.write_bigwig(tmp_path / "again", "dev", acc, r, signal=True, **kw)     # the signal stays: a second file is the same
        assert again.read_bytes() == dev.read_bytes()
        # the depth file of the same handle is the host's still, and the signal survives it
        depth = coverage.write_bigwig(tmp_path / "depth", "dev", acc, r, **kw)
        assert depth.read_bytes() == coverage.write_bigwig(tmp_path / "hdepth", "host", c, **kw).read_bytes()
        assert acc.text(r, signal=True) == SC.text_of(want)
        # the compressed doors: the file decodes to the same sections
        z = BC.read_file(coverage.write_bigwig(tmp_path / "z", "dev", acc, r, compress="device", signal=True, **kw), BC.SMALL_BLOCK)
        # no kept read at all: a valid file without a level
        acc = coverage.device_count_of(r, FC.MAPQ, ["z_empty"], 0)
        assert _totals(acc.signal(r, B, scale)) == (0, 0, 0.0, 0.0) and acc.text(r, signal=True) == b""
        empty = coverage.write_bigwig(tmp_path / "empty", "dev", acc, r, signal=True, **kw)
        assert acc.ranges(r, signal=True).tolist() == [0, 0]
    got = BC.read_file(dev, BC.SMALL_BLOCK)
    SC.check_file(got, want, small["chosen"], B, kw["zoom_base"], BC.SMALL_ITEMS)
    assert z["compressed"] and {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in got.items() if k != "compressed"}
    got = BC.read_file(empty, BC.SMALL_BLOCK)
    assert got["chroms"] == [("z_empty", 0, 700)] and got["runs"] == {} and got["zooms"] == [] and got["sections"] == []
    use = [0, 0, 0, 0, 0, 0, 1, 0]
    assert empty.read_bytes() == coverage.write_bigwig(tmp_path / "h0", "host", _host_count(small["reads"], BC.SMALL_REFS, use, 0).signal(B, scale),
                                                       **kw).read_bytes()


def _bam_of(d, name, refs, reads):
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    return SW.write_twins(d, name, refs, recs)[1]


@pytest.mark.parametrize("scale", [1.0, 0.37, SC.TINY, 1 / 128])
def test_the_planted_situations(tmp_path, scale):
    reads = SC.planted_reads()
    want0 = CC.restate(reads, SC.P_REFS, [1] * 4, 0)
    depths = BC.depth_lists(want0, SC.P_REFS, [1] * 4)
    want = SC.restate(SC.bin_sums(depths, SC.P_B), scale)
    SC.check_planted(want, scale)
    with DeviceBamReader(_bam_of(tmp_path, "planted", SC.P_REFS, reads)) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, None, 0)
        assert _totals(acc.signal(r, SC.P_B, scale)) == SC.totals(want)
        assert SC.rows_got(acc.signal_result(r)) == SC.rows_of(want) and acc.text(r, signal=True) == SC.text_of(want)
        dev = coverage.write_bigwig(tmp_path / "p", "p", acc, r, items_per_section=2, index_block=2, signal=True)
        SC.check_file(BC.read_file(dev, 2), want, SC.P_REFS, SC.P_B, None, 2)
        # two signals on one pileup, with different bins: the second replaces the first, the depth runs serve both
        for B in (1, 7, 65536):
            other = SC.restate(SC.bin_sums(depths, B), scale)
            assert _totals(acc.signal(r, B, scale)) == SC.totals(other)
            assert SC.rows_got(acc.signal_result(r)) == SC.rows_of(other) and acc.text(r, signal=True) == SC.text_of(other)
    if scale == 1 / 128:                                    # depth / 128 with an odd depth is an exact tie at six decimals
        assert b"\t0.007812\n" in SC.text_of(SC.restate(SC.bin_sums(depths, 1), scale))


def test_two_sums_that_round_to_one_value_stay_two_runs(tmp_path):
    reads = SC.tie_reads()
    want0 = CC.restate(reads, SC.T_REFS, [1], SC.T_EXTEND)
    want = SC.restate(SC.bin_sums(BC.depth_lists(want0, SC.T_REFS, [1]), SC.T_B), 1.0)
    SC.check_tie(want)
    with DeviceBamReader(_bam_of(tmp_path, "tie", SC.T_REFS, reads)) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, None, SC.T_EXTEND)
        assert _totals(acc.signal(r, SC.T_B, 1.0)) == SC.totals(want) == (2, 8192, 4097.0, 4097.0)
        assert SC.rows_got(acc.signal_result(r)) == SC.rows_of(want)
        assert acc.text(r, signal=True) == b"t0\t0\t4096\t4097\nt0\t4096\t8192\t4097\n"
        with pytest.raises(ValueError, match="2\\^40"):     # scale * max_depth
            acc.signal(r, 1, 2.0 ** 28)
        rc = r._L.pmx_dbam_coverage_signal(r._h, 1, 2.0 ** 28, np.zeros(4).ctypes.data)
        assert rc == -3
        with pytest.raises(PmxIOError, match="pmx_dbam_coverage_signal: scale \\* max_depth is 2\\^40 or more"):
            r._raise(rc)


def test_the_pair_pileup(tmp_path):
    recs = [r for _l, r in FR.planted()] + FR.random_pairs(random.Random(3), 3000)
    recs = [r for _i, r in sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))]
    bam = str(tmp_path / "pe.bam")
    FR.write_bam(bam, recs)
    with BamReader(bam) as h:
        host = coverage.from_reader(h, FR.MAPQ, None, "pair", 2000)
    scale = coverage.scale_of("cpm", host.reads, host.fragment_bases, [l for _n, l in host.refs])
    g = host.signal(50, scale, "cpm")
    assert host.reads > 500 and g.n_runs > 100
    with DeviceBamReader(bam) as r:
        acc = coverage.device_count_of(r, FR.MAPQ, None, "pair", 2000)
        assert _totals(acc.signal(r, 50, scale, "cpm")) == g.totals and acc.signal_result(r) == g
        assert coverage.write_coverage(tmp_path / "dev", "x", acc, r, signal=True).read_bytes() == coverage.write_coverage(tmp_path / "host", "x", g).read_bytes()
        assert coverage.write_bigwig(tmp_path / "dev", "x", acc, r, signal=True).read_bytes() == coverage.write_bigwig(tmp_path / "host", "x", g).read_bytes()


def test_entry_points_in_the_wrong_state_and_with_short_buffers(small):
    with DeviceBamReader(small["bam"]) as r:
        L, h = r._L, r._h
        buf, table, sums = np.zeros(4096, dtype=np.uint8), np.zeros((64, 5), dtype=np.uint32), np.zeros((64, 2), dtype=np.float64)
        first, out, tot = np.zeros(16, dtype=np.int64), np.zeros(2, dtype=np.uint64), np.zeros(4, dtype=np.float64)
        cols = [np.zeros(256, dtype=np.uint32) for _ in range(4)]
        ids = np.arange(len(BC.SMALL_REFS), dtype=np.uint32)
        stem = "pmx_dbam_coverage_signal"

        def fails(rc, text, code=-3):
            assert rc == code
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc)

        def every(text):
            fails(L.pmx_dbam_coverage_signal_runs(h, 0, 0, *(x.ctypes.data for x in cols)), stem + "_runs: " + text)
            fails(L.pmx_dbam_coverage_signal_text(h, 0, 0, None, 0), stem + "_text: " + text)
            fails(L.pmx_dbam_coverage_signal_ranges(h, first.ctypes.data, 16), stem + "_ranges: " + text)
            fails(L.pmx_dbam_coverage_signal_sections(h, 0, 0, 0, 4, None, 0, None, 0, None), stem + "_sections: " + text)
            fails(L.pmx_dbam_coverage_signal_sections_z(h, 0, 0, 0, 4, None, 0, None, 0, None, None), stem + "_sections_z: " + text)
            fails(L.pmx_dbam_coverage_signal_zoom_begin(h, 32, 1, ids.ctypes.data, out.ctypes.data), stem + "_zoom_begin: " + text)
            fails(L.pmx_dbam_coverage_signal_zoom_records(h, 0, 4, None, 0, None, 0), stem + "_zoom_records: " + text)
            fails(L.pmx_dbam_coverage_signal_zoom_records_z(h, 0, 4, None, 0, None, 0, None), stem + "_zoom_records_z: " + text)
        no_runs = "no runs: call pmx_dbam_coverage_finish first"
        every(no_runs)                                                                      # nothing begun
        fails(L.pmx_dbam_coverage_signal(h, 50, 1.0, tot.ctypes.data), stem + ": " + no_runs)
        acc = coverage.DeviceCount(r, FC.MAPQ, None, 0)
        acc.add(r)
        every(no_runs)                                                                      # a table, no runs yet
        fails(L.pmx_dbam_coverage_signal(h, 50, 1.0, tot.ctypes.data), stem + ": " + no_runs)
        assert acc.finish(r)["runs"] == 111
        every("no signal: call pmx_dbam_coverage_signal first")                             # runs, no signal yet
        fails(L.pmx_dbam_coverage_signal(h, 50, 1.0, None), stem + ": null output")
        for bad in (0, 65537):
            fails(L.pmx_dbam_coverage_signal(h, bad, 1.0, tot.ctypes.data), stem + ": a bin of 1 to 65536 bases")
        for bad in (2.0 ** -65, 0.0, -1.0, float("nan"), float("inf")):
            fails(L.pmx_dbam_coverage_signal(h, 50, bad, tot.ctypes.data), stem + ": the scale is a finite number of at least 2\\^-64")
        fails(L.pmx_dbam_coverage_signal(h, 50, 2.0 ** 39, tot.ctypes.data), stem + ": scale \\* max_depth is 2\\^40 or more")
        every("no signal: call pmx_dbam_coverage_signal first")                             # a refused signal leaves none
        covered = CC.restate(small["reads"], BC.SMALL_REFS, [1] * 8, 0)["covered_bases"]
        assert L.pmx_dbam_coverage_signal(h, 1, 1.0, tot.ctypes.data) == 0 and tot.tolist() == [111.0, float(covered), 1.0, 2.0]
        n = 111
        fails(L.pmx_dbam_coverage_signal_runs(h, 0, n + 1, *(x.ctypes.data for x in cols)), stem + "_runs: range outside the runs")
        fails(L.pmx_dbam_coverage_signal_runs(h, 0, 4, cols[0].ctypes.data, None, None, None), stem + "_runs: null output")
        size = L.pmx_dbam_coverage_signal_text(h, 0, 4, None, 0)
        assert size == len(b"s4\t0\t10\t1\ns4\t22\t32\t1\ns4\t64\t72\t1\ns4\t90\t100\t1\n")
        fails(L.pmx_dbam_coverage_signal_text(h, 0, 4, buf.ctypes.data, size - 1), stem + "_text: the buffer is too small")
        fails(L.pmx_dbam_coverage_signal_text(h, 0, 4, buf.ctypes.data, -1), stem + "_text: a negative capacity")
        assert L.pmx_dbam_coverage_signal_ranges(h, None, 0) == 9
        fails(L.pmx_dbam_coverage_signal_ranges(h, first.ctypes.data, 8), stem + "_ranges: the buffer is too small")
        assert L.pmx_dbam_coverage_signal_ranges(h, first.ctypes.data, 16) == 9 and first[:9].tolist() == [0, 4, 9, 12, 60, 109, 110, 110, 111]
        sec = stem + "_sections: "
        assert L.pmx_dbam_coverage_signal_sections(h, 0, 4, 7, 4, None, 0, None, 0, None) == 24 + 48
        fails(L.pmx_dbam_coverage_signal_sections(h, 0, 4, 7, 4, buf.ctypes.data, 71, table.ctypes.data, 64, sums.ctypes.data), sec + "the buffer is too small")
        fails(L.pmx_dbam_coverage_signal_sections(h, 12, 48, 7, 4, buf.ctypes.data, 4096, table.ctypes.data, 11, sums.ctypes.data), sec + "the table is too small")
        fails(L.pmx_dbam_coverage_signal_sections(h, 0, 4, 7, 4, buf.ctypes.data, 4096, table.ctypes.data, 64, None), sec + "null output")
        fails(L.pmx_dbam_coverage_signal_sections(h, 3, 2, 7, 4, None, 0, None, 0, None), sec + "the range holds two references")
        fails(L.pmx_dbam_coverage_signal_sections(h, 0, n + 1, 7, 4, None, 0, None, 0, None), sec + "range outside the runs")
        for items in (0, 65536):
            fails(L.pmx_dbam_coverage_signal_sections(h, 0, 4, 7, items, None, 0, None, 0, None), sec + "1 to 65535 items per section")
        fails(L.pmx_dbam_coverage_signal_sections_z(h, 0, 4, 7, 5460, None, 0, None, 0, None, None), stem + "_sections_z: at most 5459 items")
        assert L.pmx_dbam_coverage_signal_sections(h, 0, 4, 7, 3, buf.ctypes.data, 96, table.ctypes.data, 2, sums.ctypes.data) == 96
        assert table[:2].tolist() == [[7, 0, 7, 72, 60], [7, 90, 7, 100, 36]] and sums[:2].tolist() == [[28.0, 28.0], [10.0, 10.0]]
        words = buf[:96].view("<u4").tolist()
        assert words[:6] == [7, 0, 72, 0, 0, 1 | 3 << 16] and words[6:9] == [0, 10, np.float32(1).view(np.uint32)]
        # zoom: records before begin; bad arguments; the two kinds of bins replace each other
        zoom = stem + "_zoom_"
        fails(L.pmx_dbam_coverage_signal_zoom_records(h, 0, 4, None, 0, None, 0), zoom + "records: no bins of that level")
        fails(L.pmx_dbam_coverage_signal_zoom_begin(h, 32, 11, ids.ctypes.data, out.ctypes.data), zoom + "begin: at most 10 levels")
        fails(L.pmx_dbam_coverage_signal_zoom_begin(h, 32, 1, None, out.ctypes.data), zoom + "begin: null chromosome ids")
        fails(L.pmx_dbam_coverage_signal_zoom_begin(h, 32, 1, ids.ctypes.data, None), zoom + "begin: null output")
        assert L.pmx_dbam_coverage_signal_zoom_begin(h, 32, 2, ids.ctypes.data, out.ctypes.data) == 0 and out.tolist() == [0, 0]
        fails(L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0), "pmx_dbam_coverage_zoom_records: no bins of that level")
        size = L.pmx_dbam_coverage_signal_zoom_records(h, 0, 4, None, 0, None, 0)
        assert size > 0 and size % 32 == 0
        rows = -(-(size // 32) // 4)
        big, t2 = np.zeros(size, dtype=np.uint8), np.zeros((rows, 5), dtype=np.uint32)
        fails(L.pmx_dbam_coverage_signal_zoom_records(h, 0, 4, big.ctypes.data, size - 1, t2.ctypes.data, rows), zoom + "records: the buffer is too small")
        fails(L.pmx_dbam_coverage_signal_zoom_records(h, 0, 4, big.ctypes.data, size, t2.ctypes.data, rows - 1), zoom + "records: the table is too small")
        fails(L.pmx_dbam_coverage_signal_zoom_records_z(h, 0, 2049, None, 0, None, 0, None), zoom + "records_z: at most 2048 items")
        assert L.pmx_dbam_coverage_signal_zoom_records(h, 0, 4, big.ctypes.data, size, t2.ctypes.data, rows) == size
        assert int(t2[:, 4].sum()) == size
        assert L.pmx_dbam_coverage_zoom_begin(h, 32, 1, ids.ctypes.data, out.ctypes.data) == 0          # the depth's bins take their place
        fails(L.pmx_dbam_coverage_signal_zoom_records(h, 1, 4, None, 0, None, 0), zoom + "records: no bins of that level")
        assert L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0) > 0
        every8 = CC.restate(small["reads"], BC.SMALL_REFS, [1] * 8, 0)
        second = SC.restate(SC.bin_sums(BC.depth_lists(every8, BC.SMALL_REFS, [1] * 8), 7), 0.5)
        assert L.pmx_dbam_coverage_signal(h, 7, 0.5, tot.ctypes.data) == 0                         # a second signal replaces the first
        assert tuple(tot.tolist()) == SC.totals(second) and tot[0] != 111
        assert L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0) > 0                     # (and leaves the depth's bins)
        acc.begin(r)                                                                        # a new table: runs and signal are gone
        every(no_runs)


def test_the_stream_peak_counts_the_bin_table(case):
    """Few reads on long references: finish holds the table of 4 bytes per base, 24 bytes per tile of 4096 slots and 12 per run
    boundary; signal at B = 2 holds a table of the same size (8 bytes per bin of 2 bases), 12 bytes per 256 bins and 16 per entry
    and run.  With 12 / 512 against 24 / 4096 bytes per base the second peak is the higher one while the runs are few -- but only if
    the bin table is counted."""
    refs = [("long0", 3_000_000), ("long1", 1_000_001)]
    reads = [(0, 1000 * i + 1, 36, 0) for i in range(40)] + [(1, 999_990, 36, 0)]      # (the last: from an odd base to the short last bin, 3 runs)
    bam = _bam_of(case["dir"], "long", refs, reads)
    with DeviceStreamReader(bam, window_bytes=WINDOW) as r:
        acc = r.arm_coverage(FC.MAPQ, None, 0)
        for _ in r._windows():
            pass
        assert acc.finish(r)["runs"] == 41
        before = r.stream_info()["peak_device_bytes"]
        bases = sum(l for _n, l in refs)
        assert before > 4 * bases
        tot = acc.signal(r, 2, 1.0)
        after = r.stream_info()["peak_device_bytes"]
        bins = sum(-(-l // 2) for _n, l in refs)
        assert tot["runs"] == 43 and after >= before + 12 * (bins // 256) - 24 * (bases // 4096 + 2) - 4096
        assert after > before and after < before + (1 << 20)
        assert acc.signal(r, 1, 1.0)["runs"] == 41 and r.stream_info()["peak_device_bytes"] == after      # (B = 1 has no table)


def test_the_run_scales_at_its_own_estimate(tmp_path):
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=None, save_mappability_stats=False, stats=True)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage=True, coverage_normalize="cpm", **kw)
    stem = "ENCFF000RMB-test"
    assert w1[-1].name == stem + "_coverage.bedGraph" and sorted(os.listdir(tmp_path / "auto")) == sorted(p.name for p in w1)
    rows = dict(ln.rstrip("\n").split("\t") for ln in open(w1[-2]))
    extend = int(rows["Estimated library length"])
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(10))]
    host = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), extend)
    g = host.signal(1, 1e6 / host.reads, "cpm")
    assert w1[-1].read_bytes() == coverage.write_coverage(tmp_path / "host", stem, g).read_bytes() and g.n_runs > 100
    # an integer is counted on the reader that feeds the run; a bin, rpgc and the bigWig file with its sections compressed on the GPU
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 300, coverage=True, coverage_extend=extend, coverage_format="bigwig",
                           coverage_bin=50, coverage_normalize="rpgc", coverage_genome_size=3_000_000, coverage_compress="device", **kw)
    g2 = host.signal(50, 3_000_000 / host.fragment_bases)
    want = BC.read_file(coverage.write_bigwig(tmp_path / "host2", stem, g2))
    got = BC.read_file(w2[-1])
    assert got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in want.items() if k != "compressed"}
    assert sorted(os.listdir(tmp_path / "two")) == sorted(p.name for p in w2)               # (the temporary file is gone)
