"""The pileup as a bigWig file on the GPU: the sections, their tables and the zoom records of
pmx_dbam_coverage_ranges / _sections / _zoom_begin / _zoom_records, assembled into a file that is byte for byte the host path's,
read by the independent reader of tests/bigwig_out_cases and set against its loop restatement directly; through every device
reader, with and without excluded regions, a stream window by window, the pair pileup, and up to the run's file."""
import os
import random
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.bigwig_device import DeviceBigWigReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import fragments_cases as FR
from tests import io_writers as W
from tests import sam_writers as SW

pytestmark = pytest.mark.gpu

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
GOLDEN_TRACK = os.path.join(fx.GOLDEN, "hg19_36mer-test.bedGraph")
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """coverage_cases' library under the renamed references of bigwig_out_cases, as every kind of input."""
    d = tmp_path_factory.mktemp("gpu_coverage_bigwig")
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
    return dict(dir=d, bam=bam, gz=gz, indexed=indexed, tag=tag, reads=reads, less=FC.masked(reads, BC.REFS, BC.MASK), want={}, host={})


def _want(case, extend, masked):
    """(restated runs, per-base depth lists) of the whole library, computed once per parameter set and left unchanged."""
    if (extend, masked) not in case["want"]:
        want = CC.restate(case["less" if masked else "reads"], BC.REFS, CC.USES["all"], extend)
        case["want"][extend, masked] = want, BC.depth_lists(want, BC.REFS, CC.USES["all"])
    return case["want"][extend, masked]


def _host_count(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


def _host_file(case, extend, masked, use="all"):
    """The bytes of the host path's file, written once per parameter set."""
    key = extend, masked, use
    if key not in case["host"]:
        c = _host_count(case["less" if masked else "reads"], BC.REFS, CC.USES[use], extend)
        case["host"][key] = coverage.write_bigwig(case["dir"] / "host", "host", c).read_bytes()
    return case["host"][key]


def _device_file(reader, base, mask, extend, references=None, **kw):
    if mask is not None:
        reader.set_exclude(mask.resolve(reader.references, reader.lengths))
    acc = coverage.device_count_of(reader, FC.MAPQ, references, extend)
    return coverage.write_bigwig(base, "dev", acc, reader, **kw)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_every_reader_writes_the_host_paths_file(case, tmp_path, extend, masked):
    mask = region_mask.open_mask(BC.MASK) if masked else None
    want, depths = _want(case, extend, masked)
    whole = _host_file(case, extend, masked)
    with DeviceBamReader(case["bam"]) as r:
        assert r._L.pmx_dbam_version() >= 17
        path = _device_file(r, tmp_path / "bam", mask, extend)
        assert path.name == "bam_coverage.bw" and path.read_bytes() == whole
    # the device's file against the reader and the restatement directly, not only through the host twin
    got = BC.read_file(path)
    BC.check_file(got, want, BC.REFS, CC.USES["all"], depths)
    assert len(got["zooms"]) >= 4 and want["n_runs"] > 3000 and len(got["sections"]) >= 4
    with DeviceBigWigReader(str(path)) as t:
        ids = BC.chrom_ids(BC.NAMES)
        assert list(t.chromsizes.items()) == sorted(BC.REFS, key=lambda x: ids[x[0]])
        for name, rows in want["runs"].items():
            s, e, v = t.fetch_arrays(0.0, name)
            assert list(zip(s.tolist(), e.tolist(), v.tolist())) == [(a, b, float(d)) for a, b, d in rows]
    with DeviceSamReader(case["gz"]) as r:
        assert _device_file(r, tmp_path / "gz", mask, extend).read_bytes() == whole
    with DeviceBedReadsReader(case["tag"], BC.NAMES, BC.LENGTHS) as r:
        assert _device_file(r, tmp_path / "tag", mask, extend).read_bytes() == whole
    chosen = [n for n, u in zip(BC.NAMES, CC.USES["no middle"]) if u]
    with DeviceBamReader(case["indexed"], references=chosen) as r:
        assert r.indexed
        part = _device_file(r, tmp_path / "indexed", mask, extend)
    assert part.read_bytes() == _host_file(case, extend, masked, "no middle")
    assert [n for n, _i, _l in BC.read_file(part)["chroms"]] == ["c", "chr2", "chrX_alt"]
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
            acc.finish(r)
            streamed = coverage.write_bigwig(tmp_path / "fifo_out", "dev", acc, r)
            assert r.stream_info()["windows"] >= 10
    finally:
        t.join(60)
    assert streamed.read_bytes() == whole
    # compressed: the same file after inflation
    with DeviceBamReader(case["bam"]) as r:
        z = BC.read_file(_device_file(r, tmp_path / "z", mask, extend, compress=True))
    assert z["compressed"] and {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in got.items() if k != "compressed"}


@pytest.fixture(scope="module")
def small(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_coverage_bigwig_small")
    reads = BC.small_reads()
    recs = [SW.rec("q%d" % i, 16 if s else 0, BC.SMALL_REFS[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    _sam, bam = SW.write_twins(d, "small", BC.SMALL_REFS, recs)
    want = CC.restate(reads, BC.SMALL_REFS, BC.SMALL_USE, 0)
    BC.check_small(want)
    return dict(dir=d, bam=bam, reads=reads, want=want, depths=BC.depth_lists(want, BC.SMALL_REFS, BC.SMALL_USE))


@pytest.mark.parametrize("zoom_base", [2, 32, None])
def test_the_small_case(small, tmp_path, zoom_base):
    kw = dict(items_per_section=BC.SMALL_ITEMS, index_block=BC.SMALL_BLOCK, zoom_base=zoom_base)
    chosen = [n for (n, _l), u in zip(BC.SMALL_REFS, BC.SMALL_USE) if u]
    host = coverage.write_bigwig(tmp_path / "host", "host", _host_count(small["reads"], BC.SMALL_REFS, BC.SMALL_USE, 0), **kw)
    with DeviceBamReader(small["bam"]) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, chosen, 0)
        ranges = acc.ranges(r).tolist()
        assert ranges == [0, 4, 9, 12, 60, 109, 110, 110] and acc.finish(r)["runs"] == 110     # z_empty: no run; left_out: not chosen
        dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r, **kw)
        assert dev.read_bytes() == host.read_bytes()
        again = coverage.write_bigwig(tmp_path / "again", "dev", acc, r, **kw)               # the runs stay: a second file is the same
        assert again.read_bytes() == host.read_bytes()
        # no kept read at all: a valid file without a level
        acc = coverage.device_count_of(r, FC.MAPQ, ["z_empty"], 0)
        empty = coverage.write_bigwig(tmp_path / "empty", "dev", acc, r, **kw)
        assert acc.ranges(r).tolist() == [0, 0]
    got = BC.read_file(dev, BC.SMALL_BLOCK)
    BC.check_file(got, small["want"], BC.SMALL_REFS, BC.SMALL_USE, small["depths"], zoom_base, BC.SMALL_ITEMS)
    assert [n for n, _i, _l in got["chroms"]] == ["B13long", "a3", "m12", "s4", "s5x", "tiny", "z_empty"]
    got = BC.read_file(empty, BC.SMALL_BLOCK)
    assert got["chroms"] == [("z_empty", 0, 700)] and got["runs"] == {} and got["zooms"] == [] and got["sections"] == []
    use = [0, 0, 0, 0, 0, 0, 1, 0]
    assert empty.read_bytes() == coverage.write_bigwig(tmp_path / "h0", "host", _host_count(small["reads"], BC.SMALL_REFS, use, 0), **kw).read_bytes()


def test_the_pair_pileup(tmp_path):
    recs = [r for _l, r in FR.planted()] + FR.random_pairs(random.Random(3), 3000)
    recs = [r for _i, r in sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))]
    bam = str(tmp_path / "pe.bam")
    FR.write_bam(bam, recs)
    with BamReader(bam) as h:
        host = coverage.from_reader(h, FR.MAPQ, None, "pair", 2000)
    assert host.reads > 500 and [n for n, _l in host.refs] == [n for n, _l in FR.REFS]
    with DeviceBamReader(bam) as r:
        acc = coverage.device_count_of(r, FR.MAPQ, None, "pair", 2000)
        dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r)
    assert dev.read_bytes() == coverage.write_bigwig(tmp_path / "host", "host", host).read_bytes()
    ids = BC.chrom_ids([n for n, _l in FR.REFS])
    assert coverage.read_bigwig(dev).rows() == sorted(host.rows(), key=lambda x: ids[x[0]])


def test_entry_points_in_the_wrong_state_and_with_short_buffers(small):
    with DeviceBamReader(small["bam"]) as r:
        L, h = r._L, r._h
        buf, table = np.zeros(4096, dtype=np.uint8), np.zeros((64, 5), dtype=np.uint32)
        first, out = np.zeros(16, dtype=np.int64), np.zeros(2, dtype=np.uint64)
        ids = np.arange(len(BC.SMALL_REFS), dtype=np.uint32)

        def fails(rc, text, code=-3):
            assert rc == code
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc)

        def every(text):
            fails(L.pmx_dbam_coverage_ranges(h, first.ctypes.data, 16), "pmx_dbam_coverage_ranges: " + text)
            fails(L.pmx_dbam_coverage_sections(h, 0, 0, 0, 4, None, 0, None, 0), "pmx_dbam_coverage_sections: " + text)
            fails(L.pmx_dbam_coverage_zoom_begin(h, 32, 1, ids.ctypes.data, out.ctypes.data), "pmx_dbam_coverage_zoom_begin: " + text)
            fails(L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0), "pmx_dbam_coverage_zoom_records: " + text)
        no_runs = "no runs: call pmx_dbam_coverage_finish first"
        every(no_runs)                                                                      # nothing begun
        acc = coverage.DeviceCount(r, FC.MAPQ, None, 0)
        acc.add(r)
        every(no_runs)                                                                      # a table, no runs yet
        n = acc.finish(r)["runs"]
        assert n == 111 and L.pmx_dbam_coverage_ranges(h, None, 0) == 9                     # (every reference is chosen here)
        fails(L.pmx_dbam_coverage_ranges(h, first.ctypes.data, 8), "pmx_dbam_coverage_ranges: the buffer is too small")
        assert L.pmx_dbam_coverage_ranges(h, first.ctypes.data, 16) == 9 and first[:9].tolist() == [0, 4, 9, 12, 60, 109, 110, 110, 111]
        # sections: a NULL buffer gives the size; short caps; a range over two references; items out of range
        assert L.pmx_dbam_coverage_sections(h, 0, 4, 7, 4, None, 0, None, 0) == 24 + 48
        assert L.pmx_dbam_coverage_sections(h, 12, 48, 7, 4, None, 0, None, 0) == 12 * 24 + 48 * 12
        sec = "pmx_dbam_coverage_sections: "
        fails(L.pmx_dbam_coverage_sections(h, 0, 4, 7, 4, buf.ctypes.data, 71, table.ctypes.data, 64), sec + "the buffer is too small")
        fails(L.pmx_dbam_coverage_sections(h, 12, 48, 7, 4, buf.ctypes.data, 4096, table.ctypes.data, 11), sec + "the table is too small")
        fails(L.pmx_dbam_coverage_sections(h, 12, 48, 7, 4, buf.ctypes.data, 4096, None, 0), sec + "the table is too small")
        fails(L.pmx_dbam_coverage_sections(h, 3, 2, 7, 4, None, 0, None, 0), sec + "the range holds two references")
        fails(L.pmx_dbam_coverage_sections(h, 0, n + 1, 7, 4, None, 0, None, 0), sec + "range outside the runs")
        for items in (0, 65536):
            fails(L.pmx_dbam_coverage_sections(h, 0, 4, 7, items, None, 0, None, 0), sec + "1 to 65535 items per section")
        assert L.pmx_dbam_coverage_sections(h, 0, 4, 7, 3, buf.ctypes.data, 96, table.ctypes.data, 2) == 96
        assert table[:2].tolist() == [[7, 0, 7, 72, 60], [7, 90, 7, 100, 36]]
        words = buf[:96].view("<u4").tolist()
        assert words[:6] == [7, 0, 72, 0, 0, 1 | 3 << 16] and words[6:9] == [0, 10, np.float32(1).view(np.uint32)]
        assert words[15:21] == [7, 90, 100, 0, 0, 1 | 1 << 16]
        # zoom: records before begin; bad arguments; a NULL buffer gives the size; short caps; the last level frees the bins
        zoom = "pmx_dbam_coverage_zoom_"
        fails(L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0), zoom + "records: no bins of that level")
        fails(L.pmx_dbam_coverage_zoom_begin(h, 32, 11, ids.ctypes.data, out.ctypes.data), zoom + "begin: at most 10 levels")
        fails(L.pmx_dbam_coverage_zoom_begin(h, 0, 1, ids.ctypes.data, out.ctypes.data), zoom + "begin: at most 10 levels")
        fails(L.pmx_dbam_coverage_zoom_begin(h, 32, 1, None, out.ctypes.data), zoom + "begin: null chromosome ids")
        fails(L.pmx_dbam_coverage_zoom_begin(h, 32, 1, ids.ctypes.data, None), zoom + "begin: null output")
        fails(L.pmx_dbam_coverage_zoom_begin(h, 32, 1, np.zeros(8, dtype=np.uint32).ctypes.data, out.ctypes.data), zoom + "begin: the chosen")
        assert L.pmx_dbam_coverage_zoom_begin(h, 32, 2, ids.ctypes.data, out.ctypes.data) == 0
        assert out.tolist() == [sum((e - s) * d * d for v in CC.restate(small["reads"], BC.SMALL_REFS, [1] * 8, 0)["runs"].values()
                                    for s, e, d in v), 1]
        size = L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0)
        assert size > 0 and size % 32 == 0
        rows = -(-(size // 32) // 4)
        big, t2 = np.zeros(size, dtype=np.uint8), np.zeros((rows, 5), dtype=np.uint32)
        fails(L.pmx_dbam_coverage_zoom_records(h, 0, 4, big.ctypes.data, size - 1, t2.ctypes.data, rows), zoom + "records: the buffer is too small")
        fails(L.pmx_dbam_coverage_zoom_records(h, 0, 4, big.ctypes.data, size, t2.ctypes.data, rows - 1), zoom + "records: the table is too small")
        fails(L.pmx_dbam_coverage_zoom_records(h, 0, 0, None, 0, None, 0), zoom + "records: at least 1 item")
        fails(L.pmx_dbam_coverage_zoom_records(h, 2, 4, None, 0, None, 0), zoom + "records: no bins of that level")
        assert L.pmx_dbam_coverage_zoom_records(h, 0, 4, big.ctypes.data, size, t2.ctypes.data, rows) == size
        assert int(t2[:, 4].sum()) == size and big[:4].view("<u4")[0] == 0
        assert L.pmx_dbam_coverage_zoom_records(h, 1, 4, None, 0, None, 0) > 0               # level 0 pulled: level 1 is still there
        size1 = L.pmx_dbam_coverage_zoom_records(h, 1, 4, None, 0, None, 0)
        assert L.pmx_dbam_coverage_zoom_records(h, 1, 4, big.ctypes.data, size, t2.ctypes.data, rows) == size1 <= size
        fails(L.pmx_dbam_coverage_zoom_records(h, 0, 4, None, 0, None, 0), zoom + "records: no bins of that level")   # the last level freed them
        acc.begin(r)                                                                        # a new table: the runs are gone
        every(no_runs)


def test_the_stream_peak_counts_the_zoom_bins(case):
    with DeviceStreamReader(case["bam"], window_bytes=WINDOW) as r:
        acc = r.arm_coverage(FC.MAPQ, None, 200)
        for _ in r._windows():
            pass
        acc.finish(r)
        before = r.stream_info()["peak_device_bytes"]
        assert before > 4 * sum(BC.LENGTHS)
        bins = sum(-(-l // 2) for l in BC.LENGTHS)                                          # level 0 at 2 bases per bin
        assert 28 * bins > before
        acc.zoom_begin(r, 2, 3, list(range(len(BC.REFS))))
        after = r.stream_info()["peak_device_bytes"]
        assert after > 28 * bins and after < before + 28 * bins * 4 // 3 + (1 << 20)
        for level in range(3):
            acc.zoom_records(r, level, 1024)
        assert r.stream_info()["peak_device_bytes"] >= after


def test_the_run_writes_the_file_at_its_own_estimate(tmp_path):
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=GOLDEN_TRACK, save_mappability_stats=False, stats=True)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage=True, coverage_format="bigwig", **kw)
    stem = "ENCFF000RMB-test"
    assert w1[-1].name == stem + "_coverage.bw" and sorted(os.listdir(tmp_path / "auto")) == sorted(p.name for p in w1)
    rows = dict(ln.rstrip("\n").split("\t") for ln in open(w1[-2]))
    extend = int(rows["Estimated library length"])
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(10))]
    host = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), extend)
    assert w1[-1].read_bytes() == coverage.write_bigwig(tmp_path / "host", "host", host).read_bytes() and host.n_runs > 100
    # an integer is counted on the reader that feeds the run and assembled while it is open
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 300, coverage=True, coverage_extend=extend, coverage_format="bigwig",
                           complexity=True, **kw)
    assert [p.name.rsplit("_", 1)[-1] for p in w2[-2:]] == ["complexity.tab", "coverage.bw"]
    assert sorted(os.listdir(tmp_path / "two")) == sorted(p.name for p in w2)               # (the temporary file is gone)
    assert w2[-1].read_bytes() == w1[-1].read_bytes()
