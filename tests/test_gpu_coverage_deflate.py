"""The bigWig file with its sections compressed on the GPU: pmx_dbam_coverage_sections_z / _zoom_records_z
against the raw calls, the file of ``compress="device"`` read by the independent reader of tests/bigwig_out_cases (zlib inflates
it), by the host ``BigWigReader`` and by ``DeviceBigWigReader`` (the project's GPU inflater takes its own encoder's streams),
through every kind of input and up to the run; and the refusals."""
import os
import threading
import zlib

import numpy as np
import pytest

from pymasc_amd import coverage, pipeline, region_mask
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.bigwig import BigWigReader
from pymasc_amd.bigwig_device import DeviceBigWigReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import sam_writers as SW

pytestmark = pytest.mark.gpu

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
GOLDEN_TRACK = os.path.join(fx.GOLDEN, "hg19_36mer-test.bedGraph")
WINDOW = 8 << 10
EXTEND = 200


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """coverage_cases' library under the renamed references of bigwig_out_cases as BAM, SAM.gz and tagAlign; the restatement at
    extend 200, plain and masked, computed once each and left unchanged."""
    d = tmp_path_factory.mktemp("gpu_coverage_deflate")
    rows = CC.synthetic()
    recs = FC.alignment_records(rows, BC.REFS)
    _sam, bam, gz = SW.write_twins(d, "cv", BC.REFS, recs, bgzf_block=60_000)
    tag = str(d / "cv.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, BC.REFS)))
    reads = FC.kept(rows)
    want = {}
    for masked, use in ((False, reads), (True, FC.masked(reads, BC.REFS, BC.MASK))):
        w = CC.restate(use, BC.REFS, CC.USES["all"], EXTEND)
        want[masked] = w, BC.depth_lists(w, BC.REFS, CC.USES["all"])
    return dict(dir=d, bam=bam, gz=gz, tag=tag, want=want, raw={})


def _file(reader, base, compress, mask=None, extend=EXTEND, **kw):
    if mask is not None:
        reader.set_exclude(mask.resolve(reader.references, reader.lengths))
    acc = coverage.device_count_of(reader, FC.MAPQ, None, extend)
    return coverage.write_bigwig(base, "dev", acc, reader, compress=compress, **kw)


def _same_but_compressed(z, raw):
    assert z["compressed"] and not raw["compressed"] and z["largest"] == raw["largest"]      # uncompressBufSize: the largest RAW section
    assert {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in raw.items() if k != "compressed"}


def _split(blob, sizes):
    ends = np.cumsum(np.asarray(sizes).astype(np.int64))
    assert (int(ends[-1]) if len(ends) else 0) == len(blob)
    return [blob[int(z - n):int(z)] for z, n in zip(ends, sizes)]


@pytest.mark.parametrize("items", [1024, 4, 2048])
def test_the_compressed_pulls_against_the_raw_ones(case, items):
    with DeviceBamReader(case["bam"]) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, None, EXTEND)
        ranges = acc.ranges(r).tolist()
        n_sections = 0
        for k, (first, end) in enumerate(zip(ranges, ranges[1:])):
            if first == end:
                continue
            blob, table = acc.sections(r, first, end - first, k, items)
            bound = r._L.pmx_dbam_coverage_sections_z(r._h, first, end - first, k, items, None, 0, None, 0, None)
            zblob, ztable, zsizes = acc.sections_z(r, first, end - first, k, items)
            assert np.array_equal(ztable, table) and len(zblob) <= bound == sum(coverage.deflate_bound(int(x)) for x in table[:, 4])
            assert [zlib.decompress(s) for s in _split(zblob, zsizes)] == _split(blob, table[:, 4])
            n_sections += len(table)
        assert n_sections >= (4 if items >= 1024 else 1000)
        z0, levels = coverage.zoom_plan(BC.LENGTHS, acc.finish(r)["covered_bases"], acc.finish(r)["runs"])
        ids = [BC.chrom_ids(BC.NAMES)[n] for n in BC.NAMES]
        assert levels >= 4
        for z in (False, True):                             # the last level frees the bins: once raw, once compressed
            acc.zoom_begin(r, z0, levels, ids)
            out = [(acc.zoom_records_z if z else acc.zoom_records)(r, level, items) for level in range(levels)]
            if not z:
                raw = out
            with pytest.raises(PmxIOError, match="no bins of that level"):
                acc.zoom_records_z(r, 0, items)
        for (blob, table), (zblob, ztable, zsizes) in zip(raw, out):
            assert np.array_equal(ztable, table) and len(blob) > 0
            assert [zlib.decompress(s) for s in _split(zblob, zsizes)] == _split(blob, table[:, 4])


def _out_bam(d, refs, reads):
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    return SW.write_twins(d, "out", refs, recs)[1]


def _out_host(refs, reads, signal):
    c = coverage.count_host(*(np.array(x, dtype=np.int64) for x in zip(*reads)), [n for n, _l in refs], [l for _n, l in refs], [1] * len(refs), 0)
    return c.signal(1, 0.37) if signal else c


def _same_parts(got, z, want):
    """A raw pull and its compressed twin against the host's: the bytes, the table, and a signal's sums bit for bit."""
    assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(z[1], want[1]) and len(got) == len(want) == len(z) - 1
    assert [zlib.decompress(s) for s in _split(z[0], z[2])] == _split(want[0], want[1][:, 4])
    for sums in got[2:] + z[3:]:
        assert np.array_equal(sums.view(np.uint64), want[2].view(np.uint64))


@pytest.mark.parametrize("signal", [False, True], ids=["depth", "signal"])
@pytest.mark.parametrize("items", CC.OUT_ITEMS)
def test_sections_of_a_pull_from_a_references_fourth_run_on(tmp_path, items, signal):
    """k_tr_sections of both kinds, raw and compressed: a lane, a workgroup and one run more, in sections of every size around them,
    against ``HostParts.section_chunks`` over the same runs."""
    name = CC.OUT_REFS[1][0]
    host = _out_host(CC.OUT_REFS, CC.OUT_READS, signal)
    with DeviceBamReader(_out_bam(tmp_path, CC.OUT_REFS, CC.OUT_READS)) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, None, 0)
        if signal:
            acc.signal(r, 1, 0.37)
        first = int(acc.ranges(r, signal)[1]) + CC.OUT_FIRST
        assert first == CC.OUT_SHORT + CC.OUT_FIRST
        for n in CC.OUT_SECTION_COUNTS:
            cut = {name: tuple(x[CC.OUT_FIRST:CC.OUT_FIRST + n] for x in host.runs[name])}
            part = coverage.Signal(cut, 1, 0.37, CC.OUT_REFS) if signal else coverage.Coverage(cut, 0, 0, CC.OUT_REFS)
            want, = coverage.HostParts(part).section_chunks(1, 5, items, 1 << 30)
            assert len(want[1]) == -(-n // items)
            _same_parts(acc.sections(r, first, n, 5, items, signal), acc.sections_z(r, first, n, 5, items, signal), want)


@pytest.mark.parametrize("signal", [False, True], ids=["depth", "signal"])
@pytest.mark.parametrize("kept", CC.OUT_KEPT)
def test_zoom_records_of_a_level_with_empty_bins_between(tmp_path, kept, signal):
    """k_tr_zoom_emit of both kinds, raw and compressed: 1, 256 and 257 records, each in another slot than its bin's, in sections
    of 1 and of 3 (the last one short), against ``HostParts.zoom_records``."""
    refs, reads = CC.zoom_reads(kept)
    parts = coverage.HostParts(_out_host(refs, reads, signal))
    parts.zoom_begin(CC.OUT_ZOOM, 1, [0, 1])
    with DeviceBamReader(_out_bam(tmp_path, refs, reads)) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, None, 0)
        if signal:
            acc.signal(r, 1, 0.37)
        for items in (1, 3):
            want = parts.zoom_records(0, items)
            assert len(want[0]) == 32 * kept and len(want[1]) == -(-kept // items)
            got = []
            for pull in (acc.zoom_records, acc.zoom_records_z):         # (the only level is the last one: it frees the bins)
                acc.zoom_begin(r, CC.OUT_ZOOM, 1, [0, 1], signal)
                got.append(pull(r, 0, items, signal))
            _same_parts(got[0], got[1], want)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_every_input_writes_a_file_every_reader_takes(case, tmp_path, masked):
    mask = region_mask.open_mask(BC.MASK) if masked else None
    want, depths = case["want"][masked]
    with DeviceBamReader(case["bam"]) as r:
        plain = _file(r, tmp_path / "plain", False, mask)
        path = _file(r, tmp_path / "bam", "device", mask)
        again = _file(r, tmp_path / "again", "device", mask)
        host = _file(r, tmp_path / "host", True, mask)
    blob = path.read_bytes()
    assert path.name == "bam_coverage.bw" and again.read_bytes() == blob and len(blob) < len(plain.read_bytes()) // 2
    got, raw = BC.read_file(path), BC.read_file(plain)
    BC.check_file(got, want, BC.REFS, CC.USES["all"], depths)
    _same_but_compressed(got, raw)
    _same_but_compressed(BC.read_file(host), raw)           # --coverage-compress alone is what it was
    print("file bytes: raw {} device {} host zlib {}".format(len(plain.read_bytes()), len(blob), len(host.read_bytes())))
    # the host reader and the device reader (k_bgzf_inflate on k_df_deflate's streams) give the uncompressed file's arrays
    ids = BC.chrom_ids(BC.NAMES)
    with BigWigReader(path) as h, DeviceBigWigReader(str(path)) as d, BigWigReader(plain) as p:
        assert list(d.chromsizes.items()) == list(h.chromsizes.items()) == sorted(BC.REFS, key=lambda x: ids[x[0]])
        for name in BC.NAMES:
            ref = p.fetch_arrays(0.0, name)
            assert all(np.array_equal(a, b) for a, b in zip(h.fetch_arrays(0.0, name), ref))
            assert all(np.array_equal(a, b) for a, b in zip(d.fetch_arrays(0.0, name), ref))
        assert sum(p.fetch_arrays(0.0, n)[0].size for n in BC.NAMES) == want["n_runs"] > 3000
    assert coverage.read_bigwig(path).rows() == coverage.read_bigwig(plain).rows()
    # the other inputs write the same bytes: the encoder is a function of the sections alone
    with DeviceSamReader(case["gz"]) as r:
        assert _file(r, tmp_path / "gz", "device", mask).read_bytes() == blob
    with DeviceBedReadsReader(case["tag"], BC.NAMES, BC.LENGTHS) as r:
        assert _file(r, tmp_path / "tag", "device", mask).read_bytes() == blob
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    data = open(case["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(data)
    t = threading.Thread(target=writer)
    t.start()
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r:
            if mask is not None:
                r.set_exclude(mask.resolve(r.references, r.lengths))
            acc = r.arm_coverage(FC.MAPQ, None, EXTEND)
            for _ in r._windows():
                pass
            acc.finish(r)
            streamed = coverage.write_bigwig(tmp_path / "fifo_out", "dev", acc, r, compress="device")
            assert r.stream_info()["windows"] >= 10
    finally:
        t.join(60)
    assert streamed.read_bytes() == blob


def test_small_sections_no_read_and_the_pair_pileup(tmp_path):
    from tests import fragments_cases as FR
    import random
    reads = BC.small_reads()
    recs = [SW.rec("q%d" % i, 16 if s else 0, BC.SMALL_REFS[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    _sam, bam = SW.write_twins(tmp_path, "small", BC.SMALL_REFS, recs)
    want = CC.restate(reads, BC.SMALL_REFS, BC.SMALL_USE, 0)
    kw = dict(items_per_section=BC.SMALL_ITEMS, index_block=BC.SMALL_BLOCK, zoom_base=2)
    chosen = [n for (n, _l), u in zip(BC.SMALL_REFS, BC.SMALL_USE) if u]
    with DeviceBamReader(bam) as r:
        acc = coverage.device_count_of(r, FC.MAPQ, chosen, 0)
        dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r, compress="device", **kw)
        raw = coverage.write_bigwig(tmp_path / "raw", "dev", acc, r, **kw)
        acc = coverage.device_count_of(r, FC.MAPQ, ["z_empty"], 0)              # no kept read at all: no section, no level
        empty = coverage.write_bigwig(tmp_path / "empty", "dev", acc, r, compress="device", **kw)
        none = coverage.write_bigwig(tmp_path / "none", "dev", acc, r, **kw)
    got = BC.read_file(dev, BC.SMALL_BLOCK)
    BC.check_file(got, want, BC.SMALL_REFS, BC.SMALL_USE, BC.depth_lists(want, BC.SMALL_REFS, BC.SMALL_USE), 2, BC.SMALL_ITEMS)
    _same_but_compressed(got, BC.read_file(raw, BC.SMALL_BLOCK))
    got = BC.read_file(empty, BC.SMALL_BLOCK)
    assert got["runs"] == {} and got["zooms"] == [] and got["sections"] == [] and empty.read_bytes() == none.read_bytes()
    # "pair": the FR pairs at their own extent
    recs = [r for _l, r in FR.planted()] + FR.random_pairs(random.Random(3), 3000)
    recs = [r for _i, r in sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))]
    pe = str(tmp_path / "pe.bam")
    FR.write_bam(pe, recs)
    with DeviceBamReader(pe) as r:
        acc = coverage.device_count_of(r, FR.MAPQ, None, "pair", 2000)
        z = coverage.write_bigwig(tmp_path / "pez", "dev", acc, r, compress="device")
        p = coverage.write_bigwig(tmp_path / "pep", "dev", acc, r)
    _same_but_compressed(BC.read_file(z), BC.read_file(p))
    assert coverage.read_bigwig(z).rows() == coverage.read_bigwig(p).rows() and coverage.read_bigwig(z).n_runs > 500


def test_the_run_writes_the_compressed_file_at_its_own_estimate(tmp_path):
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=GOLDEN_TRACK, save_mappability_stats=False, coverage=True, coverage_format="bigwig")
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "z"), 300, coverage_compress="device", **kw)         # coverage_extend="auto"
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "raw"), 300, **kw)
    assert w1[-1].name == "ENCFF000RMB-test_coverage.bw" and sorted(os.listdir(tmp_path / "z")) == sorted(p.name for p in w1)
    _same_but_compressed(BC.read_file(w1[-1]), BC.read_file(w2[-1]))
    assert coverage.read_bigwig(w1[-1]).n_runs > 100
    with pytest.raises(ValueError, match="device ingest"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 300, coverage_compress="device", device_ingest=False, **kw)
    assert not (tmp_path / "bad").exists()


def test_refusals_states_and_the_stream_peak(case, tmp_path):
    with DeviceBamReader(case["bam"]) as r:
        L, h = r._L, r._h
        buf, table, zs = np.zeros(1 << 16, dtype=np.uint8), np.zeros((64, 5), dtype=np.uint32), np.zeros(64, dtype=np.uint32)

        def fails(rc, text, code=-3):
            assert rc == code
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc)
        no_runs = "no runs: call pmx_dbam_coverage_finish first"
        fails(L.pmx_dbam_coverage_sections_z(h, 0, 0, 0, 4, None, 0, None, 0, None), "pmx_dbam_coverage_sections_z: " + no_runs)
        fails(L.pmx_dbam_coverage_zoom_records_z(h, 0, 4, None, 0, None, 0, None), "pmx_dbam_coverage_zoom_records_z: " + no_runs)
        acc = coverage.DeviceCount(r, FC.MAPQ, None, EXTEND)
        acc.add(r)
        fails(L.pmx_dbam_coverage_sections_z(h, 0, 0, 0, 4, None, 0, None, 0, None), "pmx_dbam_coverage_sections_z: " + no_runs)
        acc.finish(r)
        first = int(acc.ranges(r)[0])
        sec = "pmx_dbam_coverage_sections_z: "
        assert L.pmx_dbam_coverage_sections_z(h, first, 8, 0, 5459, None, 0, None, 0, None) == coverage.deflate_bound(24 + 96)
        fails(L.pmx_dbam_coverage_sections_z(h, first, 8, 0, 5460, None, 0, None, 0, None), sec + "at most 5459 items")
        fails(L.pmx_dbam_coverage_sections_z(h, first, 8, 0, 4, buf.ctypes.data, 10, table.ctypes.data, 64, zs.ctypes.data), sec + "the buffer is too small")
        fails(L.pmx_dbam_coverage_sections_z(h, first, 8, 0, 4, buf.ctypes.data, buf.size, table.ctypes.data, 1, zs.ctypes.data), sec + "the table is too small")
        fails(L.pmx_dbam_coverage_sections_z(h, first, 8, 0, 4, buf.ctypes.data, buf.size, table.ctypes.data, 64, None), sec + "null output")
        got = L.pmx_dbam_coverage_sections_z(h, first, 8, 0, 4, buf.ctypes.data, buf.size, table.ctypes.data, 64, zs.ctypes.data)
        assert got == int(zs[:2].sum()) and table[:2, 4].tolist() == [72, 72]
        zoom = "pmx_dbam_coverage_zoom_records_z: "
        fails(L.pmx_dbam_coverage_zoom_records_z(h, 0, 4, None, 0, None, 0, None), zoom + "no bins of that level")
        acc.zoom_begin(r, 32, 1, [BC.chrom_ids(BC.NAMES)[n] for n in BC.NAMES])
        fails(L.pmx_dbam_coverage_zoom_records_z(h, 0, 2049, None, 0, None, 0, None), zoom + "at most 2048 items")
        assert L.pmx_dbam_coverage_zoom_records_z(h, 0, 2048, None, 0, None, 0, None) > 0
        with pytest.raises(ValueError, match="2048 items"):
            coverage.write_bigwig(tmp_path / "big", "dev", acc, r, compress="device", items_per_section=2049)
        assert os.listdir(tmp_path) == []
    # the scratch of the encoder counts in the stream's peak: above the bins of a level of 2 bases, which are the peak until then
    with DeviceStreamReader(case["bam"], window_bytes=WINDOW) as r:
        acc = r.arm_coverage(FC.MAPQ, None, EXTEND)
        for _ in r._windows():
            pass
        acc.finish(r)
        acc.zoom_begin(r, 2, 1, list(range(len(BC.REFS))))
        before = r.stream_info()["peak_device_bytes"]
        assert before > 28 * sum(-(-l // 2) for l in BC.LENGTHS)
        raw = r._L.pmx_dbam_coverage_zoom_records(r._h, 0, 1024, None, 0, None, 0)
        assert raw > 32 * 10_000 and r.stream_info()["peak_device_bytes"] < before + raw
        blob, table, zsizes = acc.zoom_records_z(r, 0, 1024)
        after = r.stream_info()["peak_device_bytes"]
        assert after >= before + raw + 4 * raw + len(blob)              # the records, a token slot per raw byte, the streams
        assert int(table[:, 4].sum()) == raw and after < before + 8 * raw
