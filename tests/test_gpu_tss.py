"""pmx_dbam_tss_* on the GPU: the device against the restatement of tests/tss_cases, offset for offset and in
every total, for every flank, extend and choice of references, through every device reader, with and without excluded regions, a
stream window by window, beside a peak count and a fingerprint, and up to the run's table.  Everything is an integer and exact."""
import os
import threading

import numpy as np
import pytest

from pymasc_amd import complexity, fingerprint, peaks, pipeline, region_mask, tss
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import fixtures as fx
from tests import io_writers as W
from tests import sam_writers as SW
from tests import tss_cases as TC
from tests.test_tss import check_statistics, chosen, expected, golden_case

pytestmark = pytest.mark.gpu

FC = TC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
GOLDEN_TRACK = os.path.join(fx.GOLDEN, "hg19_36mer-test.bedGraph")
NAMES = [n for n, _l in TC.REFS]
LENGTHS = [l for _n, l in TC.REFS]
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows
X = PMX_BAM_DEFAULT_EXCLUDE
INVALID = -3


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_tss")
    rows = TC.synthetic()
    recs = FC.alignment_records(rows, TC.REFS)
    _sam, bam, gz = SW.write_twins(d, "ts", TC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, TC.REFS, SW.bam_bytes(TC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "ts.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, TC.REFS)))
    reads = FC.kept(rows)
    less = FC.masked(reads, TC.REFS, TC.MASK)
    assert 15_000 < len(less) < len(reads) < 21_000
    sites = TC.anchor_sites()
    bed = d / "sites.bed"
    bed.write_text("".join(TC.bed_text(sites)))
    return dict(dir=d, rows=rows, bam=bam, gz=gz, indexed=indexed, tag=tag, reads=reads, less=less, sites=sites, bed=str(bed), parts={})


def _want(case, flank, extend, use="all", masked=False):
    """The restatement, computed once per (flank, extend, masked) and left unchanged."""
    key = (flank, extend, masked)
    if key not in case["parts"]:
        case["parts"][key] = TC.restate_by_reference(case["less" if masked else "reads"], TC.REFS, case["sites"], flank, extend)
    return TC.combine(case["parts"][key], TC.USES[use])


@pytest.mark.parametrize("extend", TC.EXTENDS)
@pytest.mark.parametrize("flank", TC.FLANKS)
def test_the_profile_offset_for_offset_and_the_totals(case, flank, extend):
    TC.check_situations(case["reads"], TC.REFS, case["sites"], _want(case, flank, extend), flank, extend)
    with DeviceBamReader(case["bam"]) as r:
        for use in sorted(TC.USES):
            want = _want(case, flank, extend, use)
            acc = tss.DeviceCount(r, case["bed"], FC.MAPQ, chosen(use), flank, extend)
            assert acc.add(r) == (want["N"], want["n_near"])
            got = acc.copy(r)
            assert got.dtype == np.uint64 and got.shape == (2, 2 * flank + 1)
            assert got[0].tolist() == want["same"] and got[1].tolist() == want["opposite"]
            assert acc.totals(r).tolist() == [want["N"], want["n_near"], want["anchors"], want["pairs"]]
            c = acc.result(r)
            assert c == expected(want, flank, extend)
            check_statistics(c, want, flank)
            assert r.tss_profile(case["sites"], FC.MAPQ, chosen(use), flank, extend) == c    # a dict gives what the file gives


def _fifo_counts(case, tmp_path, mask, flank, extend, more=False):
    """The profile of the BAM file fed through a FIFO in windows of WINDOW bytes (``more``: beside a peak count and a fingerprint on
    the same reader), and the number of windows."""
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
            acc = r.arm_tss(case["sites"], FC.MAPQ, None, flank, extend)
            others = (r.arm_peaks(PEAKS, FC.MAPQ, None, extend), r.arm_fingerprint(FC.MAPQ, None, 500, extend)) if more else None
            for _ in r._windows():
                pass
            got = acc.result(r)
            if more:
                others = (others[0].result(r), others[1].result(r))
            windows = r.stream_info()["windows"]
    finally:
        t.join(60)
    os.unlink(fifo)
    return got, others, windows


PEAKS = {"f0": [(11_000, 13_000), (29_900, 30_200), (60_000, 60_500)], "f2": [(100, 900)]}


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("flank,extend", [(2000, 0), (50, 1)])
def test_every_reader_gives_the_whole_file_profile(case, tmp_path, flank, extend, masked):
    mask = region_mask.open_mask(TC.MASK) if masked else None
    whole = expected(_want(case, flank, extend, "all", masked), flank, extend)
    if masked:
        plain = _want(case, flank, extend)
        assert whole.N < plain["N"] and whole.pairs < plain["pairs"]

    def count(reader, references=None):
        if mask is not None:
            reader.set_exclude(mask.resolve(reader.references, reader.lengths))
        return reader.tss_profile(case["bed"], FC.MAPQ, references, flank, extend)
    with DeviceBamReader(case["bam"]) as r:
        assert count(r) == whole
        assert r.tss_profile(case["sites"], FC.MAPQ, None, flank, extend) == whole          # begin again: a table of its own
    with DeviceSamReader(case["gz"]) as r:
        assert count(r) == whole
    with DeviceBedReadsReader(case["tag"], NAMES, LENGTHS) as r:
        assert count(r) == whole
    part = expected(_want(case, flank, extend, "no middle", masked), flank, extend)
    with DeviceBamReader(case["indexed"], references=chosen("no middle")) as r:
        assert r.indexed
        c = count(r)
        assert c == part and c.anchors == whole.anchors - len(TC.ON_F1)
        with pytest.raises(ValueError):
            r.tss_profile(case["sites"], FC.MAPQ, [NAMES[1]], flank, extend)                # (not selected)
    got, _others, windows = _fifo_counts(case, tmp_path, mask, flank, extend)
    assert got == whole and windows >= 10


def test_beside_a_peak_count_and_a_fingerprint(case, tmp_path):
    flank, extend = 2000, 0
    whole = expected(_want(case, flank, extend), flank, extend)
    with DeviceBamReader(case["bam"]) as r:
        bins_alone = r.bin_counts(FC.MAPQ, None, 500, extend)
        peaks_alone = r.peak_counts(PEAKS, FC.MAPQ, None, extend)
        assert 0 < peaks_alone.n_in < peaks_alone.N
        fp = fingerprint.DeviceCount(r, FC.MAPQ, None, 500, extend)                         # three tables on one handle
        pk = peaks.DeviceCount(r, PEAKS, FC.MAPQ, None, extend)
        ts = tss.DeviceCount(r, case["sites"], FC.MAPQ, None, flank, extend)
        fp.add(r)
        ts.add(r)
        pk.add(r)
        assert ts.result(r) == whole and pk.result(r) == peaks_alone and fp.result(r) == bins_alone
    got, others, windows = _fifo_counts(case, tmp_path, None, flank, extend, more=True)
    assert windows >= 10 and got == whole and others[0] == peaks_alone and others[1] == bins_alone


def test_many_anchors_in_reach_of_every_read(case):
    sites = TC.many_sites()
    rows = TC.few(case["rows"])
    reads = FC.kept(rows)
    _sam, bam = SW.write_twins(case["dir"], "few", TC.REFS, FC.alignment_records(rows, TC.REFS))
    crowd = TC.many_sites(20_000, seed=23)          # more than one tile of the radix sort (8192 keys)
    for sites, flank, extend, each in ((sites, 500, 0, 20), (sites, 500, 1, 20), (crowd, 50, 0, 10)):
        want = TC.restate(reads, TC.REFS, [1, 1, 1], sites, flank, extend)
        assert len(sites["f0"]) in (3000, 20_000) and want["pairs"] > each * want["n_near"] and want["n_near"] > 0.9 * want["N"]
        assert want["N"] == len(reads) > 400
        with DeviceBamReader(bam) as r:
            assert r.tss_profile(sites, FC.MAPQ, None, flank, extend) == expected(want, flank, extend)


def test_add_twice_doubles_and_begin_resets(case):
    flank, extend = 2000, 0
    want = _want(case, flank, extend)
    with DeviceBamReader(case["bam"]) as r:
        n = r.decode(30)
        before, counters, runs = r._fetch(0, n), r.counters(), r.device_runs()
        acc = tss.DeviceCount(r, case["sites"], FC.MAPQ, None, flank, extend)
        assert acc.add(r) == acc.add(r) == (want["N"], want["n_near"])
        assert acc.copy(r).tolist() == [[2 * x for x in want["same"]], [2 * x for x in want["opposite"]]]
        assert acc.totals(r).tolist() == [2 * want["N"], 2 * want["n_near"], want["anchors"], 2 * want["pairs"]]
        acc.begin(r)
        assert not acc.copy(r).any() and acc.totals(r).tolist() == [0, 0, want["anchors"], 0]
        assert acc.add(r) == (want["N"], want["n_near"]) and acc.result(r) == expected(want, flank, extend)
        # the arrays, counters and runs of the last decode are as they were
        assert all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n)))
        assert r.counters() == counters and r.device_runs() == runs
        assert r._L.pmx_dbam_version() >= 16


def test_error_paths(case):
    with DeviceBamReader(case["bam"]) as r:
        L, h = r._L, r._h
        out, totals, table = np.zeros(2, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(2 * 101, dtype=np.uint64)

        def no_table():
            for call, what in ((lambda: L.pmx_dbam_tss_add(h, 0, X, out.ctypes.data), "add"),
                               (lambda: L.pmx_dbam_tss_copy(h, table.ctypes.data), "copy"),
                               (lambda: L.pmx_dbam_tss_totals(h, totals.ctypes.data), "totals")):
                rc = call()
                assert rc == INVALID
                with pytest.raises(PmxIOError, match="pmx_dbam_tss_{}: no table: call pmx_dbam_tss_begin first".format(what)):
                    r._raise(rc)
        no_table()
        pk = peaks.DeviceCount(r, PEAKS, FC.MAPQ, None, 0)
        held = pk.add(r)
        acc = tss.DeviceCount(r, case["sites"], FC.MAPQ, None, 50, 0)
        for call, what in ((lambda: L.pmx_dbam_tss_add(h, 0, X, None), "add"), (lambda: L.pmx_dbam_tss_copy(h, None), "copy"),
                           (lambda: L.pmx_dbam_tss_totals(h, None), "totals")):
            rc = call()
            assert rc == INVALID
            with pytest.raises(PmxIOError, match="pmx_dbam_tss_{}: null output".format(what)):
                r._raise(rc)
        # a refused begin leaves no table of this family and the peak table as it was
        ref, rev = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.uint8)
        beyond = np.array([5, LENGTHS[0] + 1], dtype=np.uint32)
        many = (1 << 20) + 1
        zeros = (np.zeros(many, dtype=np.int32), np.zeros(many, dtype=np.uint32), np.zeros(many, dtype=np.uint8))
        for args, message in (((2, ref.ctypes.data, beyond.ctypes.data, rev.ctypes.data, 50, 0, None), "anchor 1: position 100004 is outside f0"),
                              ((many, zeros[0].ctypes.data, zeros[1].ctypes.data, zeros[2].ctypes.data, 50, 0, None), "more than 2\\^20 anchors"),
                              ((2, ref.ctypes.data, beyond.ctypes.data, rev.ctypes.data, 4096, 0, None), "the flank is 4096"),
                              ((2, ref.ctypes.data, beyond.ctypes.data, rev.ctypes.data, 0, 0, None), "the flank is 0")):
            acc.begin(r)
            assert acc.add(r)[0] > 0
            assert L.pmx_dbam_tss_begin(h, *args) == INVALID
            with pytest.raises(PmxIOError, match="pmx_dbam_tss_begin: " + message):
                r._raise(INVALID)
            no_table()
            assert pk.add(r) == held and pk.totals(r)[0][0] > held[0]
        with pytest.raises(ValueError, match="not among the alignment's references"):
            r.tss_profile({"chrNotThere": [(1, "+")]}, FC.MAPQ)
        acc.begin(r)                                                                        # and a begin after it starts from zero
        assert acc.totals(r).tolist()[:2] == [0, 0] and acc.add(r)[0] > 0


def test_the_run_writes_the_table_and_nothing_else_changes(tmp_path):
    refs, reads, sites = golden_case()
    bed = tmp_path / "golden.bed"
    bed.write_text("".join(TC.bed_text(sites)))
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=GOLDEN_TRACK, save_mappability_stats=False)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 300, **kw)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 300, tss=str(bed), tss_flank=300, **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w0] == [stem + x for x in ("_cc.tab", "_mscc.tab", "_nreads.tab")]
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_tss.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, block = tss.read_tss(w1[-1])
    want = TC.restate(reads, refs, [1] * len(refs), sites, 300, 0)
    assert name == stem and block["Anchor file"] == str(bed) and c == expected(want, 300, 0)
    assert 0 < c.n_near < c.N and block["TSS enrichment"] == TC.statistics(want, 300)[2] == c.enrichment > 1
    # the 5' base and the chosen chromosomes, beside the other counts, in the order of the side counts: _tss.tab comes last
    chosen_refs = [refs[0][0], refs[2][0]]
    lines = {refs[0][0]: [(100, 5000)]}
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 300, references=chosen_refs, tss=sites, tss_extend=1, peaks=lines,
                           complexity=True, **kw)
    assert [p.name.rsplit("_", 1)[-1] for p in w2[-3:]] == ["complexity.tab", "peaks.tab", "tss.tab"]
    part = TC.restate(reads, refs, [1 if n in chosen_refs else 0 for n, _l in refs], sites, 2000, 1)
    assert tss.read_tss(w2[-1])[1] == expected(part, 2000, 1)
    with DeviceBamReader(GOLDEN_BAM) as r:
        assert peaks.read_peaks(w2[-2])[1] == r.peak_counts(lines, 10, chosen_refs)
        assert complexity.read_complexity(w2[-3])[1] == r.library_complexity(10, chosen_refs)
    # anchors that do not match a file's references: in run_files that sample is skipped, the other goes on
    other = [("x" + n, l) for n, l in refs]
    (tmp_path / "in").mkdir()
    _sam, renamed = SW.write_twins(tmp_path / "in", "renamed", other, [SW.rec("q0", 0, other[0][0], 100, 40, (("M", 36),))])
    out = pipeline.run_files([renamed, GOLDEN_BAM], str(tmp_path / "files"), 300, read_len=36, mapq_criteria=10, tss=str(bed), tss_flank=300)
    assert isinstance(out[0].error, ValueError) and "anchor file" in str(out[0].error) and out[0].written == []
    assert out[1].error is None and tss.read_tss(out[1].written[-1])[1] == c
