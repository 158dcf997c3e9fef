"""pmx_dbam_peakcount_* on the GPU: the device against the loop restatement of tests/peaks_cases, line for line
and in every total, through every device reader, with and without excluded regions, a stream window by window, beside a
fingerprint and a complexity count, and up to the run's table.  Everything is an integer and exact."""
import ctypes
import os
import threading

import numpy as np
import pytest

from pymasc_amd import complexity, fingerprint, peaks, pipeline, region_mask
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import fixtures as fx
from tests import io_writers as W
from tests import peaks_cases as PC
from tests import sam_writers as SW
from tests.test_peaks import golden_case

pytestmark = pytest.mark.gpu

FC = PC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
GOLDEN_TRACK = os.path.join(fx.GOLDEN, "hg19_36mer-test.bedGraph")
NAMES = [n for n, _l in PC.REFS]
LENGTHS = [l for _n, l in PC.REFS]
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_peaks")
    rows = PC.synthetic()
    recs = FC.alignment_records(rows, PC.REFS)
    assert any(r["flag"] & 0x400 for r in recs) and any(r["flag"] & 0x80 for r in recs) and any(r["flag"] & 0x4 for r in recs)
    _sam, bam, gz = SW.write_twins(d, "pk", PC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, PC.REFS, SW.bam_bytes(PC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "pk.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, PC.REFS)))
    reads = FC.kept(rows)
    less = FC.masked(reads, PC.REFS, PC.MASK)
    assert 15_000 < len(less) < len(reads) < 21_000
    lines = PC.peak_lines()
    bed = d / "lines.narrowPeak"
    bed.write_text("".join(PC.bed_text(lines, wide=True)))
    return dict(dir=d, rows=rows, bam=bam, gz=gz, indexed=indexed, tag=tag, reads=reads, less=less, lines=lines, bed=str(bed), want={})


def _want(case, extend, use="all", masked=False):
    """The restatement, computed once per parameter set and left unchanged."""
    key = (extend, use, masked)
    if key not in case["want"]:
        case["want"][key] = PC.restate(case["less" if masked else "reads"], PC.REFS, PC.USES[use], case["lines"], extend)
    return case["want"][key]


def _chosen(use):
    return [n for n, u in zip(NAMES, PC.USES[use]) if u]


def _expected(want, lines, extend):
    """The restatement as the PeakCounts the package must return."""
    return peaks.PeakCounts({n: tuple(zip(*lines[n])) if lines.get(n) else ([], []) for n in want["counts"]}, want["counts"], want["per_ref"],
                            want["union_bases"], want["genome_bases"], extend)


@pytest.mark.parametrize("extend", PC.EXTENDS)
def test_counts_line_for_line_and_totals(case, extend):
    lines = case["lines"]
    PC.check_situations(case["reads"], PC.REFS, lines, _want(case, extend), extend)
    with DeviceBamReader(case["bam"]) as r:
        for use in sorted(PC.USES):
            want = _want(case, extend, use)
            acc = peaks.DeviceCount(r, case["bed"], FC.MAPQ, _chosen(use), extend)
            assert acc.add(r) == (want["N"], want["n_in"])
            flat = [c for n in want["counts"] for c in want["counts"][n]]
            got = acc.counts(r)
            assert got.dtype == np.uint32 and got.tolist() == flat and len(flat) > 256          # line for line, in file order
            totals, per_ref = acc.totals(r)
            assert totals.tolist() == [want["N"], want["n_in"], want["union_bases"], len(flat)]
            assert [tuple(per_ref[i].tolist()) for i, u in enumerate(PC.USES[use]) if u] == list(want["per_ref"].values())
            assert not any(per_ref[i].any() for i, u in enumerate(PC.USES[use]) if not u)
            c = acc.result(r)
            assert c == _expected(want, lines, extend) and c.frip == want["n_in"] / want["N"]
            assert r.peak_counts(lines, FC.MAPQ, _chosen(use), extend) == c                  # a dict gives what the file gives
            part = np.zeros(5, dtype=np.uint32)                                              # a range of the raw counts
            assert r._L.pmx_dbam_peakcount_copy(r._h, len(flat) - 5, 5, part.ctypes.data) == 0 and part.tolist() == flat[-5:]


def _fifo_counts(case, tmp_path, mask, extend, more=False):
    """The counts of the BAM file fed through a FIFO in windows of WINDOW bytes (``more``: beside a fingerprint and a complexity
    count on the same reader), and the number of windows."""
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
            acc = r.arm_peaks(case["lines"], FC.MAPQ, None, extend)
            others = (r.arm_fingerprint(FC.MAPQ, None, 500, extend), r.arm_complexity(FC.MAPQ, None)) if more else None
            for _ in r._windows():
                pass
            got = acc.result(r)
            if more:
                others = (others[0].result(r), others[1].result())
            windows = r.stream_info()["windows"]
    finally:
        t.join(60)
    os.unlink(fifo)
    return got, others, windows


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("extend", PC.EXTENDS)
def test_every_reader_gives_the_whole_file_counts(case, tmp_path, extend, masked):
    mask = region_mask.open_mask(PC.MASK) if masked else None
    whole = _expected(_want(case, extend, "all", masked), case["lines"], extend)
    if masked:                      # the mask takes reads out of lines: the triple's common reads go
        plain = _want(case, extend)
        assert whole.N < plain["N"] and whole.n_in < plain["n_in"]

    def count(reader, references=None):
        if mask is not None:
            reader.set_exclude(mask.resolve(reader.references, reader.lengths))
        return reader.peak_counts(case["bed"], FC.MAPQ, references, extend)
    with DeviceBamReader(case["bam"]) as r:
        assert count(r) == whole
        assert r.peak_counts(case["lines"], FC.MAPQ, None, extend) == whole                 # begin again: a table of its own
    with DeviceSamReader(case["gz"]) as r:
        assert count(r) == whole
    with DeviceBedReadsReader(case["tag"], NAMES, LENGTHS) as r:
        assert count(r) == whole
    part = _expected(_want(case, extend, "no middle", masked), case["lines"], extend)
    with DeviceBamReader(case["indexed"], references=_chosen("no middle")) as r:
        assert r.indexed
        c = count(r)
        assert c == part and list(c.lines) == _chosen("no middle")
        with pytest.raises(ValueError):
            r.peak_counts(case["lines"], FC.MAPQ, [NAMES[1]], extend)                       # (not selected)
    got, _others, windows = _fifo_counts(case, tmp_path, mask, extend)
    assert got == whole and windows >= 10


def test_beside_a_fingerprint_and_a_complexity_count(case, tmp_path):
    extend = 200
    whole = _expected(_want(case, extend), case["lines"], extend)
    with DeviceBamReader(case["bam"]) as r:
        bins_alone = r.bin_counts(FC.MAPQ, None, 500, extend)
        nrf_alone = r.library_complexity(FC.MAPQ)
        fp = fingerprint.DeviceCount(r, FC.MAPQ, None, 500, extend)                         # both tables on one handle
        pk = peaks.DeviceCount(r, case["lines"], FC.MAPQ, None, extend)
        fp.add(r)
        pk.add(r)
        assert r.library_complexity(FC.MAPQ) == nrf_alone
        assert pk.result(r) == whole and fp.result(r) == bins_alone
    got, others, windows = _fifo_counts(case, tmp_path, None, extend, more=True)
    assert windows >= 10 and got == whole and others[0] == bins_alone and others[1] == nrf_alone


def test_more_lines_than_the_merge_workgroup_has_threads(case):
    lines = PC.many_lines()
    rows = PC.few(case["rows"])
    reads = FC.kept(rows)
    d = case["dir"]
    _sam, bam = SW.write_twins(d, "few", PC.REFS, FC.alignment_records(rows, PC.REFS))
    for extend in (0, 200):
        want = PC.restate(reads, PC.REFS, [1, 1, 1], lines, extend)
        assert len(lines["f0"]) == 3000 and max(want["hits"]) > 3
        with DeviceBamReader(bam) as r:
            assert r.peak_counts(lines, FC.MAPQ, None, extend) == _expected(want, lines, extend)


def test_add_twice_doubles_and_begin_resets(case):
    want = _want(case, 200)
    flat = [c for n in want["counts"] for c in want["counts"][n]]
    with DeviceBamReader(case["bam"]) as r:
        n = r.decode(30)
        before, counters, runs = r._fetch(0, n), r.counters(), r.device_runs()
        acc = peaks.DeviceCount(r, case["lines"], FC.MAPQ, None, 200)
        assert acc.add(r) == acc.add(r) == (want["N"], want["n_in"])
        assert acc.counts(r).tolist() == [2 * c for c in flat]
        assert acc.totals(r)[0].tolist() == [2 * want["N"], 2 * want["n_in"], want["union_bases"], len(flat)]
        acc.begin(r)
        assert not acc.counts(r).any() and acc.totals(r)[0].tolist() == [0, 0, want["union_bases"], len(flat)]
        assert acc.add(r) == (want["N"], want["n_in"]) and acc.counts(r).tolist() == flat
        # the arrays, counters and runs of the last decode are as they were
        assert all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n)))
        assert r.counters() == counters and r.device_runs() == runs
        assert r._L.pmx_dbam_version() >= 12


def test_error_paths(case):
    with DeviceBamReader(case["bam"]) as r:
        L, h = r._L, r._h
        out, totals, per_ref = np.zeros(2, dtype=np.uint64), np.zeros(4, dtype=np.uint64), np.zeros(6, dtype=np.uint64)
        some = np.zeros(4, dtype=np.uint32)
        for call, what in ((lambda: L.pmx_dbam_peakcount_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out.ctypes.data), "add"),
                           (lambda: L.pmx_dbam_peakcount_copy(h, 0, 4, some.ctypes.data), "copy"),
                           (lambda: L.pmx_dbam_peakcount_totals(h, totals.ctypes.data, per_ref.ctypes.data), "totals")):
            rc = call()
            assert rc == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_peakcount_{}: no table: call pmx_dbam_peakcount_begin first".format(what)):
                r._raise(rc)
        with pytest.raises(ValueError, match="no chromosome of the peak file is among the alignment's references"):
            r.peak_counts({"chrNotThere": [(1, 5)]}, FC.MAPQ)
        assert L.pmx_dbam_peakcount_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out.ctypes.data) == -3   # still no table
        acc = peaks.DeviceCount(r, case["lines"], FC.MAPQ, None, 0)
        for call, what in ((lambda: L.pmx_dbam_peakcount_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, None), "add"),
                           (lambda: L.pmx_dbam_peakcount_copy(h, 0, 4, None), "copy"),
                           (lambda: L.pmx_dbam_peakcount_totals(h, None, per_ref.ctypes.data), "totals"),
                           (lambda: L.pmx_dbam_peakcount_totals(h, totals.ctypes.data, None), "totals")):
            rc = call()
            assert rc == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_peakcount_{}: null output".format(what)):
                r._raise(rc)
        nlines = int(acc.layout.offsets[-1])
        assert L.pmx_dbam_peakcount_copy(h, nlines - 3, 4, some.ctypes.data) == -3
        with pytest.raises(PmxIOError, match="pmx_dbam_peakcount_copy: range outside the table"):
            r._raise(-3)
        off = np.array([0, 2, 1, 1], dtype=np.int64)                                        # offsets that do not ascend
        b = np.zeros(2, dtype=np.uint32)
        assert L.pmx_dbam_peakcount_begin(h, 3, off.ctypes.data, b.ctypes.data, b.ctypes.data, 0, None) == -3
        with pytest.raises(PmxIOError, match="pmx_dbam_peakcount_begin: offsets must ascend from 0"):
            r._raise(-3)
        assert L.pmx_dbam_peakcount_copy(h, 0, 1, some.ctypes.data) == -3                   # a failed begin leaves no table


def test_the_run_writes_the_table_and_nothing_else_changes(tmp_path):
    refs, reads, lines = golden_case()
    bed = tmp_path / "golden.narrowPeak"
    bed.write_text("".join(PC.bed_text(lines, wide=True)))
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=GOLDEN_TRACK, save_mappability_stats=False)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 300, **kw)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 300, peaks=str(bed), **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w0] == [stem + x for x in ("_cc.tab", "_mscc.tab", "_nreads.tab")]
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_peaks.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, block = peaks.read_peaks(w1[-1])
    want = PC.restate(reads, refs, [1] * len(refs), lines, 0)
    assert name == stem and block["Peak file"] == str(bed) and c == _expected(want, lines, 0)
    assert 0 < c.n_in < c.N and block["FRiP"] == want["n_in"] / want["N"] and block["Enrichment"] == c.enrichment > 1
    # an extension and the chosen chromosomes, beside the other counts, in the order they are asked for
    chosen = [refs[0][0], refs[2][0]]
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 300, references=chosen, peaks=lines, peaks_extend=200, complexity=True,
                           fingerprint=True, **kw)
    assert [p.name.rsplit("_", 1)[-1] for p in w2[-3:]] == ["complexity.tab", "fingerprint.tab", "peaks.tab"]
    part = PC.restate(reads, refs, [1 if n in chosen else 0 for n, _l in refs], lines, 200)
    assert peaks.read_peaks(w2[-1])[1] == _expected(part, lines, 200)
    with DeviceBamReader(GOLDEN_BAM) as r:
        assert fingerprint.read_fingerprint(w2[-2])[1] == r.bin_counts(10, chosen)
        assert complexity.read_complexity(w2[-3])[1] == r.library_complexity(10, chosen)
    # a peak file without a matching name: an error before any table; in run_files that sample is skipped, the other goes on
    with pytest.raises(ValueError, match="no chromosome of the peak file"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 300, peaks={"chrNotThere": [(1, 5)]}, **kw)
    assert not (tmp_path / "bad").exists()
    other = [("x" + n, l) for n, l in refs]
    (tmp_path / "in").mkdir()
    _sam, renamed = SW.write_twins(tmp_path / "in", "renamed", other, [SW.rec("q0", 0, other[0][0], 100, 40, (("M", 36),))])
    out = pipeline.run_files([renamed, GOLDEN_BAM], str(tmp_path / "files"), 300, read_len=36, mapq_criteria=10, peaks=str(bed))
    assert isinstance(out[0].error, ValueError) and "peak file" in str(out[0].error) and out[0].written == []
    assert out[1].error is None and peaks.read_peaks(out[1].written[-1])[1] == c
