"""pmx_dbam_bincount_* on the GPU: the device against the loop restatement of tests/fingerprint_cases, bin for
bin, table and totals, through every device reader, with and without excluded regions, a stream window by window, and up to the
command line."""
import ctypes
import os
import threading

import numpy as np
import pytest

from pymasc_amd import fingerprint, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PMX_BINCOUNT_HIST, PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import fingerprint_cases as FC
from tests import fixtures as fx
from tests import io_writers as W
from tests import sam_writers as SW
from tests.test_gpu_cli import _command

pytestmark = pytest.mark.gpu

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
NAMES = [n for n, _l in FC.REFS]
LENGTHS = [l for _n, l in FC.REFS]
WINDOW = 32 << 10                   # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_fingerprint")
    rows = FC.synthetic()
    recs = FC.alignment_records(rows, FC.REFS)
    assert any(r["flag"] & 0x400 for r in recs) and any(r["flag"] & 0x80 for r in recs) and any(r["flag"] & 0x4 for r in recs)
    _sam, bam, gz = SW.write_twins(d, "fp", FC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, FC.REFS, SW.bam_bytes(FC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "fp.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, FC.REFS)))
    reads = FC.kept(rows)
    assert len(reads) > 85_000 and {r[3] for r in reads} == {0, 1} and len({r[2] for r in reads}) >= 4
    return dict(dir=d, bam=bam, gz=gz, indexed=indexed, tag=tag, reads=reads, less=FC.masked(reads, FC.REFS), want={})


def _want(case, bin_size, extend, use="all", masked=False):
    """(counts, reads that added) of the restatement, computed once per parameter set and left unchanged."""
    key = (bin_size, extend, use, masked)
    if key not in case["want"]:
        case["want"][key] = FC.restate(case["less" if masked else "reads"], FC.REFS, FC.USES[use], bin_size, extend)
    return case["want"][key]


def _as_table(c):
    return list(zip(c.values.tolist(), c.bins.tolist()))


def _chosen(use):
    return [n for n, u in zip(NAMES, FC.USES[use]) if u]


@pytest.mark.parametrize("bin_size,extend", FC.PARAMS)
def test_bins_table_and_totals(case, bin_size, extend):
    with DeviceBamReader(case["bam"]) as r:
        for use in sorted(FC.USES):
            assert FC.wanted_situations(FC.REFS, FC.USES[use], bin_size, extend) <= \
                FC.situations(case["reads"], FC.REFS, FC.USES[use], bin_size, extend)
            counts, added = _want(case, bin_size, extend, use)
            have = dict(FC.table(counts))
            assert 4095 in have and 4096 in have and 5000 in have and max(have) >= PMX_BINCOUNT_HIST
            assert use != "all" or len(counts) > 256               # more than one workgroup of bins
            acc = fingerprint.DeviceCount(r, FC.MAPQ, _chosen(use), bin_size, extend)
            assert acc.add(r) == added
            got = acc.counts(r)
            assert got.dtype == np.uint32 and got.tolist() == counts                        # bin for bin
            hist, totals, tail = acc.tables(r)
            values, bins = np.unique(np.array(counts), return_counts=True)
            low = values < PMX_BINCOUNT_HIST
            want_hist = np.zeros(PMX_BINCOUNT_HIST, dtype=np.int64)
            want_hist[values[low]] = bins[low]
            assert hist.astype(np.int64).tolist() == want_hist.tolist()
            assert sorted(tail.tolist()) == sorted(c for c in counts if c >= PMX_BINCOUNT_HIST) and tail.size >= 2
            assert totals.tolist() == [len(counts), sum(counts), added]
            c = acc.result(r)
            assert _as_table(c) == FC.table(counts) and (c.B, c.T, c.reads) == (len(counts), sum(counts), added)
            assert c.per_reference == {n: l // bin_size for (n, l), u in zip(FC.REFS, FC.USES[use]) if u}
            assert r.bin_counts(FC.MAPQ, _chosen(use), bin_size, extend) == c
            part = np.zeros(5, dtype=np.uint32)                                            # a range of the raw counts
            assert r._L.pmx_dbam_bincount_copy(r._h, len(counts) - 5, 5, part.ctypes.data) == 0 and part.tolist() == counts[-5:]


def _fifo_counts(case, tmp_path, mask, bin_size, extend):
    """The table of the BAM file fed through a FIFO in windows of WINDOW bytes, and every window's first and last (ref, pos1)."""
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = open(case["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    t = threading.Thread(target=writer)
    t.start()
    edges = []
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r:
            assert not r.seekable
            if mask is not None:
                r.set_exclude(mask.resolve(r.references, r.lengths))
            acc = r.arm_fingerprint(FC.MAPQ, None, bin_size, extend)
            for _ in r._windows():
                n = r.decode(FC.MAPQ)
                if n:
                    ref, pos, _l, _s = r._fetch(0, n)
                    edges.append(((int(ref[0]), int(pos[0])), (int(ref[-1]), int(pos[-1]))))
            got = acc.result(r)
            r.disarm_fingerprint()
            windows = r.stream_info()["windows"]
    finally:
        t.join(60)
    os.unlink(fifo)
    return got, edges, windows


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("bin_size,extend", FC.PARAMS)
def test_every_reader_gives_the_whole_file_table(case, tmp_path, bin_size, extend, masked):
    mask = region_mask.open_mask(FC.MASK) if masked else None
    if masked:      # the intervals cut through a pile: some of its reads go, some stay; a whole pile goes too
        lo, hi, _per = FC.SPREAD
        spread = [r for r in case["reads"] if r[0] == 0 and lo <= r[1] < hi]
        left = [r for r in case["less"] if r[0] == 0 and lo <= r[1] < hi]
        assert 0 < len(left) < len(spread) and not any(r[0] == 2 and r[1] == FC.PILES[1][0] for r in case["less"])
    counts, added = _want(case, bin_size, extend, "all", masked)

    def count(reader, references=None):
        if mask is not None:
            reader.set_exclude(mask.resolve(reader.references, reader.lengths))
        return reader.bin_counts(FC.MAPQ, references, bin_size, extend)
    with DeviceBamReader(case["bam"]) as r:
        whole = count(r)
        assert _as_table(whole) == FC.table(counts) and whole.reads == added
        assert r.bin_counts(FC.MAPQ, None, bin_size, extend) == whole                       # begin again: a table of its own
    with DeviceSamReader(case["gz"]) as r:
        assert count(r) == whole
    with DeviceBedReadsReader(case["tag"], NAMES, LENGTHS) as r:
        assert count(r) == whole
    part, part_added = _want(case, bin_size, extend, "no middle", masked)
    with DeviceBamReader(case["indexed"], references=_chosen("no middle")) as r:
        assert r.indexed
        c = count(r)
        assert _as_table(c) == FC.table(part) and c.reads == part_added and list(c.per_reference) == _chosen("no middle")
        with pytest.raises(ValueError):
            r.bin_counts(FC.MAPQ, [NAMES[1]], bin_size, extend)                             # (not selected)
    got, edges, windows = _fifo_counts(case, tmp_path, mask, bin_size, extend)
    assert got == whole and windows >= 4
    if not masked:                  # a pile-up (thousands of reads on one position) lies on both sides of a cut
        piles = {(2, p) for p, _n in FC.PILES}
        assert any(a[1] == b[0] and a[1] in piles for a, b in zip(edges, edges[1:])), edges


def test_add_twice_doubles_and_begin_resets(case):
    counts, added = _want(case, 500, 200)
    with DeviceBamReader(case["bam"]) as r:
        n = r.decode(30)
        before, counters, runs = r._fetch(0, n), r.counters(), r.device_runs()
        acc = fingerprint.DeviceCount(r, FC.MAPQ, None, 500, 200)
        assert acc.add(r) == added and acc.add(r) == added
        assert acc.counts(r).tolist() == [2 * c for c in counts]
        hist, totals, tail = acc.tables(r)
        assert totals.tolist() == [len(counts), 2 * sum(counts), 2 * added]
        assert acc.counts(r).tolist() == [2 * c for c in counts]                            # hist does not clear the table
        acc.begin(r)
        assert not acc.counts(r).any() and acc.tables(r)[1].tolist() == [len(counts), 0, 0]
        assert acc.add(r) == added and acc.counts(r).tolist() == counts
        # the arrays, counters and runs of the last decode are as they were
        assert all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n)))
        assert r.counters() == counters and r.device_runs() == runs
        assert r._L.pmx_dbam_version() >= 11


def test_error_paths(case):
    with DeviceBamReader(case["bam"]) as r:
        L, h = r._L, r._h
        added = ctypes.c_uint64()
        hist, totals = np.zeros(PMX_BINCOUNT_HIST, dtype=np.uint64), np.zeros(3, dtype=np.uint64)
        some = np.zeros(4, dtype=np.uint32)
        for call, what in ((lambda: L.pmx_dbam_bincount_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(added)), "add"),
                           (lambda: L.pmx_dbam_bincount_hist(h, hist.ctypes.data, totals.ctypes.data, 0, None), "hist"),
                           (lambda: L.pmx_dbam_bincount_copy(h, 0, 4, some.ctypes.data), "copy")):
            rc = call()
            assert rc == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_bincount_{}: no table: call pmx_dbam_bincount_begin first".format(what)):
                r._raise(rc)
        with pytest.raises(PmxIOError, match="pmx_dbam_bincount_begin: no chosen reference is as long as one bin") as ei:
            r.bin_counts(FC.MAPQ, None, 100_004)
        assert ei.value.code == -3
        with pytest.raises(PmxIOError, match="no chosen reference is as long as one bin"):
            r.bin_counts(FC.MAPQ, [NAMES[1]], 500)
        with pytest.raises(PmxIOError, match="pmx_dbam_bincount_begin: the bin size is 0") as ei:
            r.bin_counts(FC.MAPQ, None, 0)
        assert ei.value.code == -3
        assert L.pmx_dbam_bincount_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(added)) == -3     # a failed begin leaves no table
        acc = fingerprint.DeviceCount(r, FC.MAPQ, None, 500, 0)
        for call, what in ((lambda: L.pmx_dbam_bincount_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, None), "add"),
                           (lambda: L.pmx_dbam_bincount_copy(h, 0, 4, None), "copy"),
                           (lambda: L.pmx_dbam_bincount_hist(h, None, totals.ctypes.data, 0, None), "hist"),
                           (lambda: L.pmx_dbam_bincount_hist(h, hist.ctypes.data, None, 0, None), "hist")):
            rc = call()
            assert rc == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_bincount_{}: null output".format(what)):
                r._raise(rc)
        nbins = int(acc.nb.sum())
        assert L.pmx_dbam_bincount_copy(h, nbins - 3, 4, some.ctypes.data) == -3
        with pytest.raises(PmxIOError, match="range outside the table"):
            r._raise(-3)


def test_golden_command(tmp_path):
    with BamReader(GOLDEN_BAM) as b:
        host = b.bin_counts(10)
    assert host.T > 0 and host.bin_size == 500
    argv = [GOLDEN_BAM, "-d", "300", "-r", "36", "-q", "10", "--skip-plots"]
    rc, err = _command("pymasc_amd", argv + ["-o", "plain"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", argv + ["-o", "with", "--fingerprint", "--fingerprint-control", GOLDEN_BAM], tmp_path)
    assert rc == 0, err
    plain, with_ = tmp_path / "plain", tmp_path / "with"
    table = "ENCFF000RMB-test_fingerprint.tab"
    assert sorted(os.listdir(with_)) == sorted(os.listdir(plain) + [table])
    for n in os.listdir(plain):
        assert (plain / n).read_bytes() == (with_ / n).read_bytes()
    name, c, block = fingerprint.read_fingerprint(with_ / table)
    assert name == "ENCFF000RMB-test" and c == host
    assert block["JS distance"] == 0.0 and block["Control"] == GOLDEN_BAM and block["Control mean"] == block["Mean"] == host.mean
    assert block["AUC"] == host.auc and block["Synthetic JS distance"] == host.synthetic_jsd
    # in the process: the device reader that feeds the run counts, beside the complexity count
    _r, w = pipeline.run(GOLDEN_BAM, str(tmp_path / "both"), 300, read_len=36, mapq_criteria=10, stats=True, complexity=True,
                         fingerprint=True)
    assert [p.name.rsplit("_", 1)[-1] for p in w[-2:]] == ["complexity.tab", "fingerprint.tab"] and len(w) == len(os.listdir(plain)) + 2
    assert fingerprint.read_fingerprint(w[-1])[1] == host
    for p in w[:-2]:
        assert p.read_bytes() == (plain / p.name).read_bytes()
