"""pmx_dgc_* and pmx_dbam_gcbias_* on the GPU: the device against the loop restatement of tests/gcbias_cases,
element for element, through every device reader, with and without excluded regions, a stream window by window, and up to the
command line."""
import ctypes
import gzip
import os
import threading

import numpy as np
import pytest

from pymasc_amd import complexity, fingerprint, gcbias, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.gcbias import DeviceGenome
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import gcbias_cases as GC
from tests import io_writers as W
from tests import sam_writers as SW
from tests.test_gpu_cli import _command

pytestmark = pytest.mark.gpu

NAMES = [n for n, _l in GC.REFS]
LENGTHS = [l for _n, l in GC.REFS]
WINDOW = 32 << 10                   # compressed bytes per stream window: the file is cut into tens of windows


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_gcbias")
    text = GC.fasta_text()
    fasta, gz, bgz = str(d / "genome.fa"), str(d / "genome.fa.gz"), str(d / "genome.bgz.fa.gz")
    for path, blob in ((fasta, text), (gz, gzip.compress(text)), (bgz, W.bgzf_compress(text))):
        with open(path, "wb") as fp:
            fp.write(blob)
    rows = GC.synthetic()
    recs = GC.alignment_records(rows)
    assert any(r["flag"] & 0x400 for r in recs) and any(r["flag"] & 0x80 for r in recs) and any(r["flag"] & 0x4 for r in recs)
    _sam, bam, samgz = SW.write_twins(d, "gc", GC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, GC.REFS, SW.bam_bytes(GC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "gc.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(GC.tagalign_lines(rows)))
    reads = GC.kept(rows)
    assert len(reads) > 80_000 and {r[3] for r in reads} == {0, 1} and {r[2] for r in reads} == set(GC.READ_LENS)
    return dict(dir=d, fasta=fasta, gz=gz, bgz=bgz, bam=bam, samgz=samgz, indexed=indexed, tag=tag, reads=reads, less=GC.masked(reads))


@pytest.fixture(scope="module")
def genome(case):
    with DeviceGenome(case["fasta"]) as g:
        yield g


def _want(case, window, use="all", masked=False):
    """(N, F, off_end, blocked) of the restatement (its windows are made once per parameter set and left unchanged)."""
    return GC.restate(case["less" if masked else "reads"], GC.USES[use], window, masked)


def _chosen(use):
    return [n for n, u in zip(NAMES, GC.USES[use]) if u]


def _as_tuple(c):
    return c.N.tolist(), c.F.tolist(), c.off_end, c.blocked


def test_genome_handle(case, genome, tmp_path):
    g = GC.genome()
    assert genome.names == GC.FASTA_ORDER and genome.lengths == tuple(len(g[n]) for n in GC.FASTA_ORDER)
    for twin in (case["gz"], case["bgz"]):
        with DeviceGenome(twin) as t:
            assert (t.names, t.lengths) == (genome.names, genome.lengths)
    bad = tmp_path / "bad.fa"
    bad.write_text(">a\nACGT\nAC-T\n")
    with pytest.raises(PmxIOError, match="line 3: sequence byte that is not a letter") as ei:
        DeviceGenome(str(bad))
    assert ei.value.code == -2
    with pytest.raises(ValueError, match="line 3: sequence byte that is not a letter"):
        gcbias.HostGenome(str(bad))
    closed = DeviceGenome(case["fasta"])
    closed.close()
    assert closed.closed
    with DeviceBamReader(case["bam"]) as r, pytest.raises(ValueError, match="closed genome"):
        gcbias.DeviceCount(r, closed, GC.MAPQ, None, 64)


@pytest.mark.parametrize("window", GC.PARAMS)
def test_tables_and_totals(case, genome, window):
    with DeviceBamReader(case["bam"]) as r:
        for use in sorted(GC.USES):
            flags = GC.USES[use]
            assert GC.wanted_situations(flags, window, False) <= GC.situations(case["reads"], flags, window, False)
            N, F, off_end, blocked = _want(case, window, use)
            assert sum(N) + GC.blocked_windows(flags, window, False) == sum(max(0, l - window + 1) for l, u in zip(LENGTHS, flags) if u)
            assert N[0] > 0 and N[window] > 0
            acc = gcbias.DeviceCount(r, genome, GC.MAPQ, _chosen(use), window)
            assert acc.add(r) == (sum(F), off_end, blocked)                                 # the per-call out[3]
            windows, reads, totals = acc.tables(r)
            assert windows.dtype == np.uint64 and windows.tolist() == N and reads.tolist() == F
            assert totals.tolist() == [sum(N), sum(F), off_end, blocked]
            c = acc.result(r)
            assert _as_tuple(c) == (N, F, off_end, blocked) and c.window == window and c.genome == case["fasta"]
            assert c.per_reference == {n: max(0, l - window + 1) for (n, l), u in zip(GC.REFS, flags) if u}
            assert r.gc_bias(genome, GC.MAPQ, _chosen(use), window) == c
    with BamReader(case["bam"]) as b:                                                       # the host path says the same
        assert b.gc_bias(case["fasta"], GC.MAPQ, _chosen(use), window) == c


def _fifo_counts(case, genome, tmp_path, mask, window):
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
            acc = r.arm_gcbias(genome, GC.MAPQ, None, window)
            for _ in r._windows():
                n = r.decode(GC.MAPQ)
                if n:
                    ref, pos, _l, _s = r._fetch(0, n)
                    edges.append(((int(ref[0]), int(pos[0])), (int(ref[-1]), int(pos[-1]))))
            got = acc.result(r)
            r.disarm_gcbias()
            windows = r.stream_info()["windows"]
    finally:
        t.join(60)
    os.unlink(fifo)
    return got, edges, windows


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("window", [33, 100, 1024])
def test_every_reader_gives_the_whole_file_table(case, genome, tmp_path, window, masked):
    mask = region_mask.open_mask(GC.MASK) if masked else None
    if masked:      # a whole pile goes with the read filter; the read beside an interval stays and is blocked
        assert not any(r[:2] == GC.PILES[0][:2] for r in case["less"]) and GC.NEAR_READ in case["less"]
        assert GC.wanted_situations(GC.USES["all"], window, True) <= GC.situations(case["less"], GC.USES["all"], window, True)
    want = _want(case, window, "all", masked)

    def count(reader, references=None):
        if mask is not None:
            reader.set_exclude(mask.resolve(reader.references, reader.lengths))
        return reader.gc_bias(genome, GC.MAPQ, references, window)
    with DeviceBamReader(case["bam"]) as r:
        whole = count(r)
        assert _as_tuple(whole) == want
        assert r.gc_bias(case["fasta"], GC.MAPQ, None, window) == whole                     # begin again, from the path
    with DeviceSamReader(case["samgz"]) as r:
        assert count(r) == whole
    with DeviceBedReadsReader(case["tag"], NAMES, LENGTHS) as r:
        assert count(r) == whole
    part = _want(case, window, "no middle", masked)
    with DeviceBamReader(case["indexed"], references=_chosen("no middle")) as r:
        assert r.indexed
        c = count(r)
        assert _as_tuple(c) == part and list(c.per_reference) == _chosen("no middle")
        with pytest.raises(ValueError):
            r.gc_bias(genome, GC.MAPQ, [NAMES[1]], window)                                  # (not selected)
    got, edges, windows = _fifo_counts(case, genome, tmp_path, mask, window)
    assert got == whole and windows >= 4
    if not masked:                  # a pile (thousands of reads on one position) lies on both sides of a cut
        piles = {(ref, p) for ref, p, _n in GC.PILES}
        assert any(a[1] == b[0] and a[1] in piles for a, b in zip(edges, edges[1:])), edges


PEAK_LINES = {"g0": [(100, 30_000)], "g2": [(5, 900)]}
BIN, EXTEND = 500, 150


@pytest.fixture(scope="module")
def whole(case, genome):
    """``{masked: the five side counts of the whole-file reader, each through its own method}``; counted once, left unchanged."""
    out = {}
    for masked in (False, True):
        with DeviceBamReader(case["bam"]) as r:
            if masked:
                r.set_exclude(region_mask.open_mask(GC.MASK).resolve(r.references, r.lengths))
            out[masked] = dict(complexity=r.library_complexity(GC.MAPQ), fingerprint=r.bin_counts(GC.MAPQ, None, BIN, EXTEND),
                               peaks=r.peak_counts(PEAK_LINES, GC.MAPQ, None, EXTEND), coverage=r.coverage(GC.MAPQ, None, EXTEND),
                               gcbias=r.gc_bias(genome, GC.MAPQ, None, 100))
    return out


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
def test_all_five_counts_armed_on_one_stream(case, genome, whole, tmp_path, masked):
    want = whole[masked]
    assert want["complexity"].reads > want["fingerprint"].reads > 50_000 and want["peaks"].n_in > 0     # (flagged duplicates kept)
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
            if masked:
                r.set_exclude(region_mask.open_mask(GC.MASK).resolve(r.references, r.lengths))
            acc = {}                # armed in another order than the reader serves them in
            acc["gcbias"] = r.arm_gcbias(genome, GC.MAPQ, None, 100)
            acc["coverage"] = r.arm_coverage(GC.MAPQ, None, EXTEND)
            acc["complexity"] = r.arm_complexity(GC.MAPQ, None)
            acc["peaks"] = r.arm_peaks(PEAK_LINES, GC.MAPQ, None, EXTEND)
            acc["fingerprint"] = r.arm_fingerprint(GC.MAPQ, None, BIN, EXTEND)
            for _ in r._windows():
                pass
            got = {k: a.result() if k == "complexity" else a.result(r) for k, a in acc.items()}
            windows = r.stream_info()["windows"]
    finally:
        t.join(60)
    os.unlink(fifo)
    assert windows >= 4
    for kind in want:
        assert got[kind] == want[kind], kind


def test_a_second_pass_over_a_file_begins_the_tables_again(case, genome, whole):
    want = whole[False]
    with DeviceStreamReader(case["bam"], window_bytes=WINDOW) as r:
        assert r.seekable
        acc = dict(fingerprint=r.arm_fingerprint(GC.MAPQ, None, BIN, EXTEND), peaks=r.arm_peaks(PEAK_LINES, GC.MAPQ, None, EXTEND),
                   coverage=r.arm_coverage(GC.MAPQ, None, EXTEND), gcbias=r.arm_gcbias(genome, GC.MAPQ, None, 100))
        for _pass in range(2):      # the second pass opens a new handle: its tables begin at zero, so nothing is doubled
            for _ in r._windows():
                pass
        assert r.stream_info()["windows"] >= 4
        for kind, a in acc.items():
            assert a.result(r) == want[kind], kind
        nrf = r.arm_complexity(GC.MAPQ, None)       # its sums live on the host and are never begun again: armed for one pass
        for _ in r._windows():
            pass
        assert nrf.result() == want["complexity"]
        for kind, a in acc.items():                 # the four were begun once more for the third pass
            assert a.result(r) == want[kind], kind


def test_table_lifetime_and_state(case):
    N, F, off_end, blocked = _want(case, 64)
    with DeviceBamReader(case["bam"]) as r, DeviceBamReader(case["bam"]) as other:
        n = r.decode(30)
        before, counters, runs = r._fetch(0, n), r.counters(), r.device_runs()
        g = DeviceGenome(case["fasta"])
        acc = gcbias.DeviceCount(r, g, GC.MAPQ, None, 64)
        acc2 = gcbias.DeviceCount(other, g, GC.MAPQ, _chosen("no middle"), 100)            # one genome serves two readers
        g.close()                                                                           # ... and may be closed before add
        assert acc.add(r) == (sum(F), off_end, blocked) and acc.add(r) == (sum(F), off_end, blocked)
        windows, reads, totals = acc.tables(r)
        assert windows.tolist() == N and reads.tolist() == [2 * x for x in F]               # N stays, F and the counters double
        assert totals.tolist() == [sum(N), 2 * sum(F), 2 * off_end, 2 * blocked]
        acc2.add(other)
        assert _as_tuple(acc2.result(other)) == _want(case, 100, "no middle")
        with pytest.raises(ValueError, match="closed genome"):
            acc.begin(r)
        with DeviceGenome(case["fasta"]) as again:
            acc.genome = again
            acc.begin(r)                                                                    # begin resets
            windows, reads, totals = acc.tables(r)
            assert windows.tolist() == N and not reads.any() and totals.tolist() == [sum(N), 0, 0, 0]
            assert acc.add(r) == (sum(F), off_end, blocked) and _as_tuple(acc.result(r)) == (N, F, off_end, blocked)
        # the arrays, counters and runs of the last decode are as they were
        assert all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n)))
        assert r.counters() == counters and r.device_runs() == runs
        assert r._L.pmx_dbam_version() >= 14


def test_error_paths(case, genome, tmp_path):
    g = GC.genome()
    with DeviceBamReader(case["bam"]) as r:
        L, h = r._L, r._h
        out = (ctypes.c_uint64 * 3)()
        totals = np.zeros(4, dtype=np.uint64)
        some = np.zeros(65, dtype=np.uint64)
        use = np.ones(3, dtype=np.uint8)
        for call, what in ((lambda: L.pmx_dbam_gcbias_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out), "add"),
                           (lambda: L.pmx_dbam_gcbias_tables(h, some.ctypes.data, some.ctypes.data, 65, totals.ctypes.data), "tables")):
            rc = call()
            assert rc == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_gcbias_{}: no table: call pmx_dbam_gcbias_begin first".format(what)):
                r._raise(rc)
        for window in (0, 1025):
            assert L.pmx_dbam_gcbias_begin(h, genome._h, window, use.ctypes.data) == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_gcbias_begin: the window is {}: it must lie in \\[1, 1024\\]".format(window)):
                r._raise(-3)
        none = np.zeros(3, dtype=np.uint8)
        assert L.pmx_dbam_gcbias_begin(h, genome._h, 64, none.ctypes.data) == -3
        with pytest.raises(PmxIOError, match="pmx_dbam_gcbias_begin: no chosen reference"):
            r._raise(-3)
        assert L.pmx_dbam_gcbias_begin(h, None, 64, use.ctypes.data) == -3
        assert L.pmx_dbam_gcbias_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, out) == -3              # a failed begin leaves no table

        def fasta(name, records):
            p = tmp_path / name
            p.write_text("".join(">{}\n{}\n".format(n, s) for n, s in records))
            return str(p)
        with pytest.raises(PmxIOError, match="pmx_dbam_gcbias_begin: reference 'g2' has no record in the genome") as ei:
            r.gc_bias(fasta("renamed.fa", [("g0", g["g0"]), ("g1", g["g1"]), ("chr2", g["g2"])]), GC.MAPQ, None, 64)
        assert ei.value.code == -3
        shorter = fasta("shorter.fa", [("g0", g["g0"]), ("g1", g["g1"][:-1]), ("g2", g["g2"])])
        with pytest.raises(PmxIOError, match="reference 'g1' is 499 long in the alignment header and 498 in the genome"):
            r.gc_bias(shorter, GC.MAPQ, None, 64)
        assert _as_tuple(r.gc_bias(shorter, GC.MAPQ, _chosen("no middle"), 64)) == _want(case, 64, "no middle")   # g1 is not asked for
        acc = gcbias.DeviceCount(r, genome, GC.MAPQ, None, 64)
        for call, what in ((lambda: L.pmx_dbam_gcbias_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, None), "add"),
                           (lambda: L.pmx_dbam_gcbias_tables(h, some.ctypes.data, some.ctypes.data, 65, None), "tables"),
                           (lambda: L.pmx_dbam_gcbias_tables(h, None, some.ctypes.data, 65, totals.ctypes.data), "tables")):
            rc = call()
            assert rc == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_gcbias_{}: null output".format(what)):
                r._raise(rc)
        assert L.pmx_dbam_gcbias_tables(h, some.ctypes.data, some.ctypes.data, 64, totals.ctypes.data) == 65   # too little room: the size
        assert acc.add(r)[0] > 0
        # a genome on another device
        import torch
        if torch.cuda.device_count() > 1:
            with DeviceGenome(case["fasta"], device=1) as far:
                assert L.pmx_dbam_gcbias_begin(h, far._h, 64, use.ctypes.data) == -3
                with pytest.raises(PmxIOError, match="pmx_dbam_gcbias_begin: the genome is on device 1, the reads on device 0"):
                    r._raise(-3)
        else:
            with pytest.raises(PmxIOError, match="no such device"):
                DeviceGenome(case["fasta"], device=1)
    # a chosen reference shorter than the window is no error: it has no windows and all its reads are off_end
    with DeviceBamReader(case["bam"]) as r:
        c = r.gc_bias(genome, GC.MAPQ, [NAMES[1]], 1024)
        assert (c.windows, c.reads, c.blocked) == (0, 0, 0) and c.off_end == sum(1 for x in case["reads"] if x[0] == 1) > 100
        assert c.per_reference == {NAMES[1]: 0}


def test_command(case, tmp_path):
    bam, fasta = case["bam"], case["fasta"]
    argv = [bam, "-d", "300", "-r", "36", "-q", str(GC.MAPQ), "--skip-plots"]
    rc, err = _command("pymasc_amd", argv + ["-o", "plain"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", argv + ["-o", "with", "--gc-bias", fasta, "--gc-window", "64"], tmp_path)
    assert rc == 0, err
    plain, with_ = tmp_path / "plain", tmp_path / "with"
    table = "gc_gcbias.tab"
    assert sorted(os.listdir(with_)) == sorted(os.listdir(plain) + [table])
    for n in os.listdir(plain):
        assert (plain / n).read_bytes() == (with_ / n).read_bytes()
    with BamReader(bam) as b:
        host = gcbias.count_host(b, fasta, GC.MAPQ, None, 64)
    name, c, block = gcbias.read_gcbias(with_ / table)
    assert name == "gc" and c == host and _as_tuple(c) == _want(case, 64) and block["Genome"] == fasta
    assert block["Distance"] == host.distance and block["AT dropout"] == host.at_dropout
    # in the process: the device reader that feeds the run counts all three side tables
    _r, w = pipeline.run(bam, str(tmp_path / "three"), 300, read_len=36, mapq_criteria=GC.MAPQ, stats=True, complexity=True,
                         fingerprint=True, gc_bias=fasta, gc_window=64)
    assert [p.name.rsplit("_", 1)[-1] for p in w[-3:]] == ["complexity.tab", "fingerprint.tab", "gcbias.tab"]
    assert len(w) == len(os.listdir(plain)) + 3
    assert gcbias.read_gcbias(w[-1])[1] == host
    with BamReader(bam) as b:
        assert fingerprint.read_fingerprint(w[-2])[1] == b.bin_counts(GC.MAPQ)
        assert complexity.read_complexity(w[-3]) is not None
    for p in w[:-3]:
        assert p.read_bytes() == (plain / p.name).read_bytes()
