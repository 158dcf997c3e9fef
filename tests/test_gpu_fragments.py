"""pmx_dbam_fragments_* and pmx_dbam_coverage_add_fragments on the GPU: the device against the host readers and
the loop restatement of tests/fragments_cases, through every device reader, with and without excluded regions, a stream window by
window, and up to the command line."""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

from pymasc_amd import coverage, fragments, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PmxIOError
from pymasc_amd.sam import DeviceSamReader, SamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import fragments_cases as FC
from tests import io_writers as W
from tests.test_gpu_cli import _command

pytestmark = pytest.mark.gpu

NAMES = [n for n, _l in FC.REFS]
LENGTHS = [l for _n, l in FC.REFS]
WINDOW = 32 << 10                   # compressed bytes per stream window


@functools.lru_cache(maxsize=None)
def lib():
    return FC.library()


@functools.lru_cache(maxsize=None)
def small_lib():
    recs = [r for _l, r in FC.planted()] + FC.random_pairs(random.Random(3), 3000)
    return [r for _i, r in sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))]


@functools.lru_cache(maxsize=None)
def want(max_size, use, masked):
    """(rows, counters, H) of the restatement of the whole library; made once per parameter set and left unchanged."""
    return FC.restate(lib(), FC.REFS, FC.USES[use], max_size, FC.MASK if masked else None)


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_fragments")
    out = {k: str(d / n) for k, n in (("bam", "pe.bam"), ("sam", "pe.sam"), ("gz", "pe.sam.gz"), ("indexed", "indexed.bam"),
                                      ("small", "small.bam"), ("small_sam", "small.sam"))}
    FC.write_bam(out["bam"], lib())
    FC.write_bam(out["indexed"], lib(), indexed=True)
    text = FC.sam_text(lib())
    with open(out["sam"], "wb") as fh:
        fh.write(text)
    with open(out["gz"], "wb") as fh:
        fh.write(W.bgzf_compress(text, 60_000))
    FC.write_bam(out["small"], small_lib())
    with open(out["small_sam"], "wb") as fh:
        fh.write(FC.sam_text(small_lib()))
    assert os.path.getsize(out["bam"]) > 4 * WINDOW and os.path.getsize(out["gz"]) > 4 * WINDOW
    out["dir"] = d
    return out


def _chosen(use):
    return [n for n, u in zip(NAMES, FC.USES[use]) if u]


def _masked(r):
    r.set_exclude(region_mask.open_mask(FC.MASK).resolve(r.references, r.lengths))


def _device(path, **kw):
    return DeviceBamReader(path, **kw) if path.endswith(".bam") else DeviceSamReader(path, **kw)


def _host(path):
    return BamReader(path) if path.endswith(".bam") else SamReader(path)


def _as_tuple(c):
    return [c.counters[k] for k in FC.COUNTERS], c.hist.tolist()


@pytest.mark.parametrize("kind", ["bam", "sam", "gz"])
def test_rows_equal_the_host_rows(case, kind):
    for use, masked, max_size in (("all", False, 65536), ("not_chrC", True, 2000)):
        with _host(case[kind]) as h:
            if masked:
                _masked(h)
            parts = list(fragments.rows_host(h, FC.MAPQ, _chosen(use), max_size))
        host = [np.concatenate([p[k] for p in parts]) for k in range(4)]
        with _device(case[kind]) as r:
            if masked:
                _masked(r)
            n = r.decode(30)
            before = r._fetch(0, n)
            got = fragments.rows_device(r, FC.MAPQ, _chosen(use), max_size)
            assert all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n)))       # the last decode's arrays stay
        assert [g.dtype for g in got] == [np.int32, np.int32, np.int32, np.uint8]
        assert all(np.array_equal(a, b) for a, b in zip(got, host))
        assert list(zip(*(g.tolist() for g in got))) == want(max_size, use, masked)[0]


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("max_size", FC.MAX_SIZES)
def test_tables_equal_the_restatement(case, max_size, masked):
    with DeviceBamReader(case["bam"]) as r:
        if masked:
            _masked(r)
        for use in sorted(FC.USES):
            rows, counters, hist = want(max_size, use, masked)
            acc = fragments.DeviceCount(r, FC.MAPQ, _chosen(use), max_size)
            assert acc.add(r) == len(rows)
            c = acc.result(r)
            assert c.hist.dtype == np.uint64 and _as_tuple(c) == (counters, hist) and c.max_size == max_size
            assert c.per_reference == {n: l for (n, l), u in zip(FC.REFS, FC.USES[use]) if u}
            k = c.counters
            assert k["paired"] == k["mate_unmapped"] + k["mate_elsewhere"] + k["no_size"] + sum(c.over) + k["rows"]
            assert k["rows"] - k["masked"] == int(c.hist.sum())
            assert r.fragment_sizes(FC.MAPQ, _chosen(use), max_size) == c
            assert acc.add(r) == len(rows)                                                  # calls add up until the next begin
            assert acc.result(r).hist.tolist() == [[2 * x for x in row] for row in hist]
    if max_size == 2000:
        assert hist[FC.FR][FC.PILE_SIZE - 1] > 65535 and masked == (counters[9] > 0)


@pytest.mark.parametrize("kind", ["sam", "gz"])
def test_sam_tables(case, kind):
    with DeviceSamReader(case[kind]) as r:
        _masked(r)
        for max_size in (2000, 65536):
            assert _as_tuple(r.fragment_sizes(FC.MAPQ, _chosen("not_chrC"), max_size)) == want(max_size, "not_chrC", True)[1:]


@pytest.mark.parametrize("n", [0, 1, 256, 257])
def test_edge_libraries(tmp_path, n):
    path = str(tmp_path / "edge.bam")
    FC.write_bam(path, FC.edge_library(n))
    rows, counters, hist = FC.restate(FC.edge_library(n), FC.REFS, FC.USES["all"], 2000)
    assert len(rows) == n
    with DeviceBamReader(path) as r:
        assert _as_tuple(r.fragment_sizes(FC.MAPQ, None, 2000)) == (counters, hist)
        assert list(zip(*(g.tolist() for g in fragments.rows_device(r, FC.MAPQ, None, 2000)))) == rows


@pytest.mark.parametrize("kind", ["bam", "gz"])
def test_a_stream_window_by_window_and_a_second_pass(case, kind):
    whole = dict(zip(("rows", "counters", "hist"), want(4097, "all", True)))
    with DeviceStreamReader(case[kind], window_bytes=WINDOW) as r:
        assert r.seekable
        _masked(r)
        acc = r.arm_fragments(FC.MAPQ, None, 4097)
        for _pass in range(2):      # the second pass opens a new handle: ``begin`` zeroes its table, so nothing is doubled
            for _ in r._windows():
                pass
            assert r.stream_info()["windows"] >= 4
            assert _as_tuple(acc.result(r)) == (whole["counters"], whole["hist"])
        r.disarm_fragments()
        assert _as_tuple(r.fragment_sizes(FC.MAPQ, None, 4097)) == (whole["counters"], whole["hist"])     # count_over: armed for one pass


def test_an_indexed_reader_with_a_subset(case):
    with DeviceBamReader(case["indexed"], references=_chosen("not_chrC")) as r:
        assert r.indexed
        c = r.fragment_sizes(FC.MAPQ, None, 2000)
        assert _as_tuple(c) == want(2000, "not_chrC", False)[1:] and list(c.per_reference) == _chosen("not_chrC")
        with pytest.raises(ValueError):
            r.fragment_sizes(FC.MAPQ, ["chrC"], 2000)                                       # (not selected)


@pytest.mark.parametrize("kind", ["small", "small_sam"])
def test_the_pair_pileup_equals_the_host(case, kind, tmp_path):
    for use, masked, max_size in (("all", False, 2000), ("not_chrC", True, 300)):
        with _host(case[kind]) as h:
            if masked:
                _masked(h)
            host = coverage.from_reader(h, FC.MAPQ, _chosen(use), "pair", max_size)
        assert host.reads > 500 and host.runs["chrB"][1][-1] == 50000                       # (clipped to the reference's end)
        with _device(case[kind]) as r:
            if masked:
                _masked(r)
            acc = coverage.DeviceCount(r, FC.MAPQ, _chosen(use), "pair", max_size)
            assert acc.add(r) == host.reads
            assert tuple(acc.finish(r)[k] for k in coverage.TOTALS) == host.totals
            assert b"".join(acc.text_chunks(r)) == b"".join(host.text_chunks())
            assert acc.result(r) == host and r.coverage(FC.MAPQ, _chosen(use), 0).extend == 0
    with DeviceStreamReader(case[kind], window_bytes=8 << 10) as r:
        _masked(r)
        acc = r.arm_coverage(FC.MAPQ, _chosen("not_chrC"), "pair", 300)
        for _ in r._windows():
            pass
        assert r.stream_info()["windows"] >= 4 and acc.result(r) == host


def test_a_bed_handle_has_no_mates(tmp_path):
    bed = tmp_path / "reads.tagAlign"
    bed.write_text("chrA\t100\t136\tr\t30\t+\nchrA\t200\t236\tr\t30\t-\n")
    with DeviceBedReadsReader(str(bed), NAMES, LENGTHS) as r:
        L, h = r._L, r._h
        out = ctypes.c_uint64()
        some = np.zeros(30, dtype=np.uint64)
        assert r.coverage(0).reads == 2
        rc = L.pmx_dbam_coverage_begin(h, 0, None)
        assert rc == 0
        for call in (lambda: L.pmx_dbam_fragments_begin(h, 2000, None),
                     lambda: L.pmx_dbam_fragments_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(out)),
                     lambda: L.pmx_dbam_fragments_tables(h, some.ctypes.data, some.ctypes.data),
                     lambda: L.pmx_dbam_fragments_rows(h, 0, PMX_BAM_DEFAULT_EXCLUDE, 2000, None, 0, None, None, None, None),
                     lambda: L.pmx_dbam_coverage_add_fragments(h, 0, PMX_BAM_DEFAULT_EXCLUDE, 2000, ctypes.byref(out))):
            assert call() == -3
            with pytest.raises(PmxIOError, match="the input has no mate fields"):
                r._raise(-3)
        with pytest.raises(PmxIOError, match="the input has no mate fields"):
            r.fragment_sizes(0)


def test_a_malformed_sam_line_is_the_hosts_error(tmp_path):
    recs = [r for r in lib() if r.flag & 0x40][:50]
    lines = FC.sam_text(recs).split(b"\n")
    bad_at = sum(1 for ln in lines if ln[:1] == b"@") + 30
    f = lines[bad_at].split(b"\t")
    for col, text in ((8, b"12x"), (7, b"-3"), (8, b"2147483648"), (8, b"")):
        g = list(f)
        g[col] = text
        path = tmp_path / "bad.sam"
        path.write_bytes(b"\n".join(lines[:bad_at] + [b"\t".join(g)] + lines[bad_at + 1:]))
        with SamReader(str(path)) as h:
            with pytest.raises(PmxIOError) as host:
                h.fragment_sizes(0)
        assert "line {}: ".format(bad_at + 1) in host.value.msg
        with DeviceSamReader(str(path)) as r:
            assert r.decode(0) > 0                                                          # (the fields the run reads are well formed)
            with pytest.raises(PmxIOError) as dev:
                r.fragment_sizes(0)
            assert (dev.value.code, dev.value.msg) == (-2, host.value.msg)
        with DeviceStreamReader(str(path)) as r:                                            # (line numbers count from the stream's start)
            with pytest.raises(PmxIOError) as dev:
                r.fragment_sizes(0)
            assert dev.value.msg == host.value.msg


def test_error_paths_and_table_lifetime(case):
    with DeviceBamReader(case["small"]) as r:
        L, h = r._L, r._h
        out = ctypes.c_uint64()
        some = np.zeros(3 * 2000, dtype=np.uint64)
        ten = np.zeros(10, dtype=np.uint64)
        for call, what in ((lambda: L.pmx_dbam_fragments_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(out)), "add"),
                           (lambda: L.pmx_dbam_fragments_tables(h, some.ctypes.data, ten.ctypes.data), "tables")):
            assert call() == -3
            with pytest.raises(PmxIOError, match="pmx_dbam_fragments_{}: no table: call pmx_dbam_fragments_begin first".format(what)):
                r._raise(-3)
        for bad in (0, 65537):
            assert L.pmx_dbam_fragments_begin(h, bad, None) == -3
            with pytest.raises(PmxIOError, match="max_size is {}: it must lie in \\[1, 65536\\]".format(bad)):
                r._raise(-3)
            assert L.pmx_dbam_fragments_rows(h, 0, PMX_BAM_DEFAULT_EXCLUDE, bad, None, 0, None, None, None, None) == -3
        assert L.pmx_dbam_fragments_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, ctypes.byref(out)) == -3    # a failed begin leaves no table
        assert L.pmx_dbam_coverage_add_fragments(h, 0, PMX_BAM_DEFAULT_EXCLUDE, 2000, ctypes.byref(out)) == -3
        with pytest.raises(PmxIOError, match="pmx_dbam_coverage_add_fragments: no table"):
            r._raise(-3)
        assert L.pmx_dbam_coverage_begin(h, 200, None) == 0
        assert L.pmx_dbam_coverage_add_fragments(h, 0, PMX_BAM_DEFAULT_EXCLUDE, 2000, ctypes.byref(out)) == -3
        with pytest.raises(PmxIOError, match="begun with an extend"):
            r._raise(-3)
        assert L.pmx_dbam_fragments_begin(h, 2000, None) == 0 and L.pmx_dbam_fragments_add(h, 0, PMX_BAM_DEFAULT_EXCLUDE, None) == -3
        n = L.pmx_dbam_fragments_rows(h, FC.MAPQ, PMX_BAM_DEFAULT_EXCLUDE, 2000, None, 0, None, None, None, None)
        assert n > 1000
        cols = [np.zeros(n, dtype=t) for t in (np.int32, np.int32, np.int32, np.uint8)]
        assert L.pmx_dbam_fragments_rows(h, FC.MAPQ, PMX_BAM_DEFAULT_EXCLUDE, 2000, None, n - 1, *(c.ctypes.data for c in cols)) == -3
        assert L.pmx_dbam_version() >= 15
        # the fingerprint's table and the fragments' live side by side
        fp = r.bin_counts(FC.MAPQ)
        c = r.fragment_sizes(FC.MAPQ)
        assert r.bin_counts(FC.MAPQ) == fp and r.fragment_sizes(FC.MAPQ) == c and c.n == n
        sec = (ctypes.c_double * 2)()                   # the row filter by the wall clock, k_fr_hist by HIP events, since begin
        assert L.pmx_dbam_fragments_timings(h, sec) == 0 and sec[0] > 0 and sec[1] > 0
        assert L.pmx_dbam_fragments_timings(h, None) == -3


def test_command(case, tmp_path):
    bam = case["small"]
    argv = [bam, "-d", "300", "-r", "36", "-q", str(FC.MAPQ), "--skip-plots"]
    rc, err = _command("pymasc_amd", argv + ["-o", "plain"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", argv + ["-o", "with", "--fragments", "--coverage-extend", "pair"], tmp_path)
    assert rc == 0, err
    plain, with_ = tmp_path / "plain", tmp_path / "with"
    new = ["small_coverage.bedGraph", "small_fragments.tab"]
    assert sorted(os.listdir(with_)) == sorted(os.listdir(plain) + new)
    for n in os.listdir(plain):
        assert (plain / n).read_bytes() == (with_ / n).read_bytes()
    with BamReader(bam) as b:
        sizes, pile = b.fragment_sizes(FC.MAPQ), coverage.from_reader(b, FC.MAPQ, None, "pair")
    name, c, _stats = fragments.read_fragments(with_ / new[1])
    assert name == "small" and c == sizes and _as_tuple(c) == FC.restate(small_lib(), FC.REFS, FC.USES["all"], 2000)[1:]
    assert coverage.read_coverage(with_ / new[0])[1] == pile
    # in the process: the device reader that feeds the run counts both, and the host path writes the same bytes
    _r, w = pipeline.run(bam, str(tmp_path / "dev"), 300, read_len=36, mapq_criteria=FC.MAPQ, fragments=True, coverage=True,
                         coverage_extend="pair")
    _r, wh = pipeline.run(bam, str(tmp_path / "cpu"), 300, read_len=36, mapq_criteria=FC.MAPQ, fragments=True, coverage=True,
                          coverage_extend="pair", device_ingest=False)
    assert [p.name for p in w[-2:]] == new and [p.name for p in wh[-2:]] == new
    for a, b_, n in zip(w[-2:], wh[-2:], new):
        assert a.read_bytes() == b_.read_bytes() == (with_ / n).read_bytes()
