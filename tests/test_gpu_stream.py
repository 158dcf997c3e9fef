"""The windowed stream reader on the GPU: stdin through the command against the golden tables, the windows'
edges against the whole-file device reader, errors, the memory bound, a FIFO, and the large-file fallback."""
import gzip
import os
import shutil
import struct
import subprocess
import sys
import threading

import numpy as np
import pytest

from pymasc_amd import inputs, pipeline, stream_device, tables
from pymasc_amd.bam import PmxIOError
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.exceptions import InputUnseekable, ReadUnsortedError
from pymasc_amd.sharding import run_sharded
from pymasc_amd.stream_device import DeviceStreamReader

from . import fixtures as fx
from . import io_writers as W
from . import sam_cases as SC
from .test_gpu_run_files import GOLD, TABLES, _check_tables
from .test_gpu_stats import _check_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIGWIG = os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig")
REFS = [("c1", 400000), ("c2", 300000), ("c3", 200000)]


def _cli_stdin(data: bytes, cwd, argv, timeout=600):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, "-m", "pymasc_amd", "-"] + argv, input=data, cwd=str(cwd), env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    return p.returncode, p.stderr.decode("utf-8", "replace")


@pytest.mark.parametrize("kind", ["bam", "sam.bgzf", "sam"])
def test_golden_through_stdin(tmp_path, kind):
    bw = tmp_path / "hg19_36mer-test.bigwig"
    shutil.copy(BIGWIG, bw)
    if kind == "bam":
        data = open(GOLD + ".bam", "rb").read()
    else:
        data = open(SC.GOLDEN_SAM_GZ, "rb").read()
        if kind == "sam":
            data = gzip.decompress(data)
    rc, err = _cli_stdin(data, tmp_path, ["-r", "36", "-n", "S", "-m", bw.name, "-d", "300", "-q", "10", "--skip-plots",
                                          "-o", "out"])
    assert rc == 0, err
    out = tmp_path / "out"
    assert sorted(os.listdir(out)) == sorted("S" + s for s in TABLES + ["_stats.tab"])
    _check_tables([out / ("S" + s) for s in TABLES])
    _check_golden(out / "S_stats.tab", "S")


def _tables_of(path, reader, outdir, mapq=10):
    result = run_sharded(str(path), 300, 36, mapq, bam=reader, device=0)
    os.makedirs(outdir, exist_ok=True)
    written = tables.write_tables(os.path.join(outdir, "x.bam"), result)
    return {os.path.basename(p): open(p, "rb").read() for p in written}


def _records(rng, refs, n, edge_dups=0):
    recs, meta = W.synth_bam_records(rng, refs, n)
    if edge_dups:                     # runs of reads at one position (a window edge falls inside some of them)
        extra = [W.bam_record(0, 5000 + k // edge_dups, 30, 16 * (k & 1), [("M", 36)], b"dup%d" % k)
                 for k in range(edge_dups * 40)]
        recs = extra + [r for r, m in zip(recs, meta) if not (m[0] == 0 and m[1] < 5100)]
    return recs


CASES = {
    "straddling": dict(n=3000, block=0x1000, level=6, eof=True),
    "same_position_at_edges": dict(n=2000, block=0x800, level=6, eof=True, dups=50),
    "level0_members": dict(n=2000, block=0x2000, level=0, eof=True),
    "no_eof_marker": dict(n=2000, block=0x3000, level=6, eof=False),
    "long_record": dict(n=1500, block=0x1000, level=6, eof=True, long=True),
    "chromosome_change_at_edge": dict(n=1500, block=0x1000, level=6, eof=True, cut=True),
}


def _case_bam(path, case, rng):
    c = CASES[case]
    recs = _records(rng, REFS, c["n"], c.get("dups", 0))
    if c.get("long"):                 # a 45-KB record: longer than a whole window of one 4-KB member
        i = len(recs) // 3
        recs.insert(i, W.bam_record(1, 1, 40, 0, [("M", 36)], b"big", tags=b"XZZ" + b"a" * 45000 + b"\0"))
        recs.sort(key=lambda r: struct.unpack("<ii", r[4:12]))
    data = W.bam_header(REFS) + b"".join(recs)
    if c.get("cut"):                  # the last record of c1 ends exactly at a member's end
        first_c2 = next(k for k, r in enumerate(recs) if struct.unpack("<i", r[4:8])[0] == 1)
        head = W.bam_header(REFS) + b"".join(recs[:first_c2])
        blob = W.bgzf_compress(head, c["block"], c["level"], eof=False) + W.bgzf_compress(
            b"".join(recs[first_c2:]), c["block"], c["level"], c["eof"])
    else:
        blob = W.bgzf_compress(data, c["block"], c["level"], c["eof"])
    path.write_bytes(blob)
    return len(recs)


@pytest.mark.parametrize("case", sorted(CASES))
def test_window_edges_equal_the_whole_file(tmp_path, case):
    path = tmp_path / "w.bam"
    _case_bam(path, case, np.random.default_rng(len(case)))
    exp = _tables_of(path, DeviceBamReader(str(path)), tmp_path / "file")
    for window in (1, 20000):         # 1: one member per window
        with DeviceStreamReader(str(path), window_bytes=window) as r:
            got = _tables_of(path, r, tmp_path / ("s%d" % window))
            assert r.stream_info()["windows"] > 1
        assert got == exp


def test_batches_equal_the_file_reader(tmp_path):
    path = tmp_path / "b.bam"
    _case_bam(path, "straddling", np.random.default_rng(5))
    with DeviceBamReader(str(path)) as f:
        for mapq in (0, 10, 30):
            exp = [np.concatenate(x) for x in zip(*f.batches(mapq))]
            with DeviceStreamReader(str(path), window_bytes=6000) as s:
                got = [np.concatenate(x) for x in zip(*s.batches(mapq))]
            for a, b in zip(got, exp):
                np.testing.assert_array_equal(a, b)


def _err(fn):
    with pytest.raises(PmxIOError) as e:
        fn()
    return e.value.code


def _drain(path, window=4096):
    with DeviceStreamReader(str(path), window_bytes=window) as r:
        for _ in r.batches(0):
            pass


def test_errors_match_the_file_reader(tmp_path):
    rng = np.random.default_rng(7)
    recs = _records(rng, REFS, 1500)
    data = W.bam_header(REFS) + b"".join(recs)
    blob = W.bgzf_compress(data, 0x1000, 6, eof=False)
    members = []
    p = 0
    while p < len(blob):
        bsize = struct.unpack("<H", blob[p + 16:p + 18])[0]
        members.append(blob[p:p + bsize + 1])
        p += bsize + 1
    cases = {}
    cases["member"] = blob[:len(blob) - 100]
    cases["record"] = W.bgzf_compress(data[:len(data) - 10], 0x1000, 6, eof=True)
    bad = bytearray(members[-3])
    bad[-8] ^= 0xff                   # the CRC32 of a late member
    cases["crc"] = b"".join(members[:-3]) + bytes(bad) + b"".join(members[-2:])
    for name, b in cases.items():
        path = tmp_path / (name + ".bam")
        path.write_bytes(b)

        def whole():
            with DeviceBamReader(str(path)) as f:
                f.decode(0)
        assert _err(lambda: _drain(path)) == _err(whole), name
    gz = tmp_path / "plain.gz"
    gz.write_bytes(gzip.compress(data))
    assert _err(lambda: _drain(gz)) == -2


def test_unsorted_stream_raises_like_the_file(tmp_path):
    rng = np.random.default_rng(9)
    recs = _records(rng, REFS, 800)
    recs = recs[400:] + recs[:400]
    path = tmp_path / "u.bam"
    W.write_bam(str(path), REFS, recs, block=0x1000)
    with pytest.raises(ReadUnsortedError):
        run_sharded(str(path), 300, 36, 0, bam=DeviceBamReader(str(path)), device=0)
    with pytest.raises(ReadUnsortedError):
        with DeviceStreamReader(str(path), window_bytes=5000) as r:
            run_sharded(str(path), 300, 36, 0, bam=r, device=0)


def test_memory_is_bounded_by_the_window(tmp_path):
    rng = np.random.default_rng(11)
    refs = [("c1", 50_000_000)]
    recs, _m = W.synth_bam_records(rng, refs, 200_000)
    path = tmp_path / "big.bam"
    W.write_bam(str(path), refs, recs, level=0)         # level 0: >= 16 MB on disk
    size = os.path.getsize(path)
    assert size >= 16 << 20
    window = 256 << 10
    with DeviceStreamReader(str(path), window_bytes=window) as r:
        n = sum(b[0].size for b in r.batches(0))
        info = r.stream_info()
    with DeviceBamReader(str(path)) as f:
        assert n == f.decode(0)
    bound = 16 * window                                   # two window buffers of 4x the window, the record arrays, ...
    assert info["peak_device_bytes"] < bound < size // 4, info
    assert info["windows"] >= size // window


def test_fifo_reads_like_the_file_and_stdin_is_read_once(tmp_path):
    path = tmp_path / "f.bam"
    _case_bam(path, "straddling", np.random.default_rng(13))
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = path.read_bytes()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    t = threading.Thread(target=writer)
    t.start()
    try:
        assert inputs.is_stream(str(fifo))
        with inputs.open_alignments(str(fifo), True) as r:
            assert isinstance(r, DeviceStreamReader) and not r.seekable
            got = [np.concatenate(x) for x in zip(*r.batches(10))]
            with pytest.raises(InputUnseekable):
                next(r.batches(10))
            with pytest.raises(InputUnseekable):
                r.read_length_histogram(10)
    finally:
        t.join(60)
    with DeviceBamReader(str(path)) as f:
        exp = [np.concatenate(x) for x in zip(*f.batches(10))]
    for a, b in zip(got, exp):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("read_len", [36, None])
def test_large_file_fallback(tmp_path, monkeypatch, read_len):
    bam = tmp_path / "ENCFF000RMB-test.bam"
    shutil.copy(GOLD + ".bam", bam)
    bw = tmp_path / "t.bigwig"
    shutil.copy(BIGWIG, bw)
    common = dict(mapq_criteria=10, mappability_path=str(bw), device_ingest=True, stats=True)
    normal = pipeline.run_files([str(bam)], str(tmp_path / "normal"), 300, read_len=read_len, **common)
    opened = []
    real = stream_device.DeviceStreamReader

    class Spy(real):
        def __init__(self, *a, **k):
            opened.append(a[0])
            super().__init__(*a, **k)
    monkeypatch.setattr(stream_device, "DeviceStreamReader", Spy)
    monkeypatch.setattr(inputs, "device_ingest_budget", lambda device=0: 1000)
    out = pipeline.run_files([str(bam)], str(tmp_path / "fallback"), 300, read_len=read_len, **common)
    assert opened and all(p == str(bam) for p in opened)
    assert out[0].error is None and normal[0].error is None
    for s in TABLES + ["_stats.tab"]:
        name = "ENCFF000RMB-test" + s
        assert (tmp_path / "fallback" / name).read_bytes() == (tmp_path / "normal" / name).read_bytes()
    if read_len is None:
        with Spy(str(bam)) as r:
            from pymasc_amd import readlen
            assert readlen.estimate_from_reader(r, "MEDIAN", 10, 300) == 36
