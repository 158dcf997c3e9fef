"""Indexed reading on the device (pmx_dbam_open_indexed + pmx_dbam_select, DeviceBamReader(references=...)): only the BGZF
members of the chosen chromosomes are read, copied and inflated, and the records are those of the host reader's index path
(libpymasc_io.so, BamReader.fetch) and of the whole-file device reader, array for array.  DESIGN.md 7.1."""
import multiprocessing as mp
import os
import shutil
import socket
import struct

import numpy as np
import pytest

from pymasc_amd import bam as B
from pymasc_amd import bam_device as D
from . import fixtures as fx
from . import io_writers as W

pytestmark = pytest.mark.gpu

GOLD = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
REFS = [("c1", 60000), ("c2", 5000), ("c3", 90000), ("c4", 70000), ("c5", 20000), ("c6", 40000)]


def _write(path, block, pseudo, seed=0, n=400):
    """Sorted records of c1, c3, c4, c6 (c2, c5 without reads) and a few unplaced unmapped ones at the end."""
    rng = np.random.default_rng(seed)
    ids = [0, 2, 3, 5]
    recs, meta = W.synth_bam_records(rng, [REFS[i] for i in ids], n)
    rec_refs = [ids[int(m)] for m in meta[:, 0]]
    recs = [r[:4] + struct.pack("<i", rid) + r[8:] for r, rid in zip(recs, rec_refs)]
    unmapped = [W.bam_record(-1, -1, 0, 4, []) for _ in range(3)]
    W.write_bam_indexed(path, REFS, recs + unmapped, rec_refs + [-1] * 3, block=block, pseudo_bin=pseudo)
    return str(path)


def _rows(batches):
    out = [np.concatenate(x) if x else np.empty(0) for x in zip(*batches)] if batches else [np.empty(0)] * 4
    return [np.asarray(a) for a in out]


def _same(a, b):
    assert len(a) == len(b) == 4
    for x, y in zip(a, b):
        assert x.shape == y.shape and (x.astype(np.int64) == y.astype(np.int64)).all()


def _fetch(r, name, mapq):
    return _rows(list(r.fetch(name, mapq, batch=97)))


def _members(path):
    """(file offset, total bytes, ISIZE) of every BGZF member."""
    data = open(path, "rb").read()
    out, p = [], 0
    while p < len(data):
        xlen, = struct.unpack_from("<H", data, p + 10)
        bsize, = struct.unpack_from("<H", data, p + 12 + 6 - 2)   # BC is the only subfield the writer puts in
        total = bsize + 1
        isize, = struct.unpack_from("<I", data, p + total - 4)
        out.append((p, total, isize))
        p += total
    return out


def _bai_ranges(path):
    """(beg, end) virtual offsets per reference from the pseudo-bin or bin 0 of a write_bam_indexed index."""
    d = open(path + ".bai", "rb").read()
    n, = struct.unpack_from("<i", d, 4)
    p, out = 8, []
    for _ in range(n):
        nbin, = struct.unpack_from("<i", d, p)
        p += 4
        rng = None
        for _ in range(nbin):
            _b, nc = struct.unpack_from("<Ii", d, p)
            p += 8
            if rng is None:
                rng = struct.unpack_from("<QQ", d, p)
            p += 16 * nc
        nint, = struct.unpack_from("<i", d, p)
        p += 4 + 8 * nint
        out.append(rng)
    return out


SUBSETS = [["c3"], ["c1", "c6"], ["c1", "c4", "c5"], [n for n, _ in REFS], ["c2"], ["c5", "c2"]]


@pytest.mark.parametrize("block,pseudo", [(0x4000, True), (0x4000, False), (0x1000, True), (0x1000, False)])
def test_subsets_match_host_index_and_whole_file(tmp_path, block, pseudo):
    path = _write(tmp_path / "s.bam", block, pseudo, seed=block + pseudo)
    with B.BamReader(path) as host, D.DeviceBamReader(path) as whole:
        assert not whole.indexed and whole.selected == whole.references
        for subset in SUBSETS:
            with D.DeviceBamReader(path, references=subset) as r:
                assert r.indexed and r.references == whole.references and r.lengths == whole.lengths
                assert r.selected == tuple(n for n, _ in REFS if n in subset)
                assert r.counters()["bytes_in"] <= os.path.getsize(path)
                for mapq in (0, 5, 30):
                    per = []
                    for name in r.selected:
                        got = _fetch(r, name, mapq)
                        _same(got, _fetch(host, name, mapq))
                        _same(got, _fetch(whole, name, mapq))
                        per.append(got)
                    # the whole selection in one decode: every chosen reference's records, in file order
                    _same(_rows(list(r.batches(mapq))), [np.concatenate(x) for x in zip(*per)])
                    n = r.decode(mapq)
                    assert n == sum(len(p[0]) for p in per)
                    if n:
                        assert all(r.device_arrays())
                runs = r.device_runs()
                assert [r.references[x[0]] for x in runs] == [n for n in r.selected if n not in ("c2", "c5")]
        # select again on the same handle replaces the stream
        with D.DeviceBamReader(path, references=[]) as r:
            assert r.selected == () and r.decode(0) == 0
            for subset in (["c4"], ["c1", "c3"]):
                r.select(subset)
                for name in subset:
                    _same(_fetch(r, name, 5), _fetch(host, name, 5))


@pytest.mark.parametrize("block", [0x4000, 0x1000])
def test_only_the_members_of_the_subset_are_read(tmp_path, block):
    path = _write(tmp_path / "b.bam", block, True, seed=7, n=1500)
    mem = _members(path)
    head_len = len(W.bam_header(REFS))
    ranges = _bai_ranges(path)
    hdr = set()
    o = 0
    for coff, total, isize in mem:
        if o >= head_len:
            break
        hdr.add(coff)
        o += isize
    for rid in (2, 3):
        beg, end = ranges[rid]
        cb, ce, ue = beg >> 16, end >> 16, end & 0xffff
        mine = {c for c, _t, _i in mem if cb <= c < ce or (ue and c == ce)}
        expect = sum(t for c, t, _i in mem if c in hdr | mine)
        with D.DeviceBamReader(path, references=[REFS[rid][0]]) as r:
            c = r.counters()
            assert c["bytes_in"] == expect and c["members"] == len(hdr | mine)
            assert c["bytes_in"] < os.path.getsize(path)


@pytest.mark.parametrize("mapq", [0, 1, 10, 30])
def test_reference_bam_single_chromosomes(mapq):
    """tests/golden/ENCFF000RMB-test.bam and its samtools .bai: each chromosome alone equals its rows of the reads table."""
    names, _lengths = fx.load_refs()
    rows = fx.load_reads(mapq)
    for name in names:
        with D.DeviceBamReader(GOLD, references=[name]) as r:
            assert r.indexed
            got = []
            for ref, pos, rl, rev in r.fetch(name, mapq):
                got += [(bool(v), r.references[a], int(p), int(l)) for a, p, l, v in zip(ref, pos, rl, rev)]
            assert got == [x for x in rows if x[1] == name], name


def _patched_index(tmp_path, src, fn):
    dst = tmp_path / "p.bam"
    shutil.copy(src, dst)
    raw = bytearray(open(src + ".bai", "rb").read())
    fn(raw)
    (tmp_path / "p.bam.bai").write_bytes(bytes(raw))
    return str(dst)


def _patch_ref(raw, rid, beg=None, end=None):
    """Moves the [beg, end) of reference rid in every bin of a write_bam_indexed index (the others are left alone)."""
    p = 8
    for r in range(rid + 1):
        nbin, = struct.unpack_from("<i", raw, p)
        p += 4
        for _ in range(nbin):
            _b, nc = struct.unpack_from("<Ii", raw, p)
            p += 8
            if r == rid:
                b0, e0 = struct.unpack_from("<QQ", raw, p)
                struct.pack_into("<QQ", raw, p, b0 if beg is None else beg, e0 if end is None else end)
            p += 16 * nc
        nint, = struct.unpack_from("<i", raw, p)
        p += 4 + 8 * nint


def test_bad_indexes_are_refused(tmp_path):
    path = _write(tmp_path / "g.bam", 0x1000, True, seed=3)
    ranges = _bai_ranges(path)
    fsize = os.path.getsize(path)

    def refused(p, names):
        with pytest.raises(B.PmxIOError) as e:
            D.DeviceBamReader(p, references=names)
        assert e.value.code == -2, str(e.value)

    # stale: the index of another file with the same header
    other = _write(tmp_path / "o.bam", 0x1000, True, seed=4, n=300)
    stale = tmp_path / "st.bam"
    shutil.copy(path, stale)
    shutil.copy(other + ".bai", str(stale) + ".bai")
    for names in (["c3"], ["c4"], ["c1", "c6"]):
        refused(str(stale), names)
    # a range start moved 3 bytes into the first record of c4
    d = tmp_path / "shift"
    d.mkdir()
    p = _patched_index(d, path, lambda raw: _patch_ref(raw, 3, beg=ranges[3][0] + 3))
    for names in (["c4"], ["c3", "c4"], [n for n, _ in REFS]):
        refused(p, names)
    # an offset past the end of the file
    d = tmp_path / "eof"
    d.mkdir()
    p = _patched_index(d, path, lambda raw: _patch_ref(raw, 2, end=(fsize + 100) << 16))
    refused(p, ["c3"])
    # another number of references than the header
    d = tmp_path / "nref"
    d.mkdir()
    p = _patched_index(d, path, lambda raw: raw.__setitem__(slice(4, 8), struct.pack("<i", len(REFS) + 1)))
    refused(p, ["c1"])
    # a truncated index
    d = tmp_path / "trunc"
    d.mkdir()
    p = _patched_index(d, path, lambda raw: raw.__delitem__(slice(len(raw) // 2, None)))
    refused(p, ["c1"])
    # unknown names; a name that was not selected
    with pytest.raises(ValueError):
        D.DeviceBamReader(path, references=["chrNope"])
    with D.DeviceBamReader(path, references=["c1"]) as r:
        with pytest.raises(ValueError):
            r.fetch("c3")
        with pytest.raises(ValueError):
            r.fetch("chrNope")
        with pytest.raises(ValueError):
            r.select(["c1", "chrNope"])


def test_without_an_index_references_open_the_whole_file(tmp_path):
    path = _write(tmp_path / "n.bam", 0x1000, False, seed=5)
    os.remove(path + ".bai")
    with D.DeviceBamReader(path) as whole, D.DeviceBamReader(path, references=["c3", "c4"]) as r:
        assert not r.indexed and r.selected == ("c3", "c4")
        assert r.counters()["bytes_in"] == os.path.getsize(path)
        for name in ("c3", "c4"):
            _same(_fetch(r, name, 5), _fetch(whole, name, 5))
        with pytest.raises(ValueError):
            r.fetch("c1")
    with D.DeviceBamReader(GOLD, references=["chr1"], index=False) as r:
        assert not r.indexed


# ---- tables ------------------------------------------------------------------------------------------------------
def _table_bytes(result, tmp, tag):
    from pymasc_amd import tables
    paths = tables.write_tables(os.path.join(str(tmp), tag + ".bam"), result)
    return [open(p, "rb").read() for p in paths]


def test_subset_tables_through_the_index_equal_the_host_run(tmp_path, monkeypatch):
    from pymasc_amd import pipeline, sharding
    from .fake_context import FakeContext
    path = _write(tmp_path / "t.bam", 0x1000, True, seed=9, n=900)
    calls = []
    orig = D.DeviceBamReader.select

    def spy(self, names):
        calls.append(list(names))
        return orig(self, names)

    monkeypatch.setattr(D.DeviceBamReader, "select", spy)
    for subset in (["c3"], ["c1", "c4", "c5"]):
        calls.clear()
        host = sharding.run_sharded(path, 120, 36, 10, references=subset, context=FakeContext())
        gpu = sharding.run_sharded(path, 120, 36, 10, references=subset, device=0, device_ingest=True)
        assert calls == [subset]                                          # the indexed path, one select
        assert _table_bytes(gpu, tmp_path, "g") == _table_bytes(host, tmp_path, "h")
    flt = [(True, ["c*"]), (False, ["c2", "c6"]), (True, ["c6"])]
    calls.clear()
    res_f, _ = pipeline.run(path, tmp_path / "f", 120, read_len=36, mapq_criteria=10, chromfilter=flt, device=0)
    assert calls == [["c1", "c3", "c4", "c5", "c6"]]
    res_r, _ = pipeline.run(path, tmp_path / "r", 120, read_len=36, mapq_criteria=10, references=["c1", "c3", "c4", "c5", "c6"],
                            device=0)
    host = sharding.run_sharded(path, 120, 36, 10, references=["c1", "c3", "c4", "c5", "c6"], context=FakeContext())
    assert _table_bytes(res_f, tmp_path, "f") == _table_bytes(res_r, tmp_path, "r") == _table_bytes(host, tmp_path, "h2")
    with pytest.raises(ValueError):
        pipeline.run(path, tmp_path / "x", 120, read_len=36, chromfilter=[(True, ["zz*"])], device=0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_worker(rank, world, port, q, path, tmp):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from pymasc_amd import bam_device, sharding
        seen = []
        orig = bam_device.DeviceBamReader.select

        def spy(self, names):
            orig(self, names)
            seen.append((list(names), self.counters()["bytes_in"]))

        bam_device.DeviceBamReader.select = spy
        res = sharding.run_sharded(path, 120, 36, 10, device=0, device_ingest=True)
        q.put((rank, _table_bytes(res, tmp, "rank%d" % rank), seen, None))
    except Exception as e:       # reported, not hung on
        q.put((rank, None, None, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks_on_one_gpu_read_their_own_members(tmp_path):
    from pymasc_amd import sharding
    path = _write(tmp_path / "r.bam", 0x1000, True, seed=11, n=1200)
    single = sharding.run_sharded(path, 120, 36, 10, device=0)
    expect = _table_bytes(single, tmp_path, "single")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, path, str(tmp_path))) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = [q.get(timeout=600) for _ in range(2)]
    finally:
        for p in procs:
            p.join(120)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs)
    shares = []
    for rank, tabs, seen, err in got:
        assert err is None, (rank, err)
        assert tabs == expect, rank
        assert len(seen) == 1 and seen[0][1] < os.path.getsize(path), (rank, seen)
        shares += seen[0][0]
    assert sorted(shares) == sorted(n for n, _ in REFS)
