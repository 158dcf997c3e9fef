"""The record chain of the device BAM reader under load (k_bam_spec / k_bam_walk and the repair rounds of walk_chain, DESIGN.md
7.1): the files of tests/chain_cases.py plant decoy records where the speculative step looks first, so that guesses are WRONG, not
only missing, and every consumer of the chain -- decode / fetch, the read-length histogram, complexity, fragments, the stream
reader's carry point and the indexed select -- must still see exactly the true records, as the host reader (serial by construction)
and the builders' own lists give them.  tests/test_chain_cases.py shows without a GPU that the fixtures bite.

A decoy on a reference that WAS chosen cannot be told apart from a record by any reader once an index points at it: an index is
believed as far as its ranges start on a record of a chosen reference, and a decoy is one, byte for byte.  That
is not tested here; the index test below points at a decoy of a reference that was not chosen."""
import os
import threading

import numpy as np
import pytest

from pymasc_amd import bam as B
from pymasc_amd import bam_device as D
from pymasc_amd import complexity, fragments
from pymasc_amd.stream_device import DeviceStreamReader
from tests import chain_cases as CC
from tests import io_writers as W
from tests.test_gpu_ingest_indexed import _members, _patch_ref, _patched_index

pytestmark = pytest.mark.gpu

BLOCKS = (0xff00, 257)                       # at 257 members are far smaller than a piece and records straddle members
EOF_MESSAGE = "file ends inside an alignment record"


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """{(case, block): path} of every case at both member sizes."""
    d = tmp_path_factory.mktemp("record_chain")
    out = {}
    for name in CC.CASES:
        refs, records, _truth = CC.case(name)
        for block in BLOCKS:
            out[name, block] = str(d / ("%s_%d.bam" % (name, block)))
            W.write_bam(out[name, block], refs, records, block=block, level=1)
    return out


def _reads(reader, mapq, **kw):
    out = []
    for ref, pos, rl, rev in reader.batches(mapq, **kw):
        out += [(reader.references[a], int(p), int(l), bool(v)) for a, p, l, v in zip(ref, pos, rl, rev)]
    return out


def _no_decoy(rows):
    return not any(r[0] == "decoy" or r[2] == 50 or r[3] for r in rows)


# ---- decode ----

@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", CC.CASES)
def test_decode_and_fetch(files, name, block):
    _refs, records, truth = CC.case(name)
    path = files[name, block]
    off = CC.summary(name)["off"]
    assert off > 0
    with B.BamReader(path) as h:
        host = {q: _reads(h, q) for q in (0, 40)}
    with D.DeviceBamReader(path) as r:               # (fake_chain: "record chain did not close" would be raised here)
        for q in (0, 40):
            got = _reads(r, q)
            assert _no_decoy(got)
            assert got == CC.kept(truth, q) and got == host[q]
        c = r.counters()
        assert c["records"] == len(records)
        # every piece whose guess is not the true start, wrong or missing, is walked again at least once, whatever the launch order
        # (no upper bound: it depends on that order)
        print("%s/%d: rewalked %d, the model's lower bound %d" % (name, block, c["rewalked"], off))
        assert c["rewalked"] >= off
        # a second decode with another filter on the resident chain (flagged reads and read2 records are kept)
        assert _reads(r, 0, flag_exclude=0) == CC.kept(truth, 0, 0)
        assert _reads(r, 31, flag_exclude=0) == []
        assert [x for b in r.fetch("decoy", 0, 0) for x in b[0].tolist()] == []
        assert [tuple(x) for b in r.fetch("true") for x in zip(*[a.tolist() for a in b])] == \
            [(0, p, l, v) for _n, p, l, v in CC.kept(truth, 0)]
        assert r.counters()["records"] == len(records)


# ---- read length ----

@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("name", CC.CASES)
def test_read_length_histogram(files, name, block):
    _refs, records, _truth = CC.case(name)
    with B.BamReader(files[name, block]) as h, D.DeviceBamReader(files[name, block]) as d:
        for q in (0, 40):
            exp, got = h.read_length_histogram(q), d.read_length_histogram(q)
            assert 50 not in got.lengths.tolist()
            assert got.counters == exp.counters
            assert (got.lengths.tolist(), got.counts.tolist(), got.first.tolist()) == \
                (exp.lengths.tolist(), exp.counts.tolist(), exp.first.tolist())
            assert got.counters["nreads"] == len(records) and got.counters["nunmapped"] == 0
            assert got.as_counter() == ({36: len(records)} if q == 0 else {})
        assert d.counters()["rewalked"] >= CC.summary(name)["off"]      # (the histogram closed the chain itself)


# ---- complexity ----

@pytest.mark.parametrize("block", BLOCKS)
def test_complexity(files, block):
    refs, _records, truth = CC.case("saturated")
    path = files["saturated", block]
    use = np.ones(len(refs), dtype=np.uint8)
    for q in (0, 40):
        with B.BamReader(path) as h:
            cols = [np.concatenate(x) for x in zip(*h.batches(q, complexity.COMPLEXITY_EXCLUDE))] if q == 0 else [[], [], [], []]
            want = complexity.count_host(*cols, len(refs))
        with D.DeviceBamReader(path) as r:
            per, hist = complexity.count_device(r, q, use)
        assert per.tolist() == want[0].tolist() and hist.tolist() == want[1].tolist()
        # every true record has a position of its own: one decoy (they repeat 500 positions) would move NRF and PBC1 off 1
        n = len(truth) if q == 0 else 0
        assert per.tolist() == [[n, n, n, 0], [0, 0, 0, 0]]


# ---- fragments ----

@pytest.mark.parametrize("block", BLOCKS)
def test_fragments(files, block):
    refs, _records, truth = CC.case("pairs")
    path = files["pairs", block]
    planted = [(0, p, size, 0) for (_r, p, _l, _v, _m, f), size in zip([t for t in truth if t[5] & 0x1], CC.PAIR_SIZES)]
    assert len(planted) == len(CC.PAIR_SIZES)
    for q in (0, 40):
        with B.BamReader(path) as h:
            host = [x for ref, start, size, orient, _c in fragments.rows_host(h, q)
                    for x in zip(ref.tolist(), start.tolist(), size.tolist(), orient.tolist())]
        with D.DeviceBamReader(path) as r:
            got = [tuple(x) for x in zip(*[a.tolist() for a in fragments.rows_device(r, q)])]
            table = fragments.count_device(r, q)
        assert got == host and got == (planted if q == 0 else [])
        assert table.counters["paired"] == table.counters["rows"] == len(got)
        assert table.counters["reads"] == (len(truth) if q == 0 else 0)
        at = np.argwhere(table.hist)
        assert [(int(o), int(s) + 1) for o, s in at] == ([(0, s) for s in CC.PAIR_SIZES] if q == 0 else [])


# ---- stream ----

def _through_a_fifo(tmp_path, path, window, mapq=0):
    fifo = str(tmp_path / ("fifo%d" % window))
    os.mkfifo(fifo)
    blob = open(path, "rb").read()

    def writer():
        try:
            with open(fifo, "wb") as fp:
                fp.write(blob)
        except BrokenPipeError:
            pass
    th = threading.Thread(target=writer, daemon=True)
    th.start()
    try:
        with DeviceStreamReader(fifo, window_bytes=window) as r:
            rows = _reads(r, mapq)
            return rows, r.stream_info()
    finally:
        th.join(60)


def test_stream_windows_cut_host_records(tmp_path):
    """``saturated`` in members of 2000 bytes through a FIFO, 512 compressed bytes per window: nearly every carry point lies inside or
    next to a host record, in windows of a single piece.  4096 and 16384 bytes per window: windows of several pieces, whose guesses
    are decoys, those behind a cut record included.  One window for the whole file gives the same."""
    refs, records, truth = CC.case("saturated")
    path = str(tmp_path / "members.bam")
    W.write_bam(path, refs, records, block=2000, level=1)
    rows, info = _through_a_fifo(tmp_path, path, 512)
    assert _no_decoy(rows) and rows == CC.kept(truth, 0)
    assert info["windows"] >= 10 and info["max_tail"] > 0
    for window in (4096, 16384):                             # (about 34 KB and 140 KB inflated: 3 and 9 pieces a window)
        rows, info = _through_a_fifo(tmp_path, path, window)
        assert rows == CC.kept(truth, 0) and info["windows"] >= 3 and info["max_tail"] > 0
    rows, info = _through_a_fifo(tmp_path, path, 1 << 22)
    assert rows == CC.kept(truth, 0) and info["windows"] == 1
    assert _through_a_fifo(tmp_path, path, 700, mapq=40)[0] == []


# ---- indexed ----

@pytest.fixture(scope="module")
def indexed(tmp_path_factory):
    """``saturated`` and 300 true records of a third reference behind it, with an index; a host of the file whose decoys end where
    it ends, and the offset of its first decoy in the inflated stream."""
    d = tmp_path_factory.mktemp("record_chain_indexed")
    _refs, records, truth = CC.case("saturated")
    refs = CC.REFS + [("other", 50_000)]
    others = [W.bam_record(2, 50 + 5 * j, 30, 16 * (j & 1), [("M", 36)], b"o") for j in range(300)]
    out = dict(refs=refs, truth=truth, others=[("other", 51 + 5 * j, 36, bool(j & 1)) for j in range(300)])
    for block in BLOCKS:
        out[block] = str(d / ("indexed_%d.bam" % block))
        W.write_bam_indexed(out[block], refs, records + others, [0] * len(records) + [2] * len(others), block=block, level=1)
    out["decoy_at"] = len(W.bam_header(refs)) + CC.first_decoys("saturated")[300]
    return out


@pytest.mark.parametrize("block", BLOCKS)
def test_indexed_select(indexed, block):
    path = indexed[block]
    want = {"true": CC.kept(indexed["truth"], 0), "other": indexed["others"]}
    with B.BamReader(path) as h:
        assert h.has_index()
        for name in want:
            assert [(name, p, l, v) for b in h.fetch(name, 0) for _r, p, l, v in zip(*[a.tolist() for a in b])] == want[name]
        assert _reads(h, 0) == want["true"] + want["other"]
    for names in (["true"], ["other"], ["true", "other"]):
        with D.DeviceBamReader(path, references=names) as r:
            assert r.indexed and r.selected == tuple(names)
            assert _reads(r, 0) == sum((want[n] for n in names), [])
            assert _reads(r, 40) == []
    with D.DeviceBamReader(path, references=["other"]) as r:          # back and forth on one handle
        for names in (["true"], ["other"], ["true", "other"], ["true"]):
            r.select(names)
            got = _reads(r, 0)
            assert _no_decoy([x for x in got if x[0] == "true"]) and got == sum((want[n] for n in names), [])
        assert r.counters()["rewalked"] > 0


@pytest.mark.parametrize("block", BLOCKS)
def test_an_index_that_points_at_a_decoy_is_refused(indexed, block, tmp_path):
    """The range of ``true`` starts on the first byte of a decoy whose run of decoys ends where its host ends: from there on the
    stream is a valid chain, and its first two records look like records.  They are records of ``decoy``, which was not chosen."""
    path = indexed[block]
    mem = _members(path)
    k, within = divmod(indexed["decoy_at"], block)
    with D.DeviceBamReader(path) as whole:
        at = sum(m[2] for m in mem[:k]) + within
        assert at == indexed["decoy_at"] and whole.inflated(at, CC.DECOY_LEN) == CC.decoy(300)
    p = _patched_index(tmp_path, path, lambda raw: _patch_ref(raw, 0, beg=(mem[k][0] << 16) | within))
    for names in (["true"], ["true", "other"]):
        with pytest.raises(B.PmxIOError, match="not selected") as e:
            D.DeviceBamReader(p, references=names)
        assert e.value.code == -2, str(e.value)
    with D.DeviceBamReader(p, references=["other"]) as r:            # (the range of ``other`` is as it was)
        assert _reads(r, 0) == indexed["others"]


# ---- errors ----

def _consumers(path, cls=D.DeviceBamReader):
    """What each consumer of the chain raises on ``path``: {name: message}; a consumer that returns is reported as such."""
    use = np.ones(len(CC.REFS), dtype=np.uint8)
    calls = {"decode": lambda r: _reads(r, 0), "read length": lambda r: r.read_length_histogram(0),
             "complexity": lambda r: complexity.count_device(r, 0, use), "fragments": lambda r: fragments.rows_device(r, 0)}
    out = {}
    for what, call in calls.items():
        with cls(path) as r:
            try:
                out[what] = "returned %r" % (call(r),)
            except B.PmxIOError as e:
                out[what] = "%d %s" % (e.code, e.msg)
                assert r.counters()["kept"] == 0         # no partial result
    return out


def _host_message(path):
    out = []
    for call in (lambda h: _reads(h, 0), lambda h: h.read_length_histogram(0)):
        with B.BamReader(path) as h:
            with pytest.raises(B.PmxIOError) as e:
                call(h)
            out.append("%d %s" % (e.value.code, e.value.msg))
    assert out[0] == out[1]
    return out[0]


@pytest.mark.parametrize("block", BLOCKS)
def test_the_stream_ends_inside_the_last_true_record(tmp_path, block):
    """The host of ``to_the_end`` claims 40 bytes more than the stream has, while its second decoy still ends exactly at the
    stream's end and is the guess of the last piece: the true record's error is reported, by every consumer, as the host reader
    words it."""
    refs, records = CC.to_the_end_cut()
    path = str(tmp_path / "cut.bam")
    W.write_bam(path, refs, records, block=block, level=1)
    want = _host_message(path)
    assert EOF_MESSAGE in want
    assert _consumers(path) == dict.fromkeys(("decode", "read length", "complexity", "fragments"), want)
    # the stream reader: the same error at its last window, not earlier -- the windows in front were delivered
    _refs, _records, truth = CC.case("to_the_end")
    path = str(tmp_path / "cut_members.bam")
    W.write_bam(path, refs, records, block=2000, level=1)
    got, windows = [], 0
    with DeviceStreamReader(path, window_bytes=512) as r:
        with pytest.raises(B.PmxIOError, match=EOF_MESSAGE) as e:
            for _ in r._windows():
                n = r.decode(0)
                ref, pos, rlen, rev = r._fetch(0, n)
                got += [(r.references[a], int(p), int(l), bool(v)) for a, p, l, v in zip(ref, pos, rlen, rev)]
                windows += 1
        info = r.stream_info()
    assert "%d %s" % (e.value.code, e.value.msg) == want
    assert info["bytes_in"] == os.path.getsize(path)            # everything had been read when it was raised
    assert windows >= 2 and info["windows"] == windows
    assert got and _no_decoy(got) and got == CC.kept(truth, 0)[:len(got)]


@pytest.mark.parametrize("block", BLOCKS)
def test_the_first_error_is_the_true_one(tmp_path, block):
    """A true record in piece 6 of ``every_piece`` with block_size = 7.  The pieces in front start from wrong guesses, two of
    which end in records that are none, and the pieces behind keep their decoy guesses; the error reported is the true record's."""
    refs, records, k = CC.every_piece_bs7()
    path = str(tmp_path / "bs7.bam")
    W.write_bam(path, refs, records, block=block, level=1)
    want = _host_message(path)
    assert "block_size < 32" in want
    assert _consumers(path) == dict.fromkeys(("decode", "read length", "complexity", "fragments"), want)
    # the stream reader, one window for the whole file (the open makes the first window current) and windows of a few members
    with pytest.raises(B.PmxIOError) as e:
        DeviceStreamReader(path, window_bytes=1 << 22)
    assert "%d %s" % (e.value.code, e.value.msg) == want
    _refs, _records, truth = CC.case("every_piece")
    path = str(tmp_path / "bs7_members.bam")
    W.write_bam(path, refs, records, block=2000, level=1)
    got = []
    with DeviceStreamReader(path, window_bytes=2048) as r:    # (about 26 KB inflated a window; the record is 106 KB in)
        with pytest.raises(B.PmxIOError) as e:
            for batch in r.batches(0):
                got += [(r.references[a], int(p), int(l), bool(v)) for a, p, l, v in zip(*batch)]
        assert r.stream_info()["windows"] >= 3
    assert "%d %s" % (e.value.code, e.value.msg) == want
    assert got and _no_decoy(got) and got == CC.kept(truth, 0)[:len(got)] and len(got) <= k
