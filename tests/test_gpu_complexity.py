"""pmx_dbam_complexity on the GPU: device == the restatement of tests/complexity_cases (a Counter over tuples),
per reference and histogram, through every device reader, whole files in any order, streams window by window, and up to the
command line."""
import os

import numpy as np
import pytest

from pymasc_amd import complexity, pipeline
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bed_reads_cases as BC
from tests import complexity_cases as CC
from tests import io_writers as W
from tests import sam_writers as SW
from tests.test_gpu_cli import _command

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_complexity")
    rng = np.random.default_rng(7)
    refs = CC.references(3)
    cols = CC.synthetic(rng, nref=3, n=2500, pile=150)      # (900 reads on one position: more than a stream window holds)
    recs = CC.alignment_records(rng, refs, *cols)
    sam, bam = SW.write_twins(d, "lib", refs, recs)
    order = np.random.default_rng(8).permutation(len(recs))
    unsorted_bam = str(d / "unsorted.bam")
    W.write_bam(unsorted_bam, refs, SW.bam_bytes(refs, [recs[i] for i in order]))
    small = str(d / "small_members.bam")                      # members of 4 KB: a stream of many windows
    W.write_bam(small, refs, SW.bam_bytes(refs, recs), block=4096)
    ids = {n: i for i, (n, _l) in enumerate(refs)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, refs, SW.bam_bytes(refs, recs), [ids[r["rname"]] for r in recs])
    lines = CC.tagalign_lines(refs, *cols, rng)
    bed, shuf = str(d / "lib.tagAlign"), str(d / "shuffled.tagAlign")
    open(bed, "w").write("".join(lines))
    open(shuf, "w").write("".join(BC.shuffled(lines, seed=3)))
    return dict(refs=refs, recs=recs, sam=sam, bam=bam, unsorted=unsorted_bam, small=small, indexed=indexed, lines=lines, bed=bed,
                shuffled=shuf, dir=d, names=[n for n, _l in refs])


def _want(files, mapq, use=None):
    kept = CC.kept_columns(files["refs"], files["recs"], mapq)
    CC.assert_sees_duplicates(*kept, above_bins=True)
    return CC.restate(*kept, len(files["refs"]), use)


@pytest.mark.parametrize("mapq", [0, 1, 30])
@pytest.mark.parametrize("kind", ["bam", "sam", "unsorted"])
def test_alignment_files(files, kind, mapq):
    want = _want(files, mapq)
    default = CC.restate(*CC.kept_columns(files["refs"], files["recs"], mapq, PMX_BAM_DEFAULT_EXCLUDE), 3)
    assert want != default                                  # flagged duplicates are in the file and they count
    cls = DeviceSamReader if kind == "sam" else DeviceBamReader
    with cls(files[kind]) as r:
        assert CC.as_tables(r.library_complexity(mapq), files["names"]) == want
        part = r.library_complexity(mapq, [files["names"][0], files["names"][2]])
        assert list(part.per_reference) == [files["names"][0], files["names"][2]]
        assert CC.as_tables(part, files["names"]) == _want(files, mapq, [1, 0, 1])


@pytest.mark.parametrize("mapq", [0, 30])
def test_bed_reads_sorted_and_shuffled(files, mapq):
    refs = files["refs"]
    want = CC.restate_lines(files["lines"], refs, mapq)
    N, D, _M1, M2 = CC.totals(want[0])
    assert D < N and M2 > 0 and want[1][0] > CC.BINS
    for path in (files["bed"], files["shuffled"]):
        with DeviceBedReadsReader(path, files["names"], [l for _n, l in refs]) as r:
            assert CC.as_tables(r.library_complexity(mapq), files["names"]) == want


def test_indexed_handle_after_select(files):
    names = files["names"]
    with DeviceBamReader(files["indexed"], references=[names[0], names[2]]) as r:
        assert r.indexed
        c = r.library_complexity(1)
        assert list(c.per_reference) == [names[0], names[2]]
        assert CC.as_tables(c, names) == _want(files, 1, [1, 0, 1])
        r.select([names[1]])
        assert CC.as_tables(r.library_complexity(1), names) == _want(files, 1, [0, 1, 0])


def test_null_output_is_refused(files):
    with DeviceBamReader(files["bam"]) as r:
        hist = np.zeros(32, dtype=np.uint64)
        rc = r._L.pmx_dbam_complexity(r._h, 0, CC.EXCLUDE_KEEP_DUP, None, None, hist.ctypes.data)
        assert rc == -3
        assert r._L.pmx_dbam_version() >= 9


def test_decode_arrays_are_untouched_and_the_order_does_not_matter(files):
    want = _want(files, 1)
    with DeviceBamReader(files["bam"]) as r:
        n = r.decode(30)
        before, counters, runs = r._fetch(0, n), r.counters(), r.device_runs()
        c = r.library_complexity(1)
        after = r._fetch(0, n)
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
        assert r.counters() == counters and r.device_runs() == runs
        assert CC.as_tables(c, files["names"]) == want
    with DeviceBamReader(files["bam"]) as r:                # the other order: complexity before any decode
        c2 = r.library_complexity(1)
        n2 = r.decode(30)
        assert n2 == n and all(np.array_equal(a, b) for a, b in zip(before, r._fetch(0, n2)))
        assert c2 == c


@pytest.fixture(scope="module")
def pile(tmp_path_factory):
    """10^6 ordinary reads over 3000 references and 10^5 reads on one (ref, pos1), both strands, three lengths."""
    d = tmp_path_factory.mktemp("pile")
    rng = np.random.default_rng(21)
    nref, n, npile = 3000, 1_000_000, 100_000
    refs = CC.references(nref, 100_000)
    ref = rng.integers(0, nref, size=n)
    pos = rng.integers(1, 99_000, size=n)
    ln = rng.choice(np.array([36, 35, 50]), size=n, p=[0.8, 0.1, 0.1])
    rev = rng.integers(0, 2, size=n)
    dup = rng.choice(n, size=n // 10, replace=False)
    rows = np.stack([ref, pos, ln, rev], axis=1)
    heap = np.stack([np.full(npile, 1500), np.full(npile, 4242), rng.choice(np.array([36, 35, 50]), size=npile),
                     rng.integers(0, 2, size=npile)], axis=1)
    rows = np.concatenate([rows, rows[dup], rows[dup[: n // 50]], heap])
    rows = rows[rng.permutation(len(rows))]
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    mapq = np.where(rng.random(len(rows)) < 0.2, rng.integers(0, 30, size=len(rows)), rng.integers(30, 61, size=len(rows)))
    flag = np.where(rows[:, 3] == 1, 16, 0) | np.where(rng.random(len(rows)) < 0.05, 0x400, 0)
    recs = [W.bam_record(r, p - 1, q, f, [("M", l)], b"r") for (r, p, l, _s), q, f in
            zip(rows.tolist(), mapq.tolist(), flag.tolist())]
    path = str(d / "pile.bam")
    W.write_bam(path, refs, recs, level=1)
    return dict(path=path, rows=rows, mapq=mapq, nref=nref, names=[n_ for n_, _l in refs])


@pytest.mark.parametrize("mapq", [0, 1, 30])
def test_pile_and_many_references(pile, mapq):
    rows = pile["rows"][pile["mapq"] >= mapq]
    cols = (rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3])
    CC.assert_sees_duplicates(*cols, above_bins=True)
    want = CC.restate(*cols, pile["nref"])
    assert want[1][0] > 10_000                              # the pile: tens of thousands of reads on one key
    use = (np.arange(pile["nref"]) % 3 != 0).astype(np.uint8)
    with DeviceBamReader(pile["path"]) as r:
        assert CC.as_tables(r.library_complexity(mapq), pile["names"]) == want
        per, hist = complexity.count_device(r, mapq, use)
        masked = CC.restate(*cols, pile["nref"], use)
        assert [tuple(int(x) for x in row) for row in per] == masked[0] and [int(x) for x in hist] == masked[1]
        assert masked[1][0] < want[1][0]                    # (the pile's reference is left out by the mask)


def test_stream_windows_add_up(files):
    want = _want(files, 1)
    with DeviceStreamReader(files["small"], window_bytes=4096) as r:
        acc = r.arm_complexity(1)
        edges, calls = [], 0
        for _ in r._windows():
            n = r.decode(1, CC.EXCLUDE_KEEP_DUP)
            ref, pos, _l, _s = r._fetch(0, n)
            if n:
                edges.append(((int(ref[0]), int(pos[0])), (int(ref[-1]), int(pos[-1]))))
            calls += 1
        r.disarm_complexity()
        info = r.stream_info()
        assert info["windows"] >= 3 and calls >= 3
        assert any(a[1] == b[0] for a, b in zip(edges, edges[1:]))      # a (ref, pos1) group straddles a window boundary
        assert CC.as_tables(acc.result(), files["names"]) == want
        assert r.library_complexity(1) == acc.result()                  # a regular file: one more pass gives the same
    with DeviceBamReader(files["bam"]) as whole:
        assert whole.library_complexity(1) == acc.result()


def test_unsorted_stream_is_refused(files):
    with DeviceStreamReader(files["unsorted"]) as r:
        with pytest.raises(PmxIOError, match="stream is not sorted by position") as ei:
            r.library_complexity(1)
        assert ei.value.code == -3


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """The golden library (a real ChIP-seq sample: its correlation has a peak for _stats.tab) with planted duplicates, some of
    them flagged: refs, records, path."""
    from pymasc_amd.bam import BamReader
    from tests import fixtures as fx
    d = tmp_path_factory.mktemp("library")
    rng = np.random.default_rng(33)
    with BamReader(os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")) as b:
        refs = list(zip(b.references, b.lengths))
        rows = np.stack([np.concatenate(x).astype(np.int64) for x in zip(*b.batches(10))], axis=1)
    n = len(rows)
    twice, more = rows[rng.choice(n, size=n // 8, replace=False)], rows[rng.choice(n, size=n // 30, replace=False)]
    heap = np.concatenate([np.tile(rows[7] * [1, 1, 1, 0] + [0, 0, 0, s], (40, 1)) for s in (0, 1)])
    rows = np.concatenate([rows, twice, more, more, more, heap, heap[:, [0, 1, 2, 3]] + [0, 0, -1, 0]])
    rows = rows[rng.permutation(len(rows))]
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    recs, prev = [], None
    for i, (r, p, l, s) in enumerate(rows.tolist()):
        flag = (16 if s else 0) | (0x400 if prev == (r, p, l, s) and i % 2 else 0)
        prev = (r, p, l, s)
        recs.append(SW.rec("q%d" % i, flag, refs[r][0], p, 5 if i % 17 == 0 else 40, (("M", l),)))
    _sam, bam = SW.write_twins(d, "lib", refs, recs)
    return dict(refs=refs, recs=recs, bam=bam, names=[n_ for n_, _l in refs])


def test_pipeline_and_command(library, tmp_path):
    files = library
    names = files["names"]
    kept = CC.kept_columns(files["refs"], files["recs"], 10)
    CC.assert_sees_duplicates(*kept, above_bins=True)
    want = CC.restate(*kept, len(names))
    assert want != CC.restate(*CC.kept_columns(files["refs"], files["recs"], 10, PMX_BAM_DEFAULT_EXCLUDE), len(names))
    kw = dict(read_len=36, mapq_criteria=10, stats=True)
    _r0, w0 = pipeline.run(files["bam"], str(tmp_path / "plain"), 300, **kw)
    _r1, w1 = pipeline.run(files["bam"], str(tmp_path / "with"), 300, complexity=True, **kw)
    assert [p.name for p in w1] == [p.name for p in w0] + ["lib_complexity.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    name, c, _ratios = complexity.read_complexity(w1[-1])
    assert name == "lib" and CC.as_tables(c, names) == want
    _r2, w2 = pipeline.run(files["bam"], str(tmp_path / "est"), 300, mapq_criteria=10, complexity=True)   # read length estimated
    assert CC.as_tables(complexity.read_complexity(w2[-1])[1], names) == want
    argv = [files["bam"], "-d", "300", "-r", "36", "-q", "10", "--skip-plots"]
    rc, err = _command("pymasc_amd", argv + ["-o", "cmd_plain"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", argv + ["-o", "cmd_with", "--complexity"], tmp_path)
    assert rc == 0, err
    plain, with_ = tmp_path / "cmd_plain", tmp_path / "cmd_with"
    assert sorted(os.listdir(with_)) == sorted(os.listdir(plain) + ["lib_complexity.tab"])
    for n in os.listdir(plain):
        assert (plain / n).read_bytes() == (with_ / n).read_bytes()
    assert CC.as_tables(complexity.read_complexity(with_ / "lib_complexity.tab")[1], names) == want
