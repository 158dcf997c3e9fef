"""pipeline.run_files on the host readers and the test context: several alignment files in one call, as `pymasc a.bam b.bam -n A B`
runs them -- the longest estimated read length for every file, the names of -n, the files that are skipped and the ones that
still run, the work done once per call (cache, track, context, device memory), and two gloo ranks."""
import logging
import os
import shutil

import numpy as np
import pytest

from pymasc_amd import bigwig, ffi, pipeline, sam
from pymasc_amd.calculator import CCHipCalculator
from pymasc_amd.chromfilter import NoTargetChromosomesError
from pymasc_amd.exceptions import ReadUnsortedError
from pymasc_amd.mappability import MappabilityStats
from tests import gcbias_cases as GC
from tests import io_writers as W
from tests import sam_writers as SW
from tests.fake_context import FakeContext

REFS = [("c1", 30000), ("c2", 20000)]
SHIFT = 120
MAPQ = 10


def _bam(path, read_len, seed, refs=REFS, unsorted=False):
    recs, _meta = W.synth_bam_records(np.random.default_rng(seed), refs, 500, readlen=read_len, mapq_lo=5)
    if unsorted:                                    # a read of c1 below its predecessor
        recs = recs[:300] + [recs[10]] + recs[300:]
    W.write_bam(str(path), refs, recs, block=3000)
    return str(path)


def _track(path):
    tracks = {"c1": [(100, 9000, 1.0), (12000, 29000, 1.0)], "c2": [(0, 18000, 1.0)]}
    W.write_bigwig(str(path), dict(REFS), tracks, items_per_block=40)
    return str(path)


def _bytes(paths):
    return {os.path.basename(str(p)): open(p, "rb").read() for p in paths}


def _single(tmp_path, tag, bam, read_len, **kw):
    """pipeline.run of one file in a directory of its own, with a fresh copy of the track (and so its own cache)."""
    d = tmp_path / tag
    d.mkdir()
    bw = _track(d / "m.bw")
    _r, written = pipeline.run(bam, d / "out", SHIFT, read_len=read_len, mapq_criteria=MAPQ, mappability_path=bw,
                               device_ingest=False, context=FakeContext(), **kw)
    return _bytes(written), (d / "m_mappability.json").read_text()


@pytest.fixture
def pair(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    return _bam(d / "r36.bam", 36, 1), _bam(d / "r50.bam", 50, 2)


def _many(tmp_path, paths, **kw):
    bw = tmp_path / "m.bw"
    if not bw.exists():
        _track(bw)
    kw.setdefault("context", FakeContext())
    return pipeline.run_files(paths, tmp_path / "out", SHIFT, mapq_criteria=MAPQ, mappability_path=str(bw),
                              device_ingest=False, **kw)


def test_estimates_differ_every_file_runs_with_the_longest(tmp_path, pair, caplog):
    caplog.set_level(logging.INFO)
    got = _many(tmp_path, list(pair), stats=True)
    warned = [r for r in caplog.records if "multiple read length candidates" in r.getMessage()]
    assert len(warned) == 1 and "Use max length (50)" in warned[0].getMessage()
    assert [(g.basename, g.error) for g in got] == [("r36", None), ("r50", None)]
    for g, bam in zip(got, pair):
        assert g.result.read_len == 50
        want, cache = _single(tmp_path, g.basename, bam, 50, stats=True)
        assert _bytes(g.written) == want
        assert sorted(want) == sorted(g.basename + s for s in ("_cc.tab", "_mscc.tab", "_nreads.tab", "_stats.tab"))
        assert (tmp_path / "m_mappability.json").read_text() == cache


def test_given_read_len_is_used_for_every_file(tmp_path, pair):
    got = _many(tmp_path, list(pair), read_len=36)
    for g, bam in zip(got, pair):
        assert g.result.read_len == 36
        assert _bytes(g.written) == _single(tmp_path, g.basename, bam, 36)[0]


def test_one_file_equals_run(tmp_path, pair):
    got, = _many(tmp_path, [pair[1]], stats=True)
    assert got.result.read_len == 50 and got.path == pair[1]
    assert _bytes(got.written) == _single(tmp_path, "single", pair[1], None, stats=True)[0]


def test_names(tmp_path, pair):
    got = _many(tmp_path, list(pair), read_len=36, names=["A"])
    assert [g.basename for g in got] == ["A", "r50"]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(b + s for b in ("A", "r50")
                                                          for s in ("_cc.tab", "_mscc.tab", "_nreads.tab"))
    got = _many(tmp_path, list(pair), read_len=36, names=[None, "rep1.filtered"], stats=True)
    assert [os.path.basename(p) for p in got[1].written] == ["rep1.filtered" + s for s in
                                                             ("_cc.tab", "_mscc.tab", "_nreads.tab", "_stats.tab")]
    from pymasc_amd import stats as S
    assert S.load_stats(got[1].written[3])["Name"] == "rep1.filtered"
    # the tables of a named file are those of the same file without a name
    assert [open(p, "rb").read() for p in got[1].written[:3]] == \
        [open(tmp_path / "out" / ("r50" + s), "rb").read() for s in ("_cc.tab", "_mscc.tab", "_nreads.tab")]


def test_existing_outputs_are_warned_about(tmp_path, pair, caplog):
    _many(tmp_path, list(pair), read_len=36)
    caplog.set_level(logging.WARNING)
    _many(tmp_path, list(pair), read_len=36)
    msgs = [r.getMessage() for r in caplog.records if "will be overwritten" in r.getMessage()]
    assert "Existing file '{}' will be overwritten.".format(tmp_path / "out" / "r36_cc.tab") in msgs
    assert len([m for m in msgs if "_mappability.json" not in m]) == 6


def test_all_five_side_counts_in_one_run(tmp_path, caplog):
    """Every side count on in one run writes, file by file, the bytes a run with that count alone writes -- through run and through
    run_files with two names -- in the order of the table of side counts; a second call warns about exactly these outputs."""
    fasta = tmp_path / "genome.fa"
    fasta.write_bytes(GC.fasta_text())
    bam = SW.write_twins(tmp_path, "gc", GC.REFS, GC.alignment_records(GC.synthetic()))[1]
    sides = (("_complexity.tab", dict(complexity=True)), ("_fingerprint.tab", dict(fingerprint=True)),
             ("_peaks.tab", dict(peaks={"g0": [(100, 30_000)], "g2": [(5, 900)]})),
             ("_coverage.bedGraph", dict(coverage=True, coverage_extend=150)), ("_gcbias.tab", dict(gc_bias=str(fasta))))
    everything = {k: v for _suffix, options in sides for k, v in options.items()}
    kw = dict(read_len=36, mapq_criteria=GC.MAPQ, device_ingest=False, exclude_regions=GC.MASK)
    bases = ("gc", "B")

    def files(out, paths=(bam, bam), **options):
        got = pipeline.run_files(list(paths), tmp_path / out, SHIFT, names=[None, "B"][:len(paths)], context=FakeContext(),
                                 **kw, **options)
        assert [g.error for g in got] == [None] * len(paths)
        return [g.written for g in got]

    def overwritten():
        return [r.getMessage() for r in caplog.records if "will be overwritten" in r.getMessage()]
    alone = {}                      # output name -> the bytes of a call with that count alone
    for suffix, options in sides:
        for base, written in zip(bases, files("only" + suffix, **options)):
            assert written[-1].name == base + suffix and not any(p.name.endswith(x) for p in written[:-1] for x, _o in sides)
            alone[base + suffix] = written[-1].read_bytes()
    _r, written = pipeline.run(bam, tmp_path / "all", SHIFT, context=FakeContext(), **kw, **everything)
    plain = [p.name for p in written[:-5]]
    assert plain and [p.name for p in written[-5:]] == ["gc" + suffix for suffix, _o in sides]
    assert all(p.read_bytes() == alone[p.name] for p in written[-5:])
    caplog.set_level(logging.WARNING)
    again, = files("all", paths=(bam,), **everything)       # the same call once more, by the entry point that warns (run does not)
    assert again == written and all(p.read_bytes() == alone[p.name] for p in again[-5:])
    assert sorted(overwritten()) == sorted("Existing file '{}' will be overwritten.".format(p) for p in written)
    caplog.clear()
    many = files("many", **everything)
    assert not overwritten()
    for base, written in zip(bases, many):
        assert [p.name for p in written] == [base + n[2:] for n in plain] + [base + suffix for suffix, _o in sides]
        assert all(p.read_bytes() == alone[p.name] for p in written[-5:])
    assert files("many", **everything) == many
    assert sorted(overwritten()) == sorted("Existing file '{}' will be overwritten.".format(p) for w in many for p in w)


@pytest.mark.parametrize("kw", [dict(names=["a", "b", "c"]), dict(names=["a", "a"]), dict(names=["x/y"]), dict(names=[""]),
                                dict(library_length=0), dict(smooth_window=0), dict(readlen_estimator="AVERAGE"),
                                dict(references=["c1"], chromfilter=[(True, ["c1"])]), dict(same_stem=True)])
def test_bad_arguments_fail_before_any_work(tmp_path, pair, monkeypatch, kw):
    from pymasc_amd import bam, inputs, sam

    def opened(*a, **k):
        raise AssertionError("a file or a context was opened")
    for mod, name in ((bam, "BamReader"), (sam, "SamReader"), (bigwig, "BigWigReader"), (ffi, "Context"),
                      (inputs, "open_alignments"), (pipeline, "open_alignments"), (pipeline, "open_track")):
        monkeypatch.setattr(mod, name, opened)
    paths = list(pair)
    if kw.pop("same_stem", False):
        os.makedirs(tmp_path / "other")
        paths[1] = str(tmp_path / "other" / "r36.bam")
        shutil.copy(pair[0], paths[1])
    with pytest.raises(ValueError):
        pipeline.run_files(paths, tmp_path / "out", SHIFT, mappability_path=str(tmp_path / "m.bw"), **kw)
    assert not (tmp_path / "out").exists()


def _three(tmp_path, middle, **kw):
    d = tmp_path / "in"
    d.mkdir(exist_ok=True)
    paths = [_bam(d / "a.bam", 36, 3), middle, _bam(d / "c.bam", 36, 4)]
    got = _many(tmp_path, paths, **kw)
    assert [g.basename for g in got] == ["a", os.path.basename(middle).split(".")[0], "c"]
    for g in (got[0], got[2]):
        assert g.error is None and len(g.written) == 3 and all(os.path.exists(p) for p in g.written)
    bad = got[1]
    assert bad.result is None and bad.written == [] and bad.error is not None
    assert not [n for n in os.listdir(tmp_path / "out") if n.startswith(got[1].basename + "_")]
    return got


def test_a_missing_file_is_skipped(tmp_path):
    got = _three(tmp_path, str(tmp_path / "missing.bam"))
    assert isinstance(got[1].error, OSError)


def test_a_file_without_a_text_header_is_skipped(tmp_path):
    p = tmp_path / "junk.bam"
    p.write_bytes(b"not an alignment file\n" * 10)
    got = _three(tmp_path, str(p))
    assert isinstance(got[1].error, (OSError, ValueError))


def test_a_file_the_chromosome_filter_empties_is_skipped(tmp_path, caplog):
    caplog.set_level(logging.ERROR)
    other = _bam(tmp_path / "chrx.bam", 36, 5, refs=[("chrX", 30000)])
    got = _three(tmp_path, other, chromfilter=[(True, ["c*"]), (False, ["chr*"])])
    assert isinstance(got[1].error, NoTargetChromosomesError)
    assert any("Check your -i/--include-chrom" in r.getMessage() for r in caplog.records)


def test_an_unsorted_file_is_skipped(tmp_path):
    got = _three(tmp_path, _bam(tmp_path / "unsorted.bam", 36, 6, unsorted=True))
    assert isinstance(got[1].error, ReadUnsortedError)


@pytest.mark.parametrize("check", ["control", "genome"])
def test_a_file_that_fails_a_check_after_an_unsorted_file_is_skipped_too(tmp_path, check):
    """An unsorted file, then a file whose references are not the fingerprint control's / the genome's, then a good one: the first
    two are skipped with their errors and the third is run and written."""
    other = [REFS[0], ("c2", REFS[1][1] - 1000)]
    paths = [_bam(tmp_path / "unsorted.bam", 36, 6, unsorted=True), _bam(tmp_path / "other.bam", 36, 7, refs=other),
             _bam(tmp_path / "good.bam", 36, 8)]
    if check == "control":
        kw, table, said = dict(fingerprint_control=_bam(tmp_path / "control.bam", 36, 9)), "good_fingerprint.tab", "differ from those of"
    else:
        rng = np.random.default_rng(10)
        fasta = tmp_path / "genome.fa"
        fasta.write_text("".join(">{}\n{}\n".format(n, "".join(rng.choice(list("ACGT"), size=l))) for n, l in REFS))
        kw, table, said = dict(gc_bias=str(fasta)), "good_gcbias.tab", "reference 'c2' is 19000 long in the alignment header"
    got = _many(tmp_path, paths, read_len=36, **kw)
    assert isinstance(got[0].error, ReadUnsortedError) and isinstance(got[1].error, ValueError) and said in str(got[1].error)
    assert all(g.result is None and g.written == [] for g in got[:2])
    assert got[2].error is None and [p.name for p in got[2].written] == ["good_cc.tab", "good_mscc.tab", "good_nreads.tab", table]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(p.name for p in got[2].written)


def test_a_file_whose_estimate_exceeds_max_shift_is_skipped(tmp_path, caplog):
    caplog.set_level(logging.INFO)
    got = _three(tmp_path, _bam(tmp_path / "long.bam", SHIFT + 30, 7))
    assert isinstance(got[1].error, ValueError) and "longer than shift size" in str(got[1].error)
    assert got[0].result.read_len == got[2].result.read_len == 36
    assert not [r for r in caplog.records if "multiple read length candidates" in r.getMessage()]


def test_every_file_bad_is_a_value_error(tmp_path):
    long = _bam(tmp_path / "long.bam", SHIFT + 30, 7)
    with pytest.raises(ValueError):
        _many(tmp_path, [str(tmp_path / "missing.bam"), long])
    with pytest.raises(ValueError):
        _many(tmp_path, [str(tmp_path / "missing.bam")], read_len=36)


def test_shared_work_is_done_once(tmp_path, monkeypatch):
    d = tmp_path / "in"
    d.mkdir()
    paths = [_bam(d / "a.bam", 36, 3), _bam(d / "b.bam", 50, 4), _bam(d / "c.bam", 36, 5)]
    calls = {"calc_mappability": 0, "track": 0, "context": 0, "closed": 0}
    live, after = [0], []
    made = []

    real_calc = MappabilityStats.calc_mappability

    def calc_mappability(self, *a, **k):
        calls["calc_mappability"] += 1
        return real_calc(self, *a, **k)

    class Track(bigwig.BigWigReader):
        def __init__(self, *a, **k):
            calls["track"] += 1
            super().__init__(*a, **k)

    def context(device=0):
        calls["context"] += 1
        ctx = FakeContext()
        alloc, free, close = ctx.bits_alloc, ctx.bits_free, ctx.close

        def bits_alloc(nbits):
            live[0] += 1
            return alloc(nbits)

        def bits_free(p):
            live[0] -= 1
            return free(p)

        def closed():
            calls["closed"] += 1
            close()
        ctx.bits_alloc, ctx.bits_free, ctx.close = bits_alloc, bits_free, closed
        made.append(ctx)
        return ctx

    real_run = pipeline.run_sharded

    def run_sharded(*a, **k):
        assert k["context"] is made[0]
        out = real_run(*a, **k)
        after.append(live[0])
        return out

    # without the garbage collector's help: run_sharded must close each calculator itself
    monkeypatch.setattr(CCHipCalculator, "__del__", lambda self: None)
    monkeypatch.setattr(MappabilityStats, "calc_mappability", calc_mappability)
    monkeypatch.setattr(bigwig, "BigWigReader", Track)
    monkeypatch.setattr(ffi, "Context", context)
    monkeypatch.setattr(pipeline, "run_sharded", run_sharded)
    got = _many(tmp_path, paths, context=None)
    assert [g.error for g in got] == [None] * 3
    assert calls == {"calc_mappability": 1, "track": 1, "context": 1, "closed": 1}
    assert len(after) == 3 and after[0] == after[1] == after[2] == 0


def test_without_saving_the_cache_equals_run(tmp_path, pair):
    """save_mappability_stats=False and no cache: run_files computes the lag tables once without writing them, run leaves them
    to each calculator's fused pass; the tables are the same and neither writes the cache."""
    got = _many(tmp_path, list(pair), read_len=50, save_mappability_stats=False)
    assert not (tmp_path / "m_mappability.json").exists()
    for g, bam in zip(got, pair):
        d = tmp_path / ("single_" + g.basename)
        d.mkdir()
        bw = _track(d / "m.bw")
        _r, written = pipeline.run(bam, d / "out", SHIFT, read_len=50, mapq_criteria=MAPQ, mappability_path=bw,
                                   device_ingest=False, context=FakeContext(), save_mappability_stats=False)
        assert _bytes(g.written) == _bytes(written)
        assert not (d / "m_mappability.json").exists()


def test_a_sam_file_is_probed_by_its_header(tmp_path, pair, monkeypatch):
    """Step 1 reads a SAM file's header only (pmx_sam_open_header); the whole text is read by the run alone."""
    from tests import sam_writers as SW
    refs = list(REFS)
    recs = SW.synth_records(np.random.default_rng(8), refs, 400)
    sam_path, bam_path, gz = SW.write_twins(tmp_path, "twin", refs, recs, bgzf_block=3000)
    opened = []

    class Counting(sam.SamReader):
        def __init__(self, *a, **k):
            opened.append(bool(k.get("header_only")))
            super().__init__(*a, **k)

    monkeypatch.setattr(sam, "SamReader", Counting)
    got = _many(tmp_path, [pair[0], gz], read_len=36, names=[None, "gz"])
    assert [g.error for g in got] == [None, None]
    assert opened == [True, False]                  # the header of step 1, then the run's reader
    want, _cache = _single(tmp_path, "bam_twin", bam_path, 36)
    assert [v for _k, v in sorted(_bytes(got[1].written).items())] == [v for _k, v in sorted(want.items())]


# What each entry point opens on the host readers, one rank, a BigWig track and no cache: the calls of the openers as pipeline
# sees them ("p.") and as run_sharded looks them up in inputs ("i."), and for every run_sharded call whether ``bam=`` and
# ``track=`` were handed on.  An extra open is an extra read of a file, so these counts are this layer's cost.
_OPENS = {
    ("run", 1, 36): {"p.open_alignments": 0, "p.open_track": 1, "p.open_header": 0, "i.open_alignments": 1, "i.open_track": 1,
                     "run_sharded": [(False, False)]},
    ("run", 1, None): {"p.open_alignments": 1, "p.open_track": 1, "p.open_header": 0, "i.open_alignments": 1,
                       "i.open_track": 1, "run_sharded": [(False, False)]},
    ("run_files", 1, 36): {"p.open_alignments": 0, "p.open_track": 1, "p.open_header": 1, "i.open_alignments": 1,
                           "i.open_track": 0, "run_sharded": [(False, True)]},
    ("run_files", 1, None): {"p.open_alignments": 1, "p.open_track": 1, "p.open_header": 1, "i.open_alignments": 1,
                             "i.open_track": 0, "run_sharded": [(False, True)]},
    ("run_files", 2, 36): {"p.open_alignments": 0, "p.open_track": 1, "p.open_header": 2, "i.open_alignments": 2,
                           "i.open_track": 0, "run_sharded": [(False, True)] * 2},
    ("run_files", 2, None): {"p.open_alignments": 2, "p.open_track": 1, "p.open_header": 2, "i.open_alignments": 2,
                             "i.open_track": 0, "run_sharded": [(False, True)] * 2},
}


@pytest.mark.parametrize("entry,nfiles,read_len", sorted(_OPENS, key=str))
def test_opens_per_call(tmp_path, pair, monkeypatch, entry, nfiles, read_len):
    from pymasc_amd import inputs
    seen = {k: 0 for k in _OPENS[entry, nfiles, read_len] if k != "run_sharded"}
    seen["run_sharded"] = []

    def counting(key, fn):
        def call(*a, **k):
            seen[key] += 1
            return fn(*a, **k)
        return call

    for mod, tag in ((pipeline, "p."), (inputs, "i.")):
        for name in ("open_alignments", "open_track", "open_header"):
            if tag + name in seen:
                monkeypatch.setattr(mod, name, counting(tag + name, getattr(mod, name)))
    real_run = pipeline.run_sharded

    def run_sharded(*a, **k):
        seen["run_sharded"].append((k.get("bam") is not None, k.get("track") is not None))
        return real_run(*a, **k)
    monkeypatch.setattr(pipeline, "run_sharded", run_sharded)
    bw = _track(tmp_path / "m.bw")
    kw = dict(read_len=read_len, mapq_criteria=MAPQ, mappability_path=bw, device_ingest=False, context=FakeContext())
    if entry == "run":
        pipeline.run(pair[1], tmp_path / "out", SHIFT, **kw)
    else:
        got = pipeline.run_files(list(pair[:nfiles]), tmp_path / "out", SHIFT, **kw)
        assert [g.error for g in got] == [None] * nfiles
    assert seen == _OPENS[entry, nfiles, read_len]


# ---- two gloo ranks -------------------------------------------------------------------------------------------------------
def _rank_worker(rank, world, port, q, batches, tmp):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        out = []
        for tag, paths in batches:
            got = pipeline.run_files(paths, os.path.join(tmp, "%s_%d" % (tag, rank)), SHIFT, mapq_criteria=MAPQ,
                                     mappability_path=os.path.join(tmp, "m.bw"), context=FakeContext())
            out.append([(g.basename, None if g.error is None else type(g.error).__name__,
                         None if g.result is None else g.result.read_len, _bytes(g.written)) for g in got])
        q.put((rank, out, None))
    except Exception as e:          # reported, not hung on
        q.put((rank, None, repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(900)
def test_two_ranks(tmp_path):
    import torch.multiprocessing as mp
    from tests.test_gpu_ingest_indexed import _free_port
    tmp = str(tmp_path)
    d = tmp_path / "in"
    d.mkdir()
    a, c = _bam(d / "a.bam", 36, 3), _bam(d / "c.bam", 50, 4)
    batches = [("missing", [a, str(d / "b.bam"), c]), ("unsorted", [a, _bam(d / "u.bam", 36, 6, unsorted=True), c])]
    _track(tmp_path / "m.bw")
    single = [_many(tmp_path, paths) for _tag, paths in batches]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, 2, port, q, batches, tmp)) for r in range(2)]
    for p in procs:
        p.start()
    try:
        got = sorted(q.get(timeout=600) for _ in range(2))
    finally:
        for p in procs:
            p.join(120)
            if p.is_alive():
                p.kill()
                p.join(10)
    assert all(p.exitcode == 0 for p in procs)
    (_r0, out0, e0), (_r1, out1, e1) = got
    assert e0 is None and e1 is None, (e0, e1)
    for b, one, r0, r1 in zip(batches, single, out0, out1):
        assert [x[:3] for x in r0] == [x[:3] for x in r1]                   # the same outcome on both ranks
        assert [x[1] for x in r0] == [None, "PmxIOError" if b[0] == "missing" else "ReadUnsortedError", None]
        assert [x[2] for x in r0] == [50, None, 50]
        assert [x[3] for x in r0] == [_bytes(g.written) for g in one]      # rank 0 writes what one rank writes
        assert all(x[3] == {} for x in r1)
        assert not os.path.exists(os.path.join(tmp, "%s_1" % b[0]))
