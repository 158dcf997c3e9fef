"""The ``pymasc`` and ``pymasc-precalc`` commands (pymasc_amd.cli, pymasc_amd.precalc) on the host readers and the test context:
PyMaSC's options, defaults and argument errors, the option -> keyword mapping into pipeline.run_files, outputs byte-identical
to a direct run_files call, the exit statuses, what the parser and the ``-p N`` parent leave unimported, two gloo ranks, and the
precalc cache against the golden JSON."""
import json
import logging
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from pymasc_amd import cli, ffi, inputs, launch, pipeline, precalc
from pymasc_amd import stats as S
from tests import fixtures as fx
from tests import io_writers as W
from tests.fake_context import FakeContext
from tests.test_run_files import MAPQ, REFS, SHIFT, _bam, _track

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "cli_rank_child.py")
GOLDEN_JSON = os.path.join(fx.GOLDEN, "hg19_36mer-test_mappability.json")
NATURAL = ["-d", "-p", "-r", "-l", "-w", "--bg-avr-width"]


@pytest.fixture(autouse=True)
def _root_logger():
    """cli.main sets up the root logger as a command does: put it back for the tests that follow."""
    root = logging.getLogger()
    level, handlers = root.level, list(root.handlers)
    yield
    for h in list(root.handlers):
        if h not in handlers:
            root.removeHandler(h)
    root.setLevel(level)
    cli._log_handler = None


@pytest.fixture
def host(monkeypatch):
    """The host readers and the test context, whatever the machine has."""
    monkeypatch.setattr(ffi, "Context", lambda device=0: FakeContext())
    monkeypatch.setattr(pipeline, "default_device_ingest", lambda *a, **k: False)
    monkeypatch.setattr(inputs, "default_device_ingest", lambda *a, **k: False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)


@pytest.fixture
def no_run(monkeypatch):
    def refused(*a, **k):
        raise AssertionError("run_files was called")
    monkeypatch.setattr(pipeline, "run_files", refused)


@pytest.fixture
def pair(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    return _bam(d / "r36.bam", 36, 1), _bam(d / "r50.bam", 50, 2)


def _fragments(path, read_len, seed, frag=90, n=600):
    """A BAM file of fragments ~``frag`` long, both ends read: a cross-correlation peak that an expected library length
    can be measured against (the uniform reads of ``_bam`` have none)."""
    rng = np.random.default_rng(seed)
    recs = []
    for rid, (_c, ln) in enumerate(REFS):
        starts = rng.integers(0, ln - frag - 200, size=n)
        sizes = frag + rng.integers(-8, 9, size=n)
        reads = sorted([(int(s), 0) for s in starts] + [(int(s + z - read_len), 16) for s, z in zip(starts, sizes)])
        recs += [W.bam_record(rid, p, 30, f, [("M", read_len)], b"f%d" % len(recs)) for p, f in reads]
    W.write_bam(str(path), REFS, recs, block=3000)
    return str(path)


def _tree(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _env():
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        env.pop(k, None)
    return env


# ---- parser -------------------------------------------------------------------------------------------------------------
def test_defaults():
    a = cli.parse_args(["a.bam"])
    assert [str(p) for p in a.reads] == ["a.bam"]
    assert (a.read_length, a.readlen_estimator, a.mappability, a.mappability_stats, a.mapq) == (None, "MEDIAN", None, None, 1)
    assert (a.chromfilter, a.max_shift, a.library_length, a.chi2_pval, a.smooth_window, a.mask_size, a.bg_avr_width) == \
        (None, 1000, None, 0.05, 15, 5, 50)
    assert (a.name, str(a.outdir), a.process, a.successive, a.skip_ncc, a.skip_plots) == ([], ".", 1, False, False, False)
    assert (a.log_level, a.disable_progress, a.color) == (logging.INFO, False, True)
    a = cli.parse_args(["a.bam", "b.bam", "-n", "A", "-v", "debug", "--color", "false", "--readlen-estimator", "mean"])
    assert (a.name, a.log_level, a.color, a.readlen_estimator) == (["A"], logging.DEBUG, False, "MEAN")
    from pymasc_amd import readlen
    assert cli.READLEN_ESTIMATORS == readlen.ESTIMATORS
    p = precalc.get_parser().parse_args(["-m", "t.bw"])
    assert (str(p.mappability), p.mappability_stats, p.max_shift, p.max_readlen, p.process) == ("t.bw", None, 1000, 1000, 1)


@pytest.mark.parametrize("argv", [[o, "0"] for o in NATURAL] +
                         [["--readlen-estimator", "foo"], ["--skip-ncc"], ["--color", "maybe"], ["-n", "A", "B"],
                          ["-n", "x/y"], ["-n", ""], []])
def test_argument_errors_exit_2(argv, no_run, capsys):
    reads = [] if argv == [] else ["a.bam"]
    assert cli.main(reads + argv) == 2
    assert "error:" in capsys.readouterr().err


def test_same_base_name_exits_2(no_run):
    assert cli.main(["a/r.bam", "b/r.bam"]) == 2
    assert cli.main(["a/r.bam", "b/r.bam", "-n", "r"]) == 2


def test_check_names_follows_pipeline():
    cases = [(["a.bam"], []), (["a.bam", "b.bam"], ["A"]), (["a.bam"], ["A", "B"]), (["a.bam"], ["x/y"]), (["a.bam"], [""]),
             (["a.bam"], [".."]), (["x/r.bam", "y/r.bam"], []), (["x/r.bam", "y/r.bam"], ["r"]), (["a.bam", "b.bam"], ["b"]),
             (["a.bam", "b.sam.gz"], ["A", "B"]), (["a.bam"], ["rep1.filtered"])]
    for paths, names in cases:
        try:
            pipeline._basenames(paths, names)
            want = None
        except ValueError:
            want = ValueError
        try:
            cli.check_names(paths, names)
            got = None
        except ValueError:
            got = ValueError
        assert got is want, (paths, names)


def test_help_and_version(capsys):
    assert cli.main(["--help"]) == 0
    out = capsys.readouterr().out
    for opt in ("--read-length", "--readlen-estimator", "--mappability", "--mappability-stats", "--mapq", "--include-chrom",
                "--exclude-chrom", "--max-shift", "--library-length", "--chi2-pval", "--smooth-window", "--mask-size",
                "--bg-avr-width", "--name", "--outdir", "--process", "--successive", "--skip-ncc", "--skip-plots",
                "--log-level", "--disable-progress", "--color", "--version"):
        assert opt in out
    assert cli.main(["--version"]) == 0
    assert capsys.readouterr().out.startswith("pymasc_amd ")
    assert precalc.main(["--help"]) == 0


def test_options_reach_run_files(tmp_path, monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw, paths=paths, outdir=outdir, max_shift=max_shift)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bw = _track(tmp_path / "m.bw")
    assert cli.main(["a.bam", "b.bam", "-i", "chr1", "chr2", "-e", "chr2", "-i", "chr*", "-m", bw, "--mappability-stats",
                     str(tmp_path / "s.json"), "-d", "300", "-r", "36", "-q", "10", "-l", "200", "-w", "9", "--mask-size",
                     "0", "--bg-avr-width", "20", "--chi2-pval", "0.01", "-n", "A", "-o", str(tmp_path / "o"),
                     "--readlen-estimator", "max", "--skip-ncc", "--skip-plots"]) == 0
    assert seen["chromfilter"] == [(True, ["chr1", "chr2"]), (False, ["chr2"]), (True, ["chr*"])]
    assert seen == dict(paths=["a.bam", "b.bam"], outdir=str(tmp_path / "o"), max_shift=300, read_len=36, mapq_criteria=10,
                        mappability_path=bw, mappability_stats_path=str(tmp_path / "s.json"), skip_ncc=True, device=None,
                        readlen_estimator="MAX", chromfilter=seen["chromfilter"], stats=True, library_length=200,
                        smooth_window=9, mask_size=0, bg_avr_width=20, chi2_pval=0.01, names=["A"])
    seen.clear()
    assert cli.main(["a.bam"]) == 0
    assert (seen["names"], seen["chromfilter"], seen["mappability_path"], seen["read_len"], seen["stats"]) == \
        (None, None, None, None, True)


# ---- end to end on the test context -------------------------------------------------------------------------------------
def _direct(tmp_path, paths, **kw):
    d = tmp_path / "direct"
    d.mkdir()
    bw = _track(d / "m.bw")
    pipeline.run_files(paths, str(d / "out"), SHIFT, mapq_criteria=MAPQ, mappability_path=bw, device_ingest=False,
                       context=FakeContext(), stats=True, **kw)
    return d


def test_two_files_equal_run_files(tmp_path, host, caplog):
    caplog.set_level(logging.INFO)
    (tmp_path / "in").mkdir()
    pair = [_fragments(tmp_path / "in" / "f36.bam", 36, 1), _fragments(tmp_path / "in" / "f40.bam", 40, 2)]
    d = tmp_path / "cli"
    d.mkdir()
    bw = _track(d / "m.bw")
    rc = cli.main(list(pair) + ["-m", bw, "-n", "A", "-l", "100", "-w", "9", "--mask-size", "3", "-q", str(MAPQ),
                                "-d", str(SHIFT), "-o", str(d / "out"), "--skip-plots"])
    assert rc == 0
    want = _direct(tmp_path, list(pair), names=["A"], library_length=100, smooth_window=9, mask_size=3)
    got = _tree(d / "out")
    assert sorted(got) == sorted(b + s for b in ("A", "f40") for s in ("_cc.tab", "_mscc.tab", "_nreads.tab", "_stats.tab"))
    assert got == _tree(want / "out")
    assert (d / "m_mappability.json").read_bytes() == (want / "m_mappability.json").read_bytes()
    assert S.load_stats(d / "out" / "A_stats.tab")["Expected library length"] == "100"
    assert not [r for r in caplog.records if "Skip output plots" in r.getMessage()]


def test_library_length_longer_than_max_shift_is_dropped(tmp_path, pair, host, caplog):
    caplog.set_level(logging.INFO)
    bw = _track(tmp_path / "m.bw")
    assert cli.main([pair[0], "-m", bw, "-r", "36", "-q", str(MAPQ), "-d", str(SHIFT), "-l", str(SHIFT + 1),
                     "-o", str(tmp_path / "out"), "--skip-plots"]) == 0
    assert any(r.levelno == logging.ERROR and r.getMessage() == "Specified expected library length > max shift. Ignore "
               "expected length setting." for r in caplog.records)
    assert S.load_stats(tmp_path / "out" / "r36_stats.tab")["Expected library length"] == "nan"


def test_mappability_stats_equal_to_the_track_is_dropped(tmp_path, pair, host):
    bw = _track(tmp_path / "m.bw")
    before = open(bw, "rb").read()
    assert cli.main([pair[0], "-m", bw, "--mappability-stats", bw, "-r", "36", "-d", str(SHIFT), "-o",
                     str(tmp_path / "out"), "--skip-plots"]) == 0
    assert open(bw, "rb").read() == before
    assert json.load(open(tmp_path / "m_mappability.json"))["max_shift"] > 0


def test_without_skip_plots_every_file_logs_and_no_pdf(tmp_path, pair, host, caplog):
    caplog.set_level(logging.INFO)
    out = tmp_path / "out"
    assert cli.main(list(pair) + [str(tmp_path / "missing.bam"), "-r", "50", "-d", str(SHIFT), "-o", str(out)]) == 0
    msgs = [r.getMessage() for r in caplog.records if "Skip output plots" in r.getMessage()]
    assert msgs == ["Skip output plots '{}'".format(out / (b + ".pdf")) for b in ("r36", "r50")]
    assert not [n for n in os.listdir(out) if n.endswith(".pdf")]
    assert sorted(os.listdir(out)) == sorted(b + s for b in ("r36", "r50") for s in ("_cc.tab", "_nreads.tab", "_stats.tab"))


def test_every_input_skipped_exits_1(tmp_path, host):
    unsorted = _bam(tmp_path / "u.bam", 36, 6, unsorted=True)
    assert cli.main([str(tmp_path / "missing.bam"), "-d", str(SHIFT), "-o", str(tmp_path / "o1")]) == 1
    assert cli.main([str(tmp_path / "missing.bam"), "-r", "36", "-d", str(SHIFT), "-o", str(tmp_path / "o2")]) == 1
    assert cli.main([unsorted, "-r", "36", "-d", str(SHIFT), "-o", str(tmp_path / "o3")]) == 1


def test_missing_track_exits_1_before_any_context(tmp_path, pair, monkeypatch, caplog):
    def refused(*a, **k):
        raise AssertionError("a context was built")
    monkeypatch.setattr(ffi, "Context", refused)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    caplog.set_level(logging.INFO)
    assert cli.main([pair[0], "-m", str(tmp_path / "none.bw"), "-r", "36", "-o", str(tmp_path / "out")]) == 1
    assert any("none.bw" in r.getMessage() and r.levelno == logging.CRITICAL for r in caplog.records)
    assert not (tmp_path / "out").exists()
    assert precalc.main(["-m", str(tmp_path / "none.bw")]) == 1
    assert precalc.main(["-m", str(tmp_path)]) == 1


# ---- what the parser and the -p N parent import ---------------------------------------------------------------------------
_PROBE = """
import sys
from pymasc_amd import cli
rc = cli.main(sys.argv[1:])
print("RC", rc, "torch" in sys.modules, "pymasc_amd.ffi" in sys.modules, "pymasc_amd.pipeline" in sys.modules)
"""


@pytest.mark.parametrize("argv,rc", [(["--help"], 0), (["--version"], 0), (["a.bam", "-d", "0"], 2),
                                     (["a.bam", "--skip-ncc"], 2), (["a.bam", "a.sam"], 2)])
def test_parsing_imports_no_torch(argv, rc, tmp_path):
    p = subprocess.run([sys.executable, "-c", _PROBE] + argv, capture_output=True, text=True, timeout=120, env=_env(),
                       cwd=str(tmp_path))
    assert p.stdout.strip().splitlines()[-1] == "RC {} False False False".format(rc), p.stderr


_RECORDER = """
import sys
from pymasc_amd import cli, launch
calls = []
def spawn_ranks(argv, nranks, *a, **k):
    calls.append((list(argv), nranks))
    return 7
launch.spawn_ranks = spawn_ranks
rc = cli.main(sys.argv[1:])
print(repr((rc, calls, "torch" in sys.modules, "pymasc_amd.ffi" in sys.modules)))
"""


def test_p2_parent_spawns_ranks_without_torch(tmp_path):
    argv = ["a.bam", "-p", "2", "-d", "300", "-o", "out"]
    p = subprocess.run([sys.executable, "-c", _RECORDER] + argv, capture_output=True, text=True, timeout=120, env=_env(),
                       cwd=str(tmp_path))
    rc, calls, torch_in, ffi_in = eval(p.stdout.strip().splitlines()[-1])
    assert (rc, calls, torch_in, ffi_in) == (7, [([sys.executable, "-m", "pymasc_amd"] + argv, 2)], False, False), p.stderr


@pytest.mark.timeout(600)
def test_two_gloo_ranks_equal_one_process(tmp_path, pair, host, monkeypatch):
    bw = _track(tmp_path / "m.bw")
    common = ["-m", bw, "-q", str(MAPQ), "-d", str(SHIFT), "-n", "A", "--skip-plots"]
    assert cli.main(list(pair) + common + ["-o", str(tmp_path / "one")]) == 0
    os.unlink(tmp_path / "m_mappability.json")
    monkeypatch.setenv("PYTHONPATH", _env()["PYTHONPATH"])
    rc = launch.spawn_ranks([sys.executable, CHILD] + list(pair) + common + ["-o", str(tmp_path / "two"), "-p", "2"], 2,
                            timeout=480)
    assert rc == 0
    assert _tree(tmp_path / "two") == _tree(tmp_path / "one")
    assert os.path.exists(tmp_path / "m_mappability.json")


@pytest.mark.timeout(600)
def test_a_cache_error_on_two_ranks_prints_one_message(tmp_path, pair):
    """Rank 0's cache fails (its directory does not exist): both ranks exit 1, rank 0 logs why, rank 1 logs nothing of it."""
    from tests.test_gpu_ingest_indexed import _free_port
    bw = _track(tmp_path / "m.bw")
    argv = [sys.executable, CHILD, pair[0], "-m", bw, "--mappability-stats", str(tmp_path / "none" / "c.json"), "-r", "36",
            "-d", str(SHIFT), "-o", str(tmp_path / "out"), "-p", "2"]
    port = str(_free_port())
    procs = []
    for r in range(2):
        env = _env()
        env.update(RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", LOCAL_WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port)
        procs.append(subprocess.Popen(argv, env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True))
    errs = []
    try:
        for p in procs:
            errs.append(p.communicate(timeout=300)[1])
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    assert [p.returncode for p in procs] == [1, 1], errs
    assert errs[0].count("Directory is not writable") == 1 and "Traceback" not in errs[0], errs[0]
    for text in ("Traceback", "failed on rank 0", "Directory is not writable", "No input file"):
        assert text not in errs[1], errs[1]
    assert not (tmp_path / "out").exists()


# ---- precalc ----------------------------------------------------------------------------------------------------------------
def test_precalc_writes_the_golden_cache(tmp_path, host, monkeypatch, caplog):
    bw = tmp_path / "hg19_36mer-test.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    out = tmp_path / "hg19_36mer-test_mappability.json"
    assert precalc.main(["-m", str(bw), "-d", "300", "-r", "36", "-p", "4"]) == 0
    assert out.read_bytes() == open(GOLDEN_JSON, "rb").read()
    assert json.load(open(out))["max_shift"] == 265
    st = os.stat(out)

    def refused(*a, **k):
        raise AssertionError("the GPU was asked for")
    from pymasc_amd import bigwig_device
    monkeypatch.setattr(ffi, "Context", refused)
    monkeypatch.setattr(ffi, "device_count", refused)
    monkeypatch.setattr(inputs, "default_device_ingest", refused)
    monkeypatch.setattr(bigwig_device, "DeviceBigWigReader", refused)
    caplog.set_level(logging.INFO)
    assert precalc.main(["-m", str(bw), "-d", "300", "-r", "36"]) == 0
    assert any(r.getMessage() == "Mappability stats updating is not required." for r in caplog.records)
    assert out.read_bytes() == open(GOLDEN_JSON, "rb").read() and os.stat(out).st_mtime_ns == st.st_mtime_ns


def test_precalc_to_a_given_path(tmp_path, host):
    bw = tmp_path / "t.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    assert precalc.main(["-m", str(bw), "--mappability-stats", str(tmp_path / "c.json"), "-d", "300", "-r", "36"]) == 0
    assert (tmp_path / "c.json").read_bytes() == open(GOLDEN_JSON, "rb").read()
    assert not (tmp_path / "t_mappability.json").exists()


def test_precalc_without_m_exits_2(capsys):
    assert precalc.main([]) == 2
    assert "argument -m/--mappable: expected 1 argument(s)" in capsys.readouterr().err
    assert precalc.main(["-m", "t.bw", "-r", "0"]) == 2
