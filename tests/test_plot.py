"""The ``pymasc-plot`` command (pymasc_amd.plot) and the figure writer (pymasc_amd.figures), on the host: no GPU is used.

The golden tables are the reference's own (tests/golden/ENCFF000RMB-test_{stats,cc,mscc,nreads}.tab).  Two data files come
unchanged from the reference's repository: ``tests/golden/hg19.chrom.sizes`` (its tests/data/hg19.chrom.sizes) and
``tests/golden/ENCFF000RMB-test.pdf`` (its tests/golden/ENCFF000RMB-test.pdf, 5 pages drawn by PyMaSC with matplotlib 3.7.5).
``_stats.tab`` rows are compared as tests/test_stats.py does: integers and strings exactly, floats to decimal=10.

``Genome length`` sums the chromosomes of ``-s``: with the golden BAM or SAM header it is the golden value; hg19.chrom.sizes
names other contigs than that header (3137161264 in all), so there the row is checked against the file's own sum."""
import logging
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from pymasc_amd import cli, figures, inputs, plot
from pymasc_amd import stats as S
from tests import fixtures as fx
from tests.test_stats import _assert_rows, _same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEM = "ENCFF000RMB-test"
GOLD = os.path.join(fx.GOLDEN, STEM)
SIZES = os.path.join(fx.GOLDEN, "hg19.chrom.sizes")
JSON = os.path.join(fx.GOLDEN, "hg19_36mer-test_mappability.json")
GOLDEN_PDF = GOLD + ".pdf"
SUFFIXES = ("_stats.tab", "_cc.tab", "_mscc.tab", "_nreads.tab")
TITLES = ["Cross-Correlation for " + STEM, "Cross-Correlation for " + STEM,
          "MSCC and Library Length Estimation for " + STEM, "Naive CC vs MSCC", "chr1 Cross-Correlation for " + STEM]


@pytest.fixture(autouse=True)
def _root_logger():
    """plot.main sets up the root logger as a command does: put it back for the tests that follow."""
    root = logging.getLogger()
    level, handlers = root.level, list(root.handlers)
    yield
    for h in list(root.handlers):
        if h not in handlers:
            root.removeHandler(h)
    root.setLevel(level)
    cli._log_handler = None


def _pages(path) -> int:
    return len(re.findall(rb"/Type\s*/Page(?![A-Za-z])", open(path, "rb").read()))


def _sizes_sum(path=SIZES) -> int:
    return sum(int(line.split("\t")[1]) for line in open(path) if line.strip())


def _header_sum(path) -> int:
    with inputs.open_header(path) as r:
        return sum(r.lengths)


def _check_stats(path, genome_length=None, name=STEM):
    got, want = S.load_stats(path), S.load_stats(GOLD + "_stats.tab")
    want["Name"] = name
    if genome_length is not None:
        assert got["Genome length"] == str(genome_length)
        want["Genome length"] = str(genome_length)
    _assert_rows(got, want)


def _copy_inputs(d, names=SUFFIXES):
    d.mkdir(parents=True, exist_ok=True)
    for s in names:
        shutil.copy(GOLD + s, d / (STEM + s))
    return d / STEM


def _cc_rows(path):
    with open(path) as fh:
        return [line.rstrip("\n").split("\t") for line in fh]


# ---- the golden replot ------------------------------------------------------------------------------------------------
def test_golden_replot_from_the_base_path(tmp_path):
    out = tmp_path / "out"
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(out)]) == 0
    assert sorted(os.listdir(out)) == sorted(STEM + s for s in (".pdf", "_stats.tab", "_cc.tab", "_mscc.tab"))
    assert _sizes_sum() == 3137161264
    _check_stats(out / (STEM + "_stats.tab"), _sizes_sum())


def test_golden_replot_from_separate_files(tmp_path):
    out = tmp_path / "out"
    argv = ["--stats", GOLD + "_stats.tab", "--cc", GOLD + "_cc.tab", "--masc", GOLD + "_mscc.tab",
            "--nreads", GOLD + "_nreads.tab", "-s", SIZES, "-m", JSON, "-o", str(out)]
    assert plot.main(argv) == 0
    _check_stats(out / (STEM + "_stats.tab"), _sizes_sum())


@pytest.mark.parametrize("header", [GOLD + ".bam", GOLD + ".sam.gz"])
def test_golden_replot_with_an_alignment_header(tmp_path, header):
    out = tmp_path / "out"
    assert plot.main([GOLD, "-s", header, "-m", JSON, "-o", str(out)]) == 0
    total = _header_sum(header)
    assert total == 3137454505
    _check_stats(out / (STEM + "_stats.tab"))                     # every row, Genome length included
    assert S.load_stats(out / (STEM + "_stats.tab"))["Genome length"] == str(total)


def test_mappability_stats_given_as_the_track(tmp_path):
    track = tmp_path / "hg19_36mer-test.bigwig"
    track.write_bytes(b"")                                         # only its name is used: the cache sits beside it
    shutil.copy(JSON, tmp_path / "hg19_36mer-test_mappability.json")
    assert plot.main([GOLD, "-s", SIZES, "-m", str(track), "-o", str(tmp_path / "out")]) == 0
    _check_stats(tmp_path / "out" / (STEM + "_stats.tab"), _sizes_sum())


def test_sizes_as_fai_columns(tmp_path):
    fai = tmp_path / "hg19.fa.fai"
    fai.write_text("".join("{}\t{}\t0\t60\t61\n".format(*line.split("\t")[:2]) for line in open(SIZES).read().splitlines()))
    assert plot.main([GOLD, "-s", str(fai), "-m", JSON, "-o", str(tmp_path / "out")]) == 0
    _check_stats(tmp_path / "out" / (STEM + "_stats.tab"), _sizes_sum())


def test_rewritten_tables_match_the_inputs(tmp_path):
    out = tmp_path / "out"
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(out)]) == 0
    for suffix in ("_cc.tab", "_mscc.tab"):
        got, want = _cc_rows(out / (STEM + suffix)), _cc_rows(GOLD + suffix)
        assert [r[0] for r in got] == [r[0] for r in want]
        assert got[0] == want[0] == ["shift", "whole", "chr1"]
        assert [r[2:] for r in got] == [r[2:] for r in want]       # the loaded columns, byte for byte
        np.testing.assert_almost_equal([float(r[1]) for r in got[1:]], [float(r[1]) for r in want[1:]], decimal=10)


def test_changed_parameters_equal_genome_wide_stats(tmp_path):
    out = tmp_path / "out"
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(out), "-w", "30", "-l", "150", "--mask-size", "0"]) == 0
    got = S.load_stats(out / (STEM + "_stats.tab"))
    assert got["Expected library length"] == "150"

    cc, masc = plot._load_cc(GOLD + "_cc.tab"), plot._load_cc(GOLD + "_mscc.tab")
    rebuilt = plot.rebuild_result(36, plot.load_chrom_sizes(SIZES), cc, masc, plot._load_nreads(GOLD + "_nreads.tab"),
                                  plot._load_lag_tables(JSON))
    assert rebuilt.used == ["chr1"] and rebuilt.mscc_reads is None
    st = S.genome_wide_stats(rebuilt.result, 36, library_length=150, smooth_window=30, mask_size=0)
    want = dict(S.stats_rows(STEM, st))
    assert got == want
    base = S.load_stats(GOLD + "_stats.tab")
    assert (got["Estimated library length"], got["Estimated FWHM"]) != \
        (base["Estimated library length"], base["Estimated FWHM"])


def test_library_length_from_the_stats_file_and_too_long(tmp_path, caplog):
    caplog.set_level(logging.INFO)
    d = _copy_inputs(tmp_path / "in")
    st = (tmp_path / "in" / (STEM + "_stats.tab"))
    st.write_text(st.read_text().replace("Expected library length\tnan", "Expected library length\t120"))
    assert plot.main([str(d), "-s", SIZES, "-m", JSON, "-o", str(tmp_path / "a")]) == 0
    assert S.load_stats(tmp_path / "a" / (STEM + "_stats.tab"))["Expected library length"] == "120"
    assert plot.main([str(d), "-s", SIZES, "-m", JSON, "-o", str(tmp_path / "b"), "-l", "400"]) == 0
    assert S.load_stats(tmp_path / "b" / (STEM + "_stats.tab"))["Expected library length"] == "nan"
    assert plot.LIBLEN_TOO_LONG in caplog.text


# ---- the PDF ------------------------------------------------------------------------------------------------------------
def _golden_stats():
    cc, masc = plot._load_cc(GOLD + "_cc.tab"), plot._load_cc(GOLD + "_mscc.tab")
    rebuilt = plot.rebuild_result(36, plot.load_chrom_sizes(SIZES), cc, masc, plot._load_nreads(GOLD + "_nreads.tab"),
                                  plot._load_lag_tables(JSON))
    return S.genome_wide_stats(rebuilt.result, 36)


def test_golden_pdf_has_five_pages(tmp_path):
    assert _pages(GOLDEN_PDF) == 5
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(tmp_path)]) == 0
    assert _pages(tmp_path / (STEM + ".pdf")) == 5


def test_pages_titles_lines_and_band():
    st = _golden_stats()
    pages = figures.figure_pages(st, STEM)
    assert [f.axes[0].get_title() for f in pages] == TITLES
    ax = pages[0].axes[0]
    np.testing.assert_array_equal(ax.lines[0].get_ydata(), st.whole_ncc.cc)
    band = ax.collections[0].get_paths()[0].vertices
    n = len(st.whole_ncc.cc)
    # fill_between's polygon: the lower edge left to right, then the upper edge right to left
    lower = band[1:n + 1, 1]
    upper = band[n + 2:2 * n + 2, 1][::-1]
    np.testing.assert_array_equal(lower, st.whole_ncc.cc_lower)
    np.testing.assert_array_equal(upper, st.whole_ncc.cc_upper)
    assert pages[1].axes[0].get_xlim() == (0, 2 * st.whole_mscc.est_lib_len)
    mscc_ax = pages[2].axes[0]
    np.testing.assert_array_equal(mscc_ax.lines[0].get_ydata(), st.whole_mscc.cc)
    np.testing.assert_array_equal(mscc_ax.lines[1].get_ydata(), st.whole_mscc.avr_cc)


def test_two_runs_give_the_same_bytes(tmp_path):
    for d in ("a", "b"):
        assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(tmp_path / d)]) == 0
    assert (tmp_path / "a" / (STEM + ".pdf")).read_bytes() == (tmp_path / "b" / (STEM + ".pdf")).read_bytes()


def test_ncc_only_replot(tmp_path):
    out = tmp_path / "out"
    argv = ["--stats", GOLD + "_stats.tab", "--cc", GOLD + "_cc.tab", "--nreads", GOLD + "_nreads.tab", "-s", SIZES,
            "-o", str(out)]
    assert plot.main(argv) == 0
    assert sorted(os.listdir(out)) == sorted(STEM + s for s in (".pdf", "_stats.tab", "_cc.tab"))
    assert _pages(out / (STEM + ".pdf")) == 2
    got = S.load_stats(out / (STEM + "_stats.tab"))
    want = S.load_stats(GOLD + "_stats.tab")
    assert all(got[k] == "nan" for k in S._MSCC_LABELS)
    for k in ("Forward reads", "Reverse reads", "Minimum NCC", "NCC at read length"):
        _same(got[k], want[k], k)
    # without MSCC, the estimated scores are taken at NCC's own estimate
    rebuilt = plot.rebuild_result(36, plot.load_chrom_sizes(SIZES), plot._load_cc(GOLD + "_cc.tab"), None,
                                  plot._load_nreads(GOLD + "_nreads.tab"))
    assert got == dict(S.stats_rows(STEM, S.genome_wide_stats(rebuilt.result, 36)))


def test_mscc_only_replot(tmp_path):
    out = tmp_path / "out"
    argv = ["--stats", GOLD + "_stats.tab", "--masc", GOLD + "_mscc.tab", "--nreads", GOLD + "_nreads.tab", "-s", SIZES,
            "-m", JSON, "-o", str(out)]
    assert plot.main(argv) == 0
    assert sorted(os.listdir(out)) == sorted(STEM + s for s in (".pdf", "_stats.tab", "_mscc.tab"))
    assert _pages(out / (STEM + ".pdf")) == 3
    got, want = S.load_stats(out / (STEM + "_stats.tab")), S.load_stats(GOLD + "_stats.tab")
    assert all(got[k] == "nan" for k in S._NCC_LABELS)
    for k in S._MSCC_LABELS + ("Estimated library length",):
        _same(got[k], want[k], k)


# ---- overwriting the inputs ---------------------------------------------------------------------------------------------
def _tree(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def test_inputs_are_not_overwritten_without_f(tmp_path, caplog):
    caplog.set_level(logging.WARNING)
    base = _copy_inputs(tmp_path / "in")
    before = _tree(tmp_path / "in")
    assert plot.main([str(base), "-s", SIZES, "-m", JSON, "-o", str(tmp_path / "in")]) == 0
    after = _tree(tmp_path / "in")
    assert {k: v for k, v in after.items() if k != STEM + ".pdf"} == before
    assert STEM + ".pdf" in after
    assert sum("is an input: not overwritten" in r.getMessage() for r in caplog.records) == 3


@pytest.mark.parametrize("force,changed", [(["stats"], {"_stats.tab"}), (["mscc"], {"_mscc.tab"}),
                                           (["cc", "stats"], {"_cc.tab", "_stats.tab"}),
                                           (["all"], {"_stats.tab", "_cc.tab", "_mscc.tab"})])
def test_force_overwrite_names_what_is_written(tmp_path, force, changed):
    base = _copy_inputs(tmp_path / "in")
    for s in SUFFIXES:                                             # an old time stamp that a rewrite replaces
        os.utime(str(base) + s, ns=(10 ** 9, 10 ** 9))
    assert plot.main([str(base), "-s", SIZES, "-m", JSON, "-o", str(tmp_path / "in"), "-f"] + force) == 0
    rewritten = {s for s in SUFFIXES if os.stat(str(base) + s).st_mtime_ns != 10 ** 9}
    assert rewritten == changed


# ---- chromosomes --------------------------------------------------------------------------------------------------------
def test_excluding_every_chromosome_is_reads_too_few(tmp_path, caplog):
    caplog.set_level(logging.INFO)
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(tmp_path), "-e", "chr1"]) == 1
    assert "Failed to process the tables" in caplog.text
    assert not os.listdir(tmp_path)


def test_include_filter_limits_the_genome_length(tmp_path):
    out = tmp_path / "out"
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(out), "-i", "chr1", "chr2"]) == 0
    sizes = plot.load_chrom_sizes(SIZES)
    _check_stats(out / (STEM + "_stats.tab"), sizes["chr1"] + sizes["chr2"])


def _with_chr2(src, dst):
    """A copy of a golden correlation table with a second column, chr2, equal to chr1."""
    rows = _cc_rows(src)
    with open(dst, "w") as fh:
        for r in rows:
            fh.write("\t".join(r + [r[2] if r[0] != "shift" else "chr2"]) + "\n")


def test_tables_with_different_chromosomes_use_the_common_ones(tmp_path, caplog):
    caplog.set_level(logging.WARNING)
    d = tmp_path / "in"
    base = _copy_inputs(d)
    _with_chr2(GOLD + "_cc.tab", str(base) + "_cc.tab")           # chr2 in _cc.tab only
    assert plot.main([str(base), "-s", SIZES, "-m", JSON, "-o", str(tmp_path / "out")]) == 0
    assert "using the ones they share: ['chr1']" in caplog.text
    _check_stats(tmp_path / "out" / (STEM + "_stats.tab"), _sizes_sum())
    assert _cc_rows(tmp_path / "out" / (STEM + "_cc.tab"))[0] == ["shift", "whole", "chr1"]


def test_golden_tables_agree(tmp_path, caplog):
    """The golden _nreads.tab lists every reference with 0-0: that is no disagreement."""
    caplog.set_level(logging.WARNING)
    assert plot.main([GOLD, "-s", SIZES, "-m", JSON, "-o", str(tmp_path)]) == 0
    assert "differ" not in caplog.text


# ---- errors -------------------------------------------------------------------------------------------------------------
def _no_files_read(monkeypatch):
    def refused(*a, **k):
        raise AssertionError("a file was read")
    monkeypatch.setattr(plot, "_summary", refused)
    monkeypatch.setattr(plot, "load_chrom_sizes", refused)


@pytest.mark.parametrize("argv", [
    ["-s", SIZES],                                                                      # no stats file
    ["--stats", GOLD + "_stats.tab", "--cc", GOLD + "_cc.tab", "-s", SIZES],            # no nreads
    ["--stats", GOLD + "_stats.tab", "--nreads", GOLD + "_nreads.tab", "-s", SIZES],    # neither --cc nor --masc
    ["--stats", GOLD + "_stats.tab", "--nreads", GOLD + "_nreads.tab", "--cc", "missing_cc.tab", "-s", SIZES],
    ["--stats", "missing_stats.tab", "--nreads", GOLD + "_nreads.tab", "--cc", GOLD + "_cc.tab", "-s", SIZES],
    [GOLD, "-m", JSON],                                                                 # no -s
    [GOLD, "-s", "missing.sizes", "-m", JSON],
    [GOLD, "-s", SIZES],                                                                # --masc without a cache
    [GOLD, "-s", SIZES, "-m", "missing.bigwig"],                                        # the track's cache does not exist
    [GOLD, "-s", SIZES, "-m", JSON, "-f", "masc"],
    [GOLD, "-s", SIZES, "-m", JSON, "-n", "a/b"],
    [GOLD, "-s", SIZES, "-m", JSON, "-w", "0"],
])
def test_argument_errors_exit_2(argv, monkeypatch, capsys):
    _no_files_read(monkeypatch)
    assert plot.main(argv) == 2
    assert "error:" in capsys.readouterr().err


def _run_with(tmp_path, suffix, text, extra=()):
    base = _copy_inputs(tmp_path / "in")
    with open(str(base) + suffix, "w") as fh:
        fh.write(text)
    return plot.main([str(base), "-s", SIZES, "-m", JSON, "-o", str(tmp_path / "out")] + list(extra))


@pytest.mark.parametrize("suffix,text", [
    ("_cc.tab", "shift\twhole\tchr1\n0\t0.1\tnot-a-number\n"),
    ("_cc.tab", "shift\twhole\tchr1\n"),
    ("_mscc.tab", "shift\twhole\tchr1\n0\t0.1\n"),
    ("_nreads.tab", "shift\twhole\tchr1\n"),
    ("_nreads.tab", "shift\twhole\tchr1\nraw\t1-x\t1-x\n"),
    ("_stats.tab", "Name\tx\n"),
    ("_stats.tab", "Name\tx\nRead length\tthirty-six\nExpected library length\tnan\n"),
])
def test_malformed_inputs_exit_1(tmp_path, suffix, text, caplog):
    caplog.set_level(logging.INFO)
    assert _run_with(tmp_path, suffix, text) == 1
    assert "Failed to load the tables" in caplog.text


def test_chromosome_missing_from_sizes_exits_1(tmp_path, caplog):
    sizes = tmp_path / "no_chr1.sizes"
    sizes.write_text("".join(line for line in open(SIZES) if not line.startswith("chr1\t")))
    assert plot.main([GOLD, "-s", str(sizes), "-m", JSON, "-o", str(tmp_path / "out")]) == 1
    assert "'chr1' is not in the chromosome sizes" in caplog.text


def test_chromosome_missing_from_the_cache_exits_1(tmp_path, caplog):
    cache = tmp_path / "other_mappability.json"
    cache.write_text('{"max_shift": 1, "__whole__": [1, 1], "references": {"chr2": [1, 1]}}')
    assert plot.main([GOLD, "-s", SIZES, "-m", str(cache), "-o", str(tmp_path / "out")]) == 1
    assert "'chr1' is not in the mappable-length cache" in caplog.text


@pytest.mark.parametrize("text", ["chr1\t249250621\nchr2 243199373\n", "chr1\tlong\n", "chr1\n"])
def test_unparsable_sizes_line_exits_1(tmp_path, text, caplog):
    sizes = tmp_path / "bad.sizes"
    sizes.write_text(text)
    assert plot.main([GOLD, "-s", str(sizes), "-m", JSON, "-o", str(tmp_path / "out")]) == 1
    assert "not a chromosome name and a length" in caplog.text


# ---- what parsing imports ------------------------------------------------------------------------------------------------
_PROBE = """
import sys
from pymasc_amd import plot
rc = plot.main(sys.argv[1:])
maps = open("/proc/self/maps").read() if sys.platform.startswith("linux") else ""
print("RC", rc, "torch" in sys.modules, "matplotlib" in sys.modules, "libpymasc" in maps)
"""


@pytest.mark.parametrize("argv,rc", [(["--help"], 0), (["--version"], 0), (["base"], 2),
                                     ([GOLD, "-s", SIZES], 2)])
def test_parsing_imports_no_torch_or_matplotlib(argv, rc, tmp_path):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    p = subprocess.run([sys.executable, "-c", _PROBE] + argv, capture_output=True, text=True, timeout=120, env=env,
                       cwd=str(tmp_path))
    assert p.stdout.strip().splitlines()[-1] == "RC {} False False False".format(rc), p.stderr


def test_help_lists_the_options(capsys):
    assert plot.main(["--help"]) == 0
    out = capsys.readouterr().out
    for opt in ("--stats", "--cc", "--masc", "--nreads", "--sizes", "--mappability-stats", "--include-chrom",
                "--exclude-chrom", "--chi2-pval", "--smooth-window", "--mask-size", "--bg-avr-width", "--library-length",
                "--name", "--outdir", "--force-overwrite", "--log-level", "--disable-progress", "--color", "--version"):
        assert opt in out
    a = plot.get_parser().parse_args([])
    assert (a.chi2_pval, a.smooth_window, a.mask_size, a.bg_avr_width, a.library_length, str(a.outdir), a.name,
            a.force_overwrite, a.chromfilter) == (0.05, 15, 5, 50, None, ".", None, [], None)


# ---- pymasc then pymasc-plot, on the host readers and the test context ----------------------------------------------------
def test_replot_of_a_pymasc_run_equals_its_stats(tmp_path, monkeypatch):
    from pymasc_amd import ffi, pipeline
    from tests.fake_context import FakeContext
    from tests.test_cli import _fragments
    from tests.test_run_files import MAPQ, SHIFT, _track
    monkeypatch.setattr(ffi, "Context", lambda device=0: FakeContext())
    monkeypatch.setattr(pipeline, "default_device_ingest", lambda *a, **k: False)
    monkeypatch.setattr(inputs, "default_device_ingest", lambda *a, **k: False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.delenv("RANK", raising=False)
    bam = _fragments(tmp_path / "f36.bam", 36, 1)
    bw = _track(tmp_path / "m.bw")
    for extra, plot_extra in (([], []), (["-i", "c2"], ["-i", "c2"]), (["--skip-ncc"], [])):
        out, rep = tmp_path / ("out" + "".join(extra)), tmp_path / ("rep" + "".join(extra))
        assert cli.main([bam, "-m", bw, "-q", str(MAPQ), "-d", str(SHIFT), "-l", "90", "-o", str(out), "--skip-plots"]
                        + extra) == 0
        assert plot.main([str(out / "f36"), "-s", bam, "-m", bw, "-o", str(rep)] + plot_extra) == 0
        assert S.load_stats(rep / "f36_stats.tab") == S.load_stats(out / "f36_stats.tab")
        for suffix in ("_cc.tab", "_mscc.tab"):
            if not (out / ("f36" + suffix)).exists():
                assert not (rep / ("f36" + suffix)).exists()
                continue
            got, want = _cc_rows(rep / ("f36" + suffix)), _cc_rows(out / ("f36" + suffix))
            assert [r[0] for r in got] == [r[0] for r in want] and got[0] == want[0]
            assert [r[2:] for r in got] == [r[2:] for r in want]
            np.testing.assert_almost_equal([float(r[1]) for r in got[1:]], [float(r[1]) for r in want[1:]], decimal=10)
        # NCC, MSCC, NCC vs MSCC and a page per chromosome (no zoomed page: 2 x est is past max_shift here)
        assert _pages(rep / "f36.pdf") == {(): 5, ("-i", "c2"): 4, ("--skip-ncc",): 4}[tuple(extra)]
