"""pymasc_amd.stats: the fragment-length estimate and NSC / RSC / FWHM / VSN of PyMaSC's _stats.tab, on the host.

Expected rows all come from the reference:
  * the golden payloads (tests/ref_consumers_child.golden_calc) against the reference's golden ENCFF000RMB-test_stats.tab
    and against the rows its own consumers made from them (tests/golden/ref_consumers.json);
  * the branch cases of tests/stats_cases.py against what the reference's make_genome_wide_stat + output_stats made of the
    same inputs (tests/golden/ref_stats_cases.json, written by tests/ref_stats_child.py).  Where a PyMaSC checkout is at
    hand (PYMASC_REFERENCE) the child runs live and must still give the stored fixture.
Integers and strings must match exactly, floats to decimal=10 (the reference's tests/integration/test_golden_outputs.py)."""
import json
import logging
import math
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

from pymasc_amd import result as R
from pymasc_amd import stats as S
from pymasc_amd.exceptions import ReadsTooFew
from . import ref_consumers_child as RC
from . import stats_cases as SC

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYMASC_REFERENCE", "")
LIVE = bool(REF) and os.path.isdir(os.path.join(REF, "PyMaSC"))
CASES = os.path.join(HERE, "golden", "ref_stats_cases.json")
CHROM_FIELDS = ["est_lib_len", "cc_min", "ccrl"] + [p + k for p in ("expected.", "estimated.")
                                                  for k in ("fragment_length", "ccfl", "fwhm", "nsc", "rsc", "vsn")]


def _same(got, want, what):
    try:
        g, w = float(got), float(want)
    except ValueError:
        assert got == want, what
        return
    if want in ("False", "True") or got in ("False", "True"):
        assert got == want, what
    elif np.isnan(w):
        assert np.isnan(g), (what, got)
    elif "." not in want and "e" not in want and want not in ("inf", "-inf"):
        assert got == want, what                       # an integer: exactly
    else:
        np.testing.assert_almost_equal(g, w, decimal=10, err_msg=what)


def _assert_rows(got, want):
    assert list(got) == list(S.STATS_LABELS)
    assert set(got) == set(want)
    for k in want:
        _same(got[k], want[k], k)


def _file_rows(tmp_path, st, name="ENCFF000RMB-test"):
    path = S.write_stats(tmp_path / name, st)
    assert path.name == name + "_stats.tab"
    return S.load_stats(path)


@pytest.fixture(scope="module")
def golden_payloads():
    calc, names = RC.golden_calc()
    return {"single": calc.get_whole_result(),
            "aggregated": R.aggregate_results({c: pickle.loads(pickle.dumps(calc.get_result(c))) for c in names}),
            "ncc_only": RC.golden_calc(with_track=False)[0].get_whole_result(),
            "skip_ncc": RC.golden_calc(skip_ncc=True)[0].get_whole_result()}


@pytest.fixture(scope="module")
def ref_cases():
    with open(CASES) as fh:
        stored = json.load(fh)
    if LIVE:
        env = dict(os.environ, PYTHONPATH=REF + os.pathsep + os.environ.get("PYTHONPATH", ""))
        p = subprocess.run([sys.executable, os.path.join(HERE, "ref_stats_child.py")], env=env, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
        assert json.loads(p.stdout.strip().splitlines()[-1]) == stored, \
            "the reference's statistics no longer give what tests/golden/ref_stats_cases.json holds"
    return stored


# ---- the golden run ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("key", ["single", "aggregated"])
def test_golden_stats_tab(tmp_path, golden_payloads, key):
    """The golden payloads give the reference's golden _stats.tab."""
    got = _file_rows(tmp_path, S.genome_wide_stats(golden_payloads[key], 36))
    _assert_rows(got, S.load_stats(os.path.join(HERE, "golden", "ENCFF000RMB-test_stats.tab")))


@pytest.mark.parametrize("key", ["single", "aggregated", "ncc_only", "skip_ncc"])
def test_consumer_rows(tmp_path, golden_payloads, key):
    """Row for row what the reference's consumers made of the same four payloads (NCC only estimates from NCC)."""
    with open(os.path.join(HERE, "golden", "ref_consumers.json")) as fh:
        want = json.load(fh)["rows"][key]
    _assert_rows(_file_rows(tmp_path, S.genome_wide_stats(golden_payloads[key], 36)), want)


def test_golden_file_layout(tmp_path, golden_payloads):
    st = S.genome_wide_stats(golden_payloads["single"], 36)
    path = S.write_stats(tmp_path / "x", st)
    lines = path.read_text().splitlines()
    assert len(lines) == 34 and [ln.split("\t")[0] for ln in lines] == list(S.STATS_LABELS)
    assert lines[0] == "Name\tx" and lines[3] == "Estimated library length\t65"
    assert st.est_lib_len == 65 and st.whole_ncc.est_lib_len == 122      # NCC's scores are taken at MSCC's estimate
    assert st.whole_ncc.estimated.fragment_length == 65
    assert st.whole_mscc.cc_lower is not None and st.whole_mscc.avr_cc.shape == (301,)
    assert set(st.ncc) == {"chr1"} and set(st.mscc) == {"chr1"}           # chromosomes without reads have no entry


def test_result_untouched_and_cc_computed_when_missing(golden_payloads):
    """Results whose cc is not computed yet are computed on the way (as tables.build_tables does)."""
    calc, _ = RC.golden_calc(with_track=False)
    w = calc.get_whole_result()
    want = S.stats_rows("n", S.genome_wide_stats(w, 36))
    for r in w.chroms.values():
        r.cc = None
    assert S.stats_rows("n", S.genome_wide_stats(w, 36)) == want


# ---- branch cases, against the reference -----------------------------------------------------------------------------

def _all_cases():
    with open(CASES) as fh:
        return sorted(json.load(fh))


def _run_case(name, golden_payloads):
    built = SC.cases(R)
    if name in built:
        build, opts = built[name]
        return build(), opts
    key, opts = SC.golden_cases()[name]
    return golden_payloads[key], opts


def _chrom_values(s):
    vals = [s.est_lib_len, s.cc_min, s.ccrl] + [getattr(m, k) for m in (s.expected, s.estimated)
                                                for k in ("fragment_length", "ccfl", "fwhm", "nsc", "rsc", "vsn")]
    return [S._fmt(v) for v in vals]


@pytest.mark.parametrize("name", _all_cases())
def test_branch_case(tmp_path, ref_cases, golden_payloads, name):
    want = ref_cases[name]
    result, opts = _run_case(name, golden_payloads)
    assert want["options"] == opts                     # the fixture was made from these very inputs
    opts = dict(SC.PARAM_DEFAULTS, **opts)
    if "raises" in want:
        assert want["raises"] == "ReadsTooFew"
        with pytest.raises(ReadsTooFew):
            S.genome_wide_stats(result, **opts)
        return
    st = S.genome_wide_stats(result, **opts)
    _assert_rows(_file_rows(tmp_path, st, "case"), want["rows"])
    for kind, mine in (("ncc", st.ncc), ("mscc", st.mscc)):
        ref = want[kind] or {}
        assert set(mine) == set(ref), kind
        for c, vals in ref.items():
            for f, g, w in zip(CHROM_FIELDS, _chrom_values(mine[c]), vals):
                _same(g, w, (kind, c, f))


def test_cases_cover_the_branches(ref_cases):
    """The fixture holds each branch the issue names: a given library length, a failed FWHM on each side and on both,
    a NaN background, the masked estimate landing on the mask's edge, and ReadsTooFew."""
    rows = {k: v["rows"] for k, v in ref_cases.items() if "rows" in v}
    assert rows["library_length"]["FWHM"] not in ("nan", "False") and rows["library_length"]["NSC"] != "nan"
    assert rows["fwhm_both_fail"]["Estimated FWHM"] == "False" and rows["fwhm_both_fail"]["Estimated VSN"] == "0.0"
    assert rows["fwhm_forward_fails"]["Estimated FWHM"] == "29"             # twice the backward half width, plus one
    assert rows["fwhm_backward_fails"]["Estimated FWHM"] == "239"           # twice the forward half width, plus one
    assert ref_cases["cc_min_nan"]["ncc"]["c1"][1] == "nan" and ref_cases["cc_min_nan"]["ncc"]["c1"][11] == "False"
    assert rows["mask_edge_low"]["Estimated library length"] == "30"       # read_len - mask_size - 1: the mask's edge
    assert rows["mask_edge_high"]["Estimated library length"] == "42"      # read_len + mask_size + 1: the other edge
    assert rows["phantom_masked"]["Estimated library length"] == "122"     # masked: the fragment peak
    assert rows["mask_zero_near"]["Estimated library length"] == "39"       # mask_size=0: no mask near the read length
    assert sum("raises" in v for v in ref_cases.values()) == 3


# ---- logging -------------------------------------------------------------------------------------------------------

def _case(name):
    build, opts = SC.cases(R)[name]
    return build(), dict(SC.PARAM_DEFAULTS, **opts)


def test_chi2_warning(caplog):
    """1000 forward vs 500 reverse reads: the strand-balance test warns; 600 vs 640 only informs."""
    result, opts = _case("strand_imbalance")
    with caplog.at_level(logging.INFO, logger="pymasc_amd.stats"):
        S.genome_wide_stats(result, **opts)
    warned = [r for r in caplog.records if r.levelno == logging.WARNING and "imbalanced" in r.getMessage()]
    assert len(warned) == 1 and "1000 / 500" in warned[0].getMessage()
    caplog.clear()
    result, opts = _case("library_length")
    with caplog.at_level(logging.INFO, logger="pymasc_amd.stats"):
        S.genome_wide_stats(result, **opts)
    assert not [r for r in caplog.records if "imbalanced" in r.getMessage()]
    assert [r for r in caplog.records if r.levelno == logging.INFO and "600 / 640" in r.getMessage()]


def test_chi2_p_value_is_chi2_sf():
    """erfc(sqrt(x / 2)) is the survival function of chi-squared with one degree of freedom (scipy where present)."""
    sp = pytest.importorskip("scipy.stats")
    for x in (0.0, 0.1, 1.0, 3.841458820694124, 10.0, 50.0):
        np.testing.assert_allclose(math.erfc(math.sqrt(x / 2)), sp.chi2.sf(x, 1), rtol=1e-12)


def test_mask_edge_logs_error(caplog):
    result, opts = _case("mask_edge_low")
    with caplog.at_level(logging.WARNING, logger="pymasc_amd.stats"):
        S.genome_wide_stats(result, **opts)
    assert any(r.levelno == logging.ERROR and "close to the read length" in r.getMessage() for r in caplog.records)
    caplog.clear()
    result, opts = _case("phantom_masked")                                  # masked well away from the edge: no error
    with caplog.at_level(logging.WARNING, logger="pymasc_amd.stats"):
        S.genome_wide_stats(result, **opts)
    assert any("masking the phantom peak" in r.getMessage() for r in caplog.records)
    assert not any(r.levelno == logging.ERROR for r in caplog.records)


def test_mscc_without_forward_reads_warns_when_ncc_present(caplog):
    result, opts = _case("both_mscc_no_forward")
    with caplog.at_level(logging.WARNING, logger="pymasc_amd.stats"):
        S.genome_wide_stats(result, **opts)
    assert any("no forward read in mappable regions" in r.getMessage() for r in caplog.records)


# ---- options and edges ---------------------------------------------------------------------------------------------

def test_moving_average_edges():
    x = np.arange(20, dtype=np.float64) ** 2
    avr = S.moving_average(x, 5)
    assert avr[0] == np.mean(x[:2]) and avr[1] == np.mean(x[:3])
    assert avr[-1] == np.mean(x[-2:]) and avr[-2] == np.mean(x[-3:])
    assert avr[10] == pytest.approx(np.mean(x[8:13]))
    np.testing.assert_array_equal(S.moving_average(x, 1), x)


def test_fwhm_peak_below_background_is_value_error():
    avr = np.linspace(1.0, 0.0, 50)
    with pytest.raises(ValueError, match="not above the background"):
        S._fwhm(avr, 0.99, 3)


@pytest.mark.parametrize("kw", [dict(library_length=0), dict(smooth_window=0), dict(library_length=301, max_shift=300),
                                dict(read_len=0)])
def test_check_params(kw):
    args = dict(read_len=36, library_length=None, smooth_window=15, max_shift=None)
    args.update(kw)
    with pytest.raises(ValueError):
        S.check_params(**args)


def test_check_params_accepts_library_length_at_max_shift():
    S.check_params(36, 300, 15, 300)


@pytest.mark.parametrize("kw", [dict(library_length=301), dict(library_length=0), dict(smooth_window=0)])
def test_pipeline_rejects_options_before_any_work(tmp_path, monkeypatch, kw):
    """pipeline.run raises the ValueError before it opens a file or touches torch.distributed."""
    from pymasc_amd import ffi, pipeline, sharding

    def boom(*a, **k):
        raise AssertionError("work started")
    for mod, name in ((pipeline, "open_alignments"), (pipeline, "open_track"), (pipeline, "run_sharded"), (ffi, "Context"),
                      (pipeline, "rank_and_world"), (sharding, "rank_and_world")):
        monkeypatch.setattr(mod, name, boom)
    with pytest.raises(ValueError):
        pipeline.run(tmp_path / "missing.bam", tmp_path / "out", 300, stats=True, **kw)
    assert not (tmp_path / "out").exists()


def test_unsupported_result_type():
    with pytest.raises(TypeError):
        S.genome_wide_stats(object(), 36)


def test_load_stats_round_trip(tmp_path, golden_payloads):
    st = S.genome_wide_stats(golden_payloads["ncc_only"], 36, library_length=100)
    got = _file_rows(tmp_path, st, "rt")
    assert got == dict(S.stats_rows("rt", st))
    assert got["Expected library length"] == "100" and got["DMP length"] == "nan"
