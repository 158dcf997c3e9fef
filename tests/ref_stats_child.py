"""Generator of tests/golden/ref_stats_cases.json (needs a PyMaSC checkout on PYTHONPATH: PYMASC_REFERENCE).

Feeds the branch cases of tests/stats_cases.py -- synthetic curves, and the golden payloads of
tests/ref_consumers_child.golden_calc under other options -- through the REFERENCE's own statistics
(PyMaSC/stats.py make_genome_wide_stat, PyMaSC/output/stats.py output_stats) and prints, as JSON on the last line of stdout,
each case's _stats.tab rows, or the name of the exception the reference raised.

    python tests/ref_stats_child.py --write-golden     (PyMaSC on PYTHONPATH)
writes the same JSON to tests/golden/ref_stats_cases.json: what tests/test_stats.py checks where PyMaSC is absent."""
import json
import logging
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import ref_consumers_child as RC  # noqa: E402
import stats_cases as SC  # noqa: E402
from pymasc_amd import result as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "ref_stats_cases.json")


def golden_payloads():
    calc, _ = RC.golden_calc()
    return {"single": calc.get_whole_result(),
            "ncc_only": RC.golden_calc(with_track=False)[0].get_whole_result(),
            "skip_ncc": RC.golden_calc(skip_ncc=True)[0].get_whole_result()}


def chrom_values(stats, est_lib_len, cc_min, ccrl, expected, estimated):
    """One chromosome's statistics as the text _stats.tab would give them (str of the value, None as "nan")."""
    vals = [est_lib_len, cc_min, ccrl] + [getattr(m, k) for m in (expected, estimated)
                                          for k in ("fragment_length", "ccfl", "fwhm", "nsc", "rsc", "vsn")]
    return ["nan" if v is None else str(v) for v in vals]


CHROM_FIELDS = ["est_lib_len", "cc_min", "ccrl"] + [p + k for p in ("expected.", "estimated.")
                                                  for k in ("fragment_length", "ccfl", "fwhm", "nsc", "rsc", "vsn")]


def per_chrom(chroms):
    if chroms is None:
        return None
    return {c: chrom_values(s, s.est_lib_len, s.stats.cc_min, s.stats.ccrl, s.stats.metrics_at_expected_length,
                            s.stats.metrics_at_estimated_length) for c, s in chroms.items()}


def reference_rows(result, opts):
    """{"rows": {label: value}, "ncc"/"mscc": {chrom: [CHROM_FIELDS values]}} of the reference's statistics, or
    {"raises": exception class name}."""
    from PyMaSC.output.stats import output_stats
    from PyMaSC.stats import make_genome_wide_stat
    o = dict(SC.PARAM_DEFAULTS, **opts)
    config = RC.StatConfig(read_length=o["read_len"], chi2_pval=o["chi2_pval"], mv_avr_filter_len=o["smooth_window"],
                           filter_mask_len=o["mask_size"], min_calc_width=o["bg_avr_width"],
                           expected_library_length=o["library_length"])
    try:
        stats = make_genome_wide_stat(result, config, output_warnings=True)
    except Exception as e:
        return {"raises": type(e).__name__}
    with tempfile.TemporaryDirectory() as td:
        base = os.path.join(td, "case")
        output_stats(base, stats)
        with open(base + "_stats.tab") as fh:
            rows = dict(line.rstrip("\n").split("\t", 1) for line in fh if "\t" in line)
    return {"rows": rows, "ncc": per_chrom(stats.ncc_stats), "mscc": per_chrom(stats.mscc_stats)}


def main():
    assert R.REFERENCE_TYPES, "PyMaSC importable but pymasc_amd.result did not bind the reference's classes"
    logging.disable(logging.CRITICAL)
    out = {}
    for name, (build, opts) in SC.cases(R).items():
        out[name] = dict(reference_rows(build(), opts), options=opts)
    gold = golden_payloads()
    for name, (key, opts) in SC.golden_cases().items():
        out[name] = dict(reference_rows(gold[key], opts), options=opts, payload=key)
    if "--write-golden" in sys.argv:
        with open(GOLDEN, "w") as fh:
            json.dump(out, fh, sort_keys=True, indent=1)
            fh.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
