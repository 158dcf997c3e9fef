"""Drop-in proof at the Python boundary: the reference's OWN consumers accept what CCHipCalculator returns.

Where a PyMaSC checkout is at hand (PYMASC_REFERENCE, a directory holding the PyMaSC package), the consumers run live in a
child process with it on PYTHONPATH so that ``pymasc_amd.result`` binds the reference's classes there, while this pytest
process keeps the stand-alone dataclasses.  The child is tests/ref_consumers_child.py; the expected numbers are the
reference's committed golden ``ENCFF000RMB-test_stats.tab`` (tests/integration/test_golden_outputs.py:44-105, decimal=10).

Everywhere else the child's last run stands in, stored in tests/golden/ref_consumers.json: the _stats.tab rows the
reference's consumers made, and a digest of each payload they were given.  test_payloads_are_what_the_consumers_took
pins this process's payloads to those digests, so the stored rows are the rows of what the calculator returns today."""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("PYMASC_REFERENCE", "")
LIVE = bool(REF) and os.path.isdir(os.path.join(REF, "PyMaSC"))
GOLDEN = os.path.join(HERE, "golden", "ref_consumers.json")


def _stored():
    with open(GOLDEN) as fh:
        return json.load(fh)


def _golden_stats():
    with open(os.path.join(HERE, "golden", "ENCFF000RMB-test_stats.tab")) as fh:
        return dict(line.rstrip("\n").split("\t", 1) for line in fh if "\t" in line)


def _assert_rows(got, want, keys=None):
    assert set(got) == set(want)
    for k in (keys or want):
        try:
            g, w = float(got[k]), float(want[k])
        except ValueError:
            assert got[k] == want[k], k
            continue
        if np.isnan(w):
            assert np.isnan(g), (k, got[k])
        else:
            np.testing.assert_almost_equal(g, w, decimal=10, err_msg=k)


@pytest.fixture(scope="module")
def child_rows():
    if not LIVE:
        return _stored()["rows"]
    env = dict(os.environ, PYTHONPATH=REF + os.pathsep + os.environ.get("PYTHONPATH", ""))
    p = subprocess.run([sys.executable, os.path.join(HERE, "ref_consumers_child.py")], env=env,
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + "\n" + p.stderr[-4000:]
    doc = json.loads(p.stdout.strip().splitlines()[-1])
    assert doc == _stored(), "the reference's consumers no longer give what tests/golden/ref_consumers.json holds"
    return doc["rows"]


def test_payloads_are_what_the_consumers_took():
    """The stand-alone payloads of this process (single-process, aggregated, NCC only, --skip-ncc) are, field for field and
    bit for bit, the payloads whose _stats.tab rows the reference's consumers made (tests/golden/ref_consumers.json)."""
    from . import ref_consumers_child as C
    from pymasc_amd import result as R
    calc, names = C.golden_calc()
    got = {"single": calc.get_whole_result(),
           "aggregated": R.aggregate_results({c: pickle.loads(pickle.dumps(calc.get_result(c))) for c in names}),
           "ncc_only": C.golden_calc(with_track=False)[0].get_whole_result(),
           "skip_ncc": C.golden_calc(skip_ncc=True)[0].get_whole_result()}
    want = _stored()["payload"]
    assert set(want) == set(got)
    for k, obj in got.items():
        assert C.payload_digest(obj) == want[k], k


def test_single_process_payload_through_reference_stats(child_rows):
    """get_whole_result() -> make_genome_wide_stat -> output_stats == the reference's golden _stats.tab."""
    _assert_rows(child_rows["single"], _golden_stats())


def test_worker_payloads_through_reference_aggregation(child_rows):
    """pickled get_result() per chromosome -> isinstance(ChromResult) -> aggregate_results -> same _stats.tab."""
    _assert_rows(child_rows["aggregated"], _golden_stats())


def test_ncc_only_and_skip_ncc_payloads(child_rows):
    """NCCGenomeWideResult (no track) and the --skip-ncc payload go through the same consumers.  Without MSCC the
    reference estimates the library length from the NCC curve itself, so only the rows that do not depend on that
    estimate are comparable with the golden (NCC+MSCC) run."""
    want = _golden_stats()
    got = child_rows["ncc_only"]
    _assert_rows(got, dict(got, **{k: want[k] for k in want}),
                 ["Name", "Read length", "Genome length", "Forward reads", "Reverse reads", "Minimum NCC",
                  "NCC at read length"])
    assert got["DMP length"] == "nan" and got["Estimated library length"] != "nan"
    got = child_rows["skip_ncc"]
    _assert_rows(got, dict(got, **{k: want[k] for k in want}),
                 [k for k in want if "MSCC" in k or "DMP" in k] + ["Estimated library length"])


def test_standalone_types_here():
    """This process has no PyMaSC on the path: the stand-alone dataclasses are bound (what the GPU box runs)."""
    from pymasc_amd import result as R
    assert not R.REFERENCE_TYPES and R.NCCResult.__module__ == "pymasc_amd.result"
