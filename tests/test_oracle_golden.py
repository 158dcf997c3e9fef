"""Pins the CPU oracle (oracle/) to everything the reference's own tests hold for this path:
the CLI goldens of tests/integration/test_golden_outputs.py:44-226 (-d 300 -q 10 -r 36 with the
36-mer mappability track), the lag table JSON, and vectors produced by the reference's compiled
`successive` NCC calculator (oracle/make_ref_vectors.py) and by its `successive` MSCC calculator
(oracle/make_ref_mscc_vectors.py)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import model as oracle
from . import fixtures as fx
from . import ref_mscc_cases as rm
from .helpers import feed_all


@pytest.fixture(scope="module")
def golden_run():
    names, lengths = fx.load_refs()
    calc = oracle.OracleCalculator(300, 36, names, lengths, mappability=fx.load_bedgraph())
    feed_all(calc, fx.load_reads(10))
    calc.flush("chr1")
    return calc


def test_ncc_integers_and_cc_table(golden_run):
    ncc, _ = golden_run.get_result("chr1")
    assert (ncc["forward_sum"], ncc["reverse_sum"]) == (622, 670)
    assert ncc["ccbins"][:5] == [28, 26, 19, 22, 26]
    raw, _ = fx.load_nreads_table()
    assert raw["chr1"] == (622, 670) and raw["whole"] == (622, 670)
    _, cc = fx.load_cc_table("ENCFF000RMB-test_cc.tab")
    np.testing.assert_allclose(ncc["cc"], cc["chr1"], rtol=0, atol=1e-15)


def test_mscc_integers_and_cc_table(golden_run):
    _, mscc = golden_run.get_result("chr1")
    _, per = fx.load_nreads_table()
    np.testing.assert_array_equal(np.array(mscc["forward_sum"]), per["chr1"][0])
    np.testing.assert_array_equal(np.array(mscc["reverse_sum"]), per["chr1"][1])
    assert mscc["ccbins"][:4] == [16, 20, 14, 15]
    _, cc = fx.load_cc_table("ENCFF000RMB-test_mscc.tab")
    np.testing.assert_allclose(mscc["cc"], cc["chr1"], rtol=0, atol=1e-15)


def test_mappable_len_lag_table(golden_run):
    _, mscc = golden_run.get_result("chr1")
    table = fx.load_mappability_json()
    assert table["max_shift"] == 265
    assert list(mscc["mappable_len"]) == table["references"]["chr1"]
    assert len(mscc["mappable_len"]) == max(36, 300 - 36 + 2)


def test_readless_chromosome_lag_table():
    # the same track loaded as a chromosome WITHOUT reads goes through _fill_result's loop
    # (mscc.pyx:207-215) and must give the same lags (symmetry of the autocorrelation)
    names, lengths = ["chr1"], [249250621]
    bg = fx.load_bedgraph()
    # restrict to a window so the (S+1) x 4 full passes stay fast: shift coordinates to a small chromosome
    lo = min(b for b, e, v in bg["chr1"])
    hi = max(e for b, e, v in bg["chr1"])
    small = {"chr1": [(b - lo, e - lo, v) for b, e, v in bg["chr1"]]}
    calc = oracle.OracleCalculator(265, 36, names, [hi - lo], mappability=small)
    calc._fill_result("chr1")
    table = fx.load_mappability_json()
    assert list(calc.ref2mscc["chr1"]["mappable_len"]) == table["references"]["chr1"]


CASES = json.load(open(os.path.join(fx.GOLDEN, "ref_successive_ncc.json")))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_against_reference_successive_ncc(case):
    names = [n for n, _ in case["chroms"]]
    lens = [l for _, l in case["chroms"]]
    calc = oracle.OracleCalculator(case["max_shift"], 36, names, lens)
    for name, pos, rev, rl in case["reads"]:
        (calc.feed_reverse_read if rev else calc.feed_forward_read)(name, pos, rl)
    calc.finishup_calculation()
    exp = case["expected"]
    assert calc.forward_sum == exp["forward_sum"] and calc.reverse_sum == exp["reverse_sum"]
    for ch, e in exp["chroms"].items():
        ncc, _ = calc.get_result(ch)
        for k in ("forward_sum", "reverse_sum", "forward_read_len_sum", "reverse_read_len_sum"):
            assert ncc[k] == e[k], (ch, k)
        assert [int(x) for x in ncc["ccbins"]] == e["ccbins"]
        ecc = np.array([np.nan if x is None else x for x in e["cc"]])
        assert np.array_equal(np.isnan(ecc), np.isnan(ncc["cc"]))
        m = ~np.isnan(ecc)
        np.testing.assert_allclose(ncc["cc"][m], ecc[m], rtol=0, atol=1e-15)


@pytest.fixture(scope="module")
def mscc_oracle_runs():
    """every case of the reference's successive MSCC vectors through the CPU oracle, once"""
    cache = {}

    def get(case):
        if case["name"] not in cache:
            calc = oracle.OracleCalculator(case["max_shift"], case["read_len"], [n for n, _ in case["chroms"]],
                                           [g for _, g in case["chroms"]], mappability=rm.track_of(case))
            rm.feed(calc, case)
            calc.finishup_calculation()
            cache[case["name"]] = calc
        return cache[case["name"]]
    return get


@pytest.mark.parametrize("case", rm.CASES, ids=rm.IDS)
def test_against_reference_successive_mscc(case, mscc_oracle_runs):
    """The oracle restates the reference's BITARRAY calculator; its compiled SUCCESSIVE calculator is the second witness.
    Integers exactly, the lag table over the lags both sides hold (the reference's feeder: max_shift + 1, the bitarray
    calculator: max(L, S - L + 2)), cc within the tolerance used against the reference's tables.  The read-length sums: the
    successive calculator leaves out the reads that contribute to no lag and keeps them genome-wide only
    (oracle/make_ref_mscc_vectors.py, docstring, 3), so the oracle's sums less those reads must be its figures exactly."""
    S, L = case["max_shift"], case["read_len"]
    calc = mscc_oracle_runs(case)
    exp = case["expected"]
    # a chromosome absent from the track: no result in the successive calculator (mscc.pyx:213-216, :489-490), an empty
    # placeholder with an all-zero lag table in the bitarray calculator (bitarray/mscc.pyx:196-205) -- and no MSCC row of it
    assert sorted(exp["chroms"]) == sorted(n for n, _ in case["chroms"] if n in case["track"])
    for n, _g in case["chroms"]:
        if n not in case["track"]:
            ph = calc.ref2mscc[n]
            assert ph.get("empty") and not any(ph["mappable_len"]) and not np.any(ph["forward_sum"]) and np.isnan(ph["cc"]).all()
    for ch, e in exp["chroms"].items():
        mscc = calc.ref2mscc[ch]
        for k in ("forward_sum", "reverse_sum", "ccbins"):
            assert len(e[k]) == S + 1 and [int(x) for x in mscc[k]] == e[k], (ch, k)
        mlen = list(mscc["mappable_len"])
        assert len(mlen) == (S + 1 if mscc.get("empty") else max(L, S - L + 2)) and None not in mlen
        assert mlen == e["mappable_len"][:len(mlen)], ch
        ecc = rm.nan_array(e["cc"])
        assert np.array_equal(np.isnan(ecc), np.isnan(mscc["cc"])), ch
        m = ~np.isnan(ecc)
        np.testing.assert_allclose(mscc["cc"][m], ecc[m], rtol=0, atol=1e-15)
        assert (e["forward_read_len_sum"], e["reverse_read_len_sum"]) == (0, 0)     # (never incremented per chromosome there)
    fdrop, rdrop = rm.read_len_sums_of_reads_in_no_lag(case)
    assert calc.forward_read_len_sum - fdrop == exp["forward_read_len_sum"]
    assert calc.reverse_read_len_sum - rdrop == exp["reverse_read_len_sum"]
    # and the sums the bitarray rules give are what the kept reads add up to, chromosome by chromosome
    for ch in case["reads"]:
        _fp, flen, _re, rlen = rm.kept_reads(case, ch)
        res = calc.ref2ncc[ch]
        assert (res["forward_read_len_sum"], res["reverse_read_len_sum"]) == (int(flen.sum()), int(rlen.sum())), ch


RECIPE_CHILD = (
    "import gzip, os, sys\n"
    "sys.path.insert(0, os.path.join(sys.argv[1], 'oracle'))\n"
    "import make_ref_mscc_vectors as gen\n"
    "assert gen.FIXTURE == sys.argv[2], gen.FIXTURE\n"
    "data = open(os.path.join(sys.argv[1], 'tests', 'golden', gen.FIXTURE), 'rb').read()\n"
    "assert len(data) <= gen.MAX_FIXTURE_BYTES\n"
    "assert gen.dumps(gen.generate()) == gzip.decompress(data).decode(), 'the fixture is not what the recipe gives'\n"
    "print('RECIPE_OK')\n"
)


def test_reference_successive_mscc_vectors_match_their_recipe():
    """Re-runs oracle/make_ref_mscc_vectors.py in memory where the reference's modules were built (oracle/build_ref.sh):
    the JSON text in the committed fixture is exactly what the recipe gives.  In a child process, because the generator puts the reference
    tree on sys.path and loads its modules: processes that later tests of this run spawn would inherit both."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    reference = os.environ.get("PYMASC_REFERENCE", "/root/reference")
    if not os.path.isdir(os.path.join(reference, "PyMaSC")):
        pytest.skip("no reference tree here")
    if not all(glob.glob(os.path.join(root, "oracle", "_ref", m + ".*so")) for m in ("mscc", "mappability", "bigwig")):
        pytest.skip("oracle/_ref is not built (oracle/build_ref.sh)")
    res = subprocess.run([sys.executable, "-c", RECIPE_CHILD, root, rm.FIXTURE], cwd=root, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and res.stdout.strip().endswith("RECIPE_OK"), res.stderr[-3000:]


def test_bruteforce_definition_small():
    """cc_oracle.c (shift-and-count passes) vs the index-form definitions of SURVEY.md section 0,
    evaluated bit by bit in pure Python on a tiny case."""
    rng = np.random.default_rng(7)
    G, S, L = 300, 90, 12
    nbits = G + L + S + 100
    f = np.zeros(nbits, dtype=np.int64)
    r = np.zeros(nbits, dtype=np.int64)
    m = np.zeros(nbits, dtype=np.int64)
    f[rng.integers(1, G + 1, 60)] = 1
    r[rng.integers(1, G + L, 60)] = 1
    for s in range(1, G, 25):
        m[s:s + int(rng.integers(3, 22))] = 1
    m[G + 1:] = 0
    pack = lambda b: np.packbits(np.concatenate([b, np.zeros((-nbits) % 64, dtype=np.int64)]).astype(np.uint8),
                                 bitorder="little").view(np.uint64).copy()
    out = oracle.calc_correlation(pack(f), pack(r), pack(m), nbits, S, L)
    M = lambda i: int(m[i]) if 0 <= i < nbits else 0
    R = lambda i: int(r[i]) if 0 <= i < nbits else 0
    for d in range(S + 1):
        D = [M(j) & M(j + L - 1 - d) for j in range(nbits)]
        assert out["ncc_ccbins"][d] == sum(int(f[j]) & R(j + d) for j in range(nbits))
        assert out["mappable_len_by_shift"][d] == sum(D)
        assert out["mscc_forward_sum"][d] == sum(int(f[j]) & D[j] for j in range(nbits))
        assert out["mscc_reverse_sum"][d] == sum(R(j + d) & D[j] for j in range(nbits))
        assert out["mscc_ccbins"][d] == sum(int(f[j]) & R(j + d) & D[j] for j in range(nbits))


def test_fixture_read_counts_match_the_reference_summary():
    """The reference's own summary of its test BAM (tests/integration/expected_results/encode_data_summary.json:
    total_reads 2501, all on chr1, chr1_valid_reads 1292) against the fixture the
    parity tests are fed from: 1292 = 622 forward + 670 reverse reads after the -q 10 filter."""
    import csv
    import os
    with open(os.path.join(fx.GOLDEN, "ENCFF000RMB-test.reads.tsv")) as fh:
        rows = list(csv.reader(fh, delimiter="\t"))[1:]
    assert len(rows) == 2501 and {r[1] for r in rows} == {"chr1"}
    reads = fx.load_reads(mapq=10)
    assert len(reads) == 1292
    assert (sum(1 for r in reads if not r[0]), sum(1 for r in reads if r[0])) == (622, 670)
