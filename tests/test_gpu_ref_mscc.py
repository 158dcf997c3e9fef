"""GPU: the calculator and the kernels against the numbers of the reference's compiled `successive` MSCC calculator
(tests/golden/ref_successive_mscc.json.gz, oracle/make_ref_mscc_vectors.py) DIRECTLY -- not through the CPU oracle, which is
our own restatement of the reference's bitarray calculator.  Every case under every kernel_flags value that is legal for its
shape, with the kernel family that ran asserted from the launch counters (level 1: the kernels that do work, not the fallback
launches behind the event kernel), so that no family can pass for another; then once more through the raw ABI on bit vectors
built from the reads the reference kept.  Integers exactly, cc within 1e-15 (the tolerance used against its tables)."""
import numpy as np
import pytest

from oracle import model as oracle
from pymasc_amd import ffi
from pymasc_amd.calculator import CCHipCalculator
from . import ref_mscc_cases as rm
from .helpers import DictFeeder

pytestmark = pytest.mark.gpu

DENSE, SPARSE, WINDOW = ffi.PMX_FLAG_FORCE_DENSE, ffi.PMX_FLAG_FORCE_SPARSE, ffi.PMX_FLAG_WINDOW_ONLY
HINT, DEEP = ffi.PMX_FLAG_EVENTS_HINT, ffi.PMX_FLAG_DEEP_LISTS
# (name, kernel_flags, lag table handed over: the calculator then sets PMX_FLAG_SKIP_MLEN itself)
VARIANTS = [("default", 0, False), ("force_dense", DENSE, False), ("force_sparse", SPARSE, False), ("events_hint", HINT, False),
            ("events_hint_deep", HINT | DEEP, False), ("window_only", WINDOW, False), ("skip_mlen", 0, True)]
RAW_FLAGS = [0, DENSE, SPARSE, HINT, HINT | DEEP, WINDOW]


def family(case, flags):
    """The kernel family a call must run on (include/pymasc_amd.h): reads beyond 1024 bases and PMX_FLAG_FORCE_DENSE -> the dense
    kernels; PMX_FLAG_WINDOW_ONLY and max_shift beyond 8191 -> the window kernels; everything else -> the event kernel (the
    cases are sparse: the calculator's own density hint never says `window` for a pass of theirs)."""
    if (flags & DENSE) or case["read_len"] > 1024:
        return "dense"
    if (flags & WINDOW) or case["max_shift"] > 8191:
        return "window"
    return "events"


# Without a hint the raw ABI takes one from a sample of the vectors (include/pymasc_amd.h: PMX_FLAG_EVENTS_HINT): the 2202 runs of
# this chromosome, 4404 edges on a third of a tile, are beyond the 1536 of the event kernel's edge list -> the window kernels
PROBED_WINDOW = {("l_edge_densities", "l1")}


def refused(case, flags):
    return bool(flags & SPARSE) and case["read_len"] > 1024


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_claim_mode(0)
    c.close()


def launches(ctx, fn):
    """fn's result and the launches per family while it ran."""
    ctx.set_profiling(1)
    ctx.reset_kernel_times()
    try:
        out = fn()
        n = {"dense": ctx.kernel_time(ffi.PMX_KERNEL_CC_DENSE)[1], "window": ctx.kernel_time(ffi.PMX_KERNEL_CC_SPARSE)[1],
             "events": ctx.kernel_time(ffi.PMX_KERNEL_CC_EVENTS)[1], "autocorr": ctx.kernel_time(ffi.PMX_KERNEL_AUTOCORR)[1]}
    finally:
        ctx.set_profiling(False)
    return out, n


def assert_family(n, want, what):
    for fam in ("dense", "window", "events"):
        assert (n[fam] > 0) == (fam == want), (what, "expected the %s kernels" % want, n)


def run_calculator(ctx, case, flags, known):
    S, L = case["max_shift"], case["read_len"]
    table = {ch: e["mappable_len"] for ch, e in case["expected"]["chroms"].items()} if known else None
    calc = CCHipCalculator(S, L, [n for n, _ in case["chroms"]], [g for _, g in case["chroms"]],
                           bwfeeder=DictFeeder(rm.track_of(case)), kernel_flags=flags, context=ctx, chrom2mappable_len=table)
    try:
        rm.feed(calc, case)
        calc.finishup_calculation()
        return {n: calc.get_result(n) for n, _ in case["chroms"]}, (calc.forward_read_len_sum, calc.reverse_read_len_sum)
    finally:
        calc.close()


def check_against_reference(case, results, read_len_sums):
    S, L = case["max_shift"], case["read_len"]
    exp = case["expected"]
    assert sorted(exp["chroms"]) == sorted(case["track"])
    for name, _g in case["chroms"]:
        r = results[name].mappable_chrom
        if name not in exp["chroms"]:
            # absent from the track: the bitarray calculator's empty placeholder (bitarray/mscc.pyx:196-205), no MSCC row
            assert not any(r.mappable_len) and not np.any(r.forward_sum) and not np.any(r.reverse_sum) and np.isnan(r.cc).all()
            continue
        e = exp["chroms"][name]
        for k in ("forward_sum", "reverse_sum", "ccbins"):
            assert [int(x) for x in getattr(r, k)] == e[k], (name, k)
        mlen = list(r.mappable_len)
        assert len(mlen) == (S + 1 if name not in case["reads"] else max(L, S - L + 2)) and None not in mlen
        assert [int(x) for x in mlen] == e["mappable_len"][:len(mlen)], name
        ecc = rm.nan_array(e["cc"])
        got = np.asarray(r.cc, dtype=np.float64)
        assert got.shape == ecc.shape and np.array_equal(np.isnan(ecc), np.isnan(got)), name
        m = ~np.isnan(ecc)
        np.testing.assert_allclose(got[m], ecc[m], rtol=0, atol=1e-15)
    # the reference's genome-wide read-length sums leave out the kept reads that contribute to no lag (ref_mscc_cases.py)
    fdrop, rdrop = rm.read_len_sums_of_reads_in_no_lag(case)
    assert read_len_sums[0] - fdrop == exp["forward_read_len_sum"]
    assert read_len_sums[1] - rdrop == exp["reverse_read_len_sum"]


@pytest.mark.parametrize("variant", VARIANTS, ids=[v[0] for v in VARIANTS])
@pytest.mark.parametrize("case", rm.CASES, ids=rm.IDS)
def test_calculator_against_the_reference(ctx, case, variant):
    _name, flags, known = variant
    if refused(case, flags):
        with pytest.raises(ffi.PmxError):
            run_calculator(ctx, case, flags, known)
        return
    want = family(case, flags)
    # the hinted instantiations of the max_shift <= 1023 event kernel hand their tiles out by claims: also the static walk
    hinted = want == "events" and case["max_shift"] <= 1023 and (flags & HINT)
    for mode in ((0, 2) if hinted else (0,)):
        ctx.debug_set_claim_mode(mode)
        try:
            (results, sums), n = launches(ctx, lambda: run_calculator(ctx, case, flags, known))
        finally:
            ctx.debug_set_claim_mode(0)
        assert_family(n, want, (case["name"], _name, mode))
        if known and want != "dense":
            assert n["autocorr"] == 0, "the lag table was handed over: no mappable-length pass"
        check_against_reference(case, results, sums)


@pytest.mark.parametrize("case", rm.CASES, ids=rm.IDS)
def test_raw_abi_against_the_reference(ctx, case):
    """The kernels alone, without the calculator's feed: F, R and M from the reads the reference kept and the runs that pass
    its filter; the three MSCC rows, and row MLEN[d] = mappable_len[|L - 1 - d|], against its numbers."""
    S, L = case["max_shift"], case["read_len"]
    d = np.arange(S + 1)
    for name, e in case["expected"]["chroms"].items():
        if name not in case["reads"]:
            continue
        nbits = rm.vector_bits(case, name)
        fpos, _fl, rend, _rl = rm.kept_reads(case, name)
        F = oracle.bits_from_positions(fpos, nbits)
        R = oracle.bits_from_positions(rend, nbits)
        M = oracle.bits_from_intervals([(b, x) for b, x, v in case["track"][name] if np.float32(v) >= np.float32(1.0)], nbits)
        rows = {ffi.PMX_ROW_MSCC_FSUM: e["forward_sum"], ffi.PMX_ROW_MSCC_RSUM: e["reverse_sum"],
                ffi.PMX_ROW_MSCC_CCBINS: e["ccbins"], ffi.PMX_ROW_MLEN: np.asarray(e["mappable_len"])[np.abs(L - 1 - d)]}
        for flags in RAW_FLAGS:
            if refused(case, flags):
                with pytest.raises(ffi.PmxError):
                    ctx.calc_correlation(F, R, M, nbits, S, L, flags)
                continue
            out, n = launches(ctx, lambda: ctx.calc_correlation(F, R, M, nbits, S, L, flags))
            want = family(case, flags)
            if flags == 0 and want == "events" and (case["name"], name) in PROBED_WINDOW:
                want = "window"
            assert_family(n, want, (case["name"], name, flags))
            assert int(out[ffi.PMX_ROW_SCALARS, 3]) == (ffi.PMX_PATH_DENSE if want == "dense" else ffi.PMX_PATH_SPARSE)
            assert (int(out[ffi.PMX_ROW_SCALARS, 0]), int(out[ffi.PMX_ROW_SCALARS, 1])) == (fpos.size, rend.size)
            for row, want_row in rows.items():
                np.testing.assert_array_equal(out[row].astype(np.int64), np.asarray(want_row, dtype=np.int64), err_msg=str((name, flags, row)))
