"""The host branches of the set-bit launch layer that no other test takes: the on-by-default environment switches
PMX_CC_FUSE_MLEN, PMX_CC_FUSE_MLEN_BIG, PMX_EV_EE_LDS and PMX_CC_EVENTS_BIG set to 0 (read once per process: each in a
child process), and 33 jobs -- one more than a job table holds, so a second pass of the launcher in the context's other flag
area -- on the two sub-paths of the max_shift <= 1023 event pass (events then k_cc_sparse behind the plan; events then
k_windows_flagged).  Everything is bit-exact against the oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_batch import run_batch
from .test_gpu_parity import check_block

pytestmark = pytest.mark.gpu

L = 36
FLAGS = (0, ffi.PMX_FLAG_FORCE_SPARSE)
SWITCHES = [
    # variable set to "0" in the child, max_shift
    ("PMX_CC_FUSE_MLEN", 1000),        # the mappable-length pass stays a pass of its own behind the event kernel
    ("PMX_CC_FUSE_MLEN_BIG", 1500),    # ... beyond 1023 shifts
    ("PMX_EV_EE_LDS", 1500),           # the fused pairs' row of lags in the slab instead of LDS
    ("PMX_CC_EVENTS_BIG", 1500),       # the window kernel in shift chunks instead of the BIG event kernel
]


def switch_cases(S):
    return [synth.make_case(700 + i, 200000, S, L, 0.005, 0.005, True) for i in range(3)]


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def here(ctx):
    """per max_shift, computed once: the cases, their oracle results and the in-process rows for each of FLAGS"""
    cache = {}

    def get(S):
        if S not in cache:
            cases = switch_cases(S)
            refs = [oracle.calc_correlation(F, R, M, nbits, S, L) for nbits, F, R, M in cases]
            rows = {fl: [o.astype(np.int64) for o in run_batch(ctx, cases, S, L, True, fl)] for fl in FLAGS}
            cache[S] = (refs, rows)
        return cache[S]
    return get


CHILD = (
    "import json, sys, numpy as np\n"
    "from pymasc_amd import ffi\n"
    "from tests.test_gpu_batch import run_batch\n"
    "from tests.test_gpu_launch_switches import switch_cases, L, FLAGS\n"
    "S = int(sys.argv[1])\n"
    "c = ffi.Context(0)\n"
    "outs = {str(fl): [o.astype(np.int64).tolist() for o in run_batch(c, switch_cases(S), S, L, True, fl)] for fl in FLAGS}\n"
    "c.close()\n"
    "print(json.dumps(outs))\n"
)


@pytest.mark.parametrize("var,S", SWITCHES, ids=[v for v, _ in SWITCHES])
def test_switch_off_in_a_child_process(here, var, S):
    refs, rows = here(S)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env[var] = "0"
    res = subprocess.run([sys.executable, "-c", CHILD, str(S)], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    child = json.loads(res.stdout.strip().splitlines()[-1])
    for fl in FLAGS:
        for got, mine, ref in zip(child[str(fl)], rows[fl], refs):
            got = np.asarray(got, dtype=np.int64)
            np.testing.assert_array_equal(got, mine)
            check_block(got.astype(np.uint64), ref, S, True)
            assert int(got[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE


def jobs_33(S):
    """33 chromosomes: two passes of the max_shift <= 1023 kernels (32 jobs, then one), with a read-dense stretch (tiles the event
    kernel flags for the window kernels) in one chromosome of EACH pass, so that the second pass depends on finding its
    flags, counters and job statistics clear."""
    rng = np.random.default_rng(3300 + S)
    cases = []
    for i in range(33):
        n = 140000 + 7919 * i if i in (5, 32) else 4000 + 613 * i
        nbits, F, R, M = synth.make_case(900 + i, n, S, L, 0.006, 0.006, True, mean_on=1500, mean_off=400)
        if i in (5, 32):
            F |= synth.random_bits(rng, nbits, 0.06, 70000, 125000)
            R |= synth.random_bits(rng, nbits, 0.06, 66000, 120000)
        cases.append((nbits, F, R, M))
    return cases


@pytest.fixture(scope="module")
def jobs_33_with_refs():
    S = 300
    cases = jobs_33(S)
    return S, cases, [oracle.calc_correlation(F, R, M, nbits, S, L) for nbits, F, R, M in cases]


def test_33_jobs_skip_mlen_events_then_window_kernel(ctx, jobs_33_with_refs):
    """PMX_FLAG_SKIP_MLEN: nothing to fuse, so each pass is k_cc_events, k_events_finish, k_cc_sparse behind the plan"""
    S, cases, refs = jobs_33_with_refs
    outs = run_batch(ctx, cases, S, L, True, ffi.PMX_FLAG_SKIP_MLEN)
    for out, ref in zip(outs, refs):
        assert int(out[ffi.PMX_ROW_SCALARS, 0]) == ref["ncc_forward_sum"]
        assert int(out[ffi.PMX_ROW_SCALARS, 1]) == ref["ncc_reverse_sum"]
        np.testing.assert_array_equal(out[ffi.PMX_ROW_NCC_CCBINS, :S + 1].astype(np.int64), ref["ncc_ccbins"])
        np.testing.assert_array_equal(out[ffi.PMX_ROW_MSCC_FSUM].astype(np.int64), ref["mscc_forward_sum"])
        np.testing.assert_array_equal(out[ffi.PMX_ROW_MSCC_RSUM].astype(np.int64), ref["mscc_reverse_sum"])
        np.testing.assert_array_equal(out[ffi.PMX_ROW_MSCC_CCBINS].astype(np.int64), ref["mscc_ccbins"])
        assert not out[ffi.PMX_ROW_MLEN].any() and out[ffi.PMX_ROW_SCALARS, 2] == 0
        assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE


def test_33_jobs_skip_ncc_with_a_track(ctx, jobs_33_with_refs):
    """PMX_FLAG_SKIP_NCC with a track: the instantiations without the NCC counter, the mappable-length pairs fused into each pass
    (k_cc_events, k_events_finish, k_windows_flagged)"""
    S, cases, refs = jobs_33_with_refs
    outs = run_batch(ctx, cases, S, L, True, ffi.PMX_FLAG_SKIP_NCC)
    for out, ref in zip(outs, refs):
        check_block(out, ref, S, True, skip_ncc=True)
        assert not out[ffi.PMX_ROW_NCC_CCBINS].any()
        assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
