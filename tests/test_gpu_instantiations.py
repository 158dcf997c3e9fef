"""Every template instantiation of the set-bit launch layer (kernels_sparse.hip, kernels_events.h) once against the CPU
oracle, bit-exact, with the launch ledger (pmx_debug_ledger_*, include/pymasc_amd.h) asserting WHICH instantiation ran: a case
names, per ledger family, the entries its call must launch, and no other entry of any family may have been launched.

The last test needs no GPU: every entry of every family the library reports must be declared by at least one case, so an
instantiation added to a chooser's table fails the suite until it has a row here.

One input for every shift range: five 65536-bit tiles and an odd remainder (nbits is no multiple of 64), bits 0 and
nbits - 1 set, reads at 0.5 % per strand, one tile with more reads than the deep list pool holds, one stretch of the track
with more run edges per tile than the event kernel lists -- so the event kernel, both kinds of flagged tiles and the window
pass behind it all contribute to the rows.  Oracle results are computed once per (track, max_shift, read_len)."""
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np
import pytest

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_events_big import events_ran
from .test_gpu_parity import EVENT_CAP_E, EVENT_POOL_DEEP, EVENT_POOL_M, EVENT_POOL_NCC, EVENT_TILE, check_block

gpu = pytest.mark.gpu

# ledger families, in the order of include/pymasc_amd.h
EV, BIG, SP, SPCH, WF, AE, RS, AP, RP, AF, ET = range(11)
FAMILIES = {
    EV: "PMX_LEDGER_CC_EVENTS", BIG: "PMX_LEDGER_CC_EVENTS_BIG", SP: "PMX_LEDGER_CC_SPARSE", SPCH: "PMX_LEDGER_CC_SPARSE_CH",
    WF: "PMX_LEDGER_WINDOWS_FLAGGED", AE: "PMX_LEDGER_AUTOCORR_EDGES", RS: "PMX_LEDGER_REDUCE_SEGMENTS",
    AP: "PMX_LEDGER_AUTOCORR_PAIRS", RP: "PMX_LEDGER_REDUCE_PAIRS", AF: "PMX_LEDGER_AUTOCORR_FINISH", ET: "PMX_LEDGER_EVENTS_TAIL",
}

NCC, MLEN = ffi.PMX_FLAG_SKIP_NCC, ffi.PMX_FLAG_SKIP_MLEN
FORCE, DEEP, HINT, WINDOW = ffi.PMX_FLAG_FORCE_SPARSE, ffi.PMX_FLAG_DEEP_LISTS, ffi.PMX_FLAG_EVENTS_HINT, ffi.PMX_FLAG_WINDOW_ONLY
L = 36

# ---- the input -------------------------------------------------------------------------------------------------------
NBITS = 5 * EVENT_TILE + 12345
READ_TILE, EDGE_TILE = 2, 4
# reads per strand in the read-dense tile: each strand alone is beyond the largest pool (with a track, deep, NCC only)
DENSE_READS = 1.25 * max(EVENT_POOL_M, EVENT_POOL_DEEP, EVENT_POOL_NCC) / EVENT_TILE
assert NBITS % 64 and DENSE_READS * EVENT_TILE > EVENT_POOL_DEEP


def build_input():
    rng = np.random.default_rng(52)
    F = synth.random_bits(rng, NBITS, 0.005, 0, NBITS)
    R = synth.random_bits(rng, NBITS, 0.005, 0, NBITS)
    F |= synth.random_bits(rng, NBITS, DENSE_READS, READ_TILE * EVENT_TILE + 300, (READ_TILE + 1) * EVENT_TILE - 500)
    R |= synth.random_bits(rng, NBITS, DENSE_READS, READ_TILE * EVENT_TILE + 300, (READ_TILE + 1) * EVENT_TILE - 500)
    M = synth.run_bits(rng, NBITS, 2500, 700, 0, EDGE_TILE * EVENT_TILE)
    M |= synth.run_bits(rng, NBITS, 8, 6, EDGE_TILE * EVENT_TILE + 100, (EDGE_TILE + 1) * EVENT_TILE)   # ~9000 edges in the tile
    M |= synth.run_bits(rng, NBITS, 900, 300, (EDGE_TILE + 1) * EVENT_TILE + 64, NBITS)
    for w in (F, R, M):
        synth.set_bit(w, 0)
        synth.set_bit(w, NBITS - 1)
    return F, R, M


def edges_in_tile(M, tile):
    bits = np.unpackbits(M.view(np.uint8), bitorder="little")[:NBITS].astype(np.int8)
    d = np.flatnonzero(np.diff(np.concatenate([[0], bits, [0]])))
    return int(((d >= tile * EVENT_TILE) & (d < (tile + 1) * EVENT_TILE)).sum())


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    F, R, M = build_input()
    vectors = str(tmp_path_factory.mktemp("instantiations") / "vectors.npz")   # for the cases that run in a child process
    np.savez(vectors, F=F, R=R, M=M)
    assert edges_in_tile(M, EDGE_TILE) > 2 * EVENT_CAP_E and edges_in_tile(M, 0) < EVENT_CAP_E // 4
    refs, lens = {}, {}

    def ref(with_m, S):
        if (with_m, S) not in refs:
            refs[(with_m, S)] = oracle.calc_correlation(F, R, M if with_m else None, NBITS, S, L)
        return refs[(with_m, S)]

    def mlen(lag):
        if lag not in lens:
            lens[lag] = oracle.mappable_len_readless(M, NBITS, lag)
        return lens[lag]
    return F, R, M, ref, mlen, vectors


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.close()


def launched(ctx):
    """{family: set of launched entries} of the ledger, families without a launch left out"""
    led = ctx.debug_ledger()
    return {f: {i for i, n in enumerate(row) if n} for f, row in enumerate(led) if any(row)}


def names(entries):
    return {FAMILIES.get(f, f): sorted(ix) for f, ix in entries.items()}


# ---- the matrix ------------------------------------------------------------------------------------------------------
# kind "cc": ctx.calc_correlation(F, R, M or None, NBITS, S, L, flags); "mlen": ctx.mappable_len(M, NBITS, S, 0).
# big: None, or (mode, g) for max_shift 1024..8191 -- mode "fused" / "unfused" / "ncc_only", g = 0, 1, 2 for 1, 2, 4 sub-groups:
# the max_shift is the candidate whose launch the ledger shows at g (big_shifts), not a fixed mapping.
# env: None, or environment of a child process that makes the one call and prints its rows and its ledger (switches that
# are read once per process).  expect: {family: entries}, the complete set of launches of the call.
Case = namedtuple("Case", "id kind S with_m flags big expect env", defaults=(None,))


def ev_expect(with_m, skip_ncc, skip_mlen, deep, known):
    """ev_kernel's table and what runs behind it: k_windows_flagged when the mappable-length pairs are fused, else k_cc_sparse"""
    if not with_m:
        return {EV: {16 + (not known)}, SP: {2}}
    e = {EV: {8 * skip_ncc + 4 * skip_mlen + 2 * (not deep) + (not known)}}
    e[SP if skip_mlen else WF] = {1 if skip_ncc else 0}
    return e


def big_expect(mode, g, skip_ncc):
    """ev_big_kernel's table; behind it the chunked window kernel for the flagged tiles, the reduces, and with a track the tail
    (fused: also the window kernel of the mappable-length pass in chunks of lags and its recurrence)"""
    if mode == "ncc_only":
        return {BIG: {12 + g}, RS: {1}, SPCH: {2}}
    e = {BIG: {(0 if mode == "fused" else 6) + 3 * skip_ncc + g}, RS: {1}, ET: {0}, SPCH: {1 if skip_ncc else 0}}
    if mode == "fused":
        e.update({AE: {1}, AF: {0}})
    return e


def window_expect(S, with_m, skip_ncc):
    """the window kernels alone: k_cc_sparse + reduce, and with a track the mappable-length pass of its own"""
    sp = (1 if skip_ncc else 0) if with_m else 2
    e = mlen_expect(max(L - 1, S - L + 1)) if with_m else {}
    e[SP if S <= 1023 else SPCH] = {sp}
    e[RS] = e.get(RS, set()) | {0 if S <= 1023 else 1}
    return e


def mlen_expect(lag):
    return {AP: {0}, RP: {0}, AE: {1 if lag > 1023 else 0}, RS: {1}, AF: {0}}


HINTS = [("force_deep", FORCE | DEEP, True, False), ("deep", DEEP, True, True), ("hint", HINT, False, True), ("force", FORCE, False, False)]


def build_cases():
    cases = []
    for skip_ncc in (0, 1):
        for skip_mlen in (0, 1):
            for name, fl, deep, known in HINTS:
                flags = fl | (NCC if skip_ncc else 0) | (MLEN if skip_mlen else 0)
                cases.append(Case(f"ev_m_ncc{1 - skip_ncc}_mlen{1 - skip_mlen}_{name}", "cc", 1000, True, flags, None,
                                  ev_expect(True, skip_ncc, skip_mlen, deep, known)))
    for name, fl, deep, known in HINTS[2:]:
        cases.append(Case(f"ev_ncc_only_{name}", "cc", 1000, False, fl, None, ev_expect(False, 0, 0, False, known)))
    for name, fl, deep, known in HINTS:   # the other end of the shift range
        cases.append(Case(f"ev_m_S3_ncc0_mlen0_{name}", "cc", 3, True, fl | NCC | MLEN, None, ev_expect(True, 1, 1, deep, known)))
    for g in (0, 1, 2):
        for mode, fl in (("fused", 0), ("unfused", MLEN)):
            for skip_ncc in (0, 1):
                cases.append(Case(f"big_{mode}_ncc{1 - skip_ncc}_nsg{1 << g}", "cc", None, True, FORCE | fl | (NCC if skip_ncc else 0),
                                  (mode, g), big_expect(mode, g, skip_ncc)))
    # Without a track one sub-group's workgroup is at most 40.5 KB of LDS: four fit a CU at every max_shift, so ev_big_plan never
    # chooses 2 or 4 sub-groups itself; PMX_EV_NSG (A/B switch, read once per process) does, in a child process.
    cases.append(Case("big_ncc_only_nsg1", "cc", None, False, FORCE, ("ncc_only", 0), big_expect("ncc_only", 0, 0)))
    for g, S in ((1, 3000), (2, 6000)):
        cases.append(Case(f"big_ncc_only_nsg{1 << g}_forced", "cc", S, False, FORCE, None, big_expect("ncc_only", g, 0),
                          {"PMX_EV_NSG": str(1 << g)}))
    for S, fl in ((1000, WINDOW), (8200, FORCE)):
        cases.append(Case(f"window_S{S}_m", "cc", S, True, fl, None, window_expect(S, True, 0)))
        cases.append(Case(f"window_S{S}_m_skip_ncc", "cc", S, True, fl | NCC, None, window_expect(S, True, 1)))
        cases.append(Case(f"window_S{S}_ncc_only", "cc", S, False, fl, None, window_expect(S, False, 0)))
    for lag in (300, 1023, 1024, 4000):
        cases.append(Case(f"mappable_len_{lag}", "mlen", lag, True, 0, None, mlen_expect(lag)))
    return cases


CASES = build_cases()
BIG_CANDIDATES = (1500, 3000, 6000)   # one max_shift per sub-group count, as the ledger confirms (big_shifts)


@pytest.fixture(scope="module")
def big_shifts(ctx):
    """{(mode, g): max_shift}: each candidate once per mode on a small input, g read from the ledger entry that ran"""
    nbits, F, R, M = synth.make_case(5, 70000, 1024, L, 0.004, 0.004, True)
    found = {}
    for S in BIG_CANDIDATES:
        for mode, with_m, fl in (("fused", True, FORCE), ("unfused", True, FORCE | MLEN), ("ncc_only", False, FORCE)):
            ctx.debug_ledger_reset()
            ctx.calc_correlation(F, R, M if with_m else None, nbits, S, L, fl)
            ran = launched(ctx).get(BIG, set())
            assert len(ran) == 1, (S, mode, ran)
            found.setdefault((mode, next(iter(ran)) % 3), S)
    return found


# (the child takes the vectors from a file: importing this module would cost it more than the call)
CHILD = (
    "import json, sys, numpy as np\n"
    "from pymasc_amd import ffi\n"
    "nbits, S, L, flags, with_m = (int(x) for x in sys.argv[2:7])\n"
    "z = np.load(sys.argv[1])\n"
    "c = ffi.Context(0)\n"
    "c.set_profiling(2)\n"
    "out = c.calc_correlation(z['F'], z['R'], z['M'] if with_m else None, nbits, S, L, flags)\n"
    "win = c.kernel_time(ffi.PMX_KERNEL_CC_SPARSE)[1]\n"
    "led = c.debug_ledger()\n"
    "c.close()\n"
    "print(json.dumps({'out': out.astype('int64').tolist(), 'win': win, 'ledger': led}))\n"
)


def call_in_child(case, S, vectors):
    """(rows, {family: launched entries}, launches of the window kernel) of the case's call in a process with case.env"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, "-c", CHILD, vectors] + [str(int(x)) for x in (NBITS, S, L, case.flags, case.with_m)], cwd=root,
                         env=dict(os.environ, **case.env), capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    got = json.loads(res.stdout.strip().splitlines()[-1])
    ran = {f: {i for i, n in enumerate(row) if n} for f, row in enumerate(got["ledger"]) if any(row)}
    return np.asarray(got["out"], dtype=np.int64).astype(np.uint64), ran, got["win"]


def flag_area(ctx):
    """cc flags (one per 32-Kbit window tile), ac flags (one per 64-Kbit tile), flagged-tile counters of the last event pass"""
    area = ctx.debug_read_flag_area()
    fb = ((NBITS + EVENT_TILE // 2 - 1) // (EVENT_TILE // 2) + 2 + 15) // 16 * 16
    return area[:fb], area[fb:2 * fb], area[2 * fb:2 * fb + 16].view(np.uint32)


@gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_instantiation_against_the_oracle(ctx, data, big_shifts, case):
    F, R, M, ref_of, mlen_of, vectors = data
    S = case.S
    if case.big:
        assert case.big in big_shifts, f"no max_shift of {BIG_CANDIDATES} runs {case.big}: found {big_shifts}"
        S = big_shifts[case.big]
    skip_ncc, skip_mlen = bool(case.flags & NCC), bool(case.flags & MLEN)
    ctx.debug_ledger_reset()
    if case.kind == "mlen":
        got = ctx.mappable_len(M, NBITS, S, 0)
        ran = launched(ctx)
        np.testing.assert_array_equal(got.astype(np.int64), mlen_of(S))
        assert ran == case.expect, (names(ran), names(case.expect))
        return
    if case.env:
        out, ran, win = call_in_child(case, S, vectors)
    else:
        out, _ev, win = events_ran(ctx, lambda: ctx.calc_correlation(F, R, M if case.with_m else None, NBITS, S, L, case.flags))
        ran = launched(ctx)
    ref = ref_of(case.with_m, S)
    if skip_mlen:   # row MLEN is written as zeros
        ref = dict(ref, mappable_len_by_shift=np.zeros(S + 1, dtype=np.int64))
    check_block(out, ref, S, case.with_m, skip_ncc=skip_ncc)
    assert ran == case.expect, (names(ran), names(case.expect))
    assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
    assert int(out[ffi.PMX_ROW_SCALARS, 0]) == ref["ncc_forward_sum"] and int(out[ffi.PMX_ROW_SCALARS, 1]) == ref["ncc_reverse_sum"]
    if skip_mlen:
        assert not out[ffi.PMX_ROW_MLEN].any() and int(out[ffi.PMX_ROW_SCALARS, 2]) == 0
    if skip_ncc:
        assert not out[ffi.PMX_ROW_NCC_CCBINS].any()
    if not case.with_m:
        assert not out[ffi.PMX_ROW_MSCC_FSUM:ffi.PMX_ROW_MLEN + 1].any()
    # the flagged tiles: the window instantiation behind the event kernel had work to do
    if EV in case.expect:
        cc, ac, counts = flag_area(ctx)
        dense = [READ_TILE] + ([EDGE_TILE] if case.with_m else [])
        for t in dense:
            assert cc[2 * t] == 1 and cc[2 * t + 1] == 1, (t, np.flatnonzero(cc))
        assert int(counts[0]) == len(dense), (counts, np.flatnonzero(cc))   # (counted per 64-Kbit tile of the event kernel)
        if WF in case.expect:
            assert int(counts[1]) >= 1 and ac.any(), counts
    elif BIG in case.expect:
        assert win >= 1


def test_every_entry_of_every_family_has_a_case():
    """No kernel launch: the table sizes the library reports against the entries the cases above declare."""
    sizes = ffi.ledger_sizes()
    assert len(sizes) == len(FAMILIES), f"the library reports {len(sizes)} ledger families, this file knows {len(FAMILIES)}"
    for f, name in FAMILIES.items():
        assert getattr(ffi, name) == f, name
    declared = {f: set() for f in FAMILIES}
    for case in CASES:
        for f, entries in case.expect.items():
            declared[f] |= set(entries)
    for f, size in enumerate(sizes):
        missing = sorted(set(range(size)) - declared[f])
        assert not missing, f"{FAMILIES[f]}: entries {missing} of {size} have no case in CASES"
        assert max(declared[f]) < size, f"{FAMILIES[f]}: a case declares entry {max(declared[f])}, the table holds {size}"
