"""GPU parity of the event kernel's hinted instantiations below 1024 shifts (KNOWN_SPARSE, kernels_events.h): what a call
with PMX_FLAG_EVENTS_HINT or PMX_FLAG_DEEP_LISTS runs.  They carry no job-wide verdict on dense chromosomes -- every dense
tile is flagged on its own -- and take a tile's run starts from its edge totals.  Every case against the CPU oracle at
max_shift 1000 and 3, and bit for bit against the same call under PMX_FLAG_FORCE_SPARSE (the instantiation with the verdict
and the per-quad run starts).  Geometry: a tile is 65536 bits, two rows of 32768."""
import numpy as np
import pytest
import torch

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_batch import run_batch
from .test_gpu_events_big import events_ran
from .test_gpu_events_offsets import pack
from .test_gpu_parity import EVENT_TILE, check_block

pytestmark = pytest.mark.gpu

ROW = EVENT_TILE // 2
SHIFTS = [(1000, 36), (3, 36)]
HINT, DEEP, FORCE = ffi.PMX_FLAG_EVENTS_HINT, ffi.PMX_FLAG_DEEP_LISTS, ffi.PMX_FLAG_FORCE_SPARSE


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_max_workgroups(0)
    c.close()


def tile_counts(F, R, M, nbits):
    """Per 64-Kbit tile: forward + reverse reads, run edges (what the event kernel holds against its list capacities)."""
    def bits(w):
        b = np.unpackbits(w.view(np.uint8), bitorder="little")[:nbits]
        return np.concatenate([b, np.zeros((-nbits) % EVENT_TILE, dtype=np.uint8)])
    nt = (nbits + EVENT_TILE - 1) // EVENT_TILE
    reads = (bits(F).astype(np.int64) + bits(R)).reshape(nt, EVENT_TILE).sum(axis=1)
    m = bits(M)
    edges = (m != np.concatenate([[0], m[:-1]])).astype(np.int64).reshape(nt, EVENT_TILE).sum(axis=1)
    return reads, edges


POOL_DEEP, CAP_EDGES = 4328, 1536   # kernels_events.h: EV_POOL_DEEP (the larger of the two pools), EV_CAPE_SMALL


def check(ctx, F, R, M, nbits, hint=HINT, refs=None, poison=None):
    """Both shift ranges under `hint`: against the oracle, and equal to the call under PMX_FLAG_FORCE_SPARSE.
    poison: scratch buffers and LDS hold this pattern before the hinted call."""
    for S, L in SHIFTS:
        ref = refs[(S, L)] if refs else oracle.calc_correlation(F, R, M, nbits, S, L)

        def call():
            if poison is not None:
                ctx.debug_poison(poison)
            return ctx.calc_correlation(F, R, M, nbits, S, L, hint)

        out, ev, _win = events_ran(ctx, call)   # (the window launch behind the event kernel is made whether or not a tile was flagged)
        check_block(out, ref, S, M is not None)
        assert ev == 1, "the event kernel must have run"
        assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
        if M is not None:   # (row MLEN: in check_block) popcount(M)
            assert int(out[ffi.PMX_ROW_SCALARS, 2]) == int(oracle.lib().pmo_count(oracle._p(M), M.size))
        old = ctx.calc_correlation(F, R, M, nbits, S, L, FORCE | (hint & DEEP))
        assert np.array_equal(out, old), "differs from the instantiation with the verdict"


def check_all(ctx, F, R, M, nbits):
    """With a track, NCC-only and with the deep pool."""
    check(ctx, F, R, M, nbits)
    check(ctx, F, R, None, nbits)
    check(ctx, F, R, M, nbits, DEEP)


@pytest.mark.parametrize("extra", [0, 1, 127, 128])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_sparse_vectors_around_a_tile_boundary(ctx, k, extra):
    nbits = EVENT_TILE * k + extra
    rng = np.random.default_rng(7000 + 10 * k + extra)
    F = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    R = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    for w in (F, R, M):
        synth.set_bit(w, 0)
        synth.set_bit(w, nbits - 1)
    check_all(ctx, F, R, M, nbits)


NT = 20   # tiles of the dense cases: one workgroup (or each of two) sees more than the 16 tiles a verdict needs


def dense_case(kind):
    """Twenty tiles, sparse at 0.4 % per strand on an ordinary track, + the dense tiles of `kind`."""
    nbits = NT * EVENT_TILE
    rng = np.random.default_rng({"reads": 31, "edges": 32, "middle": 33, "first": 34, "last": 35}[kind])
    F = synth.random_bits(rng, nbits, 0.004, 0, nbits)
    R = synth.random_bits(rng, nbits, 0.004, 0, nbits)
    M = synth.run_bits(rng, nbits, 900, 300, 0, nbits)
    tiles = {"reads": range(3, 17), "edges": range(2, 16), "middle": [9], "first": [0], "last": [NT - 1]}[kind]
    for t in tiles:
        lo, hi = t * EVENT_TILE, (t + 1) * EVENT_TILE
        if kind == "edges":    # runs of ~10 bits: ~6500 run edges per tile, beyond the 1536 of the list
            keep = synth.run_bits(np.random.default_rng(1), nbits, 10**9, 1, 0, lo) | synth.run_bits(np.random.default_rng(1), nbits, 10**9, 1, hi, nbits)
            M = (M & keep) | synth.run_bits(rng, nbits, 6, 4, lo, hi)
        else:                  # 4 % per strand: ~5200 reads per tile, beyond both pools
            F |= synth.random_bits(rng, nbits, 0.04, lo, hi)
            R |= synth.random_bits(rng, nbits, 0.04, lo, hi)
    # the fixture is what it says: the tiles named are beyond the lists of both pools, the others far within, and the two
    # mostly-dense kinds are beyond the verdict's 60 %
    reads, edges = tile_counts(F, R, M, nbits)
    over = (edges > CAP_EDGES) if kind == "edges" else (reads > POOL_DEEP)
    assert sorted(np.flatnonzero(over)) == list(tiles), (kind, reads, edges)
    assert ((reads + edges)[~over] < 1500).all(), (kind, reads, edges)
    assert kind not in ("reads", "edges") or 10 * len(tiles) > 6 * NT
    refs = {(S, L): oracle.calc_correlation(F, R, M, nbits, S, L) for S, L in SHIFTS}
    refs_ncc = {(S, L): oracle.calc_correlation(F, R, None, nbits, S, L) for S, L in SHIFTS}
    return nbits, F, R, M, refs, refs_ncc


@pytest.fixture(scope="module", params=["reads", "edges", "middle", "first", "last"])
def dense(request):
    return dense_case(request.param)


@pytest.mark.parametrize("nwg", [1, 2])
def test_dense_tiles_under_a_hint_are_flagged_one_by_one(ctx, dense, nwg):
    """More than 60 % of the tiles read-dense / edge-dense (without a hint the job-wide verdict hands the rest of the range
    over), and one dense tile in the middle, at the start, at the end: under the hint the sums are the oracle's."""
    nbits, F, R, M, refs, refs_ncc = dense
    ctx.debug_set_max_workgroups(nwg)
    try:
        check(ctx, F, R, M, nbits, HINT, refs)
        check(ctx, F, R, None, nbits, HINT, refs_ncc)
        check(ctx, F, R, M, nbits, DEEP, refs)
    finally:
        ctx.debug_set_max_workgroups(0)


def _job(seed, tiles, dense_reads):
    nbits = tiles * EVENT_TILE - 77
    rng = np.random.default_rng(seed)
    d = 0.04 if dense_reads else 0.004
    F, R = synth.random_bits(rng, nbits, d, 0, nbits), synth.random_bits(rng, nbits, d, 0, nbits)
    M = synth.run_bits(rng, nbits, 900, 300, 0, nbits)
    reads, edges = tile_counts(F, R, M, nbits)
    assert (reads > POOL_DEEP).all() if dense_reads else ((reads + edges) < 1500).all()
    return nbits, F, R, M


VARIANTS = [(True, HINT), (False, HINT), (True, DEEP)]   # with a track, NCC-only, the deep pool
VARIANT_IDS = ["track", "ncc", "deep"]


@pytest.mark.parametrize("njobs", [2, 3])
@pytest.mark.parametrize("with_m,hint", VARIANTS, ids=VARIANT_IDS)
def test_a_dense_job_beside_sparse_ones_in_one_workgroup(ctx, njobs, with_m, hint):
    """One workgroup walks every job of the batch: a job boundary inside its range, one job all dense -- its flagged tiles are
    counted when the workgroup leaves the job, and the window kernels' sums are added exactly once."""
    cases = [_job(40 + i, 3 - (i & 1), dense_reads=(i == 1)) for i in range(njobs)]
    ctx.debug_set_max_workgroups(1)
    try:
        for S, L in SHIFTS:
            outs, ev, _win = events_ran(ctx, lambda: run_batch(ctx, cases, S, L, with_m, hint))
            assert ev == 1, "the event kernel must have run"
            olds = run_batch(ctx, cases, S, L, with_m, FORCE | (hint & DEEP))
            for (nbits, F, R, M), out, old in zip(cases, outs, olds):
                check_block(out, oracle.calc_correlation(F, R, M if with_m else None, nbits, S, L), S, with_m)
                assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
                assert np.array_equal(out, old)
    finally:
        ctx.debug_set_max_workgroups(0)


@pytest.fixture(scope="module")
def ranged():
    """Eight tiles, tiles 2..5 read-dense; + the references."""
    nbits = 8 * EVENT_TILE - 5
    rng = np.random.default_rng(51)
    F = synth.random_bits(rng, nbits, 0.004, 0, nbits) | synth.random_bits(rng, nbits, 0.04, 2 * EVENT_TILE, 6 * EVENT_TILE)
    R = synth.random_bits(rng, nbits, 0.004, 0, nbits) | synth.random_bits(rng, nbits, 0.04, 2 * EVENT_TILE, 6 * EVENT_TILE)
    M = synth.run_bits(rng, nbits, 900, 300, 0, nbits)
    reads, edges = tile_counts(F, R, M, nbits)
    assert list(np.flatnonzero(reads > POOL_DEEP)) == [2, 3, 4, 5] and ((reads + edges)[[0, 1, 6, 7]] < 1500).all()
    refs = {(with_m, S): oracle.calc_correlation(F, R, M if with_m else None, nbits, S, L) for S, L in SHIFTS for with_m in (True, False)}
    return nbits, F, R, M, refs


@pytest.mark.parametrize("nwg", [1, 0], ids=["one_workgroup", "all_workgroups"])
@pytest.mark.parametrize("with_m,hint", VARIANTS, ids=VARIANT_IDS)
def test_tile_ranges_that_start_and_end_inside_a_dense_stretch(ctx, ranged, with_m, hint, nwg):
    """pmx_cc_batch_ranges_dev (it adds the hint itself): the shares of ranges cut inside a read-dense stretch add up to the
    chromosome, and equal the shares of the same call under PMX_FLAG_FORCE_SPARSE one by one."""
    nbits, F, R, M, refs = ranged
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x.view(np.int64)).to(dev) for x in (F, R, M)]
    cuts = [0, 3, 5, 8]
    n = len(cuts) - 1

    def shares(S, L, flags):
        outs = [torch.full((ffi.PMX_NROWS, S + 1), -1, dtype=torch.int64, device=dev) for _ in range(n)]
        torch.cuda.synchronize()
        ctx.cc_batch_ranges_dev([t[0].data_ptr()] * n, [t[1].data_ptr()] * n, [t[2].data_ptr()] * n if with_m else None, [nbits] * n,
                                cuts[:-1], [b - a for a, b in zip(cuts[:-1], cuts[1:])], S, L, flags, [o.data_ptr() for o in outs])
        ctx.sync()
        return [o.cpu().numpy().view(np.uint64) for o in outs]

    ctx.debug_set_max_workgroups(nwg)
    try:
        for S, L in SHIFTS:
            outs, ev, _win = events_ran(ctx, lambda: shares(S, L, hint & DEEP))
            assert ev == 1, "the event kernel must have run"
            total = sum(outs)
            check_block(total, refs[(with_m, S)], S, with_m)
            assert int(total[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
            for out, old in zip(outs, shares(S, L, FORCE | (hint & DEEP))):
                assert np.array_equal(out, old), "differs from the instantiation with the verdict"
    finally:
        ctx.debug_set_max_workgroups(0)


def _track(nbits, kind):
    b = np.zeros(nbits, dtype=np.uint8)
    T = EVENT_TILE
    if kind == "ones":
        b[:] = 1
    elif kind == "zeros":
        pass
    elif kind == "starts_and_ends_at_1":
        b[:500] = 1
        b[nbits - 700:] = 1
        b[T + 100:T + 4000] = 1
    elif kind == "runs_on_tile_bits":       # runs that start / end exactly on the first / last bit of a tile
        b[T:T + 10] = 1                     # starts on the first bit of tile 1
        b[2 * T - 10:2 * T] = 1             # ends on the last bit of tile 1
        b[2 * T] = 1                        # a run of one bit: the first bit of tile 2
        b[3 * T - 1] = 1                    # ... the last bit of tile 2, continued into tile 3
        b[3 * T:3 * T + 5] = 1
        b[4 * T - 1:4 * T + 1] = 1          # across the boundary of tiles 3 and 4
    elif kind == "runs_on_row_bits":        # the same on the 32-Kbit row inside a tile
        b[T + ROW:T + ROW + 10] = 1
        b[T + ROW - 10:T + ROW - 3] = 1
        b[2 * T + ROW - 1] = 1
        b[3 * T + ROW] = 1
        b[4 * T + ROW - 1:4 * T + ROW + 1] = 1
    elif kind == "one_run_over_tiles":      # tiles 1..3 without a run edge, inside a run
        b[T - 3:4 * T + 3] = 1
    return pack(b)


@pytest.mark.parametrize("kind", ["ones", "zeros", "starts_and_ends_at_1", "runs_on_tile_bits", "runs_on_row_bits", "one_run_over_tiles"])
def test_run_starts_from_the_tile_totals(ctx, kind):
    """Twice the run starts of a tile = its run edges + M[its last bit] - M[the bit below it]: row MLEN and popcount(M)
    against the oracle on tracks whose runs touch exactly the bits the formula reads.  One workgroup and many."""
    nbits = 5 * EVENT_TILE + 300
    rng = np.random.default_rng(61)
    F = synth.random_bits(rng, nbits, 0.004, 0, nbits)
    R = synth.random_bits(rng, nbits, 0.004, 0, nbits)
    M = _track(nbits, kind)
    refs = {(S, L): oracle.calc_correlation(F, R, M, nbits, S, L) for S, L in SHIFTS}
    for nwg in (0, 1):
        ctx.debug_set_max_workgroups(nwg)
        try:
            check(ctx, F, R, M, nbits, HINT, refs)
            check(ctx, F, R, M, nbits, DEEP, refs)
        finally:
            ctx.debug_set_max_workgroups(0)


@pytest.fixture(scope="module")
def three_tiles():
    nbits = 3 * EVENT_TILE
    rng = np.random.default_rng(71)
    F = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    R = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    refs = {(S, L): oracle.calc_correlation(F, R, M, nbits, S, L) for S, L in SHIFTS}
    refs_ncc = {(S, L): oracle.calc_correlation(F, R, None, nbits, S, L) for S, L in SHIFTS}
    return nbits, F, R, M, refs, refs_ncc


@pytest.mark.parametrize("pattern", [0x00000000, 0xffffffff, 0x80808080, 0x7fffffff, 0x5a5a5a5a])
def test_one_workgroup_over_three_tiles_with_stale_memory(ctx, three_tiles, pattern):
    """Scratch buffers and LDS hold a pattern before every hinted call (xch[0], which now carries a sum between flushes, is
    cleared by the kernel like the rest of the shared block)."""
    nbits, F, R, M, refs, refs_ncc = three_tiles
    ctx.debug_set_max_workgroups(1)
    try:
        check(ctx, F, R, M, nbits, HINT, refs, poison=pattern)
        check(ctx, F, R, None, nbits, HINT, refs_ncc, poison=pattern)
        check(ctx, F, R, M, nbits, DEEP, refs, poison=pattern)
    finally:
        ctx.debug_set_max_workgroups(0)
