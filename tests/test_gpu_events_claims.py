"""GPU parity of the claimed tiles of the event kernel's hinted instantiations (KNOWN_SPARSE, kernels_events.h: EvClaimer).
A workgroup's static range is cut into pieces, one per job; the first tile of a piece is its owner's, the others are drawn
from the piece's counter -- by the owner, and by workgroups of the same job that have run out of their own.  Who takes a tile
cannot change an integer: every case against the CPU oracle at max_shift 1000 and 3 with the event kernel asserted, and bit
for bit against the same call under PMX_FLAG_FORCE_SPARSE (the instantiation that walks its range), with a track, NCC-only
and with the deep pool, under the three claim modes (0: claims + helping, 1: odd workgroups draw through the helping path
only, 2: nobody helps; the NCC-only instantiation walks its range whatever the mode).  Geometry: a tile is 65536 bits."""
import numpy as np
import pytest
import torch

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_batch import run_batch
from .test_gpu_events_big import events_ran
from .test_gpu_parity import EVENT_TILE, check_block

pytestmark = pytest.mark.gpu

SHIFTS = [(1000, 36), (3, 36)]
HINT, DEEP, FORCE = ffi.PMX_FLAG_EVENTS_HINT, ffi.PMX_FLAG_DEEP_LISTS, ffi.PMX_FLAG_FORCE_SPARSE
VARIANTS = [(True, HINT), (False, HINT), (True, DEEP)]   # with a track, NCC-only, the deep pool
MODES = [0, 1, 2]
POOL_SMALL, POOL_DEEP, CAP_EDGES = 2416, 4328, 1536      # kernels_events.h: EV_POOL_SMALL, EV_POOL_DEEP, EV_CAPE_SMALL


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_max_workgroups(0)
    c.debug_set_claim_mode(0)
    c.close()


class Geometry:
    """Workgroup cap and claim mode for the calls inside; both back to their defaults afterwards."""

    def __init__(self, ctx, nwg, mode):
        self.ctx, self.nwg, self.mode = ctx, nwg, mode

    def __enter__(self):
        self.ctx.debug_set_max_workgroups(self.nwg)
        self.ctx.debug_set_claim_mode(self.mode)

    def __exit__(self, *exc):
        self.ctx.debug_set_max_workgroups(0)
        self.ctx.debug_set_claim_mode(0)


def sparse_vectors(seed, nbits, density=0.005):
    rng = np.random.default_rng(seed)
    F = synth.random_bits(rng, nbits, density, 0, nbits)
    R = synth.random_bits(rng, nbits, density, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    for w in (F, R, M):
        synth.set_bit(w, 0)
        synth.set_bit(w, nbits - 1)
    return F, R, M


def references(F, R, M, nbits, shifts=SHIFTS):
    return {(with_m, S): oracle.calc_correlation(F, R, M if with_m else None, nbits, S, L) for S, L in shifts for with_m in (True, False)}


def check_single(ctx, F, R, M, nbits, refs, geometries, shifts=SHIFTS, variants=VARIANTS, poison=None):
    """One chromosome under every variant and shift range: the walked instantiation once, then every (workgroups, mode)."""
    for with_m, hint in variants:
        Mv = M if with_m else None
        for S, L in shifts:
            old = ctx.calc_correlation(F, R, Mv, nbits, S, L, FORCE | (hint & DEEP))
            check_block(old, refs[(with_m, S)], S, with_m)
            for nwg, mode in geometries:
                def call():
                    if poison is not None:
                        ctx.debug_poison(poison)
                    return ctx.calc_correlation(F, R, Mv, nbits, S, L, hint)
                with Geometry(ctx, nwg, mode):
                    out, ev, _win = events_ran(ctx, call)
                assert ev == 1, "the event kernel must have run"
                assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
                check_block(out, refs[(with_m, S)], S, with_m)
                assert np.array_equal(out, old), ("differs from the walked instantiation", with_m, hint, S, nwg, mode)


@pytest.mark.parametrize("extra", [0, 1, 127, 128])
@pytest.mark.parametrize("k", [1, 2, 3, 8, 20])
def test_vectors_around_a_tile_boundary(ctx, k, extra):
    """k = 1: one piece of one tile, helpers find nothing; more tiles on two, three and five workgroups."""
    nbits = EVENT_TILE * k + extra
    F, R, M = sparse_vectors(9000 + 10 * k + extra, nbits)
    refs = references(F, R, M, nbits)
    check_single(ctx, F, R, M, nbits, refs, [(nwg, mode) for nwg in (2, 3, 5) for mode in MODES])


def _job(seed, tiles, short=77):
    nbits = tiles * EVENT_TILE - short
    return (nbits,) + sparse_vectors(seed, nbits, 0.004)


# (tiles per job, workgroups): ranges that straddle job boundaries, a helper whose job ends inside its own range, a job that
# lies wholly inside one range, a job of one tile
BATCHES = [([5, 1, 7], 3), ([5, 1, 7], 2), ([3, 9, 1, 4], 3), ([3, 9, 1, 4], 5), ([2, 1, 1, 6], 2)]


@pytest.fixture(scope="module", params=range(len(BATCHES)), ids=[f"{'_'.join(map(str, t))}_wg{w}" for t, w in BATCHES])
def batch(request):
    tiles, nwg = BATCHES[request.param]
    cases = [_job(300 + 10 * request.param + i, t, 77 + 1000 * i) for i, t in enumerate(tiles)]
    refs = [references(F, R, M, nbits) for nbits, F, R, M in cases]
    return cases, refs, nwg


@pytest.mark.parametrize("mode", MODES)
def test_jobs_of_unequal_length_in_one_launch(ctx, batch, mode):
    """In mode 1 every tile but the first of an odd workgroup's pieces goes through the helping path: were a tile of another
    job ever claimed, or a tile left, the rows of a job would differ from the oracle's for that job alone."""
    cases, refs, nwg = batch
    for with_m, hint in VARIANTS:
        for S, L in SHIFTS:
            olds = run_batch(ctx, cases, S, L, with_m, FORCE | (hint & DEEP))
            with Geometry(ctx, nwg, mode):
                outs, ev, _win = events_ran(ctx, lambda: run_batch(ctx, cases, S, L, with_m, hint))
            assert ev == 1, "the event kernel must have run"
            for (nbits, F, R, M), ref, out, old in zip(cases, refs, outs, olds):
                check_block(out, ref[(with_m, S)], S, with_m)
                assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
                assert np.array_equal(out, old)
                with Geometry(ctx, nwg, mode):
                    alone = ctx.calc_correlation(F, R, M if with_m else None, nbits, S, L, hint)
                assert np.array_equal(out, alone), "a job's rows in the batch differ from the job run alone"


@pytest.fixture(scope="module")
def many_pieces():
    """140 tiles: on 70 workgroups a job of 70 pieces with a tile to draw each -- the scan of the counters takes a second
    load of 64 and wraps round to its own piece."""
    nbits = 140 * EVENT_TILE - 9
    F, R, M = sparse_vectors(511, nbits, 0.003)
    return nbits, F, R, M, references(F, R, M, nbits)


@pytest.mark.parametrize("nwg", [70, 0], ids=["70_pieces_of_two", "a_piece_per_tile"])
def test_more_than_64_pieces_in_a_job(ctx, many_pieces, nwg):
    """(no cap: 140 workgroups of one tile each -- every piece is its owner's first tile and no counter is ever drawn from)"""
    nbits, F, R, M, refs = many_pieces
    check_single(ctx, F, R, M, nbits, refs, [(nwg, mode) for mode in MODES])


def check_batch(ctx, cases, refs, geometries):
    """A batch under every variant and shift range: the walked instantiation once, then every (workgroups, mode); every
    job against its oracle, with the path marker, and bit for bit against the walked instantiation."""
    for with_m, hint in VARIANTS:
        for S, L in SHIFTS:
            olds = run_batch(ctx, cases, S, L, with_m, FORCE | (hint & DEEP))
            for nwg, mode in geometries:
                with Geometry(ctx, nwg, mode):
                    outs, ev, _win = events_ran(ctx, lambda: run_batch(ctx, cases, S, L, with_m, hint))
                assert ev == 1, "the event kernel must have run"
                for ref, out, old in zip(refs, outs, olds):
                    check_block(out, ref[(with_m, S)], S, with_m)
                    assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
                    assert np.array_equal(out, old), ("differs from the walked instantiation", with_m, hint, S, nwg, mode)


def test_more_workgroups_than_tiles_in_a_job(ctx):
    """Jobs of 1, 2 and 3 tiles beside one of 70, no cap: every workgroup holds one tile, jobs end after one piece."""
    cases = [_job(600 + i, t) for i, t in enumerate([1, 70, 2, 3])]
    refs = [references(F, R, M, nbits) for nbits, F, R, M in cases]
    check_batch(ctx, cases, refs, [(0, mode) for mode in MODES])


NT = 20


def tile_counts(F, R, M, nbits):
    def bits(w):
        b = np.unpackbits(w.view(np.uint8), bitorder="little")[:nbits]
        return np.concatenate([b, np.zeros((-nbits) % EVENT_TILE, dtype=np.uint8)])
    nt = (nbits + EVENT_TILE - 1) // EVENT_TILE
    reads = (bits(F).astype(np.int64) + bits(R)).reshape(nt, EVENT_TILE).sum(axis=1)
    m = bits(M)
    edges = (m != np.concatenate([[0], m[:-1]])).astype(np.int64).reshape(nt, EVENT_TILE).sum(axis=1)
    return reads, edges


def dense_case(kind):
    """Twenty tiles, sparse at 0.4 % per strand on an ordinary track, + dense tiles: one read-dense tile first, in the middle,
    last; `helped`: tiles 11 and 15 -- on three workgroups of seven tiles they lie inside the odd workgroup's range (7..13) and
    the last one's, beyond their first tiles, so in mode 1 tile 11 is taken through the helping path; `edges`: an edge-dense one."""
    nbits = NT * EVENT_TILE
    rng = np.random.default_rng({"first": 34, "middle": 33, "last": 35, "helped": 36, "edges": 37}[kind])
    F = synth.random_bits(rng, nbits, 0.004, 0, nbits)
    R = synth.random_bits(rng, nbits, 0.004, 0, nbits)
    M = synth.run_bits(rng, nbits, 900, 300, 0, nbits)
    tiles = {"first": [0], "middle": [9], "last": [NT - 1], "helped": [11, 15], "edges": [12]}[kind]
    for t in tiles:
        lo, hi = t * EVENT_TILE, (t + 1) * EVENT_TILE
        if kind == "edges":    # runs of ~10 bits: ~6500 run edges per tile, beyond the 1536 of the list
            keep = synth.run_bits(np.random.default_rng(1), nbits, 10**9, 1, 0, lo) | synth.run_bits(np.random.default_rng(1), nbits, 10**9, 1, hi, nbits)
            M = (M & keep) | synth.run_bits(rng, nbits, 6, 4, lo, hi)
        else:                  # 4 % per strand: ~5200 reads per tile, beyond both pools
            F |= synth.random_bits(rng, nbits, 0.04, lo, hi)
            R |= synth.random_bits(rng, nbits, 0.04, lo, hi)
    reads, edges = tile_counts(F, R, M, nbits)
    over = (edges > CAP_EDGES) if kind == "edges" else (reads > POOL_DEEP)
    assert sorted(np.flatnonzero(over)) == list(tiles), (kind, reads, edges)
    assert ((reads + edges)[~over] < 1500).all(), (kind, reads, edges)
    return nbits, F, R, M, references(F, R, M, nbits), len(tiles)


@pytest.fixture(scope="module", params=["first", "middle", "last", "helped", "edges"])
def dense(request):
    return dense_case(request.param)


@pytest.mark.parametrize("nwg", [2, 3])
def test_dense_tiles_are_flagged_by_whoever_takes_them(ctx, dense, nwg):
    """The window kernels take exactly the flagged tiles and add their sums to the rows: a flag missed or set twice, or a
    wrong count of flagged tiles, shows against the oracle and against the walked instantiation."""
    nbits, F, R, M, refs, _n = dense
    check_single(ctx, F, R, M, nbits, refs, [(nwg, mode) for mode in MODES])


@pytest.mark.parametrize("nwg", [2, 3])
def test_flags_and_flagged_counts_equal_the_static_walk(ctx, dense, nwg):
    """The flag area after a call -- the flags of both window kernels, the counters of flagged tiles, the job statistics and
    the chromosome's scalar totals -- byte for byte what the static walk (mode 2) leaves; only the claim counters behind them
    may differ."""
    nbits, F, R, M, _refs, ndense = dense
    claim_bytes = (torch.cuda.get_device_properties(0).multi_processor_count * 8 + 32) * 4
    claim_bytes = (claim_bytes + 15) // 16 * 16
    for with_m, hint in VARIANTS:
        areas = {}
        for mode in (2, 0, 1):
            with Geometry(ctx, nwg, mode):
                ctx.calc_correlation(F, R, M if with_m else None, nbits, 1000, 36, hint)
            areas[mode] = ctx.debug_read_flag_area()
        walked = areas[2]
        assert walked.size > claim_bytes
        for mode in (0, 1):
            assert areas[mode].size == walked.size
            assert np.array_equal(areas[mode][:-claim_bytes], walked[:-claim_bytes]), (with_m, hint, nwg, mode)
        # ... and the static walk's are the fixture's dense tiles: two flags of the 32-Kbit window tiles per event tile (the array
        # is padded by two per job and rounded up to 16 bytes), then as many for the autocorrelation kernel, then the counters
        fb = ((nbits + EVENT_TILE // 2 - 1) // (EVENT_TILE // 2) + 2 + 15) // 16 * 16
        reads, edges = tile_counts(F, R, M, nbits)
        tiles = np.flatnonzero((reads > POOL_DEEP) | ((edges > CAP_EDGES) if with_m else False))
        assert len(tiles) == (ndense if with_m or (reads > POOL_DEEP).any() else 0)
        expect = np.zeros(fb, dtype=np.uint8)
        expect[2 * tiles] = 1
        expect[2 * tiles + 1] = 1
        assert np.array_equal(walked[:fb], expect)
        assert int(walked[2 * fb:2 * fb + 4].view(np.uint32)[0]) == len(tiles)


@pytest.mark.parametrize("mode", [0, 1])
def test_calls_back_to_back_find_cleared_counters(ctx, mode):
    """Two and three calls queued without a synchronisation: the claim counters live in the flag areas, which alternate, and a
    call's last launch clears the other one.  The second pair has a job table that grows beyond one launch (40 jobs: the
    second launch of that call clears the counters of the first)."""
    dev = torch.device("cuda", 0)
    small = [_job(700 + i, 2 + i) for i in range(3)]
    large = [synth.make_case(720 + i, 1800 + 9700 * (i % 9), 1000, 36, 0.01, 0.01, True) for i in range(40)]
    refs = {id(cases): [references(F, R, M, nbits) for nbits, F, R, M in cases] for cases in (small, large)}
    tens = {id(cases): [[torch.from_numpy(x.view(np.int64)).to(dev) for x in (F, R, M)] for _n, F, R, M in cases] for cases in (small, large)}

    for with_m, hint in VARIANTS:
        for S, L in SHIFTS:
            def queue(cases):   # a call's arguments, with result blocks of its own (every call's output is kept)
                outs = [torch.full((ffi.PMX_NROWS, S + 1), -1, dtype=torch.int64, device=dev) for _ in cases]
                t = tens[id(cases)]
                return ([x[0].data_ptr() for x in t], [x[1].data_ptr() for x in t], [x[2].data_ptr() for x in t] if with_m else None,
                        [c[0] for c in cases], S, L, hint, [o.data_ptr() for o in outs]), outs

            calls = [(small, queue(small)), (small, queue(small)), (large, queue(large)), (small, queue(small))]
            olds = {id(cases): run_batch(ctx, cases, S, L, with_m, FORCE | (hint & DEEP)) for cases in (small, large)}
            ctx.debug_poison(0xffffffff)
            torch.cuda.synchronize()
            with Geometry(ctx, 3, mode):
                for _cases, (args, _outs) in calls:   # (no sync in between: the areas alternate; the large table takes two launches)
                    ctx.cc_batch_dev(*args)
                ctx.sync()
            for cases, (_args, outs) in calls:
                for ref, o, old in zip(refs[id(cases)], outs, olds[id(cases)]):
                    out = o.cpu().numpy().view(np.uint64)
                    check_block(out, ref[(with_m, S)], S, with_m)
                    assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
                    assert np.array_equal(out, old), "differs from the walked instantiation"


@pytest.fixture(scope="module")
def ranged():
    nbits = 11 * EVENT_TILE - 5
    F, R, M = sparse_vectors(51, nbits, 0.004)
    return nbits, F, R, M, references(F, R, M, nbits)


@pytest.mark.parametrize("nwg", [2, 3])
@pytest.mark.parametrize("with_m,hint", VARIANTS, ids=["track", "ncc", "deep"])
def test_tile_ranges_cut_inside_a_chromosome(ctx, ranged, with_m, hint, nwg):
    """pmx_cc_batch_ranges_dev, mode 1: the jobs are ranges [0, 4), [4, 5), [5, 11) of one chromosome; their shares add up to it
    and equal the shares of the walked instantiation one by one."""
    nbits, F, R, M, refs = ranged
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x.view(np.int64)).to(dev) for x in (F, R, M)]
    cuts = [0, 4, 5, 11]
    n = len(cuts) - 1

    def shares(S, L, flags):
        outs = [torch.full((ffi.PMX_NROWS, S + 1), -1, dtype=torch.int64, device=dev) for _ in range(n)]
        torch.cuda.synchronize()
        ctx.cc_batch_ranges_dev([t[0].data_ptr()] * n, [t[1].data_ptr()] * n, [t[2].data_ptr()] * n if with_m else None, [nbits] * n,
                                cuts[:-1], [b - a for a, b in zip(cuts[:-1], cuts[1:])], S, L, flags, [o.data_ptr() for o in outs])
        ctx.sync()
        return [o.cpu().numpy().view(np.uint64) for o in outs]

    for S, L in SHIFTS:
        olds = shares(S, L, FORCE | (hint & DEEP))
        for mode in (1, 0):
            with Geometry(ctx, nwg, mode):
                outs, ev, _win = events_ran(ctx, lambda: shares(S, L, hint & DEEP))
            assert ev == 1, "the event kernel must have run"
            total = sum(outs)
            check_block(total, refs[(with_m, S)], S, with_m)
            assert int(total[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
            for out, old in zip(outs, olds):
                assert np.array_equal(out, old), "differs from the walked instantiation"


@pytest.fixture(scope="module")
def stale():
    out = []
    for tiles in (3, 20):
        nbits = tiles * EVENT_TILE
        F, R, M = sparse_vectors(71 + tiles, nbits)
        out.append((nbits, F, R, M, references(F, R, M, nbits)))
    return out


@pytest.mark.parametrize("pattern", [0x00000000, 0xffffffff, 0x80808080, 0x7fffffff, 0x5a5a5a5a])
def test_stale_memory_under_the_helping_path(ctx, stale, pattern):
    """Scratch buffers (the flag areas with the claim counters among them) and LDS hold a pattern before every hinted call:
    three tiles on one workgroup, twenty on three, mode 1."""
    for (nbits, F, R, M, refs), nwg in zip(stale, (1, 3)):
        check_single(ctx, F, R, M, nbits, refs, [(nwg, 1)], poison=pattern)


@pytest.mark.parametrize("mode", [1, 0])
def test_a_flush_inside_a_helper(ctx, flush_case, mode):
    """Two workgroups over ~107 tiles of ~720 listed forward reads each: the packed histogram cells are flushed when the
    listed forward reads since the last flush + EV_POOL_SMALL would pass 32767, after ~42 tiles -- in mode 1 workgroup 1
    reaches that bound on tiles it has drawn through the helping path.  The DEEP instantiation flushes when they + EV_POOL_DEEP
    would pass it, a few tiles earlier; the tiles (~1500 reads and edges) fit the lists of both pools."""
    nbits, F, R, M, refs, nwg = flush_case
    check_single(ctx, F, R, M, nbits, refs, [(nwg, mode)])


@pytest.fixture(scope="module")
def flush_case():
    clen, dens, nwg = 7_000_000, 0.011, 2
    nbits, F, R, M = synth.make_case(302, clen, 1000, 36, dens, dens, True, mean_on=2000, mean_off=500)
    ntiles = (nbits + EVENT_TILE - 1) // EVENT_TILE
    per_tile = int(oracle.lib().pmo_count(oracle._p(F), F.size)) / ntiles
    for pool in (POOL_SMALL, POOL_DEEP):   # bound of the default and of the DEEP instantiation
        assert (ntiles // nwg - 1) * per_tile + pool > 32767, "the fixture does not reach the flush bound"
    reads, edges = tile_counts(F, R, M, nbits)
    assert ((reads + edges) < POOL_SMALL).all(), "a tile of the fixture is dense"
    return nbits, F, R, M, references(F, R, M, nbits), nwg
