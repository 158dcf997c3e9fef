"""GPU parity of the event kernel's per-tile bookkeeping below 1024 shifts: the cross-wave list offsets (one load of the
20 scan totals + sums inside quads of lanes) and the loop-free listing of run edges (two per 128-bit quad, a loop only for
quads with more), against the CPU oracle, bit-exact.  Geometry (kernels_events.h): a tile is 65536 bits, two rows of
32768; thread t of 256 holds bits [128 t, 128 t + 128) of each row -- a "quad" --, so wave w holds [8192 w, 8192 w + 8192)
of each row; 2048 bits of M are staged below a tile, 1152 above it, and the reverse reads of max_shift bits above it."""
import numpy as np
import pytest

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_events_big import events_ran
from .test_gpu_parity import EVENT_TILE, check_block

pytestmark = pytest.mark.gpu

ROW = EVENT_TILE // 2
WAVE_BITS = ROW // 4
QUAD = 128
SHIFTS = [(1000, 36), (3, 36)]


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_max_workgroups(0)
    c.close()


def check(ctx, F, R, M, nbits, flags=0):
    """Both shift ranges on the event kernel, each against the oracle."""
    for S, L in SHIFTS:
        ref = oracle.calc_correlation(F, R, M, nbits, S, L)

        out, ev, _win = events_ran(ctx, lambda: ctx.calc_correlation(F, R, M, nbits, S, L, ffi.PMX_FLAG_FORCE_SPARSE | flags))
        check_block(out, ref, S, M is not None)
        assert ev == 1, "the event kernel must have run"


def pack(bits):
    pad = (-bits.size) % 64
    return np.packbits(np.concatenate([bits, np.zeros(pad, dtype=np.uint8)]), bitorder="little").view(np.uint64).copy()


def track_from_edges(nbits, edges):
    """M with M[i] != M[i - 1] exactly at the positions `edges` (M[-1] = 0)."""
    e = np.zeros(nbits, dtype=np.uint8)
    e[np.asarray(sorted(edges), dtype=np.int64)] = 1
    return pack((np.cumsum(e, dtype=np.int64) & 1).astype(np.uint8))


def concentrated(seed, nbits, tile, wave, rows):
    """F, R and M with every bit (and every run edge) of the vector inside wave `wave`'s bits of tile `tile`, rows `rows`."""
    rng = np.random.default_rng(seed)
    F = np.zeros(synth.nwords(nbits), dtype=np.uint64)
    R = np.zeros(synth.nwords(nbits), dtype=np.uint64)
    M = np.zeros(synth.nwords(nbits), dtype=np.uint64)
    for q in rows:
        lo = tile * EVENT_TILE + q * ROW + wave * WAVE_BITS
        hi = lo + WAVE_BITS
        F |= synth.random_bits(rng, nbits, 0.01, lo, hi)
        R |= synth.random_bits(rng, nbits, 0.01, lo, hi)
        M |= synth.run_bits(rng, nbits, 150, 60, lo, hi - 1)   # (a run cut at hi - 1 falls at hi - 1: still this wave's bit)
        for w in (F, R, M):
            synth.set_bit(w, lo)        # first and last bit of the wave: the first edge sits in the wave's lane 0, and
        synth.set_bit(F, hi - 1)        # the bit below it belongs to the wave below (or to the row / tile below)
        synth.set_bit(R, hi - 1)
    return F, R, M


@pytest.mark.parametrize("rows", [(0, 1), (0,), (1,)], ids=["both_rows", "row0", "row1"])
@pytest.mark.parametrize("wave", [0, 1, 2, 3])
def test_all_counts_of_a_tile_in_one_wave(ctx, wave, rows):
    """The bases of a wave are 0 for the waves up to the one that holds everything and the row's total above it; a row
    without bits leaves its 16-bit half of every packed count zero.  With a track, without one (the NCC-only
    instantiation reads three of the five fields) and with the deep pool."""
    nbits = 3 * EVENT_TILE
    F, R, M = concentrated(100 + 4 * len(rows) + wave + 16 * rows[0], nbits, 1, wave, rows)
    check(ctx, F, R, M, nbits)
    check(ctx, F, R, None, nbits)
    check(ctx, F, R, M, nbits, ffi.PMX_FLAG_DEEP_LISTS)


def _holes(bits, lo, hi, rng):
    p = lo
    while True:
        p += int(rng.integers(20, 120))
        q = p + int(rng.integers(1, 60))
        if q >= hi:
            return
        bits[p:q] = 0
        p = q


def test_reverse_reads_only_in_the_halo_above_the_tile(ctx):
    """Tile 0 holds forward reads but its only reverse reads are the partners in the max_shift bits above it."""
    nbits = 2 * EVENT_TILE
    rng = np.random.default_rng(11)
    F = synth.random_bits(rng, nbits, 0.01, EVENT_TILE - 3000, EVENT_TILE)
    R = synth.random_bits(rng, nbits, 0.02, EVENT_TILE, EVENT_TILE + 1000)
    synth.set_bit(R, EVENT_TILE)
    synth.set_bit(R, EVENT_TILE + 999)
    M = synth.run_bits(rng, nbits, 300, 80, 1, nbits - 100)
    check(ctx, F, R, M, nbits)
    check(ctx, F, R, None, nbits)


@pytest.mark.parametrize("where", ["below", "above"])
def test_run_edges_only_in_a_halo_of_the_tile(ctx, where):
    """Tile 1 is mappable throughout; the only run edges staged for it lie in the 2048 bits below it / the 1152 above."""
    nbits = 3 * EVENT_TILE
    rng = np.random.default_rng(12 if where == "below" else 13)
    F = synth.random_bits(rng, nbits, 0.004, 1, nbits - 1200)
    R = synth.random_bits(rng, nbits, 0.004, 1, nbits - 1200)
    bits = np.zeros(nbits, dtype=np.uint8)
    bits[EVENT_TILE - 3000:2 * EVENT_TILE + 3000] = 1
    if where == "below":
        _holes(bits, EVENT_TILE - 2048, EVENT_TILE - 1, rng)
        bits[EVENT_TILE - 2048] = 0   # the first staged bit is an edge
    else:
        _holes(bits, 2 * EVENT_TILE, 2 * EVENT_TILE + 1152, rng)
        bits[2 * EVENT_TILE + 1151] = 0   # the last staged bit
    check(ctx, F, R, pack(bits), nbits)


# edge positions inside a quad: none / one / two / three (the loop-free path lists the lowest and the highest, so the pairs
# straddle every dword boundary and touch both ends of the quad) / all 128 (the track alternates 0101...)
QUAD_PATTERNS = [(), (0,), (127,), (37,), (0, 127), (5, 6), (31, 32), (63, 64), (95, 96), (0, 64, 127), (1, 2, 3), (30, 33, 97),
                 tuple(range(QUAD))]


def _quad_edges(first_quad_bit, stride_quads, patterns):
    """`patterns` on every `stride_quads`-th quad from `first_quad_bit` on (the quads between them stay empty)."""
    out = []
    for i, pat in enumerate(patterns):
        out += [first_quad_bit + i * stride_quads * QUAD + b for b in pat]
    return out


@pytest.mark.parametrize("flags", [0, ffi.PMX_FLAG_DEEP_LISTS], ids=["pool", "deep"])
def test_quads_with_0_1_2_3_and_128_edges(ctx, flags):
    """Every pattern next to empty quads, in both rows of tile 1 (spread over its four waves, so that waves with and without a
    quad of more than two edges list side by side) and in both of its halos (14 of the 16 quads below, all 9 above)."""
    nbits = 3 * EVENT_TILE + 4000
    rng = np.random.default_rng(14)
    F = synth.random_bits(rng, nbits, 0.003, 1, nbits - 1200)
    R = synth.random_bits(rng, nbits, 0.003, 1, nbits - 1200)
    edges = []
    for q in (0, 1):
        row0 = EVENT_TILE + q * ROW
        for w in range(4):   # four patterns per wave, rotated by row; the 128-edge quad in wave 3 (row 0) / wave 2 (row 1)
            pats = [QUAD_PATTERNS[(4 * w + k + 3 * q) % len(QUAD_PATTERNS)] for k in range(4)]
            edges += _quad_edges(row0 + w * WAVE_BITS + 5 * QUAD, 2, pats)
        edges += _quad_edges(row0 + 2 * WAVE_BITS + 30 * QUAD, 2, QUAD_PATTERNS)   # and all of them in ONE wave
    edges += _quad_edges(EVENT_TILE - 2048 + QUAD, 2, [(0, 127), (1, 2, 3), (64,), tuple(range(QUAD)), (31, 32), (127,), (0,)])
    edges += _quad_edges(2 * EVENT_TILE, 2, [(0,), tuple(range(QUAD)), (63, 64), (0, 64, 127), (127,)])
    edges += _quad_edges(2 * EVENT_TILE + QUAD, 2, [(5, 6), (), (37,), (1, 2, 3)])   # (the odd quads above the tile)
    assert len(set(edges)) == len(edges)
    M = track_from_edges(nbits, edges)
    check(ctx, F, R, M, nbits, flags)


def test_more_than_two_edges_in_a_halo_quad_only(ctx):
    """The loop takes over for a WAVE: here only the waves that hold the halo quads (1: below, 2: above) meet a quad of more
    than two edges, and their own quads of the tile hold at most two."""
    nbits = 3 * EVENT_TILE
    rng = np.random.default_rng(15)
    F = synth.random_bits(rng, nbits, 0.003, 1, nbits - 1200)
    R = synth.random_bits(rng, nbits, 0.003, 1, nbits - 1200)
    edges = _quad_edges(EVENT_TILE - 2048 + 3 * QUAD, 1, [(7, 8, 9, 100)])
    edges += _quad_edges(2 * EVENT_TILE + 2 * QUAD, 1, [(0, 1, 2)])
    edges += _quad_edges(EVENT_TILE + 3 * QUAD, 3, [(0, 127), (64,), (31, 32)] * 20)
    M = track_from_edges(nbits, edges)
    check(ctx, F, R, M, nbits)


@pytest.mark.parametrize("extra", [0, 1, 127, 128])
@pytest.mark.parametrize("k", [1, 3])
def test_vector_lengths_around_a_tile_boundary(ctx, k, extra):
    nbits = EVENT_TILE * k + extra
    rng = np.random.default_rng(1000 * k + extra)
    F = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    R = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    for w in (F, R, M):
        synth.set_bit(w, 0)
        synth.set_bit(w, nbits - 1)
    check(ctx, F, R, M, nbits)
    check(ctx, F, R, None, nbits)


@pytest.fixture(scope="module")
def three_tiles():
    """An ordinary tile, a tile with everything in wave 2 (the other waves' totals are zero right after a tile that left
    theirs non-zero in LDS), an ordinary tile; + the references, computed once for all patterns."""
    nbits = 3 * EVENT_TILE
    rng = np.random.default_rng(16)
    F, R, M = concentrated(17, nbits, 1, 2, (0, 1))
    for t in (0, 2):
        lo, hi = t * EVENT_TILE + 1, (t + 1) * EVENT_TILE - 1
        F |= synth.random_bits(rng, nbits, 0.005, lo, hi)
        R |= synth.random_bits(rng, nbits, 0.005, lo, hi)
        M |= synth.run_bits(rng, nbits, 700, 250, lo, hi - 1)
    refs = {(S, L): oracle.calc_correlation(F, R, M, nbits, S, L) for S, L in SHIFTS}
    return nbits, F, R, M, refs


@pytest.mark.parametrize("pattern", [0x00000000, 0xffffffff, 0x80808080, 0x7fffffff, 0x5a5a5a5a])
def test_one_workgroup_over_three_tiles_with_stale_memory(ctx, three_tiles, pattern):
    """One workgroup takes the three tiles in turn; scratch buffers and LDS hold a pattern before the call (the lanes beyond the
    20 scan totals load whatever lies behind them, and the dump slots of the edge listing are never read)."""
    nbits, F, R, M, refs = three_tiles
    ctx.debug_set_max_workgroups(1)
    try:
        for S, L in SHIFTS:
            def call():
                ctx.debug_poison(pattern)
                return ctx.calc_correlation(F, R, M, nbits, S, L, ffi.PMX_FLAG_FORCE_SPARSE)

            out, ev, _win = events_ran(ctx, call)
            check_block(out, refs[(S, L)], S, True)
            assert ev == 1
    finally:
        ctx.debug_set_max_workgroups(0)
