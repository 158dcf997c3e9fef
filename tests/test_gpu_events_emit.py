"""GPU parity of the joint list emit of the event kernel's hinted instantiations below 1024 shifts (ev_emit_fr,
kernels_events.h): the forward and the reverse reads of a 64-bit word are listed in ONE walk over f | r, the running
reverse cursor is the rank of a forward entry, and a lane whose bit is in one list only stores the other entry to its dump
cell.  Every case against the CPU oracle at max_shift 1000 and 3 with the event kernel asserted, and bit for bit against the
same call under PMX_FLAG_FORCE_SPARSE (the instantiation that keeps one loop per list); with a track, NCC-only and with
the deep pool.  Geometry: a tile is 65536 bits, two rows of 32768; thread t of 256 holds bits [128 t, 128 t + 128) of each
row -- a quad, two 64-bit words --, wave w threads [64 w, 64 w + 64); wave 3 also lists the reverse reads above the tile."""
import numpy as np
import pytest

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_events_hinted import DEEP, HINT, SHIFTS, check
from .test_gpu_parity import EVENT_TILE

pytestmark = pytest.mark.gpu

T = EVENT_TILE
ROW = T // 2
QUAD = 128
SIZES = [(1, 0), (2, 1), (3, 127), (2, 128)]   # 65536 k + extra bits
SIZE_IDS = ["1t", "2t+1", "3t+127", "2t+128"]


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_max_workgroups(0)
    c.close()


def check_all(ctx, F, R, M, nbits, poison=None):
    """With a track, NCC-only and with the deep pool; one oracle run per shift range and track."""
    refs = {(S, L): oracle.calc_correlation(F, R, M, nbits, S, L) for S, L in SHIFTS}
    refs_ncc = {(S, L): oracle.calc_correlation(F, R, None, nbits, S, L) for S, L in SHIFTS}
    check(ctx, F, R, M, nbits, HINT, refs, poison)
    check(ctx, F, R, None, nbits, HINT, refs_ncc, poison)
    check(ctx, F, R, M, nbits, DEEP, refs, poison)


def background(seed, nbits, density=0.002):
    rng = np.random.default_rng(seed)
    F = synth.random_bits(rng, nbits, density, 0, nbits)
    R = synth.random_bits(rng, nbits, density, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    return F, R, M


def clear(words, lo, hi):
    """Bits [lo, hi) := 0 (lo, hi multiples of 64)."""
    words[lo >> 6:hi >> 6] = 0


def d0_positions(nbits):
    """Bits 0, 63, 64 and 127 of the quads of threads 0, 63, 64, 192 and 255 in both rows of every tile (with them the
    first and the last bit of a tile and both sides of its row boundary), as far as the vector reaches."""
    pos = []
    for tile in range((nbits + T - 1) // T):
        for q in (0, 1):
            for t in (0, 63, 64, 192, 255):
                base = tile * T + q * ROW + QUAD * t
                pos += [base, base + 63, base + 64, base + 127]
    assert all(x in pos for x in (0, T - 1, ROW - 1, ROW))
    return [p for p in pos if p < nbits]


@pytest.mark.parametrize("k,extra", SIZES, ids=SIZE_IDS)
def test_the_same_position_in_both_vectors(ctx, k, extra):
    """The d = 0 pair: the forward entry is written first and its rank is the index of that reverse read."""
    nbits = T * k + extra
    F, R, M = background(8100 + 10 * k + extra, nbits)
    for p in d0_positions(nbits) + [nbits - 1]:
        synth.set_bit(F, p)
        synth.set_bit(R, p)
    check_all(ctx, F, R, M, nbits)


@pytest.mark.parametrize("thread", [0, 63, 192], ids=["lane0", "lane63", "wave3_lane0"])
@pytest.mark.parametrize("k,extra", SIZES[1:], ids=SIZE_IDS[1:])
def test_one_word_full_in_both_vectors_between_empty_lanes(ctx, k, extra, thread):
    """128 entries from one lane (64 trips of the wave for it alone) while its neighbours hold nothing: the upper word of
    the quad in row 0 of tile 0, the lower word in row 1 of the last full tile."""
    nbits = T * k + extra
    F, R, M = background(8200 + 10 * k + extra + thread, nbits)
    for base, word in ((QUAD * thread, 1), ((k - 1) * T + ROW + QUAD * thread, 0)):
        lo, hi = max(0, base - 2 * QUAD), base + 3 * QUAD
        for w in (F, R):
            clear(w, lo, hi)
            w[(base >> 6) + word] = np.uint64(0xffffffffffffffff)
    check_all(ctx, F, R, M, nbits)


@pytest.mark.parametrize("k,extra", [SIZES[0], SIZES[2]], ids=[SIZE_IDS[0], SIZE_IDS[2]])
def test_words_with_one_vector_wholly_below_the_other(ctx, k, extra):
    """A word whose forward reads all lie below its reverse reads (every rank is the cursor's start; the reverse cursor
    moves only after the last forward entry), and the reverse; in both words of a quad, both rows, waves 0 and 3."""
    nbits = T * k + extra
    F, R, M = background(8300 + 10 * k + extra, nbits)
    low, high = np.uint64(0x00000000a5a50f01), np.uint64(0x8001f0a500000000)
    i = 0
    for tile in range(k):
        for q in (0, 1):
            for t in (1, 62, 193, 254):
                for word in (0, 1):
                    j = ((tile * T + q * ROW + QUAD * t) >> 6) + word
                    F[j], R[j] = (low, high) if i & 1 else (high, low)
                    i += 1
    check_all(ctx, F, R, M, nbits)


@pytest.mark.parametrize("which", ["forward_only", "reverse_only"])
@pytest.mark.parametrize("k,extra", [SIZES[1], SIZES[3]], ids=[SIZE_IDS[1], SIZE_IDS[3]])
def test_one_vector_empty(ctx, k, extra, which):
    """Every trip stores one entry to the dump cell."""
    nbits = T * k + extra
    F, R, M = background(8400 + 10 * k + extra, nbits, 0.005)
    (R if which == "forward_only" else F)[:] = 0
    check_all(ctx, F, R, M, nbits)


def test_reverse_reads_only_in_the_halo_above_the_tile(ctx):
    """Tile 0 holds forward reads, but its only reverse reads are the partners of its last forward reads, in the max_shift
    bits above it: the joint walk of tile 0 lists forward entries only, all with the rank 0, and wave 3 lists the halo."""
    nbits = 2 * T + 1
    rng = np.random.default_rng(8500)
    F = synth.random_bits(rng, nbits, 0.01, T - 3000, T)
    R = synth.random_bits(rng, nbits, 0.02, T, T + 1000)
    for p in (T - 1,):
        synth.set_bit(F, p)
    for p in (T, T + 999):
        synth.set_bit(R, p)
    M = synth.run_bits(rng, nbits, 300, 80, 1, nbits - 100)
    check_all(ctx, F, R, M, nbits)


@pytest.mark.parametrize("k,extra", [SIZES[2], SIZES[3]], ids=[SIZE_IDS[2], SIZE_IDS[3]])
def test_forward_reads_only_in_the_last_bits_of_a_tile(ctx, k, extra):
    """Forward reads in the last max_shift bits of every tile only (wave 3 of row 1), reverse reads everywhere."""
    nbits = T * k + extra
    rng = np.random.default_rng(8600 + 10 * k + extra)
    F = np.zeros(synth.nwords(nbits), dtype=np.uint64)
    for tile in range(1, k + 1):
        F |= synth.random_bits(rng, nbits, 0.02, tile * T - 1000, tile * T)
        synth.set_bit(F, tile * T - 1000)
        synth.set_bit(F, tile * T - 1)
    R = synth.random_bits(rng, nbits, 0.005, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    check_all(ctx, F, R, M, nbits)


@pytest.fixture(scope="module")
def three_tiles():
    """Tile 0: a full word in lane 63 and d = 0 pairs; tile 1: sparse; tile 2: forward reads only -- a cursor that ran on or
    a dump cell read back shows in the tile behind."""
    nbits = 3 * T
    F, R, M = background(8700, nbits, 0.005)
    for w in (F, R):
        clear(w, QUAD * 61, QUAD * 66)
        w[(QUAD * 63) >> 6] = np.uint64(0xffffffffffffffff)
    for p in d0_positions(T):
        synth.set_bit(F, p)
        synth.set_bit(R, p)
    clear(R, 2 * T, 3 * T)
    refs = {(S, L): oracle.calc_correlation(F, R, M, nbits, S, L) for S, L in SHIFTS}
    refs_ncc = {(S, L): oracle.calc_correlation(F, R, None, nbits, S, L) for S, L in SHIFTS}
    return nbits, F, R, M, refs, refs_ncc


@pytest.mark.parametrize("pattern", [0x00000000, 0xffffffff, 0x80808080, 0x7fffffff, 0x5a5a5a5a])
def test_one_workgroup_over_three_tiles_with_stale_memory(ctx, three_tiles, pattern):
    """Scratch buffers and LDS (the dump cells among them) hold a pattern before every hinted call."""
    nbits, F, R, M, refs, refs_ncc = three_tiles
    ctx.debug_set_max_workgroups(1)
    try:
        check(ctx, F, R, M, nbits, HINT, refs, poison=pattern)
        check(ctx, F, R, None, nbits, HINT, refs_ncc, poison=pattern)
        check(ctx, F, R, M, nbits, DEEP, refs, poison=pattern)
    finally:
        ctx.debug_set_max_workgroups(0)
