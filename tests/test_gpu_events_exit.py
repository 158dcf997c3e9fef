"""GPU parity of the cold path of a workgroup of the event kernel (kernels_events.h, max_shift <= 1023): the guarded fetch of
a boundary tile (tile 0 and the last tiles of a vector, every tile of a vector that is not 16-byte aligned, the first and the
last tile of a tile-range job) and the flush (all six rows of a segment finished on chip and written in one block of 16-byte
stores; a later flush of the same segment adds to it with atomics).  Every case runs at max_shift 1000 and 3, with a track,
NCC-only and with the deep pool, with the event kernel asserted; it is compared with the CPU oracle and, bit for bit, with
the same call under PMX_FLAG_WINDOW_ONLY -- the window kernels share none of that code -- and repeated under the five patterns of
pmx_debug_poison (every case ends in the flush, which builds rows where the lists lay).  On the device every vector
is surrounded by 0xff bytes, and the bits between its end and the end of its last dword are set: a load outside [0, nbits)
that is not masked shows.  Geometry: a tile is 65536 bits, its halo 64 dwords of M below and 36 above, max_shift bits of R
above."""
import numpy as np
import pytest
import torch

from oracle import model as oracle
from pymasc_amd import ffi
from . import synth
from .test_gpu_events_big import events_ran
from .test_gpu_events_claims import Geometry, tile_counts
from .test_gpu_parity import EVENT_TILE, check_block

pytestmark = pytest.mark.gpu

HINT, DEEP, WINDOW = ffi.PMX_FLAG_EVENTS_HINT, ffi.PMX_FLAG_DEEP_LISTS, ffi.PMX_FLAG_WINDOW_ONLY
VARIANTS = [(True, HINT), (False, HINT), (True, DEEP)]   # with a track, NCC-only, the deep pool
SHIFTS = [(1000, 36), (3, 36)]
# c - d in row 5 (c = read_len - 1, d = 0 .. max_shift): never positive, both signs, always positive
SHIFTS_ROW5 = [(1000, 1), (1000, 36), (1000, 1005), (3, 1), (3, 36), (3, 8)]
PATTERNS = [0x00000000, 0xffffffff, 0x80808080, 0x7fffffff, 0x5a5a5a5a]
POOL_SMALL, POOL_DEEP = 2416, 4328                      # kernels_events.h: EV_POOL_SMALL, EV_POOL_DEEP
FLUSH_BOUND = 32767                                      # listed forward reads since the last flush + pool beyond it: flush


@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_max_workgroups(0)
    c.debug_set_claim_mode(0)
    c.close()


class Case:
    """A chromosome: host vectors, oracle results per (track, max_shift, read_len), device copies per base offset."""

    def __init__(self, nbits, F, R, M):
        self.nbits, self.F, self.R, self.M = nbits, F, R, M
        self.refs, self.dev = {}, {}

    def ref(self, with_m, S, L):
        key = (with_m, S, L)
        if key not in self.refs:
            self.refs[key] = oracle.calc_correlation(self.F, self.R, self.M if with_m else None, self.nbits, S, L)
        return self.refs[key]

    def pointers(self, offset):
        """F, R, M on the device, each `offset` bytes behind an allocation's start, 0xff around it and in the last dword's tail."""
        if offset not in self.dev:
            dev = torch.device("cuda", 0)
            keep = []
            for w in (self.F, self.R, self.M):
                raw = np.full(w.nbytes + 32, 0xff, dtype=np.uint8)
                raw[offset:offset + w.nbytes] = w.view(np.uint8)
                tail = self.nbits & 31
                if tail:   # bits nbits .. end of the last dword (dword (nbits - 1) // 32) are not the vector's: set them
                    d = raw[offset + 4 * ((self.nbits - 1) // 32):][:4].view(np.uint32)
                    d[0] |= np.uint32((0xffffffff << tail) & 0xffffffff)
                t = torch.from_numpy(raw).to(dev)
                keep.append(t)
            self.dev[offset] = keep
        return [t.data_ptr() + offset for t in self.dev[offset]]


def run(ctx, cases, S, L, with_m, flags, offset=0, ranges=None):
    """One batched call; ranges: [(case index, first tile, tiles)] for pmx_cc_batch_ranges_dev."""
    dev = torch.device("cuda", 0)
    jobs = ranges if ranges is not None else [(i, None, None) for i in range(len(cases))]
    ptrs = [cases[i].pointers(offset) for i, _a, _n in jobs]
    outs = [torch.full((ffi.PMX_NROWS, S + 1), -1, dtype=torch.int64, device=dev) for _ in jobs]
    pF, pR, pM = ([p[k] for p in ptrs] for k in range(3))
    nb = [cases[i].nbits for i, _a, _n in jobs]
    torch.cuda.synchronize()
    if ranges is None:
        ctx.cc_batch_dev(pF, pR, pM if with_m else None, nb, S, L, flags, [o.data_ptr() for o in outs])
    else:
        ctx.cc_batch_ranges_dev(pF, pR, pM if with_m else None, nb, [a for _i, a, _n in jobs], [n for _i, _a, n in jobs], S, L,
                                flags, [o.data_ptr() for o in outs])
    ctx.sync()
    return [o.cpu().numpy().view(np.uint64) for o in outs]


def check(ctx, cases, shifts=SHIFTS, variants=VARIANTS, offset=0, geometries=((0, 0),), ranges=None, patterns=PATTERNS):
    """Every variant and shift range: the window kernels once, then the event kernel under every geometry and pattern."""
    for with_m, hint in variants:
        for S, L in shifts:
            # (pmx_cc_batch_ranges_dev refuses PMX_FLAG_WINDOW_ONLY: the shares are summed and compared with the whole chromosome)
            win = run(ctx, cases, S, L, with_m, WINDOW | (hint & DEEP), offset)
            for nwg, mode in geometries:
                for pattern in [None] + list(patterns):
                    def call():
                        if pattern is not None:
                            ctx.debug_poison(pattern)
                        return run(ctx, cases, S, L, with_m, hint, offset, ranges)
                    with Geometry(ctx, nwg, mode):
                        outs, ev, _win = events_ran(ctx, call)
                    assert ev == 1, "the event kernel must have run"
                    what = (with_m, hint, S, L, offset, nwg, mode, pattern)
                    if ranges is None:
                        for case, out in zip(cases, outs):
                            check_block(out, case.ref(with_m, S, L), S, with_m)
                        for out, w in zip(outs, win):
                            assert np.array_equal(out, w), ("differs from the window kernels", what)
                    else:   # the shares of a chromosome add up to it (one case)
                        total = sum(outs)
                        check_block(total, cases[0].ref(with_m, S, L), S, with_m)
                        assert np.array_equal(total[:ffi.PMX_ROW_SCALARS], win[0][:ffi.PMX_ROW_SCALARS]), ("differs from the window kernels", what)


# ---- the boundary fetch ------------------------------------------------------------------------------------------------

def boundary_case(seed, nbits, density=0.004):
    """Sparse vectors with reads, reverse reads and run edges on the first and the last bit of the vector and of its last
    whole dword, and a run of M that ends on the last bit."""
    rng = np.random.default_rng(seed)
    F = synth.random_bits(rng, nbits, density, 0, nbits)
    R = synth.random_bits(rng, nbits, density, 0, nbits)
    M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
    marks = {0, nbits - 1}
    if nbits >= 32:
        whole = nbits // 32 - 1                       # the last whole dword
        marks |= {32 * whole, 32 * whole + 31}
    for b in sorted(marks):
        synth.set_bit(F, b)
        synth.set_bit(R, b)
    # M: one-bit runs on the marks (an edge on the bit and one behind it), then a run that ends on the last bit
    Mb = np.unpackbits(M.view(np.uint8), bitorder="little")
    for b in sorted(marks):
        Mb[max(0, b - 1):b + 2] = 0
        Mb[b] = 1
    Mb[max(0, nbits - 41):nbits] = 1
    Mb[nbits:] = 0
    M = np.packbits(Mb, bitorder="little").view(np.uint64).copy()
    return Case(nbits, F, R, M)


EXTRAS = [0, 1, 31, 32, 33, 127, 128]


@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_vectors_that_end_around_a_dword_of_a_tile_boundary(ctx, k, extra):
    """65536 k + extra bits: the last tile holds 0 .. 128 bits (k = 0: the whole vector does), its last dword is whole, one bit
    short or one bit long.  A vector of no bits is refused."""
    nbits = EVENT_TILE * k + extra
    if nbits == 0:
        z = np.zeros(1, dtype=np.uint64)
        with pytest.raises(ffi.PmxError):
            ctx.calc_correlation(z, z, z, 0, 3, 36, HINT)
        return
    case = boundary_case(4000 + 10 * k + extra, nbits)
    check(ctx, [case], geometries=[(0, 0), (1, 0)])


@pytest.mark.parametrize("extra", [500, 999, 1000, 1001, 1151, 1152, 1153, 1300])
def test_the_vector_ends_inside_the_halo_of_the_tile_below(ctx, extra):
    """Two tiles + `extra` bits: tile 1 reads its halo above -- max_shift bits of R, 36 dwords (1152 bits) of M -- across the
    end of the vector, and the third tile is shorter than either halo."""
    nbits = 2 * EVENT_TILE + extra
    case = boundary_case(4400 + extra, nbits, 0.006)
    reads, _edges = tile_counts(case.F, case.R, case.M, nbits)
    assert reads[2] > 0 and nbits - 2 * EVENT_TILE <= 36 * 32 + 148
    check(ctx, [case], geometries=[(0, 0), (1, 0)])


@pytest.mark.parametrize("offset", [4, 8, 12])
@pytest.mark.parametrize("extra", EXTRAS)
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_vectors_that_are_not_16_byte_aligned(ctx, k, extra, offset):
    """The same vectors (the same seeds) from a base pointer 4, 8 and 12 bytes behind an aligned one: no tile is interior,
    every one of them takes the guarded fetch.  (The vector of no bits is refused whatever its base: see above.)"""
    nbits = EVENT_TILE * k + extra
    if nbits == 0:
        return
    case = boundary_case(4000 + 10 * k + extra, nbits)
    assert case.pointers(offset)[0] % 16 == offset
    check(ctx, [case], offset=offset, geometries=[(0, 0), (1, 0)])


@pytest.mark.parametrize("offset", [0, 8])
def test_tile_ranges_that_begin_and_end_at_the_first_and_the_last_tiles(ctx, offset):
    """pmx_cc_batch_ranges_dev: the jobs [0, 1), [1, 4), [4, 5), [5, 6) of a chromosome of six tiles begin and end at tile 0, at
    the last tile and at the one before it; every first and last tile of a job is fetched guarded.  The shares add up to the
    oracle's chromosome and to the window kernels' (which take whole chromosomes only)."""
    nbits = 6 * EVENT_TILE - 5
    case = boundary_case(4800, nbits)
    cuts = [0, 1, 4, 5, 6]
    ranges = [(0, a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]
    variants = [(with_m, hint & DEEP) for with_m, hint in VARIANTS]   # (the ranges call takes the event kernel without a hint)
    check(ctx, [case], offset=offset, geometries=[(0, 0), (2, 1)], ranges=ranges, variants=variants)
    whole = [(0, 0, 6)]
    check(ctx, [case], offset=offset, geometries=[(2, 0)], ranges=whole, variants=variants)


# ---- the flush -----------------------------------------------------------------------------------------------------------

def flushes_of_a_walk(F_per_tile, pool):
    """Flushes of one workgroup that walks these tiles (claim mode 2), the last one included: the rows are flushed when the
    listed forward reads since the last flush + the pool would pass the bound of a 16-bit cell, and when the job ends."""
    acc, n = 0, 0
    for i, f in enumerate(F_per_tile):
        acc += int(f)
        if i == len(F_per_tile) - 1 or acc + pool > FLUSH_BOUND:
            n, acc = n + 1, 0
    return n


def forward_reads_per_tile(case):
    b = np.unpackbits(case.F.view(np.uint8), bitorder="little")[:case.nbits]
    b = np.concatenate([b, np.zeros((-case.nbits) % EVENT_TILE, dtype=np.uint8)])
    return b.reshape(-1, EVENT_TILE).sum(axis=1)


@pytest.fixture(scope="module")
def deep_reads():
    """70 tiles at 1.5 % reads per strand (~980 listed forward reads a tile, ~2030 reads and edges: inside the small pool)."""
    clen = 70 * EVENT_TILE - 1136 - 36 - 1000 - 100
    nbits, F, R, M = synth.make_case(811, clen, 1000, 36, 0.015, 0.015, True, mean_on=2000, mean_off=500)
    case = Case(nbits, F, R, M)
    reads, edges = tile_counts(F, R, M, nbits)
    assert len(reads) == 70 and ((reads + edges) < POOL_SMALL).all(), "a tile of the fixture is dense"
    return case


@pytest.mark.parametrize("mode", [2, 0, 1])
@pytest.mark.parametrize("nwg", [1, 2])
def test_a_segment_is_flushed_two_and_three_times(ctx, deep_reads, nwg, mode):
    """One workgroup over 70 tiles flushes its segment three times, each of two workgroups twice: the second and the third
    flush add to what the first one stored."""
    per_tile = forward_reads_per_tile(deep_reads)
    share = len(per_tile) // nwg
    for w in range(nwg):
        n = flushes_of_a_walk(per_tile[w * share:(w + 1) * share], POOL_SMALL)
        assert n == (3 if nwg == 1 else 2), ("the fixture does not reach the add path", nwg, w, n)
        assert flushes_of_a_walk(per_tile[w * share:(w + 1) * share], POOL_DEEP) >= n
    check(ctx, [deep_reads], geometries=[(nwg, mode)])


@pytest.fixture(scope="module")
def three_jobs():
    """Jobs of one, one and four tiles: on two workgroups of three tiles workgroup 0 leaves two jobs after one tile each --
    two flushes in a row -- and ends inside the third, which workgroup 1 finishes."""
    cases = []
    for i, tiles in enumerate([1, 1, 4]):
        nbits = tiles * EVENT_TILE - 77 - 1000 * i
        rng = np.random.default_rng(830 + i)
        F = synth.random_bits(rng, nbits, 0.004, 0, nbits)
        R = synth.random_bits(rng, nbits, 0.004, 0, nbits)
        M = synth.run_bits(rng, nbits, 700, 250, 0, nbits)
        for w in (F, R, M):
            synth.set_bit(w, 0)
            synth.set_bit(w, nbits - 1)
        cases.append(Case(nbits, F, R, M))
    return cases


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_a_workgroup_flushes_twice_in_a_row(ctx, three_jobs, mode):
    """... at read lengths 1, 36 and max_shift + 5: the recurrence row is gathered through |c - d| with c - d never positive, of
    both signs and always positive (row 5 of the segment, the mappable length)."""
    assert [(-(-c.nbits // EVENT_TILE)) for c in three_jobs] == [1, 1, 4]
    check(ctx, three_jobs, shifts=SHIFTS_ROW5, geometries=[(2, mode), (1, mode)])
