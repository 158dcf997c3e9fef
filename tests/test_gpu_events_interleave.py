"""The interleaved tile ranges of the claiming event kernel (kernels_events.h: ev_wg_virtual).  Block b of a
launch owns range v(b): the device is filled in layers of `width` blocks in launch order, and the positions' ranges lie side by
side, so that neighbouring ranges come from different layers.  Which block owns a range cannot change an integer: the map
against a restatement, and every case of the claims tests' kind three ways -- against the CPU oracle at max_shift 1000 and 3
with the event kernel asserted, bit for bit against the same call at width 1 (ranges in launch order), and bit for bit against
the same call under PMX_FLAG_FORCE_SPARSE -- with a track, NCC-only (it walks its ranges in launch order whatever the width)
and with the deep pool, under the three claim modes."""
import numpy as np
import pytest
import torch

from pymasc_amd import ffi
from .test_gpu_batch import run_batch
from .test_gpu_events_big import events_ran
from .test_gpu_events_claims import _job, dense_case, references, sparse_vectors
from .test_gpu_parity import EVENT_TILE, check_block

SHIFTS = [(1000, 36), (3, 36)]
HINT, DEEP, FORCE = ffi.PMX_FLAG_EVENTS_HINT, ffi.PMX_FLAG_DEEP_LISTS, ffi.PMX_FLAG_FORCE_SPARSE
VARIANTS = [(True, HINT), (False, HINT), (True, DEEP)]   # with a track, NCC-only, the deep pool
MODES = [0, 1, 2]
gpu = pytest.mark.gpu


# ---- the map (host only) ----------------------------------------------------------------------------------------------

def wg_order(nwg, width):
    """The issue's statement of the map, vectorised: layer = b // C, pos = b % C, nl layers of which the last holds r blocks."""
    b = np.arange(nwg, dtype=np.int64)
    nl = -(-nwg // width)
    r = nwg - (nl - 1) * width
    layer, pos = b // width, b % width
    return np.where(pos < r, pos * nl + layer, r * nl + (pos - r) * (nl - 1) + layer)


@pytest.mark.parametrize("nwg,width", [(n, w) for n in range(1, 65) for w in range(1, 10)] +
                         [(1274, 256), (1280, 256), (1024, 256), (250, 256)])
def test_the_map_is_a_permutation(nwg, width):
    got = ffi.wg_order(nwg, width).astype(np.int64)
    want = wg_order(nwg, width)
    assert np.array_equal(got, want)
    for m in (got, want):
        assert np.array_equal(np.sort(m), np.arange(nwg))
    if width == 1 or nwg <= width:
        assert np.array_equal(got, np.arange(nwg))


def test_neighbouring_ranges_come_from_different_layers():
    """1274 workgroups on 256 compute units: five layers, the last of 250; any five ranges in a row hold at least four layers."""
    nwg, width = 1274, 256
    layer_of_range = np.empty(nwg, dtype=np.int64)
    layer_of_range[ffi.wg_order(nwg, width).astype(np.int64)] = np.arange(nwg) // width
    for v in range(nwg - 4):
        assert len(set(layer_of_range[v:v + 5])) >= 4


# ---- parity -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    c = ffi.Context(0)
    yield c
    c.set_profiling(False)
    c.debug_set_max_workgroups(0)
    c.debug_set_claim_mode(0)
    c.debug_set_wg_layer(0)
    c.close()


class Geometry:
    """Workgroup cap, claim mode and layer width for the calls inside; all back to their defaults afterwards."""

    def __init__(self, ctx, nwg, mode, width):
        self.ctx, self.nwg, self.mode, self.width = ctx, nwg, mode, width

    def __enter__(self):
        self.ctx.debug_set_max_workgroups(self.nwg)
        self.ctx.debug_set_claim_mode(self.mode)
        self.ctx.debug_set_wg_layer(self.width)

    def __exit__(self, *exc):
        self.ctx.debug_set_max_workgroups(0)
        self.ctx.debug_set_claim_mode(0)
        self.ctx.debug_set_wg_layer(0)


def three_ways(ctx, call, olds, oracle_check, nwg, mode, widths, what):
    """call() -> a list of result blocks.  At every width: the event kernel ran, the oracle, width 1, the walked instantiation."""
    with Geometry(ctx, nwg, mode, 1):
        base = call()
    for width in widths:
        with Geometry(ctx, nwg, mode, width):
            outs, ev, _win = events_ran(ctx, call)
        assert ev == 1, "the event kernel must have run"
        oracle_check(outs)
        for out, b, old in zip(outs, base, olds):
            assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
            assert np.array_equal(out, b), ("differs from width 1", what, nwg, mode, width)
            assert np.array_equal(out, old), ("differs from the walked instantiation", what, nwg, mode, width)


def check_single(ctx, F, R, M, nbits, refs, geometries, poison=None, modes=MODES):
    """One chromosome; geometries: (workgroups, widths)."""
    for with_m, hint in VARIANTS:
        Mv = M if with_m else None
        for S, L in SHIFTS:
            old = ctx.calc_correlation(F, R, Mv, nbits, S, L, FORCE | (hint & DEEP))

            def call():
                if poison is not None:
                    ctx.debug_poison(poison)
                return [ctx.calc_correlation(F, R, Mv, nbits, S, L, hint)]
            for nwg, widths in geometries:
                for mode in modes:
                    three_ways(ctx, call, [old], lambda outs: check_block(outs[0], refs[(with_m, S)], S, with_m), nwg, mode, widths,
                               (with_m, hint, S))


@gpu
@pytest.mark.parametrize("extra", [0, 1, 127, 128])
@pytest.mark.parametrize("k", [3, 8, 20])
def test_vectors_around_a_tile_boundary(ctx, k, extra):
    """Widths 2, 3 and the grid size on 2, 3, 5 and 7 workgroups: the partial last layers 5 / 2 and 7 / 3, and the identity."""
    nbits = EVENT_TILE * k + extra
    F, R, M = sparse_vectors(9100 + 10 * k + extra, nbits)
    refs = references(F, R, M, nbits)
    check_single(ctx, F, R, M, nbits, refs, [(nwg, (2, 3, nwg)) for nwg in (2, 3, 5, 7)])


BATCHES = [[5, 1, 7], [3, 9, 1, 4], [2, 1, 1, 6]]


@pytest.fixture(scope="module", params=range(len(BATCHES)), ids=["_".join(map(str, t)) for t in BATCHES])
def batch(request):
    tiles = BATCHES[request.param]
    cases = [_job(1300 + 10 * request.param + i, t, 77 + 1000 * i) for i, t in enumerate(tiles)]
    refs = [references(F, R, M, nbits) for nbits, F, R, M in cases]
    return cases, refs


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_jobs_of_unequal_length_in_one_launch(ctx, batch, mode):
    """Ranges that straddle jobs, a job inside one range, a job of one tile, on 2, 3 and 5 workgroups at widths 2 and 3; every job
    of the batch also equals the job run alone."""
    cases, refs = batch
    for with_m, hint in VARIANTS:
        for S, L in SHIFTS:
            olds = run_batch(ctx, cases, S, L, with_m, FORCE | (hint & DEEP))

            def oracle_check(outs):
                for ref, out in zip(refs, outs):
                    check_block(out, ref[(with_m, S)], S, with_m)
            for nwg in (2, 3, 5):
                three_ways(ctx, lambda: run_batch(ctx, cases, S, L, with_m, hint), olds, oracle_check, nwg, mode, (2, 3), (with_m, hint, S))
                for width in (2, 3):
                    for (nbits, F, R, M), old in zip(cases, olds):
                        with Geometry(ctx, nwg, mode, width):
                            alone = ctx.calc_correlation(F, R, M if with_m else None, nbits, S, L, hint)
                        assert np.array_equal(alone, old), "a job run alone differs from its rows in the batch"


@pytest.fixture(scope="module", params=["first", "middle", "last"])
def dense(request):
    return dense_case(request.param)


@gpu
def test_a_dense_tile_and_the_flag_area(ctx, dense):
    """One dense tile first, in the middle and last among twenty on five workgroups at width 2.  The flag area -- the flags of both
    window kernels, the counters of flagged tiles, the job statistics, the chromosome's totals and the claim counters -- is byte
    for byte that of width 1.  The claim counters, the area's last (compute units x 8 + 32) words, are compared under the
    static walk (mode 2) only: where workgroups help, a counter also counts the draws that came too late, and those depend on
    who was faster -- two calls at the SAME width may differ there (tests/test_gpu_events_claims.py compares the modes likewise)."""
    nbits, F, R, M, refs, _n = dense
    check_single(ctx, F, R, M, nbits, refs, [(5, (2,))])
    claim_bytes = (torch.cuda.get_device_properties(0).multi_processor_count * 8 + 32) * 4
    claim_bytes = (claim_bytes + 15) // 16 * 16
    for with_m, hint in VARIANTS:
        for mode in MODES:
            areas = {}
            for width in (1, 2):
                with Geometry(ctx, 5, mode, width):
                    ctx.calc_correlation(F, R, M if with_m else None, nbits, 1000, 36, hint)
                areas[width] = ctx.debug_read_flag_area()
            assert areas[1].size == areas[2].size > claim_bytes
            keep = areas[1].size if mode == 2 else areas[1].size - claim_bytes
            assert np.array_equal(areas[2][:keep], areas[1][:keep]), (with_m, hint, mode)


@pytest.fixture(scope="module")
def flush_case():
    """70 tiles at 1.5 % per strand: ~980 listed forward reads per tile, and the packed histogram cells are flushed when the
    listed forward reads since the last flush + the pool would pass 32767 -- after ~30 tiles."""
    nbits = 70 * EVENT_TILE - 3
    F, R, M = sparse_vectors(1402, nbits, 0.015)
    return nbits, F, R, M, references(F, R, M, nbits)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_a_segment_flushed_more_than_once(ctx, flush_case, mode):
    """Two workgroups at width 2 (a helper -- in mode 1 the odd workgroup, for every tile but its first -- flushes its segment
    more than once); three workgroups at width 2 on top: there the map is no identity."""
    nbits, F, R, M, refs = flush_case
    check_single(ctx, F, R, M, nbits, refs, [(2, (2,)), (3, (2,))], modes=[mode])


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_calls_back_to_back_at_two_widths(ctx, mode):
    """Four calls queued without a synchronisation, at widths 2 and 1 in turn: the width is an argument of each launch."""
    dev = torch.device("cuda", 0)
    cases = [_job(1500 + i, 2 + 3 * i) for i in range(3)]   # 2, 5 and 8 tiles
    refs = [references(F, R, M, nbits) for nbits, F, R, M in cases]
    tens = [[torch.from_numpy(x.view(np.int64)).to(dev) for x in (F, R, M)] for _n, F, R, M in cases]
    for with_m, hint in VARIANTS:
        for S, L in SHIFTS:
            olds = run_batch(ctx, cases, S, L, with_m, FORCE | (hint & DEEP))
            calls = []
            for _ in range(4):
                outs = [torch.full((ffi.PMX_NROWS, S + 1), -1, dtype=torch.int64, device=dev) for _ in cases]
                calls.append((([x[0].data_ptr() for x in tens], [x[1].data_ptr() for x in tens], [x[2].data_ptr() for x in tens] if with_m else None,
                               [c[0] for c in cases], S, L, hint, [o.data_ptr() for o in outs]), outs))
            torch.cuda.synchronize()
            ctx.set_profiling(2)
            ctx.reset_kernel_times()
            with Geometry(ctx, 3, mode, 2):
                for i, (args, _outs) in enumerate(calls):
                    ctx.debug_set_wg_layer(2 if i % 2 == 0 else 1)
                    ctx.cc_batch_dev(*args)
                ctx.sync()
            ev = ctx.kernel_time(ffi.PMX_KERNEL_CC_EVENTS)[1]
            ctx.set_profiling(False)
            assert ev == len(calls), "the event kernel must have run in every call"
            for _args, outs in calls:
                for ref, o, old in zip(refs, outs, olds):
                    out = o.cpu().numpy().view(np.uint64)
                    check_block(out, ref[(with_m, S)], S, with_m)
                    assert int(out[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
                    assert np.array_equal(out, old), "differs from the walked instantiation"


@pytest.fixture(scope="module")
def stale():
    out = []
    for tiles in (3, 20):
        nbits = tiles * EVENT_TILE
        F, R, M = sparse_vectors(1671 + tiles, nbits)
        out.append((nbits, F, R, M, references(F, R, M, nbits)))
    return out


@gpu
@pytest.mark.parametrize("pattern", [0x00000000, 0xffffffff, 0x80808080, 0x7fffffff, 0x5a5a5a5a])
def test_stale_memory(ctx, stale, pattern):
    """Scratch buffers and LDS hold a pattern before every hinted call: three tiles on one workgroup, twenty on three at width 2."""
    for (nbits, F, R, M, refs), nwg in zip(stale, (1, 3)):
        check_single(ctx, F, R, M, nbits, refs, [(nwg, (2,))], poison=pattern)


@pytest.fixture(scope="module")
def ranged():
    nbits = 11 * EVENT_TILE - 5
    F, R, M = sparse_vectors(1751, nbits, 0.004)
    return nbits, F, R, M, references(F, R, M, nbits)


@gpu
@pytest.mark.parametrize("mode", MODES)
def test_tile_ranges_cut_inside_a_chromosome(ctx, ranged, mode):
    """pmx_cc_batch_ranges_dev: the jobs are the tiles [0, 4), [4, 5), [5, 11) of one chromosome, on three workgroups at width
    2; their shares add up to the chromosome and equal the shares at width 1 and of the walked instantiation one by one."""
    nbits, F, R, M, refs = ranged
    dev = torch.device("cuda", 0)
    t = [torch.from_numpy(x.view(np.int64)).to(dev) for x in (F, R, M)]
    cuts = [0, 4, 5, 11]
    n = len(cuts) - 1
    for with_m, hint in VARIANTS:
        def shares(S, L, flags):
            outs = [torch.full((ffi.PMX_NROWS, S + 1), -1, dtype=torch.int64, device=dev) for _ in range(n)]
            torch.cuda.synchronize()
            ctx.cc_batch_ranges_dev([t[0].data_ptr()] * n, [t[1].data_ptr()] * n, [t[2].data_ptr()] * n if with_m else None, [nbits] * n,
                                    cuts[:-1], [b - a for a, b in zip(cuts[:-1], cuts[1:])], S, L, flags, [o.data_ptr() for o in outs])
            ctx.sync()
            return [o.cpu().numpy().view(np.uint64) for o in outs]

        for S, L in SHIFTS:
            olds = shares(S, L, FORCE | (hint & DEEP))
            with Geometry(ctx, 3, mode, 1):
                base = shares(S, L, hint & DEEP)
            with Geometry(ctx, 3, mode, 2):
                outs, ev, _win = events_ran(ctx, lambda: shares(S, L, hint & DEEP))
            assert ev == 1, "the event kernel must have run"
            total = sum(outs)
            check_block(total, refs[(with_m, S)], S, with_m)
            assert int(total[ffi.PMX_ROW_SCALARS, 3]) == ffi.PMX_PATH_SPARSE
            for out, b, old in zip(outs, base, olds):
                assert np.array_equal(out, b), "differs from width 1"
                assert np.array_equal(out, old), "differs from the walked instantiation"
