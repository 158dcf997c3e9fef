"""Cases and the yardstick of the signal track's tests (tests/test_coverage_signal.py, tests/test_gpu_coverage_signal.py;
DESIGN.md 7.18.3).

The yardstick is the restatement below: Python loops over the per-base depth lists of ``bigwig_out_cases.depth_lists`` -- the bins,
``S``, the merge rule, ``v``, the text, the zoom records and the total summary, each float sum in its stated order.  It uses none of
``pymasc_amd.coverage``'s numpy; a Python ``float`` is an IEEE float64 and every ``*``, ``/`` and ``+`` on it is rounded on its own.

The definitions.  Reference ``r`` of length ``len`` has the bins ``j = 0 .. ceil(len / B) - 1``; bin ``j`` covers ``[j * B,
min((j + 1) * B, len))`` and has the width ``w_j`` (only the last bin can be short); ``S_j`` is the integer sum of the depth over its
bases; ``B`` is 1 .. 65536.  ``v_j = np.float32((float(S_j) * scale) / float(w_j))``.  Consecutive bins of one reference are one run
when they have the same ``S`` and the same width (the rule is on ``S``, not on ``v``); bins with ``S = 0`` are in no run; a run is
``(start0, end0, v)``, the references in header order.  Totals: ``runs``, ``covered_bases`` (the runs' widths summed), the smallest
and the largest ``v``.  The text of a value is ``'%.6f' % float(v)`` without trailing zeros and without a trailing ``.``.
bigWig: ``z_0`` is ``zoom_base`` (a multiple of ``B``) or ``B * p`` with the smallest power of two ``p`` that makes it at least
``max(32, 10 * covered_bases / runs)``; a zoom bin of level 0 takes the signal runs that overlap it in ascending start order, each by
``ov`` bases: ``validCount = sum ov``, min and max over ``v``, ``sum``: ``acc += float(ov) * float(v)``, ``sumSquares``:
``acc += float(ov) * (float(v) * float(v))``, both from 0.0; a bin of level ``k + 1`` adds its up to four bins of level ``k`` in index
order the same way; the records hold the four floats as float32.  Total summary: ``validCount = covered_bases``, min, max, then the
two sums as float64: per data section its runs in order with the two products from 0.0, the sections' partial sums then added in
file order from 0.0.
"""
import struct

import numpy as np

from tests import bigwig_out_cases as BC

BINS = (1, 2, 7, 50, 4096, 65536)
TINY = 2.0 ** -30                   # a scale at which every value of the planted library prints ``0``


def bin_sums(depths, B):
    """{name: [(lo, hi, S), ...]} of every bin, in header order (the order of ``depths``)."""
    out = {}
    for name, row in depths.items():
        bins = []
        for lo in range(0, len(row), B):
            hi = min(lo + B, len(row))
            total = 0
            for p in range(lo, hi):
                total += row[p]
            bins.append((lo, hi, total))
        out[name] = bins
    return out


def value(S, scale, w):
    return np.float32((float(S) * scale) / float(w))


def restate(sums, scale):
    """``sums`` = ``bin_sums(...)``.  Returns ``runs``: {name: [(start0, end0, v, S), ...]} of the references that have a run, in
    header order, and the four totals by name."""
    runs = {}
    for name, bins in sums.items():
        out, cur = [], None                                 # cur = [start, end, S, width]
        for lo, hi, S in bins:
            if cur is not None and cur[2] == S and cur[3] == hi - lo:
                cur[1] = hi
                continue
            if cur is not None and cur[2] != 0:
                out.append((cur[0], cur[1], value(cur[2], scale, cur[3]), cur[2]))
            cur = [lo, hi, S, hi - lo]
        if cur is not None and cur[2] != 0:
            out.append((cur[0], cur[1], value(cur[2], scale, cur[3]), cur[2]))
        if out:
            runs[name] = out
    flat = [r for v in runs.values() for r in v]
    return dict(runs=runs, n_runs=len(flat), covered_bases=sum(e - s for s, e, _v, _S in flat),
                min=min((float(v) for _s, _e, v, _S in flat), default=0.0), max=max((float(v) for _s, _e, v, _S in flat), default=0.0))


def totals(want):
    return want["n_runs"], want["covered_bases"], want["min"], want["max"]


def rows_of(want):
    """Every run as (name, start0, end0, the bits of v), in file order."""
    return [(n, s, e, int(np.float32(v).view(np.uint32))) for n, rows in want["runs"].items() for s, e, v, _S in rows]


def rows_got(signal):
    """``rows_of`` of a ``pymasc_amd.coverage.Signal``."""
    return [(n, int(a), int(b), int(c)) for n, (s, e, v) in signal.runs.items() for a, b, c in zip(s, e, v.view(np.uint32))]


def text_value(v) -> str:
    text = "%.6f" % float(v)
    while text.endswith("0"):
        text = text[:-1]
    return text[:-1] if text.endswith(".") else text


def text_of(want) -> bytes:
    return "".join("%s\t%d\t%d\t%s\n" % (n, s, e, text_value(v)) for n, rows in want["runs"].items() for s, e, v, _S in rows).encode()


def reductions(want, lengths, B, zoom_base=None):
    """[z_0, z_1, ...] of the levels that exist; ``lengths``: of the chosen references."""
    if not want["n_runs"]:
        return []
    z0 = zoom_base
    if z0 is None:
        z0 = B
        while z0 < 32 or z0 * want["n_runs"] < 10 * want["covered_bases"]:
            z0 *= 2
    assert z0 % B == 0
    return [z0 * 4 ** k for k in range(10) if z0 * 4 ** k <= max(lengths) / 2]


def _level0(rows, length, z):
    """{bin: [valid, min, max, sum, squares]} of one reference."""
    bins = {}
    for s, e, v, _S in rows:                                # ascending start order
        for j in range(s // z, (e - 1) // z + 1):
            lo, hi = j * z, min((j + 1) * z, length)
            ov = min(e, hi) - max(s, lo)
            b = bins.setdefault(j, [0, v, v, 0.0, 0.0])
            b[0] += ov
            b[1], b[2] = min(b[1], v), max(b[2], v)
            b[3] += float(ov) * float(v)
            b[4] += float(ov) * (float(v) * float(v))
    return bins


def _fold(bins):
    out = {}
    for j in sorted(bins):                                  # a parent's children in index order; an empty child adds nothing
        c = bins[j]
        b = out.setdefault(j // 4, [0, c[1], c[2], 0.0, 0.0])
        b[0] += c[0]
        b[1], b[2] = min(b[1], c[1]), max(b[2], c[2])
        b[3] += c[3]
        b[4] += c[4]
    return out


def restate_zooms(want, refs, zs):
    """[(z, [32-byte records in file order])] of the levels ``zs`` = ``reductions(...)``; ``refs``: the chosen references."""
    ids = BC.chrom_ids([n for n, _l in refs])
    order = sorted(refs, key=lambda x: ids[x[0]])
    level = {n: _level0(want["runs"].get(n, []), l, zs[0]) for n, l in order} if zs else {}
    out = []
    for k, z in enumerate(zs):
        if k:
            level = {n: _fold(level[n]) for n, _l in order}
        recs = []
        for n, l in order:
            for j in sorted(level[n]):
                valid, lo, hi, total, squares = level[n][j]
                recs.append(struct.pack("<IIII", ids[n], j * z, min((j + 1) * z, l), valid) + np.float32(lo).tobytes() + np.float32(hi).tobytes()
                            + np.float32(total).tobytes() + np.float32(squares).tobytes())
        out.append((z, recs))
    return out


def restate_summary(want, refs, items) -> bytes:
    """The 40 bytes of the total summary of a file with ``items`` runs per data section."""
    ids = BC.chrom_ids([n for n, _l in refs])
    total = squares = 0.0
    for n in sorted(want["runs"], key=lambda n: ids[n]):    # file order
        rows = want["runs"][n]
        for a in range(0, len(rows), items):
            part = part2 = 0.0
            for s, e, v, _S in rows[a:a + items]:
                part += float(e - s) * float(v)
                part2 += float(e - s) * (float(v) * float(v))
            total += part
            squares += part2
    return struct.pack("<Qdddd", want["covered_bases"], want["min"], want["max"], total, squares)


def check_file(got, want, refs, B, zoom_base=None, items=1024):
    """What ``bigwig_out_cases.read_file`` read against the restatement; ``refs``: the chosen references in header order."""
    ids = BC.chrom_ids([n for n, _l in refs])
    by_id = sorted(want["runs"], key=lambda n: ids[n])
    assert got["chroms"] == sorted(((n, ids[n], l) for n, l in refs), key=lambda x: x[1])
    assert list(got["runs"]) == by_id
    for n in by_id:
        assert [(s, e, np.float32(v).tobytes()) for s, e, v in got["runs"][n]] == [(s, e, np.float32(v).tobytes()) for s, e, v, _S in want["runs"][n]]
    assert got["sections"] == [min(items, len(want["runs"][n]) - a) for n in by_id for a in range(0, len(want["runs"][n]), items)]
    zs = reductions(want, [l for _n, l in refs], B, zoom_base)
    assert [z for z, _r in got["zooms"]] == zs
    for (z, recs), (_z, wanted) in zip(got["zooms"], restate_zooms(want, refs, zs)):
        assert recs == wanted
    assert got["summary"] == restate_summary(want, refs, items)


# ---------------------------------------------------------------------------------------------------------------------------------
# the planted library: forward reads that lie apart or exactly on each other, each a depth run [pos1 - 1, pos1 - 1 + read_len)
# ---------------------------------------------------------------------------------------------------------------------------------

P_REFS = [("p0", 1000), ("p1", 30), ("p2", 1030), ("p3", 600)]
P_B = 50                            # the bin the situations below are planted for


def planted_reads():
    rows = [(0, 101, 100, 0)]                               # p0 [100, 200): bins 2 and 3 whole, begins on a bin's first base, ends on a last
    rows += [(0, 301, 400, 0)]                              # p0 [300, 700): a depth run over 8 bins
    rows += [(0, 901, 100, 0)]                              # p0 [900, 1000): the last two bins of a length that is a multiple of B
    rows += [(1, 6, 10, 0)]                                 # p1: shorter than B
    rows += [(2, 971, 60, 0)]                               # p2 [970, 1030): 30 bases in bin 19 and 30 in the short last bin
    rows += [(3, 11, 20, 0), (3, 11, 20, 0), (3, 61, 40, 0)]     # p3: S = 40 in bin 0 (depth 2) and in bin 1 (depth 1): they merge
    rows += [(3, 201, 100, 0), (3, 251, 50, 0)]             # p3 [200, 300): depth 1 then 2: S = 50 and 100, the mean is 1 and 2
    return sorted(rows)


def check_planted(want, scale):
    """The situations of the planted library at ``P_B``, asserted from the restatement (``want``: at ``scale``)."""
    B = P_B
    r = {n: [(s, e, S) for s, e, _v, S in rows] for n, rows in want["runs"].items()}
    v = {n: {(s, e): x for s, e, x, _S in rows} for n, rows in want["runs"].items()}
    assert (100, 200, B) in r["p0"]                         # equal S in neighbouring bins: one run; on a bin's first and last base
    assert (300, 700, B) in r["p0"]                         # a depth run crossing many bins
    assert r["p0"][-1] == (900, 1000, B)                    # a length that is a multiple of B: the last bin merges
    assert [s for s, _e, _S in r["p0"]] == [100, 300, 900]  # zero bins between the runs
    assert r["p1"] == [(0, 30, 10)]                         # a reference shorter than B: one bin of its length
    assert r["p2"] == [(950, 1000, 30), (1000, 1030, 30)]   # equal S in the short last bin: it stays apart
    assert r["p3"][0] == (0, 100, 40)                       # equal S from different depths merges: the rule is on S
    assert r["p3"][1:] == [(200, 250, 50), (250, 300, 100)]
    if scale == 1.0:
        assert text_value(v["p1"][0, 30]) == "0.333333"     # six decimals
        assert text_value(v["p0"][100, 200]) == "1" and text_value(v["p3"][250, 300]) == "2"      # whole numbers
        assert text_value(v["p2"][950, 1000]) == "0.6" and text_value(v["p3"][0, 100]) == "0.8"
    if scale == TINY:
        assert all(text_value(x) == "0" for rows in v.values() for x in rows.values())            # 0.0000004 and less is 0
        assert all(float(x) > 0 for rows in v.values() for x in rows.values())


# the tie: 4097 reads over both bins of 4096 bases of a reference of 8192, one more on its last base: the sums differ by 1, above 2^24,
# and both values are the float32 4097.0 (4097 + 1/4096 is a tie that rounds to even).  Read at extend = T_EXTEND.
T_REFS = [("t0", 8192)]
T_B, T_EXTEND = 4096, 8192


def tie_reads():
    return [(0, 1, 36, 0)] * 4097 + [(0, 8192, 36, 0)]


def check_tie(want):
    assert [(s, e, S) for s, e, _v, S in want["runs"]["t0"]] == [(0, 4096, 4097 * 4096), (4096, 8192, 4097 * 4096 + 1)]
    assert 4097 * 4096 > 1 << 24
    a, b = (x for _s, _e, x, _S in want["runs"]["t0"])
    assert a.tobytes() == b.tobytes() == np.float32(4097.0).tobytes()       # one float32, two runs
    assert (4097 * 4096 + 1) / 4096 != 4097.0
