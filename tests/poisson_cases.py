"""Cases and the yardstick of the p-score track's tests (tests/test_coverage_poisson.py, tests/test_gpu_coverage_poisson.py;
DESIGN.md 7.18.6): the treatment scored against the control, -log10 of a Poisson upper tail per bin.

The yardstick is the restatement below: Python loops over the per-base depth lists of ``bigwig_out_cases.depth_lists`` of the two
pileups -- the bins and both sums (``signal_cases.bin_sums``), its own ``lg2``, ``ln``, ``F``, series, window and run rule.  The
zoom records and the total summary are ``signal_cases``' own loops over the restated runs.  It takes nothing from
``pymasc_amd.coverage``; a Python ``float`` is an IEEE float64 and every ``*``, ``/``, ``+`` and ``-`` on it is rounded on its own.

The definitions (this project's own: nothing is compared with MACS2).  Everything is integer arithmetic or float64.

* Two pileups over the same chosen references; ``B`` (1 .. 65536) with the bins, the widths ``w_j`` and the sums ``S_t[j]``,
  ``S_c[j]`` of ``signal_cases``; reference ``r`` has the bins ``0 .. n_r - 1`` and the length ``len_r``.  ``a_c`` is a float64
  factor; the treatment is not scaled.  ``W_s`` and ``W_l`` are two window sizes in bases, each 0 (off) .. 2^31 - 1.
* ``k[j] = S_t[j] // w_j``, an integer division.
* Window mean, for ``W > 0``: ``h = (W // B) // 2`` bins; ``lo = max(0, j - h)`` and ``hi = min(n_r - 1, j + h)``, inside the bin
  range of ``j``'s own reference (a window never crosses into another reference); ``N = sum S_c[lo .. hi]``, an integer;
  ``D = min(len_r, (hi + 1) * B) - lo * B``; ``c_W = (float(N) * a_c) / float(D)``.  ``h = 0`` gives the bin's own value; a window
  that is off contributes nothing.
* Lambda: ``c_0 = (float(S_c[j]) * a_c) / float(w_j)``; ``l_bg = (float(sum of every S_c) * a_c) / float(sum of the chosen
  lengths)``; ``l[j] = max(l_bg, c_0, c_Ws, c_Wl)``.  The sum of every ``S_c`` is above 0, so ``l > 0`` and normal everywhere.
* ``ln(x) = lg2(x) * 0.6931471805599453`` with ``lg2`` the stated algorithm of ``compare_cases`` (written out again here);
  ``F[0] = F[1] = 0.0``, ``F[i] = F[i - 1] + ln(float(i))``, a sequential sum.
* Score: if ``float(k) <= l`` then ``v = 0.0`` (not enriched; equality counts as not enriched).  Otherwise ``S = 1.0``,
  ``T = 1.0`` and for ``i = 1, 2, ...``: ``r = l / float(k + i)``; ``T = T * r``; ``S' = S + T``; stop when ``S' == S``, else
  ``S = S'``.  Then ``A = float(k) * ln(l)``; ``C = (l - A) + F[k]``;
  ``v = np.float32(C * 0.4342944819032518 - lg2(S) * 0.3010299956639812)``: -log10 of ``P(X >= k | l)``.
* Runs: a bin with ``S_t = 0`` is in no run.  A kept bin begins a run when it is the first bin of its reference, when the bin before
  it is not kept, or when ``k`` or the bits of ``l`` differ from the bin before: the rule is on ``(k, l)``, not on ``v`` and not on
  the width.  Rows are ``(start0, end0, v)``, the references in header order; the totals are the signal's four.
"""
import math
import struct

import numpy as np

from tests import bigwig_out_cases as BC
from tests import compare_cases as PC
from tests import coverage_cases as CC
from tests import signal_cases as SC

BINS = (1, 2, 7, 50, 4096)
WINDOWS = (1000, 10000)             # the defaults
ROOT_HALF = 0.7071067811865476


def lg2(x: float) -> float:
    m, e = math.frexp(x)
    if m < ROOT_HALF:
        m = 2.0 * m
        e = e - 1
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    P = 1.0 / 21.0
    for k in range(9, -1, -1):
        P = P * z
        P = P + 1.0 / float(2 * k + 1)
    t = (2.0 * s) * P
    return float(e) + t * 1.4426950408889634


def ln(x: float) -> float:
    return lg2(x) * 0.6931471805599453


def lnfact(n: int):
    """``[F[0], ..., F[n - 1]]``, a sequential sum."""
    F = [0.0, 0.0][:n]
    for i in range(2, n):
        F.append(F[i - 1] + ln(float(i)))
    return F


_F = lnfact(2)                      # grown when a larger k is asked for: F[k] does not depend on the table's length


def fact(k: int) -> float:
    while len(_F) <= k:
        _F.append(_F[-1] + ln(float(len(_F))))
    return _F[k]


def series(k: int, lam: float):
    """(S, the number of steps) of a pair with ``float(k) > lam``."""
    S, T, i = 1.0, 1.0, 0
    while True:
        i += 1
        r = lam / float(k + i)
        T = T * r
        S2 = S + T
        if S2 == S:
            return S, i
        S = S2


def value(k: int, lam: float):
    if float(k) <= lam:
        return np.float32(0.0)
    S, _steps = series(k, lam)
    A = float(k) * ln(lam)
    C = (lam - A) + fact(k)
    return np.float32(C * 0.4342944819032518 - lg2(S) * 0.3010299956639812)


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def candidates(sums_c, B, a_c, small, large):
    """{name: [(l_bg, c_0, c_Ws, c_Wl) of every bin]}, an entry None where the window is off."""
    total = length = 0
    for bins in sums_c.values():
        length += bins[-1][1]
        for _lo, _hi, Sc in bins:
            total += Sc
    assert total > 0
    bg = (float(total) * a_c) / float(length)
    out = {}
    for name, bins in sums_c.items():
        n, ref_len = len(bins), bins[-1][1]
        upto = [0]                                          # upto[i]: the sum of the bins in front of i
        for _lo, _hi, Sc in bins:
            upto.append(upto[-1] + Sc)
        rows = []
        for j, (lo_base, hi_base, Sc) in enumerate(bins):
            c = [bg, (float(Sc) * a_c) / float(hi_base - lo_base)]
            for W in (small, large):
                if W == 0:
                    c.append(None)
                    continue
                h = (W // B) // 2
                lo, hi = max(0, j - h), min(n - 1, j + h)
                N = upto[hi + 1] - upto[lo]
                D = min(ref_len, (hi + 1) * B) - lo * B
                c.append((float(N) * a_c) / float(D))
            rows.append(tuple(c))
        out[name] = rows
    return out


def restate(sums_t, sums_c, B, a_c=1.0, small=WINDOWS[0], large=WINDOWS[1]):
    """``sums_t``, ``sums_c`` = ``signal_cases.bin_sums(...)`` of the two pileups over the same references.  Returns what
    ``signal_cases.restate`` returns, a run's last field being ``(k, l)``; ``bins``: {name: [(kept, k, l, the candidates)]} of every
    bin; ``steps``: the longest series."""
    cands = candidates(sums_c, B, a_c, small, large)
    runs, every, longest = {}, {}, 0
    for name, rows in sums_t.items():
        out, cur, here = [], None, []                       # cur = [start, end, k, l]
        for j, (lo, hi, St) in enumerate(rows):
            assert (lo, hi) == sums_c[name][j][:2]
            lam = max(x for x in cands[name][j] if x is not None)
            k = St // (hi - lo)
            here.append((St != 0, k, lam, cands[name][j]))
            if St == 0:
                if cur is not None:
                    out.append(cur)
                cur = None
                continue
            if cur is not None and cur[2] == k and bits(cur[3]) == bits(lam):
                cur[1] = hi
                continue
            if cur is not None:
                out.append(cur)
            cur = [lo, hi, k, lam]
        if cur is not None:
            out.append(cur)
        every[name] = here
        if out:
            runs[name] = [(s, e, value(k, lam), (k, lam)) for s, e, k, lam in out]
            longest = max([longest] + [series(k, lam)[1] for _s, _e, k, lam in out if float(k) > lam])
    flat = [r for v in runs.values() for r in v]
    return dict(runs=runs, n_runs=len(flat), covered_bases=sum(e - s for s, e, _v, _S in flat), bins=every, steps=longest,
                min=min((float(v) for _s, _e, v, _S in flat), default=0.0), max=max((float(v) for _s, _e, v, _S in flat), default=0.0))


totals, rows_of, rows_got, check_file, text_of, text_value = SC.totals, SC.rows_of, SC.rows_got, SC.check_file, PC.text_of, PC.text_value


def entries(want) -> int:
    """The boundaries the device's first compaction lists: a bin begins one where its reference begins, where it is kept and the bin
    before is not (or the other way round), or where ``k`` or ``l`` differs between two kept bins."""
    n = 0
    for rows in want["bins"].values():
        for j, (kept, k, lam, _c) in enumerate(rows):
            before = rows[j - 1] if j else None
            n += before is None or kept != before[0] or (kept and (k != before[1] or bits(lam) != bits(before[2])))
    return n


def sums_of(reads_t, reads_c, refs, B, extend=0):
    use = [1] * len(refs)
    return [SC.bin_sums(BC.depth_lists(CC.restate(x, refs, use, extend), refs, use), B) for x in (reads_t, reads_c)]


def narrowpeak_of(want_peaks, first=0) -> bytes:
    """``call_cases.text_of`` with the value in column 8 as well: the lines of a p-score track's peaks."""
    from tests import call_cases
    return "".join("%s\t%d\t%d\tpeak_%d\t%d\t.\t%s\t%s\t-1\t%d\n" % (name, s, e, first + i + 1, call_cases.score(v), text_value(v), text_value(v), m - s)
                   for i, (name, s, e, m, v, _r) in enumerate(want_peaks["peaks"])).encode()


# ---------------------------------------------------------------------------------------------------------------------------------
# the planted pair on signal_cases.P_REFS at B = 50 and the windows (200, 500): h = 2 and 5 bins.  Forward reads, each a depth run
# [pos1 - 1, pos1 - 1 + read_len)
# ---------------------------------------------------------------------------------------------------------------------------------

P_REFS = SC.P_REFS                  # p0 1000 (20 bins), p1 30 (shorter than B), p2 1030 (a short last bin), p3 600
P_B = SC.P_B
P_WINDOWS = (200, 500)
P_SETS = [(1.0, 200, 500), (1.0, 1000, 10000), (1.0, 40, 500), (1.0, 0, 500), (1.0, 200, 0), (1.0, 0, 0), (0.37, 200, 500), (1.9, 1000, 10000)]
P_ZOOM = 50


def planted_treatment():
    rows = [(0, 1, 50, 0)] * 7                              # p0 bin 0: k = 7 against c_0 = 6: floor(l) + 1; the windows clipped at 0
    rows += [(0, 51, 50, 0)]                                # p0 bin 1: the large window (bins 0 .. 6, clipped) wins
    rows += [(0, 301, 50, 0)] * 8                           # p0 bin 6: k = 8 on the control's spike of 8: float(k) == l, v = 0
    rows += [(0, 351, 50, 0)] * 3                           # p0 bin 7: the small window (the spike next door) wins
    rows += [(0, 451, 50, 0)] * 3                           # p0 bin 9: only the large window sees a control; bin 8 has S_t = 0
    rows += [(0, 701, 50, 0), (0, 751, 10, 0)]              # p0 bin 14: k = 1 < l; bin 15: S_t = 10, k = 0: both v = 0, kept apart
    rows += [(0, 951, 50, 0)] * 25                          # p0 bin 19: k = 25 = max_depth_t on the deep end; the windows clipped at the end
    rows += [(1, 1, 30, 0)] * 3                             # p1: one bin of 30 bases between p0's deep end and p2's deep beginning
    rows += [(2, 951, 80, 0)]                               # p2 [950, 1030): bin 19 and the short last bin, k = 1 in both: one run
    rows += [(3, 101, 100, 0), (3, 251, 50, 0)]             # p3, treatment only: bins 2, 3 merge, bin 4 has S_t = 0, bin 5 a run of its own
    return sorted(rows)


def planted_control():
    rows = [(0, 1, 50, 0)] * 6                              # p0 bin 0
    rows += [(0, 301, 50, 0)] * 8                           # p0 bin 6: the spike
    rows += [(0, 601, 200, 0)] * 4                          # p0 bins 12 .. 15: depth 4
    rows += [(0, 951, 50, 0)] * 10                          # p0 bin 19: the deep end
    rows += [(2, 1, 50, 0)] * 10                            # p2 bin 0: the deep beginning
    return sorted(rows)


def planted_lonely():
    """A control with reads on p1 only."""
    return [(1, 1, 30, 0)] * 2


def check_planted(want, a_c, small, large):
    """The situations of the planted pair at ``P_B``, asserted from the restatement."""
    B = P_B
    b = want["bins"]
    r = {n: [(s, e, S[0]) for s, e, _v, S in rows] for n, rows in want["runs"].items()}
    v = {n: {(s, e): float(x) for s, e, x, _S in rows} for n, rows in want["runs"].items()}
    hs, hl = (small // B) // 2, (large // B) // 2

    def wins(name, j, i):                                   # candidate i is l, alone
        c = b[name][j][3]
        return c[i] is not None and b[name][j][2] == c[i] and all(x is None or x < c[i] for q, x in enumerate(c) if q != i)
    # the runs: on (k, l)
    assert [(s, e) for s, e, _k in r["p0"]][:2] == [(0, 50), (50, 100)] and r["p0"][-1] == (950, 1000, 25)
    assert (700, 750, 1) in r["p0"] and (750, 800, 0) in r["p0"]       # equal v = 0, different k: kept apart; S_t > 0 with k = 0 is kept
    assert v["p0"][700, 750] == v["p0"][750, 800] == 0.0
    assert not b["p0"][8][0] and b["p0"][7][0] and b["p0"][9][0] and not any(s <= 400 < e for s, e, _k in r["p0"])     # S_t = 0 is in no run
    assert r["p1"] == [(0, 30, 3)]                          # a reference shorter than B
    assert r["p2"] == [(950, 1030, 1)]                      # the short last bin merges: the rule is not on the width
    assert r["p3"] == [(100, 200, 1), (250, 300, 1)]        # equal (k, l) merge; the bin with S_t = 0 splits equal neighbours
    assert b["p3"][2][1:3] == b["p3"][3][1:3] == b["p3"][5][1:3]
    assert all(wins("p3", j, 0) for j in range(12))         # a reference with reads in the treatment only: the background
    assert b["p0"][19][1] == 25 == max(k for rows in b.values() for _kept, k, _l, _c in rows) and v["p0"][950, 1000] > 0      # F's last entry
    # two references back to back: the deep end of p0 and the deep beginning of p2 do not reach p1
    assert b["p1"][0][3][1] == 0.0 and wins("p1", 0, 0) and b["p0"][19][2] > b["p1"][0][2] < b["p2"][0][2]
    for c in b["p1"][0][3][2:]:
        assert c is None or c == 0.0                        # a window wider than its reference: the reference's own mean
    if small and hs == 0:                                   # W < B: the bin's own value
        assert all(c[2] == c[1] for rows in b.values() for _kept, _k, _l, c in rows)
    assert all((c[2] is None) == (small == 0) and (c[3] is None) == (large == 0) for rows in b.values() for _kept, _k, _l, c in rows)
    if (small, large) == (0, 0):
        assert all(lam == max(c[0], c[1]) for rows in b.values() for _kept, _k, lam, c in rows)
    if large >= 2 * 1030:                                   # wider than every reference: one value per reference
        assert all(len({c[3] for _kept, _k, _l, c in rows}) == 1 for rows in b.values())
    if (a_c, small, large) == (1.0,) + P_WINDOWS:
        assert wins("p0", 0, 1) and b["p0"][0][1:3] == (7, 6.0) and v["p0"][0, 50] > 0         # k = floor(l) + 1
        assert b["p0"][0][3][2] == 300.0 / 150.0 and b["p0"][0][3][3] == 300.0 / 300.0         # clipped at the beginning: bins 0 .. 2, 0 .. 5
        assert wins("p0", 1, 3) and b["p0"][1][3][3] == 700.0 / 350.0                          # bins 0 .. 6
        assert wins("p0", 6, 1) and b["p0"][6][1:3] == (8, 8.0) and v["p0"][300, 350] == 0.0    # float(k) == l: not enriched
        assert (300, 350, 8) in r["p0"]
        assert wins("p0", 7, 2) and b["p0"][7][3][2] == 400.0 / 250.0 and v["p0"][350, 400] > 0
        assert wins("p0", 9, 3) and b["p0"][9][3][2] == 0.0 and b["p0"][9][3][3] == 1000.0 / 550.0
        assert b["p0"][14][1] == 1 < b["p0"][14][2] and b["p0"][15][1] == 0                    # k < l; k = 0
        assert b["p0"][19][3][2] == 500.0 / 150.0 and b["p0"][19][3][3] == 900.0 / 300.0       # clipped at the end: bins 17 .. 19, 14 .. 19
        assert wins("p0", 19, 1)
        assert wins("p2", 19, 0) and wins("p2", 20, 0) and b["p2"][20][3][3] == 0.0            # the short last bin: D = 280


# the long series beside short ones in one wave: 64 bins of 50 bases, a control of depth 3000 in bin 10 and nowhere else, the
# treatment 3001 there and 60 + j in every other bin j; both windows off and a_c = 1: l = 3000 in bin 10 and k = floor(l) + 1, the
# background 46.875 < k elsewhere.  Every bin is a run of its own (k differs), so the 64 series run in the lanes of one wave
D_REFS = [("d0", 3200)]
D_B, D_DEPTH, D_BIN = 50, 3000, 10


def deep_treatment():
    return sorted((0, 50 * j + 1, 50, 0) for j in range(64) for _i in range(D_DEPTH + 1 if j == D_BIN else 60 + j))


def deep_control():
    return [(0, 50 * D_BIN + 1, 50, 0)] * D_DEPTH


def check_deep(want):
    rows = want["runs"]["d0"]
    assert [(s, e, S[0]) for s, e, _v, S in rows] == [(50 * j, 50 * j + 50, D_DEPTH + 1 if j == D_BIN else 60 + j) for j in range(64)]
    assert rows[D_BIN][3] == (D_DEPTH + 1, float(D_DEPTH)) and series(*rows[D_BIN][3])[1] == want["steps"] > 400
    assert all(S[1] == 46.875 and 0 < series(*S)[1] < 100 for j, (_s, _e, _v, S) in enumerate(rows) if j != D_BIN)
    assert 0.0 < float(rows[D_BIN][2]) < 1.0 < min(float(v) for j, (_s, _e, v, _S) in enumerate(rows) if j != D_BIN)


# the new scan's edges: one reference of that many bins at B = 1 carrying a handful of reads (256 bins per workgroup, 1024 workgroup
# sums per thread of the one workgroup that scans them)
SCAN_SMALL = (1, 255, 256, 257)
SCAN_LARGE = (262_143, 262_144, 262_145)
SCAN_WINDOWS = (4, 600)             # at B = 1: h = 2 and 300 bases, so that a window sum crosses a workgroup's edge


def scan_reads(n):
    """(the treatment, the control) on one reference of ``n`` bases: reads of 3 bases around every edge that exists."""
    at = sorted({p for e in (1, 64, 256, 512, 65_536, 131_072, 261_888, 262_144, n) for p in (e - 3, e - 1, e, e + 1) if 1 <= p <= n})
    t = [(0, p, min(3, n - p + 1), 0) for p in at]
    c = [(0, p, min(3, n - p + 1), 0) for p in at[::2]] + [(0, n, 1, 0)] * 2
    return sorted(t), sorted(c)
