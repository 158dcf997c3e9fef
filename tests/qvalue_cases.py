"""Cases and the yardstick of the q-score table's tests (tests/test_coverage_qvalue.py, tests/test_gpu_coverage_qvalue.py; DESIGN.md
7.18.7): Benjamini-Hochberg q-scores for the p-score track, over every base of the chosen references.

The yardstick is the restatement below: plain Python loops, a dict and ``sorted`` over a list of runs, with its own ``lg2``.  It
takes nothing from ``pymasc_amd.coverage``; a Python ``float`` is an IEEE float64 and every ``*``, ``+`` and ``-`` on it is rounded on
its own.  The planted tracks are made of treatment / control read sets through the p-score track (``poisson_cases``' machinery for
the small ones, tagAlign sawtooth pileups for the large ones); every situation a case is for is asserted from the restatement itself.

The definitions (this project's own: nothing is compared with MACS2).  Everything is integer arithmetic or float64.

* Input: the runs ``(ref, start0, end0, v)`` of a p-score track, ``v`` float32: ``+0.0`` or the float32 of a positive number, so
  ``v >= 0`` and never a NaN.  A track whose smallest value is negative is refused.
* Tests: ``N`` = the sum of the lengths of the chosen references.  Every base of the chosen genome is one test; a base in no run has
  p = 1 and counts in ``N`` only.
* Distinct values: ``u_1 > u_2 > ... > u_m`` are the distinct values of the runs, compared as floats.  ``W_i`` = the sum of
  ``end0 - start0`` over the runs with the value ``u_i``.
* Rank: ``r_1 = 1``, ``r_i = 1 + W_1 + ... + W_(i-1)``.  ``r_i <= N`` always.
* Raw score: ``x_i = float(u_i) + (lg2(float(r_i)) - lg2(float(N))) * 0.3010299956639812`` with ``lg2`` the stated algorithm of
  ``compare_cases`` (written out again here).  ``r_i`` and ``N`` are below 2^53, so the conversions are exact.
* Monotone, clamped: ``Q_i = max(0.0, min(x_1 .. x_i))`` and ``q_i = np.float32(Q_i)``.  ``q`` is non-increasing in ``i``, hence
  non-decreasing in the p-score.
* Table: ``m`` rows ``(u_i, W_i, q_i)``, descending in ``u``.
* Cutoff: ``pcut(X)`` for a finite ``X`` is ``float(u_i)`` of the largest ``i`` with ``float(q_i) >= X``, the smallest p-score whose
  q-score reaches ``X``; ``2^40`` when no row reaches ``X``; ``X <= 0`` gives ``float(u_m)``.
* Lookup: the q-score of a peak is ``q_i`` of the row with ``u_i == value``; the row exists.
"""
import math

import numpy as np

ROOT_HALF = 0.7071067811865476
LOG10_2 = 0.3010299956639812
NONE = 2.0 ** 40


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


def bits32(v) -> int:
    return int(np.float32(v).view(np.uint32))


def rows_of_runs(runs):
    """The rows (name, start0, end0, v) of ``{name: (start0[], end0[], v[])}``, in file order."""
    return [(n, int(a), int(b), np.float32(c)) for n, (s, e, v) in runs.items() for a, b, c in zip(s, e, v)]


def restate(rows, refs):
    """``rows``: (name, start0, end0, v) of every run; ``refs``: (name, length) of the chosen references.  ``table``: the rows
    (u, W, q); ``x``, ``r``: the raw score and the rank of every row; ``where``: the references that hold a run of the row's value."""
    N = 0
    for _n, length in refs:
        N += length
    W, where = {}, {}
    covered = 0
    for name, s, e, v in rows:
        u = float(v)
        assert u >= 0.0 and e > s
        if u == 0.0:
            u = 0.0                                         # (no -0.0 in a p-score track; the key is +0.0 either way)
        W[u] = W.get(u, 0) + (e - s)
        where.setdefault(u, set()).add(name)
        covered += e - s
    table, xs, rs = [], [], []
    r, low, positive = 1, None, 0
    for u in sorted(W, reverse=True):
        x = u + (lg2(float(r)) - lg2(float(N))) * LOG10_2
        if low is None or x < low:
            low = x
        Q = low if low > 0.0 else 0.0
        q = np.float32(Q)
        table.append((np.float32(u), W[u], q))
        xs.append(x)
        rs.append(r)
        if float(q) > 0.0:
            positive += W[u]
        r += W[u]
    assert r - 1 == covered <= N and all(x <= N for x in rs)
    return dict(table=table, x=xs, r=rs, tests=N, covered=covered, positive=positive, where=[where[float(u)] for u, _W, _q in table],
                n_runs=len(rows))


def totals(want):
    """(m, N, the covered bases, the bases with q > 0): the four totals."""
    return len(want["table"]), want["tests"], want["covered"], want["positive"]


def table_of(want):
    """Every row as (the bits of u, W, the bits of q)."""
    return [(bits32(u), int(W), bits32(q)) for u, W, q in want["table"]]


def table_got(p, bases, q):
    """``table_of`` of three columns (float32, uint64, float32)."""
    return [(int(a), int(b), int(c)) for a, b, c in zip(np.asarray(p, dtype=np.float32).view(np.uint32), bases,
                                                        np.asarray(q, dtype=np.float32).view(np.uint32))]


def pcut(want, X: float) -> float:
    out = NONE
    for u, _W, q in want["table"]:                          # descending in u: the last row that reaches X stays
        if float(q) >= X:
            out = float(u)
    return out


def lookup(want, v):
    for u, _W, q in want["table"]:
        if float(u) == float(v):
            return q
    raise AssertionError("a value without a row")


def cutoffs(want):
    """The X of the cutoff cases of a table that has a positive q: at a row's q exactly (equality passes), between two rows, above
    the top (2^40), at 0 and at a negative X (the last row's u); each with the answer, asserted to be the case it is for."""
    t = want["table"]
    qs = sorted({float(q) for _u, _W, q in t if float(q) > 0.0})
    assert qs
    out = [(qs[-1], pcut(want, qs[-1])), (qs[-1] * 2.0 + 1.0, NONE), (0.0, float(t[-1][0])), (-3.5, float(t[-1][0]))]
    assert pcut(want, qs[-1] * 2.0 + 1.0) == NONE and pcut(want, 0.0) == pcut(want, -3.5) == float(t[-1][0])
    assert out[0][1] == max(float(u) for u, _W, q in t if float(q) == qs[-1]) or len({float(q) for _u, _W, q in t}) < len(t)
    lower = [x for x in qs[:-1]] or [0.0]
    between = (lower[-1] + qs[-1]) / 2.0                    # between the two largest q (or between 0 and the only one)
    assert lower[-1] < between < qs[-1] and pcut(want, between) == pcut(want, qs[-1])
    out.append((between, pcut(want, between)))
    if len(qs) > 1:                                         # at a lower row's q exactly
        assert pcut(want, qs[0]) < pcut(want, qs[-1])
        out.append((qs[0], pcut(want, qs[0])))
    return out


def digits(want):
    """The 8-bit digits (0: the lowest) in which the keys of the table's values differ: the radix passes that run."""
    keys = [~bits32(u) & 0xffffffff for u, _W, _q in want["table"]]
    acc_or, acc_and = 0, 0xffffffff
    for k in keys:
        acc_or |= k
        acc_and &= k
    return [d for d in range(4) if ((acc_or ^ acc_and) >> (8 * d)) & 255]


def text_value(v) -> str:
    text = "%.6f" % float(v)
    while text.endswith("0"):
        text = text[:-1]
    return text[:-1] if text.endswith(".") else text


def narrowpeak_of(want_peaks, want, first=0) -> bytes:
    """The lines of a p-score track's peaks (``call_cases.restate``) with the table: the value in columns 7 and 8, the q-score in 9."""
    from tests import call_cases
    return "".join("%s\t%d\t%d\tpeak_%d\t%d\t.\t%s\t%s\t%s\t%d\n" % (name, s, e, first + i + 1, call_cases.score(v), text_value(v), text_value(v),
                                                                      text_value(lookup(want, v)), m - s)
                   for i, (name, s, e, m, v, _r) in enumerate(want_peaks["peaks"])).encode()


# ---------------------------------------------------------------------------------------------------------------------------------
# the planted pairs: reads (ref, pos1, read_len, reverse), forward, each a depth run [pos1 - 1, pos1 - 1 + read_len); blocks of one
# depth at B = 50 with both windows off, so that l = max(l_bg, c_0)
# ---------------------------------------------------------------------------------------------------------------------------------

S_REFS = [("a", 2000), ("b", 1500), ("empty", 700)]         # "empty" never has a read: N exceeds the covered bases
S_B = 50
FAR = [(1, 1401, 50, 0)]                                     # a control of one read far from every block: l = l_bg, tiny


def block(ref, start0, width, depth):
    return [(ref, start0 + 1, width, 0)] * depth


def _at(places, depth_of):
    return sorted(x for i, (ref, s, w) in enumerate(places) for x in block(ref, s, w, depth_of(i)))


PLACES = [(0, 0, 50), (0, 500, 1000), (1, 0, 50), (1, 200, 50), (1, 400, 50)]


def small_case(name):
    """(refs, treatment, control, B, a_c, small, large) of a planted pair."""
    three = [(0, 100, 50), (0, 300, 50), (1, 200, 50)]
    t, c = dict(
        single=(block(0, 100, 50, 5), FAR),
        one_value=(_at(three, lambda i: 3), FAR),                                   # two references, one value: one row
        all_zero=(_at(three, lambda i: 2), _at(three, lambda i: 4)),                # k <= l everywhere: every v = 0, every q clamps
        # l = 3 under every block; k = 30 on 50 bases, 14 on 1000 (the heavy W in the middle), 13, 4 and 2 (k <= l: v = 0) on 50 each
        bites=(_at(PLACES, lambda i: (30, 14, 13, 4, 2)[i]), _at(PLACES, lambda i: 3)),
        # k = 14, 13, 12 against l = 3: every v lies in [2, 8), whose float32 bits share the top byte
        shared_digit=(_at(PLACES[:3], lambda i: (14, 13, 12)[i]), _at(PLACES[:3], lambda i: 3)),
    )[name]
    return S_REFS, sorted(t), sorted(c), S_B, 1.0, 0, 0


SMALL = ("single", "one_value", "all_zero", "bites", "shared_digit")


def check_small(name, want):
    t = want["table"]
    m, N, covered, positive = totals(want)
    assert N == 4200 > covered                              # a reference without a run
    low = [min(want["x"][:i + 1]) for i in range(m)]
    if name == "single":
        assert want["n_runs"] == 1 == m and float(t[0][0]) > 0.0 and digits(want) == []
    if name == "one_value":
        assert want["n_runs"] == 3 and m == 1 and want["where"][0] == {"a", "b"} and t[0][1] == 150 and digits(want) == []
    if name == "all_zero":
        assert want["n_runs"] == 3 and m == 1 and bits32(t[0][0]) == 0 and positive == 0 and want["x"][0] < 0.0 and bits32(t[0][2]) == 0
    if name == "bites":
        assert m == 5 and t[1][1] == 1000 and bits32(t[-1][0]) == 0
        assert want["x"][2] > want["x"][1] and bits32(t[2][2]) == bits32(t[1][2])      # the prefix min bites behind the heavy row
        assert want["x"][1] < want["x"][0] and bits32(t[1][2]) != bits32(t[0][2])      # ... and does not in front of it
        assert float(t[2][2]) > 0.0 and low[3] < 0.0 and bits32(t[3][2]) == 0          # the clamp bites below a row where it does not
        assert 0 < positive < covered and digits(want) == [0, 1, 2, 3]                 # keys that differ in all four digits
    if name == "shared_digit":
        assert m == 3 and all(2.0 <= float(u) < 8.0 for u, _W, _q in t) and 3 not in digits(want) and digits(want)     # a pass is skipped


# run counts at the wave, workgroup and sort-tile edges: n blocks of 2 bases every 4 bases at B = 1, depth 1 + i % 3
RUN_COUNTS = (1, 255, 256, 257, 8191, 8192, 8193)


def run_count_case(n):
    refs = [("r", 4 * n + 60)]
    t = sorted(x for i in range(n) for x in block(0, 4 * i, 2, 1 + i % 3))
    return refs, t, [(0, 4 * n + 11, 40, 0)], 1, 1.0, 0, 0


def check_run_count(n, want):
    assert want["n_runs"] == n and len(want["table"]) == min(n, 3) and want["covered"] == 2 * n


# distinct counts: two co-prime sawtooth pileups at B = 1 on the first L bases of one reference of SAW_R bases, both windows off.  The
# treatment's depth is 1 + x % SAW_P; the control's is SAW_C0 + 1 + x % SAW_Q (SAW_C0 reads over all L bases under a sawtooth), so that
# its smallest depth stays above its mean over the reference: l = c * a_c everywhere, never l_bg, and the value of a base depends on its
# own pair (k, c) alone.  One more base then adds at most one distinct value and takes none away: every m is reached, and the
# builder bisects for the L that gives it
SAW_P, SAW_Q, SAW_C0, SAW_AC, SAW_R = 751, 757, 1024, 2.0 ** -10, 1_200_000
DISTINCT_SMALL = (1, 2, 255, 256, 257)
DISTINCT_LARGE = (262_143, 262_144, 262_145)                # the edge of the one-workgroup scan's 1024 shares of 256
SAW_REFS = [("saw", SAW_R)]


def sawtooth_columns(L, period, under=0):
    """(ref, pos1, read_len, reverse) as four int64 arrays: one read per base, from the base to the end of its period or of the L
    bases, so that the depth at x < L is 1 + x % period, over ``under`` reads of all L bases."""
    x = np.arange(L, dtype=np.int64)
    pos1 = np.concatenate([np.ones(under, dtype=np.int64), x + 1])
    length = np.concatenate([np.full(under, L, dtype=np.int64), np.minimum(period - x % period, L - x)])
    return np.zeros(pos1.size, dtype=np.int64), pos1, length, np.zeros(pos1.size, dtype=np.int64)


def sawtooth_case(L):
    """(refs, the treatment's columns, the control's columns, B, a_c, small, large)."""
    assert 1 <= L and L * (SAW_C0 + SAW_Q + 1) < SAW_R * SAW_C0                      # l_bg stays below every c * a_c
    return SAW_REFS, sawtooth_columns(L, SAW_P), sawtooth_columns(L, SAW_Q, SAW_C0), 1, SAW_AC, 0, 0


def sawtooth_distinct(L):
    """The number of distinct float32 p-scores of the sawtooth pair on L bases (numpy, through ``pymasc_amd.coverage``'s series: the
    builder's search only -- the case itself is asserted from the restatement)."""
    from pymasc_amd import coverage
    x = np.arange(L, dtype=np.int64)
    pair = np.unique((1 + x % SAW_P) * 4096 + (SAW_C0 + 1 + x % SAW_Q))
    k, c = pair // 4096, pair % 4096
    v = coverage.poisson_values(k, (c.astype(np.float64) * SAW_AC) / 1.0, coverage.lnfact(SAW_P + 1))
    return int(np.unique(v.view(np.uint32)).size)


_SAW = {}


def sawtooth_length(m):
    """The smallest number of bases whose pair has ``m`` distinct values: the count never falls and rises by at most one per base."""
    if m not in _SAW:
        lo, hi = 1, 3 * m + 8                               # (about one new value per base and a half)
        assert sawtooth_distinct(hi) >= m
        while lo < hi:
            mid = (lo + hi) // 2
            if sawtooth_distinct(mid) >= m:
                hi = mid
            else:
                lo = mid + 1
        assert sawtooth_distinct(lo) == m, "no length gives %d distinct values" % m
        _SAW[m] = lo
    return _SAW[m]


def check_distinct(m, want):
    assert len(want["table"]) == m
