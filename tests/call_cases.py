"""Cases and the yardstick of the peak caller's tests (tests/test_coverage_call.py, tests/test_gpu_coverage_call.py).

The yardstick is the restatement below: plain Python loops over the rows ``(name, start0, end0, v)`` of a track, taken from the
restatements of ``signal_cases`` / ``compare_cases`` (``rows_of_want``).  It has its own pass / link / length / summit / score / text
rules and uses none of ``pymasc_amd.coverage``.

The definitions.  Within a reference the rows ascend and do not overlap; bases in no row are uncovered.  ``cutoff`` is a finite float,
``max_gap`` 0 .. 2^31 - 1, ``min_length`` 1 .. 2^31 - 1.  Values compare as floats (``float(v)``; ``-0.0 == 0.0``).  A row passes
when ``float(v) >= cutoff``.  Two consecutive passing rows ``a``, ``b`` of one reference are linked when ``b.start0 - a.end0 <=
max_gap``, whatever lies between; rows of different references are never linked.  A candidate is a maximal chain, from its first row's
``start0`` to its last row's ``end0``; it is a peak when ``end - start >= min_length``.  Per peak: ``value``, the largest ``v`` of its
passing rows; ``summit = s + (e - s) // 2`` of the first passing row ``(s, e)`` with that value; ``runs``, its passing rows.  Totals:
``passing_runs``, ``candidates``, ``peaks``, ``peak_bases`` (``end - start`` over the peaks), ``passing_bases`` (the widths of the
passing rows inside peaks).  The narrowPeak line of peak ``n`` (1-based in file order):
``chrom start end peak_<n> score . value -1 -1 (summit - start)``, TAB-separated; ``score = trunc(min(max(float(value) * 10.0, 0.0),
1000.0))``; ``value`` as ``compare_cases.text_value`` writes it.
"""
import numpy as np

from tests import bigwig_out_cases as BC
from tests import compare_cases as PC
from tests import coverage_cases as CC
from tests import signal_cases as SC

TOTALS = ("passing_runs", "candidates", "peaks", "peak_bases", "passing_bases")


def rows_of_want(want):
    """The rows (name, start0, end0, v) of what ``signal_cases.restate`` / ``compare_cases.restate`` returned, in file order."""
    return [(n, s, e, np.float32(v)) for n, rows in want["runs"].items() for s, e, v, _S in rows]


def restate(rows, cutoff, max_gap=30, min_length=200):
    """``peaks``: [(name, start, end, summit, value, runs), ...] in file order, and the five totals by name."""
    chains, cur = [], None                                  # a chain: the passing rows of a candidate
    passing = 0
    for name, s, e, v in rows:
        if not float(v) >= cutoff:
            continue
        passing += 1
        if cur is not None and cur[-1][0] == name and s - cur[-1][2] <= max_gap:
            cur.append((name, s, e, v))
        else:
            cur = [(name, s, e, v)]
            chains.append(cur)
    peaks, inside = [], 0
    for chain in chains:
        start, end = chain[0][1], chain[-1][2]
        if end - start < min_length:
            continue
        best = chain[0]
        for row in chain[1:]:
            if float(row[3]) > float(best[3]):              # strictly larger: the first of equal values stays
                best = row
        peaks.append((chain[0][0], start, end, best[1] + (best[2] - best[1]) // 2, best[3], len(chain)))
        for _n, s, e, _v in chain:
            inside += e - s
    return dict(peaks=peaks, passing_runs=passing, candidates=len(chains), n_peaks=len(peaks),
                peak_bases=sum(e - s for _n, s, e, _m, _v, _r in peaks), passing_bases=inside)


def totals(want):
    return dict(zip(TOTALS, (want["passing_runs"], want["candidates"], want["n_peaks"], want["peak_bases"], want["passing_bases"])))


def peaks_of(want):
    """Every peak as (name, start, end, summit, the bits of value, runs), in file order."""
    return [(n, s, e, m, int(np.float32(v).view(np.uint32)), r) for n, s, e, m, v, r in want["peaks"]]


def peaks_got(p):
    """``peaks_of`` of a ``pymasc_amd.coverage.Peaks``."""
    return [(n, int(a), int(b), int(c), int(d), int(f)) for n, (s, e, m, v, r) in p.rows.items()
            for a, b, c, d, f in zip(s, e, m, v.view(np.uint32), r)]


def score(v) -> int:
    x = float(v) * 10.0
    if not x > 0.0:
        x = 0.0
    if x > 1000.0:
        x = 1000.0
    return int(x)


def text_of(want, first=0, n=None) -> bytes:
    """The lines of the peaks ``[first, first + n)``."""
    rows = want["peaks"][first:] if n is None else want["peaks"][first:first + n]
    return "".join("%s\t%d\t%d\tpeak_%d\t%d\t.\t%s\t-1\t-1\t%d\n" % (name, s, e, first + i + 1, score(v), PC.text_value(v), m - s)
                   for i, (name, s, e, m, v, _r) in enumerate(rows)).encode()


def lines_of(want):
    """``{name: [(start, end), ...]}``: what ``Peaks.lines()`` gives."""
    out = {}
    for name, s, e, _m, _v, _r in want["peaks"]:
        out.setdefault(name, []).append((s, e))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# tracks planted as integer depth runs (ref, start0, end0, depth): ``depth`` forward reads [start0 + 1, end0] each, so that a BAM
# file of them piles up to exactly these runs (neighbouring runs differ in depth)
# ---------------------------------------------------------------------------------------------------------------------------------

def reads_of(track):
    """Rows (ref, pos1, read_len, reverse) in (ref, pos1) order."""
    return sorted((r, s + 1, e - s, 0) for r, s, e, d in track for _k in range(d))


def track_rows(reads, refs, B=1, scale=1.0):
    """The restated signal rows of ``reads`` at bin ``B``: through ``coverage_cases.restate`` and ``signal_cases.restate``."""
    use = [1] * len(refs)
    depths = BC.depth_lists(CC.restate(reads, refs, use, 0), refs, use)
    return rows_of_want(SC.restate(SC.bin_sums(depths, B), scale))


def compared_rows(reads_t, reads_c, refs, B, op, a_t=1.0, a_c=1.0, p=1.0):
    use = [1] * len(refs)
    sums = [SC.bin_sums(BC.depth_lists(CC.restate(x, refs, use, 0), refs, use), B) for x in (reads_t, reads_c)]
    return rows_of_want(PC.restate(*sums, op, a_t, a_c, p))


# the edges: cutoff 2 (depth 2 passes: equality), max_gap 10, min_length 50, at scale 1; and at scale 0.25 with the cutoff 0.5
E_REFS = [("q0", 1200), ("q1", 2000), ("q2", 400), ("q3", 300), ("q4", 20)]
E_ARGS = (2.0, 10, 50)
E_TRACK = [
    (0, 0, 30, 2), (0, 30, 40, 1), (0, 40, 60, 3),          # a failing run of 10 bases between: gap == max_gap, linked: [0, 60)
    (0, 71, 121, 4),                                        # 11 bases behind 60: max_gap + 1, not linked; 50 bases == min_length: kept
    (0, 200, 249, 5),                                       # 49 bases == min_length - 1: dropped
    (0, 300, 320, 7), (0, 320, 340, 9), (0, 340, 345, 1), (0, 345, 365, 9), (0, 365, 366, 2),     # two equal maxima: the first wins
    (0, 400, 460, 1),                                       # fails
    (0, 1140, 1200, 3),                                     # ends on the last base of q0 ...
    (1, 5, 65, 3),                                          # ... and q1 begins at 5: closer than max_gap by their numbers, two peaks
    (1, 100, 130, 2), (1, 140, 150, 6), (1, 160, 170, 2),   # uncovered gaps of 10: linked, [100, 170); the maximum in the middle
    (3, 10, 200, 1),                                        # q2 has no run; q3 only a failing one
    (4, 0, 20, 8),                                          # q4: a reference of 20 bases, all passing, below min_length
]


def check_edges(want):
    """The situations of ``E_TRACK`` with ``E_ARGS``, asserted from the restatement."""
    p = {(n, s, e): (m, float(v), r) for n, s, e, m, v, r in want["peaks"]}
    assert [k for k in p] == [("q0", 0, 60), ("q0", 71, 121), ("q0", 300, 366), ("q0", 1140, 1200), ("q1", 5, 65), ("q1", 100, 170)]
    assert p["q0", 0, 60] == (50, 3.0, 2)                   # linked across the failing run; v == cutoff passes
    assert p["q0", 71, 121] == (96, 4.0, 1)
    assert p["q0", 300, 366] == (330, 9.0, 4)               # the first of the two runs of 9: [320, 340)
    assert p["q1", 100, 170] == (145, 6.0, 3)
    assert want["candidates"] == 8 and want["passing_runs"] == 14      # [200, 249) and q4 are candidates, not peaks
    assert want["peak_bases"] == 60 + 50 + 66 + 60 + 60 + 70
    assert want["passing_bases"] == 50 + 50 + 61 + 60 + 60 + 50


# a signed pair for ``subtract`` at bin 1: treatment minus control
S_REFS = [("s0", 1000), ("s1", 500)]
S_ARGS = (-2.0, 10, 50)
S_TREATMENT = [(0, 0, 100, 1), (0, 300, 400, 2), (0, 600, 700, 3), (1, 0, 60, 1), (1, 100, 200, 1)]
S_CONTROL = [(0, 0, 50, 2), (0, 50, 100, 3), (0, 300, 400, 6), (0, 600, 650, 3), (0, 650, 700, 2), (1, 0, 60, 1), (1, 100, 200, 4)]


def check_signed(want):
    """treatment - control: s0 [0, 50) -1, [50, 100) -2 (== cutoff), [300, 400) -4 (fails), [600, 650) 0, [650, 700) 1; s1 [0, 60) 0,
    [100, 200) -3 (fails)."""
    p = {(n, s, e): (m, float(v), r) for n, s, e, m, v, r in want["peaks"]}
    assert list(p) == [("s0", 0, 100), ("s0", 600, 700), ("s1", 0, 60)]
    assert p["s0", 0, 100] == (25, -1.0, 2)                 # every value negative: the largest is -1
    text = text_of(want).decode().split("\n")
    assert text[0] == "s0\t0\t100\tpeak_1\t0\t.\t-1\t-1\t-1\t25"      # score 0, the value's text begins with '-'
    assert text[1] == "s0\t600\t700\tpeak_2\t10\t.\t1\t-1\t-1\t75"
    assert text[2] == "s1\t0\t60\tpeak_3\t0\t.\t0\t-1\t-1\t30"


# the long chain: 5000 forward reads of 3 bases at 1, 3, 5, ...: depth 1 on [0, 2), then 2 and 1 in turn, one base each, and 1 on the
# last two bases: 9999 runs, of which the 4999 on the even bases 2 .. 9998 have depth 2
L_REFS = [("long", 10_100), ("after", 100)]
L_READS = [(0, 1 + 2 * k, 3, 0) for k in range(5000)]
L_CASES = [(1.0, 0, 200), (2.0, 1, 200), (2.0, 0, 2), (2.0, 0, 1)]


def check_long(rows, want, args):
    assert len(rows) == 9999 and [(s, e, float(v)) for _n, s, e, v in rows[:3]] == [(0, 2, 1.0), (2, 3, 2.0), (3, 4, 1.0)]
    assert rows[-1][1:3] == (9999, 10_001)
    if args == (1.0, 0, 200):                               # one peak of more runs than a scan tile of 4096, over many workgroups
        assert peaks_of(want) == [("long", 0, 10_001, 2, int(np.float32(2.0).view(np.uint32)), 9999)]
    if args == (2.0, 1, 200):                               # every passing run a base from the next
        assert [(s, e, m, r) for _n, s, e, m, _v, r in want["peaks"]] == [(2, 9999, 2, 4999)]
    if args == (2.0, 0, 2):
        assert want["candidates"] == 4999 and want["n_peaks"] == 0
    if args == (2.0, 0, 1):
        assert want["candidates"] == 4999 and want["n_peaks"] == 4999 and want["passing_bases"] == 4999


def summit_reads(at, twice=None):
    """The long chain with one more read on the passing run number ``at`` of cutoff 2 (the base 2 + 2 * at: depth 3 there), and with
    ``twice`` another one on that passing run: two equal maxima."""
    more = [(0, 3 + 2 * k, 1, 0) for k in ([at] if twice is None else [at, twice])]
    return sorted(L_READS + more)


# (at, twice): the maximum in the first and in the last run of the peak, either side of a wave's and of a workgroup's end in the
# passing list, and two equal maxima either side of them: the first one wins
SUMMITS = [(0, None), (4998, None), (63, None), (64, None), (255, None), (256, None), (63, 64), (255, 256), (64, 4000)]


def check_summit(want, at):
    assert [(s, e, m, float(v), r) for _n, s, e, m, v, r in want["peaks"]] == [(2, 9999, 2 + 2 * at, 3.0, 4999)]


# boundaries in the three lists: ``f`` failing runs, then units of one passing run each with one uncovered base between; unit ``k``
# is three abutting runs of depth 2, 3, 2.  With max_gap 0 every unit is a candidate, so the chain of three begins at element
# ``k + f`` of the runs, ``k`` of the passing list and ``k`` of the candidates, and ends two elements on
B_REFS = [("b0", 2000), ("b1", 50)]
B_ARGS = [(2.0, 0, 1), (2.0, 0, 3)]
BOUNDARIES = [(k, f) for k in (63, 64, 255, 256) for f in (0, 7)]


def boundary_track(k, f):
    track, at = [], 0
    for _i in range(f):
        track.append((0, at, at + 2, 1))
        at += 3
    for u in range(k + 3):
        if u == k:
            track += [(0, at, at + 2, 2), (0, at + 2, at + 4, 3), (0, at + 4, at + 6, 2)]
            at += 7
        else:
            track.append((0, at, at + 2, 2))
            at += 3
    assert at < B_REFS[0][1]
    return track


def check_boundary(want, k, f, args):
    chain = [(i, p) for i, p in enumerate(want["peaks"]) if p[5] == 3]
    assert len(chain) == 1 and want["candidates"] == k + 3 and want["passing_runs"] == k + 5
    i, (_n, s, e, m, v, _r) = chain[0]
    assert (e - s, m - s, float(v)) == (6, 3, 3.0) and s == 3 * (f + k)
    assert (i, want["n_peaks"]) == ((k, k + 3) if args[2] == 1 else (0, 1))
