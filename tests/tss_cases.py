"""Cases and the yardstick of the anchor-profile tests (tests/test_tss.py, tests/test_gpu_tss.py).

The yardstick is ``restate``, on plain ints, written here and nowhere in the package.  The definitions it restates: an anchor is
``(reference, a, s)``, a 1-based position and a strand; a read's extent is ``L = extend`` bases (its own length at 0) from its 5' end
-- forward ``[pos1, pos1 + L - 1]``, reverse ``[pos1 + read_len - L, pos1 + read_len - 1]`` -- clipped to ``[1, len]``; for an anchor
on its reference the read covers the offsets ``o = s * (p - a)`` for ``p`` in ``[lo, hi]`` with ``|o| <= F``; every such ``o`` adds 1
to ``same[o + F]`` when the read's strand equals the anchor's, to ``opposite[o + F]`` otherwise; ``pairs`` counts the (read, anchor)
pairs with at least one such offset, ``n_near`` the reads in at least one pair, ``N`` every kept read on a chosen reference, and
``anchors`` the anchors on chosen references.

``restate_literal`` is the definition as it reads: a triple loop over reads, anchors and bases.  At ``F = 4095`` and ``extend =
1300`` this library holds about half a million pairs of more than a thousand bases each, 10^9 steps of the innermost loop, so
``restate`` takes the same sums in another order: a loop over reads and bases piles the reads up per strand, a loop over anchors
and offsets reads the pile, and a loop over reads and anchors counts the pairs.  Both are exact; ``tests/test_tss.py`` holds them
to each other wherever the literal loop is affordable.
"""
import bisect

import numpy as np

from tests import fingerprint_cases as FC
from tests import peaks_cases as PC

REFS = PC.REFS                      # f0 100 003, f1 499, f2 70 001 bases
MAPQ = FC.MAPQ
FLANKS = (1, 50, 2000, 4095)
EXTENDS = (0, 1, 1300)
USES = PC.USES
MASK = {"f0": [(11_990, 12_020), (50_000, 50_400)], "f2": [(10_000, 10_050)]}          # 0-based, half-open; the first lies on OPPOSED
MISSING = PC.MISSING
READ = 36                           # the length of every planted read

F0, F1, F2 = (l for _n, l in REFS)
ENDS = [(1, "+"), (1, "-"), (F0, "+"), (F0, "-")]                   # windows clipped by the chromosome's ends
ON_F1 = [(250, "+"), (10, "-")]                                     # at F = 2000 the window is wider than the reference
OPPOSED = [(12_000, "+"), (12_000, "-")]                            # one position, both strands
TWIN = [(15_000, "+"), (15_000, "+")]                               # the same anchor twice
CLUSTER = [(30_000 + k // 3, "+-"[k % 2]) for k in range(300)]      # 300 anchors within 100 bases
EDGE = [(40_000, "+"), (45_000, "-")]                               # the planted edge reads are placed against these two
EMPTY_ABOVE = 50_000                # no anchor on f0 between here and its last base


def anchor_sites(seed=21):
    """An ordered ``{name: [(a, strand), ...]}`` in an unsorted order: the planted anchors and about 150 random ones."""
    rng = np.random.default_rng(seed)
    rows = [("f0", x) for x in ENDS + OPPOSED + TWIN + CLUSTER + EDGE] + [("f1", x) for x in ON_F1]
    for name, lo, hi, n in (("f0", 2_000, EMPTY_ABOVE, 90), ("f2", 1, F2 + 1, 60)):
        rows += [(name, (int(a), "+-"[int(s)])) for a, s in zip(rng.integers(lo, hi, size=n), rng.integers(0, 2, size=n))]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    out = {}
    for name, site in rows:
        out.setdefault(name, []).append(site)
    return out


def many_sites(n=3000, seed=22):
    """``n`` anchors on f0 alone, unsorted: several anchors in reach of every read."""
    rng = np.random.default_rng(seed)
    return {"f0": [(int(a), "+-"[int(s)]) for a, s in zip(rng.integers(1, F0 + 1, size=n), rng.integers(0, 2, size=n))]}


def edge_reads(a, flank, extend, reverse):
    """Four planted reads (pos1, READ, reverse) against the anchor position ``a``: their extent ends exactly at ``a + F`` and at
    ``a + F + 1``, and begins exactly at ``a - F`` and at ``a - F - 1``."""
    span = extend if extend else READ
    out = []
    for hi in (a + flank, a + flank + 1):
        out.append((hi - READ + 1 if reverse else hi - span + 1, READ, reverse))
    for lo in (a - flank, a - flank - 1):
        out.append((lo - READ + span if reverse else lo, READ, reverse))
    return out


def synthetic():
    """Rows (ref, pos1, read_len, reverse, mapq) in (ref, pos1) order: ``peaks_cases.synthetic()`` and the planted edge reads (all
    at MAPQ 40) for every flank and extend, on both read strands, against anchors of both strands."""
    rows = PC.synthetic()
    plant = [(0, p, l, s, 40) for (a, _s) in EDGE for f in FLANKS for e in EXTENDS for s in (0, 1) for p, l, s in edge_reads(a, f, e, s)]
    assert all(p >= 1 for _r, p, _l, _s, _q in plant)
    rows = np.concatenate([rows, np.array(plant, dtype=np.int64)])
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def few(rows, n=600, seed=3):
    return PC.few(rows, n, seed)


def extent(pos1, read_len, reverse, extend, length):
    return PC.extent(pos1, read_len, reverse, extend, length)


def restate_literal(reads, refs, use, anchors, flank, extend):
    """The definition as a triple loop over reads, anchors and bases."""
    width = 2 * flank + 1
    same, opposite = [0] * width, [0] * width
    n = n_near = pairs = 0
    for ref, pos1, read_len, reverse in reads:
        name, length = refs[ref]
        if not use[ref]:
            continue
        n += 1
        lo, hi = extent(pos1, read_len, reverse, extend, length)
        mine = 0
        for a, strand in anchors.get(name, []):
            sign = 1 if strand == "+" else -1
            row = same if (strand == "-") == bool(reverse) else opposite
            hit = False
            for p in range(lo, hi + 1):
                o = sign * (p - a)
                if -flank <= o <= flank:
                    row[o + flank] += 1
                    hit = True
            mine += hit
        pairs += mine
        n_near += mine > 0
    count = sum(len(anchors.get(name, [])) for (name, _l), u in zip(refs, use) if u)
    return dict(same=same, opposite=opposite, N=n, n_near=n_near, pairs=pairs, anchors=count)


def restate_by_reference(reads, refs, anchors, flank, extend):
    """Per reference, the dict of ``restate`` for that reference alone (see the module's docstring for the order of the loops)."""
    width = 2 * flank + 1
    out = []
    for ref, (name, length) in enumerate(refs):
        sites = anchors.get(name, [])
        spots = sorted(a for a, _s in sites)
        pile = [{}, {}]                     # the depth of forward / reverse reads at every position that has any
        n = n_near = pairs = 0
        for r, pos1, read_len, reverse in reads:
            if r != ref:
                continue
            n += 1
            lo, hi = extent(pos1, read_len, reverse, extend, length)
            if lo > hi:
                continue
            row = pile[1 if reverse else 0]
            for p in range(lo, hi + 1):
                row[p] = row.get(p, 0) + 1
            mine = bisect.bisect_right(spots, hi + flank) - bisect.bisect_left(spots, lo - flank)   # a with a - F <= hi and a + F >= lo
            pairs += mine
            n_near += mine > 0
        same, opposite = [0] * width, [0] * width
        for a, strand in sites:
            sign, minus = (1, 0) if strand == "+" else (-1, 1)
            for o in range(-flank, flank + 1):
                p = a + sign * o
                same[o + flank] += pile[minus].get(p, 0)
                opposite[o + flank] += pile[1 - minus].get(p, 0)
        out.append(dict(same=same, opposite=opposite, N=n, n_near=n_near, pairs=pairs, anchors=len(sites)))
    return out


def combine(parts, use):
    """The chosen references' parts of ``restate_by_reference`` added up."""
    chosen = [p for p, u in zip(parts, use) if u]
    out = {k: sum(p[k] for p in chosen) for k in ("N", "n_near", "pairs", "anchors")}
    for k in ("same", "opposite"):
        out[k] = [sum(col) for col in zip(*(p[k] for p in chosen))]
    return out


def restate(reads, refs, use, anchors, flank, extend):
    """``reads``: rows (ref, pos1, read_len, reverse); ``anchors``: ``{name: [(a, "+" | "-"), ...]}``.  A dict: ``same`` /
    ``opposite`` (lists of ``2 * flank + 1`` ints), ``N``, ``n_near``, ``pairs``, ``anchors``."""
    return combine(restate_by_reference(reads, refs, anchors, flank, extend), use)


def statistics(want, flank):
    """(background, normalized, enrichment, at_tss, peak_offset) by the formula, on the restated ints."""
    width = 2 * flank + 1
    total = [s + o for s, o in zip(want["same"], want["opposite"])]
    edge = max(1, min(100, flank // 4))
    edge_sum = sum(total[:edge]) + sum(total[width - edge:])
    background = edge_sum / (2 * edge)
    if edge_sum == 0:
        return background, None, None, None, None
    normalized = [t / background for t in total]
    best = max(normalized)
    return background, normalized, best, normalized[flank], normalized.index(best) - flank


def check_situations(reads, refs, anchors, want, flank, extend):
    """Asserts, from the restatement ``want`` (all references chosen) and plain arithmetic, that the cases bite for these parameters."""
    width = 2 * flank + 1
    assert 0 < want["n_near"] < want["N"] == len(reads) and want["pairs"] > want["n_near"]
    assert want["same"] != want["opposite"] and want["anchors"] == sum(len(v) for v in anchors.values())
    if flank == 50:
        assert all(row[0] > 0 and row[-1] > 0 for row in (want["same"], want["opposite"]))
    f0 = anchors["f0"]
    assert all(x in f0 for x in ENDS + OPPOSED + CLUSTER + EDGE) and f0.count(TWIN[0]) == 2
    assert max(a for a, _s in CLUSTER) - min(a for a, _s in CLUSTER) < 100 and len(CLUSTER) == 300
    assert not any(EMPTY_ABOVE < a < F0 for a, _s in f0) and len(anchors["f1"]) == 2 and 2 * 2000 + 1 > F1
    assert any(x[0] > y[0] for x, y in zip(f0, f0[1:]))                                 # an unsorted order
    assert sum(1 for r in reads if r[0] == 0 and EMPTY_ABOVE + 4095 + 1300 < r[1] < F0 - 4095 - 1300 - 101) > 2 * 1024
    # the edge reads: against a single anchor, the read one base further out covers exactly one offset less (none less when its
    # extent is wider than the window: both are clipped on the far side too)
    span = extend if extend else READ
    present = {tuple(r) for r in reads}
    for a, strand in EDGE:
        for reverse in (0, 1):
            four = [(0,) + r for r in edge_reads(a, flank, extend, reverse)]
            assert all(r in present for r in four)
            bases = [sum(x["same"]) + sum(x["opposite"]) for x in
                     (restate_literal([r], refs, [1, 1, 1], {"f0": [(a, strand)]}, flank, extend) for r in four)]
            assert bases[0] == min(span, width) and bases[2] == min(span, width)
            assert bases[0] - bases[1] == bases[2] - bases[3] == (1 if span <= width else 0)
            ends = [extent(r[1], r[2], r[3], extend, F0) for r in four]
            assert [ends[0][1], ends[1][1], ends[2][0], ends[3][0]] == [a + flank, a + flank + 1, a - flank, a - flank - 1]


def bed_text(anchors):
    """The anchors as BED6 lines of a few bases each, the names interleaved: a ``+`` anchor is the line's start + 1, a ``-`` anchor
    its end."""
    rows = [(n, a, s) for n, sites in anchors.items() for a, s in sites]
    for i in np.random.default_rng(2).permutation(len(rows)):
        n, a, s = rows[i]
        start, end = (a - 1, a + 9) if s == "+" else (a - min(a, 7), a)
        yield "{}\t{}\t{}\tsite{}\t0\t{}\n".format(n, start, end, i, s)
