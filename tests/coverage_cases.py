"""Cases and the yardstick of the coverage tests (tests/test_coverage.py, tests/test_gpu_coverage.py).

The yardstick is ``restate``: a Python loop that adds 1 to a per-base list for every base of every read's clipped extent and then
walks the list base by base into runs.  It is written here and nowhere in the package, and uses no running sum.

The definitions (this project's own).  The reads are the ones the correlation sees: the filter, the chosen references, less the
reads an exclude mask drops.  ``L = extend``, or the read's own length at 0; a forward read covers ``[pos1, pos1 + L - 1]``, a
reverse read ``[pos1 + read_len - L, pos1 + read_len - 1]``; the extent is clipped to ``[1, len]`` of its reference; a read with
nothing left adds nothing and is not in ``reads``.  ``depth[r][p]`` is the number of kept reads whose clipped extent holds position
``p``.  Per chosen reference, in header order, the maximal intervals of constant depth above 0 are the runs ``(start0, end0,
depth)``, 0-based and half-open; reads that abut at equal depth form one run; depth 0 is no run.  Totals: ``reads``, ``runs``,
``covered_bases = sum (end0 - start0)``, ``fragment_bases = sum depth * (end0 - start0)``, ``max_depth``.
"""
import numpy as np

from pymasc_amd import coverage
from tests import fingerprint_cases as FC

T = coverage.TILE                                   # slots per scan tile of the device code; slot = pos1 - 1 = start0
REFS = FC.REFS + [("f3", 8191)]                     # f3: no read at all
USES = {"all": [1, 1, 1, 1], "no middle": [1, 0, 1, 1]}
EXTENDS = (0, 200, 1300)
MAPQ = FC.MAPQ
RL = 36                                             # the planted reads' length unless a row says otherwise
MASK = {"f0": [(19_990, 20_010)], "f2": [(10_000, 10_050)]}      # 0-based, half-open
MASKED_READ = (0, 20_000, RL, 0)
PILE = (2, 60_000, 5000)                            # (ref, pos1, reads), forward
GROUPS = {36: 22_000, 200: 34_000, 1300: 46_000}    # on f0: where the reads planted for the span L begin
assert T == 4096                                    # the positions below are laid out for it


def span(extend):
    return extend if extend > 0 else RL


def planted():
    """Rows (ref, pos1, read_len, reverse), see ``check_situations``."""
    rows = [MASKED_READ]
    rows += [(0, 1, 9, 1), (0, 1, 10, 1), (0, 11, RL, 0), (0, 11, RL, 0)]                   # ends and starts at 9 and 10; below position 1
    for L, b in GROUPS.items():
        rows += [(0, b, RL, 0), (0, b + L, RL, 0)]                                           # abut
        rows += [(0, b + 4000, RL, 0), (0, b + 4000 + L - 1, RL, 0)]                         # overlap by one base
        rows += [(0, b + 8000, RL, 0), (0, b + 8000 + L - RL, RL, 1)]                        # both strands, the same extent
    rows += [(0, 15 * T - 9, RL, 0)]                                                         # across a tile's edge
    rows += [(0, 16 * T + 1, RL, 0)]                                                         # begins on a tile's first slot
    rows += [(0, 18 * T - 1 - RL + 1, RL, 1)]                                                # its -1 lands on a tile's last slot
    rows += [(0, 19 * T - RL + 1, RL, 1)]                                                    # its last base is a tile's last slot; tiles 20, 21 empty
    rows += [(0, 90_200, RL, 0)] * 99 + [(0, 90_205, RL, 0)]                                 # depth 99 -> 100
    rows += [(0, 92_200, RL, 0)] * 9 + [(0, 92_205, RL, 0)]                                  # depth 9 -> 10
    rows += [(0, 99_999 - RL + 1, RL, 1), (0, 100_000 - RL + 1, RL, 1)]                      # ends at 99 999 and 100 000
    rows += [(0, 100_001, RL, 0)] * 2                                                        # past the end: clipped onto the closing slot
    rows += [(1, REFS[1][1], RL, 0), (2, 1, RL, 0)]                                          # f1's last base, f2's first
    rows += [(PILE[0], PILE[1], RL, 0)] * PILE[2]
    return rows


def synthetic(seed=11, n=17_000):
    """Rows (ref, pos1, read_len, reverse, mapq) in (ref, pos1) order: ``n`` reads on the front of f0, on f1 and on the front of
    f2, both strands, several lengths, MAPQs either side of MAPQ, and the planted reads (all at MAPQ 40)."""
    rng = np.random.default_rng(seed)
    lens = np.array([36, 35, 50, 101])
    rows = []
    for ref, lo, hi, share in ((0, 3_000, 18_000, 0.5), (1, 40, 300, 0.004), (2, 1_400, 50_000, 0.496)):
        m = int(n * share)
        rows.append(np.stack([np.full(m, ref), rng.integers(lo, hi, size=m), rng.choice(lens, size=m, p=[0.7, 0.1, 0.1, 0.1]),
                              rng.integers(0, 2, size=m),
                              np.where(rng.random(m) < 0.15, rng.integers(0, MAPQ, size=m), rng.integers(MAPQ, 61, size=m))], axis=1))
    rows.append(np.array([r + (40,) for r in planted()], dtype=np.int64))
    rows = np.concatenate(rows)
    rows = rows[rng.permutation(len(rows))]
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def tile_case(seed=12, n=400):
    """(refs, kept reads): three references one base shorter than, exactly, and one base longer than two tiles, with reads over
    all of them and on their first and last bases."""
    rng = np.random.default_rng(seed)
    refs = [("t0", 2 * T - 1), ("t1", 2 * T), ("t2", 2 * T + 1)]
    reads = []
    for r, (_n, length) in enumerate(refs):
        reads += [(r, int(p), int(l), int(s)) for p, l, s in zip(rng.integers(1, length + 1, size=n), rng.choice([36, 50], size=n),
                                                                  rng.integers(0, 2, size=n))]
        reads += [(r, 1, 36, 0), (r, length, 36, 0), (r, length - 35, 36, 1), (r, T, 36, 0), (r, T + 1, 36, 1), (r, 2 * T - 40, 36, 0)]
    return refs, sorted(reads)


def extent(pos1, read_len, reverse, extend):
    L = extend if extend > 0 else read_len
    return (pos1 + read_len - L, pos1 + read_len - 1) if reverse else (pos1, pos1 + L - 1)


def restate(reads, refs, use, extend):
    """``reads`` = rows (ref, pos1, read_len, reverse).  Returns ``runs``: {name: [(start0, end0, depth), ...]} of the chosen
    references that have a run, in header order; the five totals by name; ``extents``: the sum of the clipped extents' lengths."""
    depth = [[0] * (length + 2) if u else None for (_n, length), u in zip(refs, use)]      # depth[r][p], p = 1 .. len; [0], [len + 1] stay 0
    added = extents = 0
    for ref, pos1, read_len, reverse in reads:
        if depth[ref] is None:
            continue
        lo, hi = extent(pos1, read_len, reverse, extend)
        lo, hi = max(lo, 1), min(hi, refs[ref][1])
        if lo > hi:
            continue
        added += 1
        extents += hi - lo + 1
        row = depth[ref]
        for p in range(lo, hi + 1):
            row[p] += 1
    runs = {}
    for (name, length), row in zip(refs, depth):
        if row is None:
            continue
        out, start = [], None
        for p in range(1, length + 2):
            if start is not None and row[p] != row[start]:
                out.append((start - 1, p - 1, row[start]))
                start = None
            if start is None and row[p] > 0:
                start = p
        if out:
            runs[name] = out
    flat = [r for v in runs.values() for r in v]
    return dict(runs=runs, reads=added, n_runs=len(flat), covered_bases=sum(e - s for s, e, _d in flat),
                fragment_bases=sum((e - s) * d for s, e, d in flat), max_depth=max((d for _s, _e, d in flat), default=0), extents=extents)


def select(want, refs, reads, use, extend):
    """The restatement over fewer references: a reference's runs do not depend on the others, so only the totals are taken again,
    from the runs that are left and, for ``reads``, from a loop over the reads."""
    runs = {n: v for n, v in want["runs"].items() if use[[x for x, _l in refs].index(n)]}
    flat = [r for v in runs.values() for r in v]
    added = 0
    for ref, pos1, read_len, reverse in reads:
        lo, hi = extent(pos1, read_len, reverse, extend)
        added += bool(use[ref]) and max(lo, 1) <= min(hi, refs[ref][1])
    return dict(runs=runs, reads=added, n_runs=len(flat), covered_bases=sum(e - s for s, e, _d in flat),
                fragment_bases=sum((e - s) * d for s, e, d in flat), max_depth=max((d for _s, _e, d in flat), default=0),
                extents=sum((e - s) * d for s, e, d in flat))


def totals(want):
    return want["reads"], want["n_runs"], want["covered_bases"], want["fragment_bases"], want["max_depth"]


def rows_of(want):
    """Every run as (name, start0, end0, depth), in file order."""
    return [(n, *r) for n, v in want["runs"].items() for r in v]


def text_of(want) -> bytes:
    return "".join("%s\t%d\t%d\t%d\n" % r for r in rows_of(want)).encode()


def as_coverage(want, extend):
    return coverage.Coverage({n: tuple(zip(*v)) for n, v in want["runs"].items()}, want["reads"], extend)


def check_situations(reads, want, extend):
    """The planted situations of the issue, each asserted from the restatement of the whole library (every reference, no mask)."""
    L = span(extend)
    f0, f1, f2 = (want["runs"][n] for n in ("f0", "f1", "f2"))
    s0 = set(f0)
    b = GROUPS[L]
    assert (b - 1, b - 1 + 2 * L, 1) in s0                                      # two reads that abut: one run
    assert (b + 3999 + L - 1, b + 3999 + L, 2) in s0                            # two that overlap by one base
    assert (b + 7999, b + 7999 + L, 2) in s0                                    # a forward and a reverse read with the same extent
    assert f0[:3] == [(0, 9, 2), (9, 10, 1), (10, 10 + L, 2)]                   # starts and ends 9 -> 10; clipped at position 1
    if extend:
        assert any(s and p + l - extend < 1 for r, p, l, s in reads if r == 0)  # a reverse extension below position 1
    assert f0[-3:] == [(100_000 - L, 99_999, 2), (99_999, 100_000, 1), (100_000, 100_003, 2)]   # 99 999 -> 100 000; clipped onto the closing slot
    assert any(not s and p + (extend or l) - 1 > 100_003 for r, p, l, s in reads if r == 0)
    assert f1[-1][1] == 499 and f2[0][0] == 0                                   # f1's last base in front of f2's first: nothing carries
    assert f2[0][2] == sum(1 for r, p, l, s in reads if r == 2 and max(extent(p, l, s, extend)[0], 1) <= 1 <= extent(p, l, s, extend)[1])
    assert (15 * T - 10, 15 * T - 10 + L, 1) in s0 and 15 * T - 10 < 15 * T < 15 * T - 10 + L    # a run across a tile's edge
    assert (16 * T, 16 * T + L, 1) in s0                                        # a read that begins on a tile's first slot
    assert (18 * T - 1 - L, 18 * T - 1, 1) in s0                                # one whose -1 lands on a tile's last slot
    assert (19 * T - L, 19 * T, 1) in s0                                        # one whose last base is a tile's last slot
    after = [r for r in f0 if r[0] >= 19 * T]
    assert after[0][0] == 90_199 and after[0][0] - 19 * T > 2 * T               # whole tiles without a read between two runs
    assert not any(s < 22 * T and e > 20 * T for s, e, _d in f0)
    assert (PILE[1] - 1, PILE[1] - 1 + L, PILE[2]) in set(f2) and want["max_depth"] == PILE[2]   # a pile of 5000 at one position
    assert (90_199, 90_204, 99) in s0 and (90_204, 90_199 + L, 100) in s0       # depth 99 -> 100
    assert (92_199, 92_204, 9) in s0 and (92_204, 92_199 + L, 10) in s0         # depth 9 -> 10
    assert "f3" not in want["runs"]                                             # a reference without reads has no run
    assert MASKED_READ in reads and MASKED_READ not in FC.masked(reads, REFS, MASK)        # a read the mask leaves out
    assert want["fragment_bases"] == want["extents"]                            # the identity of the totals


# ---------------------------------------------------------------------------------------------------------------------------------
# the shapes of the output kernels (the line writer, the sections, the zoom records): isolated short reads a few
# bases apart, a few hundred runs
# ---------------------------------------------------------------------------------------------------------------------------------

OUT_REFS = [("c", 400), ("chromosome12", 2400)]                 # names of 1 and of 12 characters
OUT_SHORT, OUT_LONG = 43, 490                                   # their runs: the reference changes at run 43
OUT_READS = sorted([(0, 1 + 8 * k, 3, 0) for k in range(OUT_SHORT) for _d in range(1 + k % 3)] +
                   [(1, 1 + 4 * k, 2, 0) for k in range(OUT_LONG) for _d in range(1 + k % 4)])
OUT_FIRST = 3                                                   # a pull begins at the fourth row ...
OUT_COUNTS = (1, 63, 64, 65, 255, 256, 257, 513)                # ... and ends on lane 63, on a workgroup's edge, in the third workgroup
OUT_SECTION_COUNTS, OUT_ITEMS = (1, 255, 256, 257), (1, 3, 256, 257, 1024)
OUT_ZOOM, OUT_KEPT = 16, (1, 256, 257)                          # the bins of a zoom level that hold a base: every other bin of 16


def check_line_pulls(pull, whole: bytes, names=OUT_REFS) -> None:
    """``pull(first, n)`` against the same lines of ``whole`` for every count of ``OUT_COUNTS``; the reference changes on line 43,
    which is lane 40 of a pull's first wave."""
    lines = whole.splitlines(True)
    assert len(lines) >= OUT_FIRST + max(OUT_COUNTS)
    assert lines[OUT_SHORT - 1].startswith(names[0][0].encode() + b"\t") and lines[OUT_SHORT].startswith(names[1][0].encode() + b"\t")
    for n in OUT_COUNTS:
        assert pull(OUT_FIRST, n) == b"".join(lines[OUT_FIRST:OUT_FIRST + n]), n


def zoom_reads(kept: int):
    """Reads on ``OUT_REFS[1]`` lengthened to hold them: ``kept`` bins of ``OUT_ZOOM`` bases hold one, an empty bin between two."""
    refs = [OUT_REFS[0], (OUT_REFS[1][0], 2 * OUT_ZOOM * kept + 5)]
    return refs, [(1, 4 + 2 * OUT_ZOOM * k, 2, 0) for k in range(kept) for _d in range(1 + k % 3)]
