"""Cases and the yardstick of the peak-count tests (tests/test_peaks.py, tests/test_gpu_peaks.py).

The yardstick is ``restate``: a Python double loop over reads and lines on plain ints, written here and nowhere in the package.
The definitions it restates: a line ``(b, e)`` is 0-based and half-open and is clipped to its reference's length; a read's extent is
``L = extend`` bases (its own length at 0) from its 5' end -- forward ``[pos1, pos1 + L - 1]``, reverse ``[pos1 + read_len - L,
pos1 + read_len - 1]`` -- clipped to ``[1, len]``; the read is in the line when ``b + 1 <= hi and lo <= e``; ``N`` counts every kept
read on a chosen reference, ``n_in`` those in at least one line, once each.
"""
import numpy as np

from tests import fingerprint_cases as FC

REFS = FC.REFS                      # f0 100 003, f1 499, f2 70 001 bases
MAPQ = FC.MAPQ
EXTENDS = (0, 200, 1300)
USES = {"all": [1, 1, 1], "no middle": [1, 0, 1]}
MASK = {"f0": [(8_340, 8_360), (50_000, 50_400)], "f2": [(10_000, 10_050)]}          # 0-based, half-open
MISSING = "zz"                      # a name the header lacks

EDGE = (1_000, 1_200)               # reads end on its first base and a base short of it, begin on its last base and behind it
TWINS = (5_000, 5_300)              # twice in the file
TRIPLE = [(8_000, 8_400), (8_200, 8_600), (8_300, 8_900)]
NEST = (20_000, 30_000)             # nests INNER; reads at its far end walk past all of them
INNER = [(20_100 + 200 * k, 20_150 + 200 * k) for k in range(40)]
ABUT = [(40_000, 40_100), (40_100, 40_200)]
PAIR = [(45_000, 45_010), (45_020, 45_030)]                                            # a read of 36 bases spans both
CLIPPED = (99_900, 100_500)         # past the end of f0
BEYOND = (100_100, 100_200)         # wholly past it
FRONT = (0, 50)                     # a reverse read extended below position 1 still reaches it
LAST_OF_F1 = (450, 499)
FIRST_OF_F2 = (0, 40)


def peak_lines(seed=11):
    """An ordered ``{name: [(start, end), ...]}`` in an unsorted file order: the planted lines and about 200 random ones."""
    rng = np.random.default_rng(seed)
    rows = [("f0", x) for x in [EDGE, TWINS, TWINS, NEST, CLIPPED, BEYOND, FRONT] + TRIPLE + INNER + ABUT + PAIR]
    rows += [("f1", LAST_OF_F1), ("f1", (100, 160)), ("f2", FIRST_OF_F2), (MISSING, (10, 20)), (MISSING, (5, 9))]
    for name, top, n in (("f0", 99_000, 110), ("f2", 69_000, 100)):
        starts = rng.integers(50_000 if name == "f0" else 100, top, size=n)
        rows += [(name, (int(s), int(s) + int(w))) for s, w in zip(starts, rng.integers(50, 500, size=n))]
    rows = [rows[i] for i in rng.permutation(len(rows))]
    out = {}
    for name, iv in rows:
        out.setdefault(name, []).append(iv)
    return out


def many_lines(n=3000, seed=12):
    """``n`` lines on f0 alone, unsorted, many overlapping: more than the 1024 threads of the merge workgroup, several each."""
    rng = np.random.default_rng(seed)
    starts = rng.integers(0, 99_000, size=n)
    return {"f0": [(int(s), int(s) + int(w)) for s, w in zip(starts, rng.integers(20, 900, size=n))]}


def synthetic(seed=7, n=20_000):
    """Rows (ref, pos1, read_len, reverse, mapq) in (ref, pos1) order: ``n`` reads anywhere on the three references, both strands,
    several lengths, MAPQs either side of MAPQ, and the planted reads (all at MAPQ 40)."""
    rng = np.random.default_rng(seed)
    lens = np.array([36, 35, 50, 101])
    rows = []
    for ref, hi, share in ((0, 99_990, 0.6), (1, 470, 0.01), (2, 69_990, 0.39)):
        m = int(n * share)
        rows.append(np.stack([np.full(m, ref), rng.integers(1, hi, size=m), rng.choice(lens, size=m, p=[0.7, 0.1, 0.1, 0.1]),
                              rng.integers(0, 2, size=m),
                              np.where(rng.random(m) < 0.15, rng.integers(0, MAPQ, size=m), rng.integers(MAPQ, 61, size=m))], axis=1))
    b, e = EDGE
    plant = [(0, b + 1 - 35, 36, 0), (0, b - 35, 36, 0), (0, e, 36, 0), (0, e + 1, 36, 0)]
    plant += [(0, b + 1 - 35, 36, 1), (0, b - 35, 36, 1), (0, e, 36, 1), (0, e + 1, 36, 1)]
    plant += [(0, 3, 36, 1), (0, 60, 36, 1), (0, 8_350, 36, 0), (0, 8_350, 36, 1), (0, 5_100, 36, 0)]
    plant += [(0, p, 36, s) for p in range(29_000, 29_900, 30) for s in (0, 1)]         # the far end of NEST
    plant += [(0, 45_005, 36, 0), (0, 40_090, 36, 0), (0, 99_990, 36, 0), (0, 100_003, 36, 1), (0, 99_950, 101, 0)]
    plant += [(1, 440, 36, 0), (1, 480, 36, 0), (1, 499, 36, 1), (2, 1, 36, 0), (2, 30, 36, 1), (2, 41, 36, 0)]
    rows.append(np.array([r + (40,) for r in plant], dtype=np.int64))
    rows = np.concatenate(rows)
    rows = rows[rng.permutation(len(rows))]
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


def few(rows, n=600, seed=3):
    """``n`` of the rows of ``synthetic`` on f0, in order: the reads of the ``many_lines`` case."""
    rows = rows[rows[:, 0] == 0]
    pick = np.sort(np.random.default_rng(seed).choice(len(rows), size=n, replace=False))
    return rows[pick]


def extent(pos1, read_len, reverse, extend, length):
    span = extend if extend > 0 else read_len
    lo, hi = (pos1 + read_len - span, pos1 + read_len - 1) if reverse else (pos1, pos1 + span - 1)
    return max(lo, 1), min(hi, length)


def restate(reads, refs, use, peaks, extend):
    """``reads``: rows (ref, pos1, read_len, reverse); ``peaks``: ``{name: [(b, e), ...]}``.  A dict: ``counts`` ``{name: [reads
    of every line]}`` and ``per_ref`` ``{name: (N, n_in)}`` of the chosen references in header order, ``N``, ``n_in``,
    ``union_bases``, ``genome_bases``, and ``hits``: in how many lines every counted read is."""
    names = [n for (n, _l), u in zip(refs, use) if u]
    counts = {n: [0] * len(peaks.get(n, [])) for n in names}
    per_ref = {n: [0, 0] for n in names}
    hits = []
    for ref, pos1, read_len, reverse in reads:
        name, length = refs[ref]
        if not use[ref]:
            continue
        per_ref[name][0] += 1
        lo, hi = extent(pos1, read_len, reverse, extend, length)
        inside = 0
        if lo <= hi:
            row = counts[name]
            for k, (b, e) in enumerate(peaks.get(name, [])):
                e = min(e, length)
                if b < e and b + 1 <= hi and lo <= e:
                    row[k] += 1
                    inside += 1
        per_ref[name][1] += inside > 0
        hits.append(inside)
    union = 0
    for (name, length), u in zip(refs, use):
        top = 0                     # a sweep over the clipped lines by begin: the bases behind the furthest end so far
        for b, e in sorted((b, min(e, length)) for b, e in peaks.get(name, []) if u):
            if e > max(b, top):
                union += e - max(b, top)
                top = e
    return dict(counts=counts, per_ref={n: tuple(v) for n, v in per_ref.items()}, N=sum(v[0] for v in per_ref.values()),
                n_in=sum(v[1] for v in per_ref.values()), union_bases=union,
                genome_bases=sum(l for (_n, l), u in zip(refs, use) if u), hits=hits)


def check_situations(reads, refs, peaks, want, extend):
    """Asserts, from the restatement ``want`` (all references chosen) and plain arithmetic, that the library holds the issue's
    situations for this ``extend``."""
    f0 = dict(zip(peaks["f0"], want["counts"]["f0"]))           # (a repeated line: its last count, equal to the others')
    where = {iv: [k for k, x in enumerate(peaks["f0"]) if x == iv] for iv in (TWINS,)}
    length = refs[0][1]
    ext = [(r, extent(r[1], r[2], r[3], extend, refs[r[0]][1])) for r in reads]
    b, e = EDGE
    on0 = [x for r, x in ext if r[0] == 0]
    assert any(hi == b + 1 for _lo, hi in on0) and any(hi == b for _lo, hi in on0)          # ends on the first base / a base short
    assert any(lo == e for lo, _hi in on0) and any(lo == e + 1 for lo, _hi in on0)          # begins on the last base / behind it
    if extend:
        assert any(r[3] and r[1] + r[2] - extend < 1 <= r[1] + r[2] - 1 for r in reads)    # reverse, extended below position 1
    assert any(r[1] + (extend or r[2]) - 1 > refs[r[0]][1] for r in reads if not r[3])      # a read past the reference's end
    assert CLIPPED[0] < length < CLIPPED[1] and f0[CLIPPED] > 0 and BEYOND[0] >= length and f0[BEYOND] == 0
    twins = where[TWINS]
    assert len(twins) == 2 and want["counts"]["f0"][twins[0]] == want["counts"]["f0"][twins[1]] > 0
    assert all(x < y for (x, _), (_, y) in zip(TRIPLE[1:], TRIPLE)) and max(want["hits"]) >= 3 and all(f0[x] > 0 for x in TRIPLE)
    assert all(NEST[0] <= x and y <= NEST[1] for x, y in INNER) and f0[NEST] > max(f0[x] for x in INNER)
    assert sum(1 for lo, hi in on0 if lo > INNER[-1][1] and hi <= NEST[1]) >= 20            # reads at the far end of the nest
    assert ABUT[0][1] == ABUT[1][0] and any(lo <= ABUT[0][1] and hi >= ABUT[1][0] + 1 for lo, hi in on0)
    assert PAIR[0][1] < PAIR[1][0] and any(lo <= PAIR[0][1] and hi >= PAIR[1][0] + 1 for lo, hi in on0)
    assert want["n_in"] < sum(want["hits"])                                                 # once per read, not the sum of the counts
    assert LAST_OF_F1[1] == refs[1][1] and FIRST_OF_F2[0] == 0
    assert dict(zip(peaks["f1"], want["counts"]["f1"]))[LAST_OF_F1] > 0 and dict(zip(peaks["f2"], want["counts"]["f2"]))[FIRST_OF_F2] > 0
    assert MISSING in peaks and MISSING not in [n for n, _l in refs]
    assert any(x[0] > y[0] for x, y in zip(peaks["f0"], peaks["f0"][1:]))                   # an unsorted file order
    assert 0 < want["n_in"] < want["N"] == len(want["hits"])


def bed_text(peaks, wide=False):
    """The lines as a BED3 file (``wide``: narrowPeak's ten columns), the names interleaved as they come."""
    rows = [(n, b, e) for n, ivs in peaks.items() for b, e in ivs]
    order = np.random.default_rng(2).permutation(len(rows))
    per = {}
    for i in order:                 # interleaved names, each name's lines in their own order
        n = rows[i][0]
        per[n] = per.get(n, -1) + 1
        b, e = peaks[n][per[n]]
        yield "{}\t{}\t{}{}\n".format(n, b, e, "\tp\t500\t.\t7.5\t-1\t-1\t{}".format((e - b) // 2) if wide else "")
