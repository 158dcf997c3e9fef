"""Cases and the yardstick of the fingerprint tests (tests/test_fingerprint.py, tests/test_gpu_fingerprint.py).

The yardstick is ``restate``: a Python loop over reads and bins on plain ints, written here and nowhere in the package.
"""
import collections

import numpy as np

from tests import sam_writers as SW

REFS = [("f0", 100_003), ("f1", 499), ("f2", 70_001)]
PARAMS = [(500, 0), (500, 200), (500, 1300), (64, 0), (1, 0)]       # (bin, extend)
USES = {"all": [1, 1, 1], "no middle": [1, 0, 1], "no first": [0, 1, 1]}
HIST = 4096
PILES = ((53_250, 4095), (57_250, 4096), (61_250, 5000))            # (pos1, reads) on f2, forward, 36 long: nothing else is near
SPREAD = (20_000, 20_300, 20)                                        # on f0: 20 reads on every pos1 in [20000, 20300)
MASK = {"f0": [(20_100, 20_180), (50_000, 50_400)], "f2": [(57_000, 57_400), (10_000, 10_050)]}   # 0-based, half-open
MAPQ = 10


def layout(refs, use, bin_size):
    """[(first bin, bins)] per reference (None for one without bins of its own) and the number of bins, in plain ints."""
    out, total = [], 0
    for (_name, length), u in zip(refs, use):
        nb = length // bin_size if u else 0
        out.append((total, nb) if u else None)
        total += nb
    return out, total


def extent(pos1, read_len, reverse, extend):
    span = extend if extend > 0 else read_len
    return (pos1 + read_len - span, pos1 + read_len - 1) if reverse else (pos1, pos1 + span - 1)


def restate(reads, refs, use, bin_size, extend):
    """(the count of every bin as a list, the reads that added to a bin) of ``reads`` = rows (ref, pos1, read_len, reverse):
    every read walks the bins of its reference from the one its clipped extent begins in, and adds 1 where the two overlap."""
    where, total = layout(refs, use, bin_size)
    counts = [0] * total
    added = 0
    for ref, pos1, read_len, reverse in reads:
        if where[ref] is None:
            continue
        first, nb = where[ref]
        lo, hi = extent(pos1, read_len, reverse, extend)
        lo, hi = max(lo, 1), min(hi, refs[ref][1])
        hit = False
        j = max((lo - 1) // bin_size, 0)
        while j < nb and j * bin_size + 1 <= hi:
            if (j + 1) * bin_size >= lo:
                counts[first + j] += 1
                hit = True
            j += 1
        added += hit
    return counts, added


def table(counts):
    """H as a sorted list of (count, bins)."""
    return sorted(collections.Counter(counts).items())


def situations(reads, refs, use, bin_size, extend):
    """The names of the situations of the issue that ``reads`` hold for these parameters, from the reads and plain arithmetic."""
    where, _total = layout(refs, use, bin_size)
    seen = set()
    for ref, pos1, read_len, reverse in reads:
        if where[ref] is None or where[ref][1] == 0:
            continue
        first, nb = where[ref]
        length = refs[ref][1]
        lo, hi = extent(pos1, read_len, reverse, extend)
        if pos1 >= bin_size and pos1 % bin_size == 0:
            seen.add("pos1 = j * bin")
        if pos1 > bin_size and pos1 % bin_size == 1 % bin_size:
            seen.add("pos1 = j * bin + 1")
        clo, chi = max(lo, 1), min(hi, nb * bin_size)
        if clo <= chi:
            edges = (chi - 1) // bin_size - (clo - 1) // bin_size
            seen.add("crosses {} edge(s)".format(edges))
        if reverse and lo < 1 and hi >= 1:
            seen.add("reverse, extended below position 1")
        if not reverse and lo <= nb * bin_size < hi <= length:
            seen.add("forward, into the binless tail")
        if not reverse and lo <= length < hi:
            seen.add("forward, past the reference end")
        later = any(w is not None and w[1] > 0 for w in where[ref + 1:])
        if later and lo <= nb * bin_size < hi:
            seen.add("on the last bin, in front of another reference's first")
    return seen


def wanted_situations(refs, use, bin_size, extend):
    """What a case has to hold for its parameters (a situation that cannot exist for them is not asked for)."""
    want = {"pos1 = j * bin", "pos1 = j * bin + 1", "crosses 1 edge(s)", "forward, past the reference end"}
    with_bins = [bool(u) and length >= bin_size for (_n, length), u in zip(refs, use)]
    if sum(with_bins) > 1:
        want.add("on the last bin, in front of another reference's first")
    if (bin_size, extend) == (500, 1300):
        want.add("crosses 3 edge(s)")
    if extend > 0:
        want.add("reverse, extended below position 1")
    if any(u and length >= bin_size and length % bin_size for (_n, length), u in zip(refs, use)):
        want.add("forward, into the binless tail")
    return want


def synthetic(seed=5, n=85_000):
    """Rows (ref, pos1, read_len, reverse, mapq) in (ref, pos1) order: ``n`` reads anywhere on f0 and f1 and on the front of f2,
    both strands, several lengths, MAPQs either side of MAPQ, and the planted reads (all at MAPQ 40)."""
    rng = np.random.default_rng(seed)
    lens = np.array([36, 35, 50, 101])
    rows = []
    for ref, hi, share in ((0, 99_900, 0.6), (1, 460, 0.01), (2, 50_000, 0.39)):
        m = int(n * share)
        rows.append(np.stack([np.full(m, ref), rng.integers(1, hi, size=m), rng.choice(lens, size=m, p=[0.7, 0.1, 0.1, 0.1]),
                              rng.integers(0, 2, size=m),
                              np.where(rng.random(m) < 0.15, rng.integers(0, MAPQ, size=m), rng.integers(MAPQ, 61, size=m))], axis=1))
    plant = []
    for ref, length in ((0, REFS[0][1]), (2, REFS[2][1])):
        for b in (500, 64):
            for j in (1, 2, 7):
                for rev in (0, 1):
                    plant += [(ref, j * b, 36, rev), (ref, j * b + 1, 36, rev)]                 # on and behind a bin's last position
                    plant += [(ref, j * b - 10, 36, rev), (ref, j * b - 1, 2, rev), (ref, j * b, 1, rev)]   # across one edge; short
        for rev in (0, 1):
            plant += [(ref, 3, 36, rev), (ref, 1, 50, rev), (ref, 120, 36, rev)]                # an extension runs below position 1
            last_bin = (length // 500) * 500
            plant += [(ref, last_bin + 2 - span, 36, rev) for span in (36, 200, 1300)]          # one base into the binless tail
            plant += [(ref, (length // 64) * 64 - 10, 36, rev)]
            plant += [(ref, last_bin - 20, 36, rev), (ref, last_bin - 400, 36, rev),            # the last bin and the tail behind it
                      (ref, length - 1, 1, rev), (ref, length - 20, 36, rev), (ref, length - 2, 36, rev), (ref, length, 36, rev)]
    plant += [(0, 30_000 - 20, 36, 0), (0, 30_000 - 20, 36, 1)]
    plant += [(1, p, l, rev) for p in (1, 64, 65, 440, 448, 449, 480, 499) for l in (36, 2) for rev in (0, 1)]
    for pos1, count in PILES:
        plant += [(2, pos1, 36, 0)] * count
    lo, hi, per = SPREAD
    plant += [(0, p, 36, k % 2) for p in range(lo, hi) for k in range(per)]
    rows.append(np.array([r + (40,) for r in plant], dtype=np.int64))
    rows = np.concatenate(rows)
    rows = rows[rng.permutation(len(rows))]
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]
    return rows


def kept(rows, mapq=MAPQ):
    """The reads the filter keeps, as a list of plain tuples (ref, pos1, read_len, reverse)."""
    return [tuple(r[:4]) for r in rows.tolist() if r[4] >= mapq]


def masked(reads, refs, mask=None):
    """``reads`` less those whose own extent [pos1, pos1 + read_len - 1] overlaps an interval of ``mask``."""
    mask = MASK if mask is None else mask
    out = []
    for ref, pos1, read_len, reverse in reads:
        last = pos1 + read_len - 1
        length = refs[ref][1]
        if any(b < min(e, length) and b + 1 <= last and pos1 <= min(e, length) for b, e in mask.get(refs[ref][0], [])):
            continue
        out.append((ref, pos1, read_len, reverse))
    return out


def alignment_records(rows, refs, seed=6, noise=0.03):
    """The rows as SAM / BAM records, with records the filter drops in between: flagged duplicates, read2, unmapped."""
    rng = np.random.default_rng(seed)
    out = []
    u = rng.random(len(rows))
    for i, (r, p, l, s, q) in enumerate(rows.tolist()):
        flag = 16 if s else 0
        out.append(SW.rec("q%d" % i, flag, refs[r][0], p, q, (("M", l),)))
        if u[i] < noise:
            extra = (0x400, 0x80 | 0x1, 0x4)[i % 3]
            out.append(SW.rec("x%d" % i, flag | extra, refs[r][0], p, 40, (("M", l),)))
    return out


def tagalign_lines(rows, refs):
    return ["{}\t{}\t{}\tN\t{}\t{}\n".format(refs[r][0], p - 1, p - 1 + l, q, "-" if s else "+") for r, p, l, s, q in rows.tolist()]
