"""Cases and the yardstick of the library-complexity tests (tests/test_complexity.py, tests/test_gpu_complexity.py).

The yardstick is ``restate``: a ``collections.Counter`` over tuples of plain ints, written here and nowhere in the package.
"""
import collections

import numpy as np

from tests import sam_writers as SW

BINS = 32
EXCLUDE_KEEP_DUP = 0x80 | 0x4           # read2, unmapped: the run's default mask without the duplicate flag


def restate(ref, pos1, read_len, reverse, nref, use=None):
    """([(N, D, M1, M2)] per reference, hist[BINS]) of the reads given as four columns; ``use``: the references that count."""
    c = collections.Counter(zip([int(x) for x in ref], [int(x) for x in pos1], [int(x) for x in read_len],
                                [int(bool(x)) for x in reverse]))
    per = [[0, 0, 0, 0] for _ in range(nref)]
    hist = [0] * BINS
    for (r, _p, _l, _s), v in c.items():
        if use is not None and not use[r]:
            continue
        per[r][0] += v
        per[r][1] += 1
        per[r][2] += v == 1
        per[r][3] += v == 2
        hist[min(v, BINS - 1)] += 1
        hist[0] = max(hist[0], v)
    return [tuple(p) for p in per], hist


def totals(per):
    N, D = sum(p[0] for p in per), sum(p[1] for p in per)
    return N, D, sum(p[2] for p in per), sum(p[3] for p in per)


def assert_sees_duplicates(ref, pos1, read_len, reverse, above_bins=False):
    """A case that holds no duplicate shows nothing: keys of multiplicity 1, 2 and at least 3 (one above BINS when asked), on
    both strands, with at least two read lengths -- from the restatement alone."""
    c = collections.Counter(zip([int(x) for x in ref], [int(x) for x in pos1], [int(x) for x in read_len],
                                [int(bool(x)) for x in reverse]))
    for want in (lambda v: v == 1, lambda v: v == 2, lambda v: v >= 3):
        strands = {k[3] for k, v in c.items() if want(v)}
        assert strands == {0, 1}, strands
    assert len({k[2] for k in c}) >= 2
    if above_bins:
        assert max(c.values()) > BINS


def synthetic(rng, nref=3, n=3000, ref_len=200_000, pile=40, lengths=(36, 35, 50)):
    """Reads in (ref, pos1) order with planted duplicates: pairs, triples and more, and ``pile`` copies of one key on each
    strand.  Returns int64 arrays (ref, pos1, read_len, reverse)."""
    ref = rng.integers(0, nref, size=n)
    pos = rng.integers(1, ref_len - 100, size=n)
    ln = rng.choice(np.array(lengths), size=n, p=[0.8] + [0.2 / (len(lengths) - 1)] * (len(lengths) - 1))
    rev = rng.integers(0, 2, size=n)
    rows = np.stack([ref, pos, ln, rev], axis=1)
    twice = rows[rng.choice(n, size=n // 10, replace=False)]
    more = rows[rng.choice(n, size=n // 25, replace=False)]
    parts = [rows, twice, more, more, more[: len(more) // 2]]
    for strand in (0, 1):                       # one position, both strands, every length: keys that differ in one field each
        for k, length in enumerate(lengths):
            parts.append(np.tile(np.array([[nref - 1, 777, length, strand]]), (pile + k, 1)))
    rows = np.concatenate(parts)
    rows = rows[rng.permutation(len(rows))]
    rows = rows[np.lexsort((rows[:, 1], rows[:, 0]))]          # (stable: ties keep their shuffled order)
    return rows[:, 0], rows[:, 1], rows[:, 2], rows[:, 3]


def references(nref, ref_len=200_000):
    return [("c{}".format(i), ref_len) for i in range(nref)]


def alignment_records(rng, refs, ref, pos1, read_len, reverse, mapq_low=0.15, dup_flag=0.3, noise=0.05):
    """The reads as SAM / BAM records (tests/sam_writers.rec) with what a filter has to see: MAPQs either side of any threshold
    up to 30, some of the reads that repeat their predecessor flagged 0x400, and read2 / unmapped records in between."""
    out = []
    prev = None
    for i, (r, p, l, s) in enumerate(zip(ref.tolist(), pos1.tolist(), read_len.tolist(), reverse.tolist())):
        flag = 16 if s else 0
        if prev == (r, p, l, s) and rng.random() < dup_flag:
            flag |= 0x400
        prev = (r, p, l, s)
        mapq = int(rng.integers(0, 30)) if rng.random() < mapq_low else int(rng.integers(30, 61))
        out.append(SW.rec("q%d" % i, flag, refs[r][0], p, mapq, (("M", l),)))
        u = rng.random()
        if u < noise / 2:
            out.append(SW.rec("m%d" % i, flag | 0x80 | 0x1, refs[r][0], p, 40, (("M", l),)))
        elif u < noise:
            out.append(SW.rec("u%d" % i, flag | 0x4, refs[r][0], p, 0, (("M", l),)))
    return out


def kept_columns(refs, recs, mapq_min, flag_exclude=EXCLUDE_KEEP_DUP):
    """What the filter keeps of ``recs``, from the records themselves: four lists."""
    ids = {n: i for i, (n, _l) in enumerate(refs)}
    cols = ([], [], [], [])
    for r in recs:
        if (r["flag"] & flag_exclude) or r["mapq"] < mapq_min or r["rname"] not in ids or r["seq_len"] == 0:
            continue
        for c, v in zip(cols, (ids[r["rname"]], r["pos"], r["seq_len"], 1 if r["flag"] & 16 else 0)):
            c.append(v)
    return cols


def tagalign_lines(refs, ref, pos1, read_len, reverse, rng, mapq_low=0.15):
    """The reads as tagAlign lines (chrom, start, end, name, score, strand), with MAPQs either side of a threshold."""
    out = []
    for r, p, l, s in zip(ref.tolist(), pos1.tolist(), read_len.tolist(), reverse.tolist()):
        mapq = int(rng.integers(0, 30)) if rng.random() < mapq_low else int(rng.integers(30, 61))
        out.append("{}\t{}\t{}\tN\t{}\t{}\n".format(refs[r][0], p - 1, p - 1 + l, mapq, "-" if s else "+"))
    return out


def restate_lines(lines, refs, mapq_min):
    """ENCODE's count over the TEXT lines: a Counter over (chrom, start, end, strand); the per-reference tuples and hist."""
    ids = {n: i for i, (n, _l) in enumerate(refs)}
    c = collections.Counter()
    for ln in lines:
        chrom, start, end, _name, score, strand = ln.rstrip("\n").split("\t")
        if int(score) >= mapq_min:
            c[(chrom, int(start), int(end), strand)] += 1
    per = [[0, 0, 0, 0] for _ in refs]
    hist = [0] * BINS
    for (chrom, _s, _e, _st), v in c.items():
        p = per[ids[chrom]]
        p[0] += v
        p[1] += 1
        p[2] += v == 1
        p[3] += v == 2
        hist[min(v, BINS - 1)] += 1
        hist[0] = max(hist[0], v)
    return [tuple(p) for p in per], hist


def as_tables(c, names):
    """A LibraryComplexity as (per-reference tuples in ``names`` order with zeros for the ones left out, hist list)."""
    return [tuple(c.per_reference.get(n, (0, 0, 0, 0))) for n in names], [int(x) for x in c.hist]
