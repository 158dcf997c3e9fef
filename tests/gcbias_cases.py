"""Cases and the yardstick of the GC-bias tests (tests/test_gcbias.py, tests/test_gpu_gcbias.py).

The yardstick is ``restate``: a Python loop over every window start and every read, on strings (slices and ``str.count``), written
here and nowhere in the package.  It uses neither ``gcbias.count_host`` nor a cumulative sum.
"""
import functools

import numpy as np

from tests import fingerprint_cases as FC

REFS = [("g0", 100_003), ("g1", 499), ("g2", 70_001)]       # the alignment header's order
EXTRA = ("gx", 777)                                          # a record no header names
FASTA_ORDER = ("g2", "gx", "g0", "g1")
PARAMS = [1, 31, 32, 33, 64, 100, 1024]
USES = {"all": [1, 1, 1], "no middle": [1, 0, 1]}
MAPQ = 10
READ_LENS = (36, 50, 101)

# planted in g0 (0-based, half-open)
SINGLE_N = (5000, 7777, 9999)
EDGE_N = (6397, 6406)                   # across the edge of a 64-position word of the table (g0 is its first reference)
LONG_N = (30_000, 31_100)               # longer than 1024
GC_ONLY = (40_000, 41_200)              # longer than 1024 + 64
AT_ONLY = (42_000, 43_200)
ACGT = (48_000, 98_000)                 # ACGT repeated: for even W more than two workgroups' worth of windows with one g
# planted in g2: first and last base N, a G at PILE_X and an A at PILE_X + W for every W, so that neighbouring piles differ in g
PILE_X = 53_000
PILES = ((2, 57_251, 5000), (2, PILE_X + 1, 5000), (2, PILE_X + 2, 5000))      # (ref, pos1, reads), forward, 36 long
NEAR_READ = (0, 12_000, 36, 0)          # its extent ends at 12 035, its window of 42 or more reaches the interval behind it
MASK = {"g0": [(49_000, 49_040), (12_040, 12_060)], "g2": [(57_000, 57_400)]}  # 0-based, half-open


@functools.lru_cache(maxsize=None)
def genome(seed=11):
    """``{name: the record's bases, uppercase}`` with the planted situations."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, length in REFS + [EXTRA]:
        block = np.arange(length) // 1000
        p_gc = 0.30 + 0.35 * (0.5 + 0.5 * np.sin(block / 3.0 + len(out)))
        gc = rng.random(length) < p_gc
        second = rng.random(length) < 0.5
        out[name] = np.where(gc, np.where(second, "G", "C"), np.where(second, "A", "T"))
    g0, g2 = out["g0"], out["g2"]
    for p in SINGLE_N:
        g0[p] = "N"
    g0[EDGE_N[0]:EDGE_N[1]] = "N"
    g0[LONG_N[0]:LONG_N[1]] = "N"
    g0[GC_ONLY[0]:GC_ONLY[1]] = np.where(rng.random(GC_ONLY[1] - GC_ONLY[0]) < 0.5, "G", "C")
    g0[AT_ONLY[0]:AT_ONLY[1]] = np.where(rng.random(AT_ONLY[1] - AT_ONLY[0]) < 0.5, "A", "T")
    g0[ACGT[0]:ACGT[1]] = np.array(list("ACGT" * ((ACGT[1] - ACGT[0]) // 4)))
    g0[20_000] = "R"                    # an IUPAC code is masked like N
    g2[0] = g2[-1] = "N"
    g2[PILE_X:PILE_X + 1100] = np.where(g2[PILE_X:PILE_X + 1100] == "N", "T", g2[PILE_X:PILE_X + 1100])
    g2[PILE_X] = "G"
    for w in PARAMS:
        g2[PILE_X + w] = "A"
    g2[33_333] = "N"
    return {n: "".join(v.tolist()) for n, v in out.items()}


def fasta_text() -> bytes:
    """The FASTA file: the records in FASTA_ORDER, 60 bases a line; g1 in uneven lines; one ``\\r\\n`` line; some lines lowercase;
    a blank line; a header with a description."""
    g = genome()
    out = []
    for name in FASTA_ORDER:
        seq = g[name]
        out.append(">{}{}\n".format(name, " the record of " + name if name == "g0" else ""))
        if name == "g1":
            cuts = [0, 7, 60, 61, 200, 333, len(seq)]
            lines = [seq[a:b] for a, b in zip(cuts, cuts[1:])]
        else:
            lines = [seq[i:i + 60] for i in range(0, len(seq), 60)]
        for k, ln in enumerate(lines):
            if k % 7 == 3:
                ln = ln.lower()
            out.append(ln + ("\r\n" if k == 5 else "\n"))
        if name == "g2":
            out.append("\n")
    return "".join(out).encode()


def synthetic(seed=12, n=80_000):
    """Rows (ref, pos1, read_len, reverse, mapq) in (ref, pos1) order: ``n`` reads anywhere, both strands, lengths 36 / 50 / 101,
    MAPQs either side of MAPQ, and the planted reads (all at MAPQ 40)."""
    rng = np.random.default_rng(seed)
    rows = []
    for ref, share in ((0, 0.6), (1, 0.01), (2, 0.39)):
        m = int(n * share)
        rows.append(np.stack([np.full(m, ref), rng.integers(1, REFS[ref][1] - 30, size=m), rng.choice(READ_LENS, size=m, p=[0.7, 0.15, 0.15]),
                              rng.integers(0, 2, size=m),
                              np.where(rng.random(m) < 0.15, rng.integers(0, MAPQ, size=m), rng.integers(MAPQ, 61, size=m))], axis=1))
    plant = []

    def both(ref, s, w):
        """a forward and (where its pos1 exists) a reverse read of every length whose window of w starts at s"""
        for rl in READ_LENS:
            plant.append((ref, s, rl, 0))
            if s + w - rl >= 1:
                plant.append((ref, s + w - rl, rl, 1))
    for ref in (0, 2):
        length = REFS[ref][1]
        plant.append((ref, 1, 36, 0))                                   # a forward read at position 1
        plant += [(ref, length - rl + 1, rl, 1) for rl in READ_LENS]       # reverse reads that end on len
        for w in PARAMS:
            both(ref, length - w + 1, w)                                # the last window
            if w > 1:
                both(ref, length - w + 2, w)                            # past len by 1
            both(ref, 1, w)                                             # s = 1
        plant += [(ref, length - 3, 36, 0), (ref, length - 20, 101, 0)] # past len by many
        for w in PARAMS:                                                # reverse reads with s = 0 (and below)
            plant += [(ref, w - rl, rl, 1) for rl in READ_LENS if w - rl >= 1]
            plant += [(ref, 1, rl, 1) for rl in READ_LENS if 1 + rl - w < 0]
    n1 = SINGLE_N[0] + 1                                                # the single N, 1-based
    for w in PARAMS:
        both(0, n1 - w + 1, w)          # touches the N with its last base
        both(0, n1 - w, w)              # abuts it in front
        both(0, n1, w)                  # touches it with its first base
        both(0, n1 + 1, w)              # abuts it behind
    plant += [(1, p, rl, rev) for p in (1, 64, 200, 400, 440, 464) for rl in READ_LENS for rev in (0, 1)]
    plant.append(NEAR_READ)
    plant += [(0, 48_990, 36, 0), (0, 49_100, 36, 1), (0, 60_000, 50, 0), (0, 60_001, 50, 1)]     # around the ACGT stretch
    for ref, pos1, count in PILES:
        plant += [(ref, pos1, 36, 0)] * count
    rows.append(np.array([r + (40,) for r in plant], dtype=np.int64))
    rows = np.concatenate(rows)
    rows = rows[rng.permutation(len(rows))]
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]


kept = FC.kept


def masked(reads, mask=None):
    """``reads`` less those whose own extent overlaps an interval of the mask."""
    return FC.masked(reads, REFS, MASK if mask is None else mask)


def alignment_records(rows):
    return FC.alignment_records(rows, REFS, seed=13)


def tagalign_lines(rows):
    return FC.tagalign_lines(rows, REFS)


def blocked_genome(mask=None):
    """The genome with every position of a mask interval replaced by N: excluded regions act as runs of N."""
    g = dict(genome())
    for name, intervals in (mask or {}).items():
        s = g[name]
        for b, e in intervals:
            e = min(e, len(s))
            s = s[:b] + "N" * (e - b) + s[e:]
        g[name] = s
    return g


_WINDOWS = {}


def windows(name, w, with_mask):
    """g of the window at every 1-based start of record ``name`` (index s - 1; -1: blocked), by slices and counts; made once."""
    key = (name, w, bool(with_mask))
    if key not in _WINDOWS:
        seq = blocked_genome(MASK if with_mask else None)[name]
        out = []
        for s0 in range(len(seq) - w + 1):
            win = seq[s0:s0 + w]
            c, g = win.count("C"), win.count("G")
            out.append(c + g if c + g + win.count("A") + win.count("T") == w else -1)
        _WINDOWS[key] = out
    return _WINDOWS[key]


def place(read, w):
    """The 1-based start of the read's window."""
    _ref, pos1, read_len, reverse = read
    return pos1 + read_len - w if reverse else pos1


def restate(reads, use, w, with_mask):
    """(N, F as lists of w + 1, off_end, blocked) of ``reads`` = rows (ref, pos1, read_len, reverse), the filter and the mask's
    read filter applied already; ``with_mask``: the windows are blocked by MASK too."""
    N, F = [0] * (w + 1), [0] * (w + 1)
    off_end = blocked = 0
    for (name, _length), u in zip(REFS, use):
        if u:
            for g in windows(name, w, with_mask):
                if g >= 0:
                    N[g] += 1
    for read in reads:
        ref = read[0]
        if not use[ref]:
            continue
        s = place(read, w)
        if s < 1 or s + w - 1 > REFS[ref][1]:
            off_end += 1
            continue
        g = windows(REFS[ref][0], w, with_mask)[s - 1]
        if g < 0:
            blocked += 1
        else:
            F[g] += 1
    return N, F, off_end, blocked


def blocked_windows(use, w, with_mask):
    return sum(sum(1 for g in windows(name, w, with_mask) if g < 0) for (name, _l), u in zip(REFS, use) if u)


def situations(reads, use, w, with_mask):
    """The names of the situations of the issue that the genome and ``reads`` hold for these parameters."""
    seen = set()
    g = genome()
    n1 = SINGLE_N[0] + 1
    for read in reads:
        ref, pos1, read_len, reverse = read
        if not use[ref]:
            seen.add("a read on a reference that is not chosen")
            continue
        length = REFS[ref][1]
        s = place(read, w)
        strand = "reverse" if reverse else "forward"
        if not reverse and pos1 == 1:
            seen.add("forward at position 1")
        if reverse and pos1 + read_len - 1 == length:
            seen.add("reverse ending on len")
        if not reverse and s + w - 1 == length + 1:
            seen.add("forward past len by 1")
        if not reverse and s + w - 1 > length + 1:
            seen.add("forward past len by many")
        if reverse and s == 0:
            seen.add("reverse with s = 0")
        if reverse and s == 1:
            seen.add("reverse with s = 1")
        if ref == 0 and 1 <= s and s + w - 1 <= length:
            if s + w - 1 == n1:
                seen.add(strand + " touches an N with its last base")
            if s == n1:
                seen.add(strand + " touches an N with its first base")
            if s + w - 1 == n1 - 1 or s == n1 + 1:
                assert w > 1024 or windows("g0", w, False)[s - 1] >= 0
                seen.add(strand + " abuts an N")
        if ref == 1:
            seen.add("on the short record")
        seen.add("read_len above W" if read_len > w else "read_len below W" if read_len < w else "read_len = W")
        if with_mask and read == NEAR_READ and 1 <= s and windows("g0", w, False)[s - 1] >= 0 and windows("g0", w, True)[s - 1] < 0:
            seen.add("kept by the filter, blocked by the mask")
    counts = {}
    for read in reads:
        counts[read] = counts.get(read, 0) + 1
    piles = sorted(r for r, c in counts.items() if c >= 5000)
    if piles:
        seen.add("a pile of 5000")
    for a, b in zip(piles, piles[1:]):
        if a[0] == b[0] and a[1] + 1 == b[1] and a[2:] == b[2:] and use[a[0]]:
            tab = windows(REFS[a[0]][0], w, with_mask)
            sa, sb = place(a, w), place(b, w)
            if 0 <= tab[sa - 1] != tab[sb - 1] >= 0:
                seen.add("neighbouring piles with different g")
    tab = windows("g0", w, with_mask)
    longest = run = 0
    for s0 in range(ACGT[0] + 1100, ACGT[1] - w):
        run = run + 1 if tab[s0] == tab[s0 - 1] >= 0 else 0
        longest = max(longest, run)
    if longest > 2 * 256 * 64:
        seen.add("one g over more than two workgroups' windows")
    if all(windows(n, w, with_mask).count(k) > 0 for k in (0, w) for n in ("g0",)):
        seen.add("both end bins filled")
    assert g["g2"][0] == "N" and g["g2"][-1] == "N" and "N" * 1025 in g["g0"]
    return seen


def wanted_situations(use, w, with_mask):
    """What a case has to hold for its parameters (a situation that cannot exist for them is not asked for)."""
    want = {"forward at position 1", "reverse ending on len",
            "forward touches an N with its last base", "forward touches an N with its first base", "forward abuts an N",
            "reverse touches an N with its last base", "reverse abuts an N", "a pile of 5000", "both end bins filled"}
    if not with_mask:
        want.add("neighbouring piles with different g")
    if w > 22:                          # (a forward read lies inside its reference: its window of 1 cannot pass the end)
        want |= {"forward past len by 1", "forward past len by many"}
    if w > min(READ_LENS):              # (a reverse read's window lies inside the read unless it is longer)
        want |= {"reverse with s = 0", "reverse with s = 1", "read_len below W"}
    if w < max(READ_LENS):
        want.add("read_len above W")
    if w % 2 == 0:
        want.add("one g over more than two workgroups' windows")
    if not all(use):
        want.add("a read on a reference that is not chosen")
    else:
        want.add("on the short record")
    if with_mask and w >= 64:
        want.add("kept by the filter, blocked by the mask")
    return want
