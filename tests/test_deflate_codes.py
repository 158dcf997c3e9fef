"""The serial half of the device DEFLATE encoder (pymasc_amd/csrc/ingest/deflate_codes.inc) on the host, no GPU:
tests/deflate_codes_host.cpp is built twice into the test's directory -- plain, and with the address and undefined-behaviour
sanitizers -- and run as a child process that reads cases and prints results.  All judging is done here, against the tables of
tests/deflate_streams.py and the reference lengths of tests/deflate_dissect.py: nothing is compared with C++ written beside the
code under test.

Code lengths are judged against two restatements: the package-merge optimum under the limit, which no code may beat, and the
Huffman optimum, which df_lengths must MEET whenever the Huffman tree fits the limit.  huffman_lengths makes a leaf win a tie, as
df_lengths does, so its depth is that of the minimum-variance tree: the least depth an optimal tree can have, and "the limit does
not act" means exactly that this depth is within it.

Where the limit acts df_lengths is a heuristic (cut, then repair Kraft's sum a unit at a time).  Its worst cost against the
package-merge optimum over the generator below (SEED = 7181) is WORST_RATIO = 1.110333; the test asserts ratio <= 1.02 * WORST_RATIO,
which guards the heuristic against getting worse, not against noise: the run is deterministic."""
import itertools
import os
import random
import subprocess

import pytest

from tests import deflate_streams as DS
from tests.deflate_dissect import chained_rle, cost, dissect, huffman_lengths, package_merge

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "deflate_codes_host.cpp")
INCLUDE = os.path.join(HERE, "..", "pymasc_amd", "csrc", "ingest")
SEED = 7181
CAP = 65537                      # a chunk's tokens and its end-of-block symbol: no histogram of the encoder sums to more
WORST_RATIO = 1.110333           # measured with SEED 7181: see test_df_lengths
ALPHABETS = [(286, 15), (30, 15), (19, 7)]
LIMITED = ("powers_of_two", "geometric", "fibonacci", "fibonacci_jittered")


# ---------------------------------------------------------------- the program ---------------------------------------------------
@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    """(plain, sanitized): both built from the same source.  The sanitizers' runtime is linked into the program, which is
    started directly: nothing is loaded into Python and nothing is preloaded."""
    d = tmp_path_factory.mktemp("deflate_codes_host")
    cxx = os.environ.get("CXX", "g++")
    base = [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-DDF_HD=static inline", "-I", INCLUDE, SOURCE]
    plain, sanitized = str(d / "codes_plain"), str(d / "codes_sanitized")
    subprocess.check_call(base + ["-O2", "-o", plain])
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
    static = ["-static-libasan", "-static-libubsan"] if "g++" in os.path.basename(cxx) else ["-static-libsan"]
    if subprocess.call(base + flags + static + ["-o", sanitized], stderr=subprocess.DEVNULL) != 0:
        subprocess.check_call(base + flags + ["-o", sanitized])          # (a toolchain without the static runtimes)
    return plain, sanitized


def run(programs, lines):
    """The program's output lines for these input lines: the same from both builds, and the sanitized one ends clean."""
    text = "".join(l + "\n" for l in lines).encode()
    outs = []
    for exe in programs:
        p = subprocess.run([exe], input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        outs.append(p.stdout.decode().splitlines())
    assert outs[0] == outs[1]
    return [[int(x) if x.isdigit() else x for x in l.split()] for l in outs[0]]


# ---------------------------------------------------------------- histograms ----------------------------------------------------
def fib(m):
    f = [1, 1]
    while len(f) < m:
        f.append(f[-1] + f[-2])
    return f[:m]


def place(rng, counts, nsym):
    """The counts on distinct symbols of the alphabet, in random order; the literal / length alphabet always uses its
    end-of-block symbol, as every histogram of the encoder does."""
    assert len(counts) <= nsym
    where = rng.sample(range(nsym), len(counts))
    if nsym == 286 and counts and 256 not in where:
        where[0] = 256
    out = [0] * nsym
    for s, c in zip(where, counts):
        out[s] = c
    return out


def histograms(nsym, maxbits):
    """[(family, counts)]: every family of the issue, totals at most CAP; for the families of LIMITED the number of used symbols
    runs from the limit itself to the most the total allows, so that depth = m - 1 lies on both sides of the limit."""
    rng = random.Random(SEED * 1000 + nsym)
    out = []
    for m in sorted({2, 3, 5, nsym // 2, nsym}):
        for c in (1, 7, CAP // nsym):
            out.append(("flat", place(rng, [c] * m, nsym)))
    for _ in range(40):
        m = rng.randint(2, nsym)
        out.append(("uniform", place(rng, [rng.randint(1, CAP // m) for _ in range(m)], nsym)))
    top = min(nsym, 17)                                                      # 1 1 2 4 ... 2^15 sums to 65536
    for m in range(maxbits, top + 1):
        for _ in range(3):
            out.append(("powers_of_two", place(rng, [1] + [1 << k for k in range(m - 1)], nsym)))
    for k in range(44):
        r = 1.3 + k / 43.0
        counts = []
        while len(counts) < nsym and sum(counts) + round(r ** len(counts)) <= CAP:
            counts.append(round(r ** len(counts)))
        counts = counts[:len(counts) - k % 2]
        out.append(("geometric", place(rng, counts, nsym)))
    top = min(nsym, 22)                                                      # 22 Fibonacci numbers sum to 46367
    for m in range(maxbits, top + 1):
        for _ in range(3):
            out.append(("fibonacci", place(rng, fib(m), nsym)))
    for m in range(maxbits + 4, top + 1):                                    # (a jitter breaks ties and costs a few levels)
        for _ in range(6):
            out.append(("fibonacci_jittered", place(rng, [c + rng.choice((-1, 0, 1)) * (c >= 3) for c in fib(m)], nsym)))
    for m in (2, 3, nsym // 3, nsym):
        out.append(("giant_and_ones", place(rng, [CAP - (m - 1)] + [1] * (m - 1), nsym)))
    for _ in range(12):
        out.append(("m_2", place(rng, [rng.randint(1, CAP // 2), rng.randint(1, CAP // 2)], nsym)))
        out.append(("m_3", place(rng, [rng.randint(1, CAP // 3) for _ in range(3)], nsym)))
        out.append(("m_all", [rng.randint(1, CAP // nsym) for _ in range(nsym)]))
    out.append(("m_1", place(rng, [rng.randint(1, CAP)], nsym)))
    out.append(("m_1", place(rng, [1], nsym)))
    out.append(("m_0", [0] * nsym))
    # sums near 2^31, for the 32-bit node weights: no chunk makes them, the routine's contract allows them
    for m in (min(nsym, 44), min(nsym, 30), 19):
        counts = fib(m)
        counts[-1] += (1 << 31) - sum(counts)
        out.append(("u32", place(rng, counts, nsym)))
    out.append(("u32", place(rng, [(1 << 31) // nsym] * nsym, nsym)))
    return out


def judge_lengths(freq, lens, maxbits, partner=False):
    """What holds for every result of df_lengths; returns (the limit acts, cost / package-merge optimum)."""
    used = [s for s, f in enumerate(freq) if f]
    assert all(lens[s] == 0 for s in range(len(freq)) if not freq[s] and not (partner and len(used) == 1))
    if not used:
        assert not any(lens)
        return False, 1.0
    if len(used) == 1:
        assert lens[used[0]] == 1 and sum(lens) == (2 if partner else 1)
        if partner:                      # symbol 1, or symbol 0 when the used one is not 0: a complete code of two
            assert lens[0 if used[0] else 1] == 1
        return False, 1.0
    assert all(1 <= lens[s] <= maxbits for s in used)
    assert DS.kraft(lens) == 32768
    ranked = sorted(used, key=lambda s: (freq[s], s))
    assert all(lens[a] >= lens[b] for a, b in zip(ranked, ranked[1:])), "a rarer symbol has the shorter code"
    h = huffman_lengths(freq)
    best = cost(freq, package_merge(freq, maxbits))
    c = cost(freq, lens)
    assert c >= best
    acts = max(h) > maxbits
    if not acts:
        assert c == cost(freq, h) == best
    return acts, c / best


def bit_reversed(lens):
    return [0 if c is None else (c[1] << 16 | int(format(c[0], "0%db" % c[1])[::-1], 2)) for c in DS.canonical(lens)]


@pytest.fixture(scope="module")
def lengths(programs):
    """{alphabet: [(family, counts, lengths, table)]}: every histogram through df_lengths and df_codes, once."""
    out = {}
    for nsym, maxbits in ALPHABETS:
        cases = histograms(nsym, maxbits)
        res = run(programs, ["L %d %d %s" % (maxbits, nsym, " ".join(map(str, f))) for _fam, f in cases])
        assert len(res) == 2 * len(cases)
        out[nsym, maxbits] = [(fam, f, res[2 * i], res[2 * i + 1]) for i, (fam, f) in enumerate(cases)]
    return out


# ---------------------------------------------------------------- the tests -----------------------------------------------------
def test_df_lengths(lengths):
    """Measured with SEED 7181: the worst cost / package-merge optimum where the limit acts is 1.110333 (WORST_RATIO; printed below
    with the share of every limited family in which the limit acts, 0.27 at the least)."""
    worst = 1.0
    for (nsym, maxbits), rows in lengths.items():
        acting = {}
        for fam, freq, lens, _tab in rows:
            acts, ratio = judge_lengths(freq, lens, maxbits)
            acting.setdefault(fam, []).append(acts)
            if acts:
                worst = max(worst, ratio)
        for fam in LIMITED:
            share = sum(acting[fam]) / len(acting[fam])
            print("df_lengths, %d symbols at %d bits, %s: the limit acts in %d of %d cases (%.2f)" % (
                nsym, maxbits, fam, sum(acting[fam]), len(acting[fam]), share))
            assert share >= 0.25
        assert any(acting["u32"]) and not any(acting["flat"])
    print("df_lengths: worst cost / package-merge optimum where the limit acts: %.6f (WORST_RATIO %.6f)" % (worst, WORST_RATIO))
    assert worst <= WORST_RATIO * 1.02


def test_df_codes(lengths):
    n = 0
    for rows in lengths.values():
        for _fam, _freq, lens, tab in rows:
            assert tab == bit_reversed(lens)
            n += "0" in "".join("1" if l else "0" for l in lens).strip("0")
    assert n > 100                       # lengths with unused symbols in between


def test_df_cl_lengths(programs, lengths):
    rows = lengths[19, 7]
    res = run(programs, ["C " + " ".join(map(str, f)) for _fam, f, _l, _t in rows])
    assert len(res) == 3 * len(rows)
    singles = 0
    for i, (_fam, freq, lens, _tab) in enumerate(rows):
        cl, tab, (hclen,) = res[3 * i], res[3 * i + 1], res[3 * i + 2]
        judge_lengths(freq, cl, 7, partner=True)
        used = [s for s, f in enumerate(freq) if f]
        if len(used) == 1:
            singles += 1
            assert DS.kraft(cl) == 32768
        else:
            assert cl == lens            # df_cl_sort ranks as a stable sort by count does
        assert tab == bit_reversed(cl)
        assert hclen == max([4] + [k + 1 for k, s in enumerate(DS.CL_ORDER) if cl[s]])
    assert singles >= 2
    for s in (0, 1, 18):                 # the partner of symbol 0 is symbol 1, of any other symbol 0
        (cl, _tab, _h) = run(programs, ["C " + " ".join("5" if k == s else "0" for k in range(19))])
        assert [k for k, l in enumerate(cl) if l] == sorted({s, 0 if s else 1}) and sum(cl) == 2


def test_the_symbol_tables(programs):
    lcode, dcode, lextra, dextra, fixed = run(programs, ["T"])
    assert len(lcode) == 3 * 256 and len(dcode) == 3 * 32768
    for length in range(3, 259):
        sym, nbits, extra = lcode[3 * (length - 3):3 * (length - 2)]
        assert 257 <= sym <= 285 and nbits == DS.LEXTRA[sym - 257] == lextra[sym - 257]
        assert DS.LBASE[sym - 257] + extra == length and extra < 1 << nbits
        assert (sym, extra) == DS.length_symbol(length)
    assert lcode[-3:] == [285, 0, 0]                              # 258 is symbol 285, not 284 with 31 extra
    for dist in range(1, 32769):
        sym, nbits, extra = dcode[3 * (dist - 1):3 * dist]
        assert 0 <= sym <= 29 and nbits == DS.DEXTRA[sym] == dextra[sym]
        assert DS.DBASE[sym] + extra == dist and extra < 1 << nbits
    assert lextra == DS.LEXTRA and dextra == DS.DEXTRA and fixed == DS.FIXED_LL


def crafted_vectors():
    """(name, hlit or 0, lengths): runs of every kind at chosen places, in vectors of 258 .. 316 entries.  hlit 0: only the
    sequence is judged (the lengths need not be a code)."""
    def fill(v, n):                      # 1 2 1 2 ...: no run
        return v + [1 + (k & 1) for k in range(n - len(v))]
    out = []
    v = []
    for z in (1, 2, 3, 10, 11, 138):
        v += [0] * z + [7]
    out.append(("zero_runs_1_2_3_10_11_138", 0, fill(v, 258)))
    out.append(("zero_runs_139_149", 0, fill([5] + [0] * 139 + [5] + [0] * 149 + [3], 300)))
    out.append(("zero_run_to_the_end", 0, fill([], 316 - 139) + [0] * 139))
    v = []
    for k in range(1, 9):
        v += [3 + (k & 1)] * k
    out.append(("non_zero_runs_1_to_8_and_70", 0, fill(v + [9] * 70 + [0], 259)))
    out.append(("non_zero_run_to_the_end", 0, fill([], 200) + [15] * 70))
    out.append(("all_one_length", 0, [8] * 316))
    out.append(("all_zero_but_one", 0, [0] * 256 + [1] + [0] * 30))
    # a run of 6s that begins in the literal / length lengths and ends in the distance lengths (complete codes both)
    ll, dl = [8] * 240 + [0] * 16 + [6] * 4, [6, 6, 1, 2, 3, 4, 5] + [0] * 12
    assert DS.kraft(ll) == 32768 == DS.kraft(dl)
    out.append(("run_across_hlit", 260, ll + dl))
    return out


def test_the_header(programs, lengths):
    """df_header_seq, df_hclen, df_header_bits, df_header_write over the code lengths of test_df_lengths (a literal / length code
    with every distance code in turn) and the crafted runs."""
    ll_rows = [r for r in lengths[286, 15] if any(r[1])]
    dl_rows = lengths[30, 15]
    vectors = []
    for i, (_fam, _f, ll, _t) in enumerate(ll_rows):
        ll = list(ll)
        if sum(1 for l in ll if l) == 1:
            ll[0] = 1                    # (the encoder's second code beside the end-of-block symbol alone)
        dl = list(dl_rows[i % len(dl_rows)][2])
        if not any(dl):
            dl[0] = 1
        hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
        hdist = max(s for s in range(30) if dl[s]) + 1
        vectors.append(("lengths_%d" % i, hlit, ll[:hlit] + dl[:hdist]))
    vectors += crafted_vectors()
    assert all(258 <= len(v) <= 316 for _n, _h, v in vectors) and {len(v) for _n, _h, v in vectors} >= {258, 316}
    res = iter(run(programs, ["S %d %d %s" % (hlit, len(v), " ".join(map(str, v))) for _n, hlit, v in vectors]))
    differ = crossing = 0
    for name, hlit, v in vectors:
        seq, cfreq, cl, (hclen, hbits) = next(res), next(res), next(res), next(res)
        ops = [(x & 255) if x & 255 < 16 else (x & 255, (x >> 8) + (11 if x & 255 == 18 else 3)) for x in seq[1:]]
        assert seq[0] == len(ops) and all(x >> 8 == 0 for x in seq[1:] if x & 255 < 16), name
        assert DS.expand_rle(ops) == v, name
        # the rule of chained_rle: greedy_rle, but a run goes on with 16s.  The same list unless a non-zero run exceeds 9.
        assert ops == chained_rle(v), name
        if max(len(list(g)) for l, g in itertools.groupby(v) if l) <= 9:
            assert ops == DS.greedy_rle(v), name
        else:
            differ += ops != DS.greedy_rle(v)
            assert len(ops) <= len(DS.greedy_rle(v)), name
        want = [0] * 19
        for o in ops:
            want[o if isinstance(o, int) else o[0]] += 1
        assert cfreq == want, name
        judge_lengths(cfreq, cl, 7, partner=True)
        assert hclen == max([4] + [k + 1 for k, s in enumerate(DS.CL_ORDER) if cl[s]]), name
        extra = sum({16: 2, 17: 3, 18: 7}[o[0]] for o in ops if not isinstance(o, int))
        assert hbits == 14 + 3 * hclen + cost(cfreq, cl) + extra, name
        if not hlit:
            continue
        written, blob = next(res)
        assert written == hbits, name
        # a whole stream around it: the block's three bits, the header, a hand-made end-of-block code, the Adler-32 of no bytes
        w = DS.BitWriter()
        w.bits(1, 1)
        w.bits(2, 2)
        blob = bytes.fromhex(blob[1:])
        for k in range(written):
            w.bits(blob[k >> 3] >> (k & 7) & 1, 1)
        ll = v[:hlit]
        w.code(DS.canonical(ll)[256])
        (b,) = dissect(DS.zlib_wrap(w.getvalue(), b"")).blocks
        assert (b.hlit, b.hdist, b.hclen, b.cl, b.ops, b.header_bits) == (hlit, len(v) - hlit, hclen, cl, ops, hbits), name
        assert b.ll + b.dl == v and not b.tokens, name
        at = 0
        for o in ops:
            n = 1 if isinstance(o, int) else o[1]
            crossing += at < hlit < at + n
            at += n
    assert differ >= 2 and crossing >= 1
    assert next(res, None) is None

