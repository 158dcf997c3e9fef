#!/usr/bin/env python3
"""TEST INFRASTRUCTURE ONLY.  Generates tests/golden/ref_successive_mscc.json.gz by running the REFERENCE's own
compiled `successive` MSCCCalculator, fed by its own BWFeederWithMappableRegionSum (both built by
oracle/build_ref.sh into oracle/_ref/), on seeded synthetic tracks and reads.  The only stand-in is
oracle/ref_shims/pyBigWig.py, which serves the track's intervals from a JSON file.  Runs in the build container
only; the committed JSON holds the inputs (chromosomes, track intervals with their values, reads) and the
reference's outputs (forward_sum, reverse_sum, ccbins, mappable_len, read-length sums, cc) -- data, no reference code.

The project is modelled on the reference's BITARRAY calculator (core/bitarray/mscc.pyx), whose C library is an empty
submodule of the reference tree; the successive calculator is the witness that can be built.  Read from its text
(core/successive/mscc.pyx), it departs from the bitarray calculator in four places.  The cases below stay where
the two agree, and assertions keep them there:

1. Reads near the chromosome start crash it.  `_get_reverse_read_mappability` (:397-401) pads with
   `np.zeros(self._forward_buff_size - (reverse_to + 1) / 2)` when `reverse_from < 0`; under language_level=3 that is
   a float and numpy raises TypeError.  `reverse_from = pos + readlen + read_len - 2 - (2 * max_shift + 1)`, so
   every case keeps ALL reads at `pos >= 2 * max_shift + 2` (asserted per case in `run_reference`).
2. Below max_shift = read_len - 1 its forward window is anchored wrongly.  `_get_forward_mappabiility` (:363-373)
   takes `from_ = min(to - (max_shift + 1), pos - 1)` with `to = pos + read_len - 1` and returns
   `mappability[max_shift::-1]`: for max_shift < read_len - 1 the minimum is `pos - 1`, the slice starts at the
   read's own base instead of at `pos + read_len - 1 - d`, and forward_sum / ccbins differ from the bitarray loop
   (bitarray/mscc.pyx:281-310: M shifted by read_len - 1 - d for every d) while reverse_sum agrees.  Every case has
   max_shift >= read_len - 1 (asserted); max_shift = read_len - 1 itself is case a_S35.
3. Its read-length sums are not the bitarray calculator's.  `feed_forward_read` (:296-301) returns before
   `self.forward_read_len_sum += readlen` when the read's own base is unmappable, `feed_reverse_read` (:342-347)
   when no lag of the read is doubly mappable, and both add to the GENOME-WIDE attribute: the per-chromosome
   `_forward_read_len_sum` / `_reverse_read_len_sum` that `flush` (:201-202, :225-226) stores are never
   incremented and stay 0.  The bitarray calculator (bitarray/mscc.pyx:388-393, :416-418) adds the length of every
   read it keeps, mappable or not, per chromosome.  So the JSON records both what the reference returned
   (`forward_read_len_sum` / `reverse_read_len_sum`: per chromosome 0, genome-wide the sum over counted reads) and,
   for the tests, nothing else: they take the bitarray sum of all kept reads and subtract the kept reads that
   contribute to no lag, which must give the reference's genome-wide figure exactly.  `counted_read_len_sums`
   below restates that rule in numpy and the generator asserts it reproduces the reference's figures, so the rule
   itself is pinned by the reference.  forward_sum / reverse_sum / ccbins are not affected: a read dropped there
   contributes zero to every lag (case d_unmappable_reads is made of such reads).

4. A chromosome that has reads but is absent from the track gets no MSCC result at all (`flush`, :213-216: `get_mappable_len`
   returns None; `finishup_calculation`, :489-490, only fills chromosomes of the track), where the bitarray calculator leaves
   an empty placeholder with an all-zero lag table (bitarray/mscc.pyx:196-205).  Neither has an MSCC row for it; the tests
   check the placeholder (case e_three_chromosomes, chromosome e3).

Everything else agreed on every case when these vectors were made (tests/test_oracle_golden.py holds the CPU oracle
to them, tests/test_gpu_ref_mscc.py the kernels).

The reference's loop costs O(forward reads x max_shift) Python steps, so the genome is small where max_shift is large.
The sixteen cases hold some 36,000 integers and 12,900 doubles of the reference (S + 1 per row, S up to 8200): 750 KB as JSON
text.  The fixture is that JSON text gzip-compressed (level 9, no time stamp, so the same text gives the same bytes), 250 KB:
smaller than the largest fixture there was before (ref_successive_ncc.json), which `main` asserts.
"""
import gzip
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REFERENCE = os.environ.get("PYMASC_REFERENCE", "/root/reference")
for p in (REFERENCE, os.path.join(HERE, "ref_shims")):
    if p not in sys.path:
        sys.path.insert(0, p)

import PyMaSC.core as _core  # noqa: E402
import PyMaSC.core.successive as _succ  # noqa: E402
import PyMaSC.reader as _reader  # noqa: E402
for _pkg in (_reader, _core, _succ):
    if os.path.join(HERE, "_ref") not in _pkg.__path__:
        _pkg.__path__.append(os.path.join(HERE, "_ref"))
from PyMaSC.core.mappability import BWFeederWithMappableRegionSum  # noqa: E402
from PyMaSC.core.successive.mscc import MSCCCalculator  # noqa: E402

MAX_FIXTURE_BYTES = 438890      # tests/golden/ref_successive_ncc.json


# ---- tracks: lists of [begin, end, value], 0-based half-open like BigWig intervals, sorted and disjoint ------------

def runs(rng, lo, hi, on, off, value=1.0):
    """Runs of 1..2*on-1 bp and gaps of 1..2*off-1 bp on [lo, hi)."""
    out, p = [], lo
    while True:
        b = p + int(rng.integers(1, 2 * off))
        e = b + int(rng.integers(1, 2 * on))
        if e > hi:
            return out
        out.append([b, e, value])
        p = e


def tiny_runs(rng, lo, hi, most=8):
    """Runs and gaps of 1..most bp: a dense-edge track."""
    out, p = [], lo
    while True:
        b = p + int(rng.integers(1, most + 1))
        e = b + int(rng.integers(1, most + 1))
        if e > hi:
            return out
        out.append([b, e, 1.0])
        p = e


def threshold_track(rng, G):
    """Values around the `>= 1` filter, abutting runs (a kept run touching a dropped one, and two kept ones), 1-bp runs,
    1-bp gaps, a run that starts at 0 and one that ends exactly at the chromosome end; beyond 6000 ordinary long runs, so
    that the average tile stays within the event kernel's lists."""
    values = [0.5, 0.999, 1.0, 2.0]
    out = [[0, 40, 1.0], [40, 90, 2.0], [90, 130, 0.999], [130, 131, 1.0], [132, 133, 2.0], [133, 134, 0.5], [134, 190, 1.0]]
    p = 200
    k = 0
    while p < 6000:
        n = int(rng.integers(1, 60)) if k % 5 else 1            # every fifth run is 1 bp long
        out.append([p, p + n, values[k % 4] if k % 7 else values[int(rng.integers(0, 4))]])
        gap = (0, 1, 0, int(rng.integers(2, 50)))[k % 4] if k % 3 else int(rng.integers(1, 30))   # abutting, 1-bp and longer gaps
        p += n + gap
        k += 1
    out += runs(rng, p + 50, G - 200, 400, 100)
    out.append([G - 150, G - 60, 0.999])
    out.append([G - 60, G, 1.0])
    return out


# ---- reads: per chromosome, arrays in file order (sorted by position, ties in the order they were drawn) ------------

def sort_reads(pos, rev, rl):
    order = np.argsort(np.asarray(pos), kind="stable")
    return {"pos": [int(pos[i]) for i in order], "rev": [int(bool(rev[i])) for i in order], "len": [int(rl[i]) for i in order]}


def uniform_reads(rng, lo, hi, n, lengths, dup_frac=0.1, same_end=0):
    """n reads on [lo, hi]; dup_frac of them copy the POSITION of another read (strand and length drawn on their own, so
    duplicates differ in length); same_end reverse reads get a shorter partner further right that ends on the same base."""
    pos = rng.integers(lo, hi + 1, size=n)
    ndup = int(n * dup_frac)
    if ndup:
        pos[rng.integers(0, n, size=ndup)] = pos[rng.integers(0, n, size=ndup)]
    rev = rng.random(n) < 0.5
    rl = rng.choice(lengths, size=n)
    pos, rev, rl = pos.tolist(), rev.tolist(), rl.tolist()
    short = min(lengths)
    for i in rng.permutation(n)[:same_end].tolist():
        if rl[i] > short:
            pos.append(pos[i] + rl[i] - short)
            rev.append(True)
            rl.append(short)
            rev[i] = True
    return pos, rev, rl


def placed_reads(points, lo, hi, length):
    """A forward read starting on and a reverse read ENDING on every point (those that fit into [lo, hi])."""
    pos, rev, rl = [], [], []
    for p in points:
        if lo <= p and p + length - 1 <= hi:
            pos.append(p), rev.append(False), rl.append(length)
        if lo <= p - length + 1 and p <= hi:
            pos.append(p - length + 1), rev.append(True), rl.append(length)
    return pos, rev, rl


def join(*parts):
    return tuple(sum((list(p[i]) for p in parts), []) for i in range(3))


# ---- the cases --------------------------------------------------------------------------------------------------

def case_handover(S):
    """a: max_shift = L-1, L, L+1, 2L-2, 2L-1 -- the 2L-1 hand-over between `shift left` and `shift right` of M."""
    L, G = 36, 40000
    rng = np.random.default_rng(1000 + S)
    return dict(name="a_S%d" % S, max_shift=S, read_len=L, chroms=[["a", G]],
                track={"a": runs(rng, 0, G, 150, 50)},
                reads={"a": sort_reads(*uniform_reads(rng, 2 * S + 2, G - L, 700, [L]))})


def case_mixed_lengths():
    """b: forward dedupe by start, reverse dedupe by 3' end, duplicates that differ only in length."""
    S, L, G = 150, 50, 60000
    rng = np.random.default_rng(2)
    return dict(name="b_mixed_lengths", max_shift=S, read_len=L, chroms=[["b", G]],
                track={"b": runs(rng, 0, G, 200, 60)},
                reads={"b": sort_reads(*uniform_reads(rng, 2 * S + 2, G - 76, 1200, [25, 36, 50, 76], dup_frac=0.3, same_end=60))})


def case_threshold():
    """c: the `>= 1` filter and the shapes of runs."""
    S, L, G = 100, 36, 40000
    rng = np.random.default_rng(3)
    track = threshold_track(rng, G)
    edges = [x for b, e, _v in track for x in (b, b + 1, e, e + 1)]
    reads = join(uniform_reads(rng, 2 * S + 2, G - L, 250, [L]), placed_reads(edges[::7], 2 * S + 2, G, L))
    return dict(name="c_threshold_values", max_shift=S, read_len=L, chroms=[["c", G]], track={"c": track},
                reads={"c": sort_reads(*reads)})


def case_unmappable_reads():
    """d: reads dense in an unmappable gap and on run edges -- reads whose own base (forward) or every lag (reverse) is
    unmappable contribute nothing, and the reference leaves them out of its read-length sums (docstring, 3)."""
    S, L, G = 120, 36, 30000
    rng = np.random.default_rng(4)
    track = runs(rng, 0, 4000, 150, 50) + runs(rng, 5000, G, 150, 50)
    edges = [x for b, e, _v in track for x in (b, b + 1, e, e + 1)]
    reads = join(uniform_reads(rng, 4000, 5000 - L, 200, [L], dup_frac=0.2), uniform_reads(rng, 2 * S + 2, G - L, 100, [L]),
                 placed_reads(edges[::3], 2 * S + 2, G, L))
    return dict(name="d_unmappable_reads", max_shift=S, read_len=L, chroms=[["d", G]], track={"d": track},
                reads={"d": sort_reads(*reads)})


def case_three_chromosomes():
    """e: track and reads; track and no reads (empty result with a lag table); reads but absent from the track (skipped)."""
    S, L = 90, 36
    rng = np.random.default_rng(5)
    chroms = [["e1", 30000], ["e2", 7000], ["e3", 6000]]
    return dict(name="e_three_chromosomes", max_shift=S, read_len=L, chroms=chroms,
                track={"e1": runs(rng, 0, 30000, 150, 50), "e2": runs(rng, 0, 7000, 90, 30)}, track_chroms=["e1", "e2"],
                reads={"e1": sort_reads(*uniform_reads(rng, 2 * S + 2, 30000 - L, 400, [L])),
                       "e3": sort_reads(*uniform_reads(rng, 2 * S + 2, 6000 - L, 300, [L]))})


def case_long_read_short_shift():
    """f: max_shift < 2L-1 with a long read."""
    S, L, G = 255, 100, 50000
    rng = np.random.default_rng(6)
    return dict(name="f_L100_S255", max_shift=S, read_len=L, chroms=[["f", G]], track={"f": runs(rng, 0, G, 250, 80)},
                reads={"f": sort_reads(*uniform_reads(rng, 2 * S + 2, G - L, 900, [L, 75]))})


def case_big(name, S, L, G, n, on, off, seed, lengths=None):
    """g, h, i, j: the longest read of the set-bit kernels, the dense kernels only, the BIG event kernel, the window kernels
    beyond 8191 shifts.  Few reads and long runs: the average 64-Kbit tile stays within the event kernel's lists."""
    rng = np.random.default_rng(seed)
    lengths = lengths or [L]
    return dict(name=name, max_shift=S, read_len=L, chroms=[[name[0], G]], track={name[0]: runs(rng, 0, G, on, off)},
                reads={name[0]: sort_reads(*uniform_reads(rng, 2 * S + 2, G - max(lengths), n, lengths, same_end=n // 20))})


def case_tile_boundaries():
    """k: a vector of exactly 65536 bits and one that ends 7 bits into a new 32-Kbit tile (the sizes of FULL_RANGE_CASES in
    tests/test_gpu_parity.py at S=300, L=36); reads and run edges on the tile and 64-bit word boundaries."""
    S, L = 300, 36
    rng = np.random.default_rng(11)
    ext = L + S + 100
    chroms = [["k1", 65536 - ext], ["k2", 32768 + 7 - ext]]
    track, reads = {}, {}
    for name, G in chroms:
        marks = sorted({m + d for m in list(range(1024, G, 4096)) + [16384, 32768, G - 64, G] for d in (-65, -64, -63, -1, 0, 1, 63, 64, 65)})
        marks = [m for m in marks if 2 * S + 2 <= m <= G]
        cuts = sorted({m for m in marks if m % 64 in (0, 63)} | {0, G})     # a run edge on every word boundary we marked
        iv = [[b, e, 1.0] for i, (b, e) in enumerate(zip(cuts[:-1], cuts[1:])) if i % 3 != 1]
        track[name] = iv
        reads[name] = sort_reads(*join(placed_reads(marks, 2 * S + 2, G, L), uniform_reads(rng, 2 * S + 2, G - L, 300, [L])))
    return dict(name="k_tile_boundaries", max_shift=S, read_len=L, chroms=chroms, track=track, reads=reads)


def case_edge_densities():
    """l: a dense-edge track (runs and gaps of 1..8 bp) and a sparse-edge track with a dense island: both arms of the
    mappable-length pass."""
    S, L = 300, 36
    rng = np.random.default_rng(12)
    chroms = [["l1", 20000], ["l2", 40000]]
    track = {"l1": tiny_runs(rng, 0, 20000),
             "l2": runs(rng, 0, 15000, 2000, 600) + tiny_runs(rng, 15000, 18000) + runs(rng, 18000, 40000, 2000, 600)}
    reads = {n: sort_reads(*uniform_reads(rng, 2 * S + 2, G - L, 500, [L])) for n, G in chroms}
    return dict(name="l_edge_densities", max_shift=S, read_len=L, chroms=chroms, track=track, reads=reads)


FIXTURE = "ref_successive_mscc.json.gz"


def cases():
    return [case_handover(S) for S in (35, 36, 37, 70, 71)] + [
        case_mixed_lengths(), case_threshold(), case_unmappable_reads(), case_three_chromosomes(),
        case_long_read_short_shift(), case_tile_boundaries(), case_edge_densities(),
        case_big("g_L1024_S1100", 1100, 1024, 12000, 260, 500, 150, 7, [1024, 700]),
        case_big("h_L1100_S1100", 1100, 1100, 12000, 260, 500, 150, 8),
        case_big("i_S2500_L100", 2500, 100, 20000, 400, 400, 120, 9),
        case_big("j_S8200_L36", 8200, 36, 30000, 300, 300, 100, 10)]


# ---- running the reference ------------------------------------------------------------------------------------------

def counted_read_len_sums(case):
    """The read-length sums as the successive calculator counts them (docstring, 3), restated on bit arrays: of the reads the
    bitarray rules keep (first forward read per start, first reverse read per 3' end), those that contribute to at least one
    lag -- forward: M[pos] & M[pos + L-1-d] for some d, reverse with 3' end e: M[e-d] & M[e-d + L-1-d] for some d."""
    S, L = case["max_shift"], case["read_len"]
    fsum = rsum = 0
    d = np.arange(S + 1)
    for name, G in case["chroms"]:
        r = case["reads"].get(name)
        if r is None or name not in case["track"]:
            continue
        n = G + L + S + 100
        m = np.zeros(n + 2 * (S + L) + 2, dtype=bool)       # (zero-padded on both sides: indices below are shifted by `off`)
        off = S + L + 1
        for b, e, v in case["track"][name]:
            if np.float32(v) >= np.float32(1.0):
                m[off + b + 1:off + e + 1] = True
        seen_f, seen_r = set(), set()
        for p, rev, rl in zip(r["pos"], r["rev"], r["len"]):
            if rev:
                e = p + rl - 1
                if e not in seen_r:
                    seen_r.add(e)
                    if (m[off + e - d] & m[off + e - d + L - 1 - d]).any():
                        rsum += rl
            elif p not in seen_f:
                seen_f.add(p)
                if (m[off + p] & m[off + p + L - 1 - d]).any():
                    fsum += rl
    return fsum, rsum


def run_reference(case):
    S, L = case["max_shift"], case["read_len"]
    names = [n for n, _ in case["chroms"]]
    lengths = [g for _, g in case["chroms"]]
    # the regime in which successive and bitarray agree (docstring, 1 and 2)
    assert S >= L - 1, (case["name"], "max_shift below read_len - 1: the successive calculator's forward window is wrong there")
    for name, r in case["reads"].items():
        assert min(r["pos"]) >= 2 * S + 2, (case["name"], name, "a read within 2 * max_shift + 1 of the chromosome start crashes the reference")
        assert r["pos"] == sorted(r["pos"]) and max(p + l for p, l in zip(r["pos"], r["len"])) - 1 <= dict(case["chroms"])[name]
    for name, iv in case["track"].items():
        assert all(b < e for b, e, _v in iv) and all(x[1] <= y[0] for x, y in zip(iv, iv[1:])) and iv[-1][1] <= dict(case["chroms"])[name]
    track_chroms = case.get("track_chroms", names)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "track.json")
        with open(path, "w") as fh:
            json.dump({"chroms": {n: g for n, g in case["chroms"] if n in track_chroms}, "intervals": case["track"]}, fh)
        calc = MSCCCalculator(S, L, names, lengths, BWFeederWithMappableRegionSum(path, S))
        for name in names:
            r = case["reads"].get(name)
            if r is None:
                continue
            for p, rev, rl in zip(r["pos"], r["rev"], r["len"]):
                (calc.feed_reverse_read if rev else calc.feed_forward_read)(name, p, rl)
        calc.finishup_calculation()
        whole = calc.get_whole_result()
    out = {"forward_read_len_sum": int(whole.forward_read_len_sum), "reverse_read_len_sum": int(whole.reverse_read_len_sum),
           "chroms": {}}
    for name, res in whole.chroms.items():
        out["chroms"][name] = {
            "forward_sum": [int(x) for x in res.forward_sum], "reverse_sum": [int(x) for x in res.reverse_sum],
            "ccbins": [int(x) for x in res.ccbins], "mappable_len": [int(x) for x in res.mappable_len],
            "forward_read_len_sum": int(res.forward_read_len_sum), "reverse_read_len_sum": int(res.reverse_read_len_sum),
            "cc": [None if np.isnan(x) else float(x) for x in np.asarray(res.cc, dtype=np.float64)],
        }
        assert all(len(out["chroms"][name][k]) == S + 1 for k in ("forward_sum", "reverse_sum", "ccbins", "mappable_len", "cc"))
    assert (out["forward_read_len_sum"], out["reverse_read_len_sum"]) == counted_read_len_sums(case), case["name"]
    return out


def generate():
    """The content of the fixture: the cases with the reference's results."""
    out = []
    for case in cases():
        case["expected"] = run_reference(case)
        out.append(case)
    return out


def dumps(cs):
    return json.dumps(cs, separators=(",", ":"))


def main():
    cs = generate()
    for c in cs:
        print(c["name"], "S", c["max_shift"], "L", c["read_len"], {n: len(r["pos"]) for n, r in c["reads"].items()}, "reads;",
              "results for", sorted(c["expected"]["chroms"]), "read-length sums", c["expected"]["forward_read_len_sum"],
              c["expected"]["reverse_read_len_sum"])
    path = os.path.join(ROOT, "tests", "golden", FIXTURE)
    text = dumps(cs).encode()
    data = gzip.compress(text, compresslevel=9, mtime=0)
    assert len(data) <= MAX_FIXTURE_BYTES, len(data)
    with open(path, "wb") as fh:
        fh.write(data)
    print("wrote", path, len(data), "bytes,", len(text), "of JSON text")


if __name__ == "__main__":
    main()
