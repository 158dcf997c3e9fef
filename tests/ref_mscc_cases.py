"""The vectors of the reference's compiled `successive` MSCC calculator (tests/golden/ref_successive_mscc.json.gz, made by
oracle/make_ref_mscc_vectors.py) and what the CPU and GPU tests share to read them: plain numpy, no oracle, no kernel."""
import gzip
import json
import os

import numpy as np

from . import fixtures as fx

FIXTURE = "ref_successive_mscc.json.gz"      # gzip-compressed JSON text


def load_cases():
    with gzip.open(os.path.join(fx.GOLDEN, FIXTURE), "rt") as fh:
        return json.load(fh)


CASES = load_cases()
IDS = [c["name"] for c in CASES]


def track_of(case):
    """{chrom: [(begin, end, value)]} as the calculators' feeders take it."""
    return {n: [tuple(x) for x in iv] for n, iv in case["track"].items()}


def feed(calc, case):
    """Every read of the case in file order through the per-read protocol."""
    for name, _g in case["chroms"]:
        r = case["reads"].get(name)
        if r is None:
            continue
        for p, rev, rl in zip(r["pos"], r["rev"], r["len"]):
            (calc.feed_reverse_read if rev else calc.feed_forward_read)(name, p, rl)


def nan_array(xs):
    return np.array([np.nan if x is None else x for x in xs], dtype=np.float64)


def vector_bits(case, name):
    """Length of the chromosome's bit vectors (mscc.pyx:134,:165-167)."""
    return dict(map(tuple, case["chroms"]))[name] + case["read_len"] + case["max_shift"] + 100


def kept_reads(case, name):
    """The reads the bitarray rules keep (mscc.pyx:388-393, :416-418), in file order: (forward starts, their lengths,
    reverse 3' ends, their lengths) -- the first forward read per start, the first reverse read per 3' end."""
    r = case["reads"][name]
    fpos, flen, rend, rlen = [], [], [], []
    seen_f, seen_r = set(), set()
    for p, rev, rl in zip(r["pos"], r["rev"], r["len"]):
        if rev:
            if p + rl - 1 not in seen_r:
                seen_r.add(p + rl - 1)
                rend.append(p + rl - 1), rlen.append(rl)
        elif p not in seen_f:
            seen_f.add(p)
            fpos.append(p), flen.append(rl)
    return (np.array(fpos, dtype=np.int64), np.array(flen, dtype=np.int64),
            np.array(rend, dtype=np.int64), np.array(rlen, dtype=np.int64))


def read_len_sums_of_reads_in_no_lag(case):
    """(forward, reverse) read-length sums, over all chromosomes, of the kept reads that contribute to NO lag of the MSCC rows:
    forward at p with M[p] & M[p + L-1-d] false for every d, reverse with 3' end e with M[e-d] & M[e-d + L-1-d] false for
    every d -- every read of a chromosome without a track.  The reference's successive calculator leaves exactly these out of
    its (genome-wide) read-length sums, the bitarray calculator counts them (oracle/make_ref_mscc_vectors.py, docstring, 3)."""
    S, L = case["max_shift"], case["read_len"]
    d = np.arange(S + 1)
    off = S + L + 1
    fsum = rsum = 0
    for name in case["reads"]:
        fpos, flen, rend, rlen = kept_reads(case, name)
        if name not in case["track"]:
            fsum += int(flen.sum())
            rsum += int(rlen.sum())
            continue
        m = np.zeros(vector_bits(case, name) + 2 * off, dtype=bool)
        for b, e, v in case["track"][name]:
            if np.float32(v) >= np.float32(1.0):
                m[off + b + 1:off + e + 1] = True
        for p, rl in zip(fpos.tolist(), flen.tolist()):
            if not (m[off + p] & m[off + p + L - 1 - d]).any():
                fsum += rl
        for e, rl in zip(rend.tolist(), rlen.tolist()):
            if not (m[off + e - d] & m[off + e - d + L - 1 - d]).any():
                rsum += rl
    return fsum, rsum
