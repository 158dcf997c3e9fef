"""Read-length estimation cases shared by tests/test_readlen.py (host reader) and tests/test_gpu_readlen.py (device reader).

``restate_counter`` / ``restate_estimate`` restate the reference's estimator (PyMaSC core/readlen.pyx) over a plain dict in
insertion order; they are written from the rules, independently of pymasc_amd.readlen, which they check."""
import os

import numpy as np

from tests import io_writers as W

ESTIMATORS = ("MEAN", "MEDIAN", "MODE", "MIN", "MAX")
COUNTERS = ("nreads", "nunmapped", "ncounted", "npaired", "nread2", "nnoqlen")


def qlen(cigar):
    return sum(n for op, n in cigar if op in "MIS=X")


def restate_counter(descs, mapq):
    """descs: (ref, flag, mapq, cigar) per record in file order -> ({length: count} in first-insertion order, counters)."""
    counter, c = {}, dict.fromkeys(COUNTERS, 0)
    for ref, flag, mq, cigar in descs:
        if ref < 0:
            continue
        c["nreads"] += 1
        if flag & 0x1:
            c["npaired"] += 1
            if flag & 0x80:
                c["nread2"] += 1
        if flag & 0x4:
            c["nunmapped"] += 1
        elif not flag & 0x400 and mq >= mapq:
            q = qlen(cigar)
            if q == 0:
                c["nnoqlen"] += 1
            else:
                counter[q] = counter.get(q, 0) + 1
                c["ncounted"] += 1
    return counter, c


def restate_estimate(counter, esttype):
    if not counter:
        raise ValueError("empty")
    if esttype == "MIN":
        return min(counter)
    if esttype == "MAX":
        return max(counter)
    if esttype == "MEAN":
        return int(round(sum(k * v for k, v in counter.items()) / float(sum(counter.values()))))
    if esttype == "MODE":
        return [k for k, v in sorted(counter.items(), key=lambda x: x[1])][-1]
    num = sum(counter.values())
    target = num / 2
    s = 0
    keys = sorted(counter)
    for i, k in enumerate(keys):
        s += counter[k]
        if num % 2:
            if target <= s:
                return k
        elif target < s:
            return k
        elif target == s:
            return int(round((k + float(keys[i + 1])) / 2))


REFS = [("c1", 1_000_000), ("c2", 1_000_000)]


def _rec(ref, pos, mq, flag, cigar, i, l_seq=None):
    return W.bam_record(ref, pos, mq, flag, cigar, b"q%d" % i, l_seq=l_seq)


def synthetic_cases():
    """name -> list of (ref, flag, mapq, cigar, kind) records; kind: None (plain), "long" (CIGAR in the CG tag),
    "noseq" (l_seq = 0: a long query length in a short record)."""
    M = lambda n: [("M", n)]      # noqa: E731
    cases = {}
    cases["flags"] = [
        (0, 0, 30, M(36), None),
        (0, 0x1 | 0x40, 30, M(36), None),
        (0, 0x1 | 0x80, 30, M(50), None),               # read2: counted here
        (0, 0x100, 30, M(51), None),                    # secondary: counted
        (0, 0x800, 30, M(52), None),                    # supplementary: counted
        (0, 0x200, 30, M(53), None),                    # QC fail: counted
        (0, 0x400, 30, M(99), None),                    # duplicate: not counted
        (0, 0x4, 30, M(98), None),                      # unmapped, placed: nunmapped only
        (0, 0x4 | 0x1 | 0x80, 30, M(97), None),         # unmapped read2: nunmapped, npaired, nread2
        (-1, 0x4, 30, M(96), None),                     # ref_id -1: invisible
        (-1, 0, 30, M(95), None),                       # ref_id -1 even when "mapped": invisible
        (0, 0, 5, M(94), None),                         # below MAPQ 10 (counted at MAPQ 0)
        (0, 0x10, 30, [("H", 5), ("S", 3), ("M", 25), ("I", 2), ("D", 4), ("N", 7), ("=", 1), ("X", 1), ("H", 9)], None),
        (1, 0, 30, [("S", 10)] + [("M", 1), ("I", 1)] * 35000 + [("M", 20)], "long"),   # 70030 operations: CG tag
        (1, 0, 30, [], None),                           # no CIGAR: nnoqlen
        (1, 0, 30, [("H", 5)], None),                   # hard clip only: nnoqlen
        (1, 0, 30, M(36), None),
        (1, 0x1 | 0x80 | 0x10, 30, M(36), None),
    ]
    cases["even_35_36"] = [(0, 0, 30, M(35), None), (0, 0, 30, M(36), None)]
    cases["even_36_37"] = [(0, 0, 30, M(37), None), (0, 0, 30, M(36), None)]
    cases["mean_half"] = [(0, 0, 30, M(35), None), (0, 0, 30, M(36), None)] * 3 + [(0, 0, 30, M(20), None)]
    cases["mode_tie_a"] = [(0, 0, 30, M(36), None), (0, 0, 30, M(35), None), (0, 0, 30, M(36), None), (0, 0, 30, M(35), None)]
    cases["mode_tie_b"] = [(0, 0, 30, M(35), None), (0, 0, 30, M(36), None), (0, 0, 30, M(36), None), (0, 0, 30, M(35), None)]
    long_lens = [1000, 1023, 1024, 1025, 4000, 65535, 65536, 70000, 150000, 200000, 200000, 70000, 1024, 36, 36]
    cases["long_reads"] = [(i % 2, 0, 30, M(n), "noseq" if n > 5000 and i % 3 else None) for i, n in enumerate(long_lens)]
    return cases


def write_case(path, recs, block=0xff00):
    out = []
    for i, (ref, flag, mq, cigar, kind) in enumerate(recs):
        if kind == "long":
            out.append(W.long_cigar_record(ref, 100 + i, mq, flag, cigar, name=b"L%d" % i))
        elif kind == "noseq":
            out.append(_rec(ref, 100 + i, mq, flag, cigar, i, l_seq=0))
        else:
            out.append(_rec(ref, 100 + i, mq, flag, cigar, i))
    W.write_bam(path, REFS, out, block=block)
    return [(r, f, m, c) for r, f, m, c, _k in recs]


def golden_descs():
    """(ref, flag, mapq, cigar) of tests/golden/ENCFF000RMB-test.bam from its reference-derived reads table."""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = []
    with open(os.path.join(here, "ENCFF000RMB-test.reads.tsv")) as fh:
        next(fh)
        for line in fh:
            flag, rname, _pos, mq, q = line.rstrip("\n").split("\t")
            out.append((-1 if rname == "*" else 0, int(flag), int(mq), [("M", int(q))]))
    return out


# ---- big files, written with numpy (one fixed record layout: 42 bytes, name "r", one CIGAR operation, no sequence) -----
_REC = np.dtype([("bs", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"),
                 ("n_cig", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"), ("npos", "<i4"), ("tlen", "<i4"),
                 ("name", "S2"), ("cig", "<u4")])


def write_big(path, lengths, flags=None, mapq=None, level=1):
    """One record per entry of ``lengths`` (query length = the one M operation), coordinate-sorted on one reference."""
    n = len(lengths)
    a = np.zeros(n, dtype=_REC)
    a["bs"] = _REC.itemsize - 4
    a["pos"] = np.arange(n, dtype=np.int64) * 7 // 10
    a["l_name"] = 2
    a["mapq"] = 30 if mapq is None else mapq
    a["bin"] = 4680
    a["n_cig"] = 1
    a["flag"] = 0 if flags is None else flags
    a["nref"] = -1
    a["npos"] = -1
    a["name"] = b"r"
    a["cig"] = (np.asarray(lengths, dtype=np.uint32) << 4)
    data = W.bam_header([("c1", 250_000_000)]) + a.tobytes()
    with open(path, "wb") as fp:
        fp.write(W.bgzf_compress(data, level=level))


def trimmed_mix(rng, n):
    """A realistic trimmed-read length mix: most reads full length (36), a tail down to 20."""
    lens = np.arange(20, 37)
    p = np.where(lens == 36, 40.0, 1.0) * np.exp((lens - 36) / 6.0)
    return rng.choice(lens, size=n, p=p / p.sum()).astype(np.uint32)

