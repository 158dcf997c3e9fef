"""Genome FASTA files for the k-mer track tests (tests/test_kmer_track.py on the host, tests/test_gpu_kmer_track.py on the
device): a plain-Python oracle of the uniqueness rule (a dict of canonical k-mers), small synthetic genomes
with every case the rule has to get right, their plain / gzip / BGZF copies, and one malformed file per error rule with the
message it must give."""
import gzip
import os

import numpy as np

from . import io_writers as W

KS = (16, 31, 32, 33, 36, 64, 101)
_COMP = str.maketrans("ACGT", "TGCA")


def revcomp(s: str) -> str:
    return s.translate(_COMP)[::-1]


def parse(text: bytes):
    """[(name, sequence)] of a well-formed FASTA text, by the rules of io/fasta_parse.h."""
    recs = []
    for raw in text.split(b"\n"):
        line = raw[:-1] if raw.endswith(b"\r") else raw
        if not line:
            continue
        if line.startswith(b">"):
            name = line[1:].replace(b"\t", b" ").split(b" ")[0]
            recs.append([name.decode(), []])
        else:
            recs[-1][1].append(line.decode())
    return [(n, "".join(s)) for n, s in recs]


def oracle(records, k):
    """{name: [(begin, end), ...]}: the maximal runs of uniquely mappable positions of every record."""
    seqs = [(n, s.upper()) for n, s in records]
    counts = {}
    kmers = []
    for n, s in seqs:
        row = []
        for p in range(len(s) - k + 1):
            f = s[p:p + k]
            if f.strip("ACGT"):
                row.append(None)
                continue
            c = min(f, revcomp(f))
            counts[c] = counts.get(c, 0) + 1
            row.append((f, c))
        kmers.append(row)
    out = {}
    for (n, s), row in zip(seqs, kmers):
        runs, start = [], None
        for p in range(len(s) + 1):
            x = row[p] if p < len(row) else None
            u = x is not None and x[0] != revcomp(x[0]) and counts[x[1]] == 1
            if u and start is None:
                start = p
            elif not u and start is not None:
                runs.append((start, p))
                start = None
        out[n] = runs
    return out


def fasta_bytes(records, width=60, crlf=False, blank_lines=False) -> bytes:
    """A FASTA text; width 0: each record's sequence on one line."""
    eol = "\r\n" if crlf else "\n"
    out = []
    for n, s in records:
        out.append(">" + n + " some description" + eol)
        w = width or max(len(s), 1)
        for i in range(0, len(s), w):
            out.append(s[i:i + w] + eol)
        if blank_lines:
            out.append(eol)
    return "".join(out).encode()


def compress(data: bytes, how: str) -> bytes:
    if how == "gzip":
        return gzip.compress(data, mtime=0)
    if how == "bgzf":
        return W.bgzf_compress(data, block=4096)
    return data


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(list(alphabet), n))


def genome_cases(seed=7):
    """[(name, records)]: small genomes that hold every case of the rule."""
    rng = np.random.default_rng(seed)
    rep = _rand(rng, 150)                     # an exact repeat, within and across records
    rcrep = _rand(rng, 140)                   # present once forward and once reverse-complemented
    half = _rand(rng, 8)                      # palindromes of even length: X revcomp(X)
    pal16, pal32 = half + revcomp(half), _rand(rng, 16)
    pal32 = pal32 + revcomp(pal32)
    c1 = (_rand(rng, 300) + rep + _rand(rng, 200) + rep + _rand(rng, 100) + "N" * 40 + _rand(rng, 90)
          + "RYKMSWBDHVX" + _rand(rng, 70) + rcrep + _rand(rng, 60))
    c2 = (rep + _rand(rng, 250) + revcomp(rcrep) + _rand(rng, 120) + pal16 + _rand(rng, 40) + pal32 + _rand(rng, 200)
          + _rand(rng, 90).lower() + c1[500:560].lower() + _rand(rng, 80) + rep[:120])       # (a repeat touching the end)
    c3 = _rand(rng, 20)                       # shorter than most k
    c4 = "n" * 30 + _rand(rng, 410) + "acgtNNacgt" + _rand(rng, 200)
    c5 = _rand(rng, 64)                       # exactly k = 64 long
    basic = [("chr1", c1), ("chr2", c2), ("chrS", c3), ("chr4", c4), ("chr5", c5)]
    tandem = [("sat", ("ACGTTGCA" * 40) + _rand(rng, 300) + ("AT" * 60) + _rand(rng, 100)), ("x", _rand(rng, 500))]
    return [("basic", basic), ("tandem", tandem)]


def layouts():
    """[(tag, fasta_bytes keyword arguments)]: line widths 1, 60, 80 and whole-record lines, CRLF and blank lines."""
    return [("w60", dict(width=60)), ("w1", dict(width=1)), ("w80crlf", dict(width=80, crlf=True)),
            ("whole", dict(width=0, blank_lines=True))]


def write_cases(d, which=("plain", "gzip", "bgzf")):
    """Every genome in every layout and compression under d: [(path, records)]."""
    out = []
    for gname, recs in genome_cases():
        for tag, kw in layouts():
            raw = fasta_bytes(recs, **kw)
            for how in which:
                suffix = {"plain": ".fa", "gzip": ".fa.gz", "bgzf": ".fasta.bgz"}[how]
                p = os.path.join(d, "{}_{}{}".format(gname, tag, suffix))
                with open(p, "wb") as fh:
                    fh.write(compress(raw, how))
                out.append((p, recs))
    return out


#: one malformed FASTA per error rule: (file name, text, message the open must name)
MALFORMED = [
    ("before.fa", b"\nACGT\n>c1\nACGTACGTACGTACGTACGT\n", "line 2: sequence before the first header"),
    ("noname.fa", b">c1\nACGTACGTACGTACGTACGT\n> c2\nACGT\n", "line 3: empty sequence name"),
    ("dup.fa", b">c1 a\nACGTACGTACGTACGTACGT\n>c2\nACGT\n>c1 b\nACGT\n", "line 5: duplicate sequence name"),
    ("nobases.fa", b">c1\nACGTACGTACGTACGTACGT\n>c2\n\n>c3\nACGT\n", "line 3: record with no bases"),
    ("byte.fa", b">c1\nACGTACGTACGT\nACG-TACGT\n", "line 3: sequence byte that is not a letter"),
    ("digit.fa", b">c1\r\nACGTACGTACGT\r\nAC1T\r\n", "line 3: sequence byte that is not a letter"),
    ("lastempty.fa", b">c1\nACGTACGTACGTACGTACGT\n>c2\n", "line 3: record with no bases"),
    ("first.fa", b">c1\nAC GT\n>c1\nACGT\n", "line 2: sequence byte that is not a letter"),
    ("empty.fa", b"\n\n", "no FASTA record"),
]


def write_malformed(d):
    out = []
    for name, text, msg in MALFORMED:
        p = os.path.join(d, name)
        with open(p, "wb") as fh:
            fh.write(text)
        out.append((p, msg))
    return out


def big_genome(seed, nbases, nchrom=6, families=40, copies=30, famlen=(50, 2000)):
    """[(name, sequence)] of ~nbases with planted repeat families (exact copies, either strand), N runs and tandem repeats."""
    rng = np.random.default_rng(seed)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    seqs = []
    per = nbases // nchrom
    fams = [lut[rng.integers(0, 4, int(rng.integers(*famlen)))] for _ in range(families)]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    for c in range(nchrom):
        a = lut[rng.integers(0, 4, per + c * 1000)]
        for f in fams:
            for _ in range(copies // nchrom + 1):
                x = f if rng.random() < 0.5 else comp[f][::-1]
                p = int(rng.integers(0, len(a) - len(x)))
                a[p:p + len(x)] = x
        for _ in range(20):
            p = int(rng.integers(0, len(a) - 5000))
            a[p:p + int(rng.integers(10, 5000))] = ord("N")
        unit = lut[rng.integers(0, 4, 171)]
        p = int(rng.integers(0, len(a) - 171 * 200))
        a[p:p + 171 * 200] = np.tile(unit, 200)
        seqs.append(("chr{}".format(c + 1), a.tobytes().decode()))
    return seqs
