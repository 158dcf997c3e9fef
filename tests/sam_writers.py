"""TEST INFRASTRUCTURE: SAM / BAM twins -- one list of record fields rendered as SAM text (SAM spec v1 section 1.4) and as BAM
(through tests/io_writers.py), so that the SAM readers can be checked against the BAM readers record for record."""
import os

import numpy as np

from . import io_writers as W


def rec(qname="r", flag=0, rname="c1", pos=1, mapq=30, cigar=(("M", 36),), seq_len=None):
    """One alignment: rname None or '*' = unplaced; cigar None = '*'; pos is 1-based (0 = none)."""
    cig = [] if cigar is None else list(cigar)
    if seq_len is None:
        seq_len = sum(n for op, n in cig if op in "MIS=X")
    return dict(qname=qname, flag=flag, rname=rname or "*", pos=pos, mapq=mapq, cigar=cig, seq_len=seq_len)


def sam_line(r, eol="\n") -> str:
    cig = "".join("%d%s" % (n, op) for op, n in r["cigar"]) or "*"
    seq = "A" * r["seq_len"] if r["seq_len"] else "*"
    qual = "I" * r["seq_len"] if r["seq_len"] else "*"
    return "\t".join([r["qname"], str(r["flag"]), r["rname"], str(r["pos"]), str(r["mapq"]), cig, "*", "0", "0", seq, qual]) + eol


def sam_header(refs, eol="\n") -> str:
    return "@HD\tVN:1.0\tSO:coordinate" + eol + "".join("@SQ\tSN:{}\tLN:{}{}".format(n, l, eol) for n, l in refs)


def sam_text(refs, recs, crlf=False, final_newline=True) -> bytes:
    eol = "\r\n" if crlf else "\n"
    t = sam_header(refs, eol) + "".join(sam_line(r, eol) for r in recs)
    if not final_newline and t.endswith(eol):
        t = t[:-len(eol)]
    return t.encode()


def bam_bytes(refs, recs):
    ids = {n: i for i, (n, _l) in enumerate(refs)}
    out = []
    for r in recs:
        ref = ids.get(r["rname"], -1)
        name = r["qname"].encode()
        if len(r["cigar"]) > 65535:          # (BAM keeps such a CIGAR in the CG tag, SAM spec 4.2.2)
            out.append(W.long_cigar_record(ref, r["pos"] - 1, r["mapq"], r["flag"], r["cigar"], name))
        else:
            out.append(W.bam_record(ref, r["pos"] - 1, r["mapq"], r["flag"], r["cigar"], name, r["seq_len"]))
    return out


def write_twins(directory, name, refs, recs, crlf=False, final_newline=True, bgzf_block=None):
    """(sam path, bam path); bgzf_block: also write <name>.sam.gz, BGZF members of that many bytes of text (returned third)."""
    directory = os.fspath(directory)
    sam = os.path.join(directory, name + ".sam")
    bam = os.path.join(directory, name + ".bam")
    text = sam_text(refs, recs, crlf, final_newline)
    with open(sam, "wb") as fh:
        fh.write(text)
    W.write_bam(bam, refs, bam_bytes(refs, recs), text=sam_header(refs))
    if bgzf_block is None:
        return sam, bam
    gz = os.path.join(directory, name + ".sam.gz")
    with open(gz, "wb") as fh:
        fh.write(W.bgzf_compress(text, bgzf_block))
    return sam, bam, gz


def synth_records(rng, refs, n_per_ref, readlen=36):
    """Coordinate-sorted single-end reads with strands, duplicates, read2s, low MAPQs and a few trimmed lengths."""
    out = []
    for name, ln in refs:
        pos = np.sort(rng.integers(1, ln - readlen - 1, size=n_per_ref))
        for p in pos.tolist():
            f = 16 if rng.random() < 0.5 else 0
            if rng.random() < 0.02:
                f |= 0x400
            if rng.random() < 0.02:
                f |= 0x81
            q = int(rng.integers(0, 61))
            l = readlen - 1 if rng.random() < 0.1 else readlen
            out.append(rec("read%d" % len(out), f, name, p, q, [("M", l)]))
    return out
