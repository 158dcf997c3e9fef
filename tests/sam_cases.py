"""TEST INFRASTRUCTURE: the synthetic SAM / BAM twins of tests/test_sam.py and tests/test_gpu_sam.py, and the malformed SAM
texts with the line each reader must name."""
import gzip
import os

import numpy as np

from . import sam_writers as SW

REFS = [("c1", 50000), ("c2", 40000), ("c3", 30000)]

#: the reference's tests/data/ENCFF000RMB-test.sam (the text twin of ENCFF000RMB-test.bam), BGZF-compressed as a data fixture
GOLDEN_SAM_GZ = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ENCFF000RMB-test.sam.gz")


def golden_sam_text() -> bytes:
    with gzip.open(GOLDEN_SAM_GZ, "rb") as fh:
        return fh.read()


def twin_cases():
    """name -> (refs, records, write_twins keyword arguments)."""
    rng = np.random.default_rng(7)
    many = [("contig%05d" % i, 1000 + i) for i in range(3200)]
    many_recs = [SW.rec("m%d" % i, 16 * (i % 2), many[i * 7 % 3200][0], 1 + i % 500, 10 + i % 40) for i in range(0, 3000)]
    many_recs.sort(key=lambda r: ([n for n, _ in many].index(r["rname"]), r["pos"]))
    long_cigar = [("M", 1), ("I", 1)] * 50000                               # 100 000 operations, query length 100 000
    base = SW.synth_records(rng, REFS, 300)
    mixed = [SW.rec("u0", 4, None, 0, 0, None), SW.rec("u1", 4, "c1", 5, 0, [("M", 36)])] + base[:200] + [
        SW.rec("star", 0, "c1", 9000, 40, None), SW.rec("unpl", 0, "*", 0, 40, [("M", 36)]),
        SW.rec("clip", 0, "c2", 10, 40, [("H", 5), ("S", 3), ("M", 30), ("D", 2), ("N", 10), ("=", 2), ("X", 1), ("P", 1)]),
        SW.rec("only_d", 0, "c2", 20, 40, [("D", 5)], 0)] + base[300:400]
    return {
        "synthetic": (REFS, base, {}),
        "many_contigs": (many, many_recs, {}),
        "long_cigar": (REFS, base[:5] + [SW.rec("long", 0, "c1", 40000, 50, long_cigar)] + base[5:20], {}),
        "megabyte_line": (REFS, base[:5] + [SW.rec("big", 16, "c1", 40000, 50, [("S", 10), ("M", 1 << 20)])] + base[5:20], {}),
        "crlf": (REFS, base[:100], {"crlf": True}),
        "no_final_newline": (REFS, base[:50], {"final_newline": False}),
        "crlf_no_final_newline": (REFS, base[:50], {"crlf": True, "final_newline": False}),
        "header_only": (REFS, [], {}),
        "unmapped_and_star": (REFS, mixed, {}),
        "bgzf_small_members": (REFS, base, {"bgzf_block": 997}),
    }


GOOD = "r\t0\tc1\t5\t30\t36M\t*\t0\t0\t*\t*"
HDR = "@HD\tVN:1.0\n@SQ\tSN:c1\tLN:1000\n@SQ\tSN:c2\tLN:500\n"


def malformed_cases():
    """name -> (text, line number named in the error, words of the message)."""
    g = GOOD + "\n"
    return {
        "ten_fields": (HDR + g + "r\t0\tc1\t5\t30\t36M\t*\t0\t0\t*\n", 5, "fields"),
        "flag_big": (HDR + g + g + GOOD.replace("\t0\tc1", "\t65536\tc1") + "\n", 6, "FLAG"),
        "flag_text": (HDR + GOOD.replace("\t0\tc1", "\t0x10\tc1") + "\n", 4, "FLAG"),
        "rname_unknown": (HDR + g + GOOD.replace("c1", "chrZ") + "\n", 5, "RNAME"),
        "pos_negative": (HDR + GOOD.replace("\t5\t", "\t-5\t") + "\n", 4, "POS"),
        "pos_big": (HDR + GOOD.replace("\t5\t", "\t2147483648\t") + "\n", 4, "POS"),
        "mapq_big": (HDR + g + GOOD.replace("\t30\t", "\t256\t") + "\n", 5, "MAPQ"),
        "cigar_op": (HDR + GOOD.replace("36M", "36Q") + "\n", 4, "CIGAR"),
        "cigar_len": (HDR + GOOD.replace("36M", "268435456M") + "\n", 4, "CIGAR"),
        "cigar_tail": (HDR + GOOD.replace("36M", "36M5") + "\n", 4, "CIGAR"),
        "cigar_empty": (HDR + GOOD.replace("36M", "") + "\n", 4, "CIGAR"),
        "empty_line": (HDR + g + "\n" + g, 5, "empty"),
        "late_header": (HDR + g + "@CO\tlate\n" + g, 5, "header"),
        "no_sq": ("@HD\tVN:1.0\n" + g, None, "@SQ"),
        "sq_without_ln": ("@HD\tVN:1.0\n@SQ\tSN:c1\n" + g, 2, "LN"),
        "sq_without_sn": ("@HD\tVN:1.0\n@SQ\tLN:5\n" + g, 2, "SN"),
        "sq_ln_zero": ("@SQ\tSN:c1\tLN:0\n" + g, 1, "LN"),
        "sq_ln_big": ("@SQ\tSN:c1\tLN:2147483648\n" + g, 1, "LN"),
        "sq_duplicate": ("@SQ\tSN:c1\tLN:5\n@SQ\tSN:c2\tLN:5\n@SQ\tSN:c1\tLN:9\n" + g, 3, "duplicate"),
        "error_in_last_of_many": (HDR + g * 70000 + GOOD.replace("c1", "c9"), 70004, "RNAME"),
    }
