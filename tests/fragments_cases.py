"""TEST INFRASTRUCTURE for the paired-end fragment sizes: a library of paired records with every case planted,
its writers as BAM and as SAM text, and the yardstick ``restate`` -- a plain Python loop over the record tuples that uses no numpy
and nothing from the package.

The definitions (this project's own), as pymasc_amd/fragments.py and DESIGN.md 7.21 state them.

The pair rule.  A record that passes the run's filter (MAPQ >= -q, none of the flags 0x4 / 0x80 / 0x400, ref_id >= 0, query
length > 0, on a chosen reference) counts in ``reads``.  With flag 0x1 it also counts in ``paired`` and in exactly one of, the first
that holds: (1) flag 0x8: ``mate_unmapped``; (2) the mate's reference is not the record's own (BAM next_refID != refID; SAM RNEXT
neither ``=`` nor byte-equal to RNAME): ``mate_elsewhere``; (3) tlen == 0, tlen == -2^31 or the mate's position unknown (BAM
next_pos < 0; SAM PNEXT 0): ``no_size``; (4) a fragment of size |tlen|, start1 = min(pos1, mate_pos1) and orientation TANDEM (2)
when bit 0x10 equals bit 0x20 shifted down, FR (0) when the read is forward and tlen > 0 or reverse and tlen < 0, RF (1) otherwise.

Size bound.  size > max_size: ``over[orientation]``, and no further.  Otherwise a row (ref_id, start1, size, orientation) in ``rows``.

Mask.  A row is dropped, and counted in ``masked``, when a read with the extent [start1, start1 + size - 1] would be: when a merged
region [b, e) (0-based, half open) has b + 1 <= start1 + size - 1 and start1 <= e.

Table.  H[o][s - 1] = the rows left with orientation o and size s.  paired == mate_unmapped + mate_elsewhere + no_size + sum(over)
+ rows, and rows - masked == sum(H).
"""
import random
import struct
from collections import namedtuple

from . import io_writers as W

REFS = [("chrA", 200000), ("chrB", 50000), ("chrC", 30000), ("chrD", 5000)]
MAPQ = 10
EXCLUDE = 0x4 | 0x80 | 0x400            # PMX_BAM_DEFAULT_EXCLUDE
MAX_SIZES = (1, 2000, 4096, 4097, 65536)
USES = {"all": (1, 1, 1, 1), "not_chrC": (1, 1, 0, 1)}
MASK = {"chrB": [(10000, 10100)], "chrA": [(150000, 150050), (150040, 150200)]}      # 0-based, half open; chrA's two merge
READ = 36
PILE, PILE_SIZE = 70000, 180
FR, RF, TANDEM = 0, 1, 2
COUNTERS = ("reads", "paired", "mate_unmapped", "mate_elsewhere", "no_size", "over_fr", "over_rf", "over_tandem", "rows", "masked")

#: one alignment record: 0-based positions as in BAM; cigar a list of (op, length), empty for '*'; rnext: the SAM spelling of RNEXT
#: (None: '*' for mref < 0, '=' for the record's own reference, the name otherwise); long: the CIGAR goes to the CG:B,I tag in BAM
Rec = namedtuple("Rec", "ref pos0 mapq flag cigar mref mpos0 tlen rnext long", defaults=(None, False))


def pair(ref, start0, size, orient, left=True, mapq=30, more=0, **kw):
    """The read1 record of a pair whose fragment is [start0, start0 + size) with orientation ``orient``; ``left``: the record is
    the fragment's left end (tlen > 0)."""
    span = max(size - READ, 0)
    pos0, mpos0 = (start0, start0 + span) if left else (start0 + span, start0)
    if orient == TANDEM:
        rev = mate_rev = bool(more & 0x10)
    else:
        rev = left == (orient == RF)
        mate_rev = not rev
    flag = 0x1 | 0x40 | (0x10 if rev else 0) | (0x20 if mate_rev else 0) | (more & ~0x10)
    return Rec(ref, pos0, mapq, flag, [("M", READ)], ref, mpos0, size if left else -size, **kw)


def planted():
    """Every case of the issue's list that one file can hold, as (label, Rec); the labels are only for reading."""
    out = []

    def add(label, rec):
        out.append((label, rec))
    a, b, c = 0, 1, 2
    # each branch of the rule, in precedence order, and records that satisfy two of them
    add("unpaired", Rec(a, 100, 30, 0, [("M", READ)], -1, -1, 0))
    add("unpaired with mate fields", Rec(a, 110, 30, 0x10, [("M", READ)], a, 300, 250))
    add("mate unmapped", Rec(a, 120, 30, 0x1 | 0x40 | 0x8, [("M", READ)], a, 120, 0))
    add("mate unmapped and elsewhere", Rec(a, 130, 30, 0x1 | 0x40 | 0x8, [("M", READ)], b, 500, 0))
    add("mate unmapped with a size", Rec(a, 140, 30, 0x1 | 0x40 | 0x8 | 0x20, [("M", READ)], a, 300, 200))
    add("mate elsewhere", Rec(a, 150, 30, 0x1 | 0x40 | 0x20, [("M", READ)], b, 150, 0))
    add("mate elsewhere with a size", Rec(a, 160, 30, 0x1 | 0x40 | 0x20, [("M", READ)], c, 400, 300))
    add("mate nowhere", Rec(a, 170, 30, 0x1 | 0x40 | 0x20, [("M", READ)], -1, -1, 0))
    # tlen edge values, next_pos -1 on a mapped mate
    add("tlen 0", Rec(a, 200, 30, 0x1 | 0x40 | 0x20, [("M", READ)], a, 350, 0))
    add("tlen -2^31", Rec(a, 210, 30, 0x1 | 0x40 | 0x20, [("M", READ)], a, 350, -(1 << 31)))
    add("tlen 2^31 - 1", Rec(a, 220, 30, 0x1 | 0x40 | 0x20, [("M", READ)], a, 350, (1 << 31) - 1))
    add("tlen -(2^31 - 1)", Rec(a, 230, 30, 0x1 | 0x40 | 0x10, [("M", READ)], a, 50, -((1 << 31) - 1)))
    add("next_pos -1", Rec(a, 240, 30, 0x1 | 0x40 | 0x20, [("M", READ)], a, -1, 150))
    # sizes 1, max_size - 1, max_size, max_size + 1 of every max_size, in FR and (the global path of the histogram) RF
    for m in MAX_SIZES:
        for s in {1, m - 1, m, m + 1} - {0}:
            add("FR size %d" % s, pair(a, 70000, s, FR))
            add("RF size %d" % s, pair(a, 70000, s, RF, left=False))
    # all three orientations at one size, from either end; the two orientation rules spelled out
    for o in (FR, RF, TANDEM):
        for left in (True, False):
            add("orientation %d at 300" % o, pair(a, 3000, 300, o, left))
    add("TANDEM both reverse", pair(a, 3100, 300, TANDEM, True, more=0x10))
    add("forward read, negative tlen: RF", Rec(a, 3400, 30, 0x1 | 0x40 | 0x20, [("M", READ)], a, 3200, -236))
    add("reverse read, positive tlen: RF", Rec(a, 3200, 30, 0x1 | 0x40 | 0x10, [("M", READ)], a, 3400, 236))
    # a wave's worth of 64 distinct sizes, in a row in the file, in each orientation
    for o in (FR, RF, TANDEM):
        for k in range(64):
            add("64 distinct", pair(a, 5000 + k, 500 + k, o))
    # the mask (chrB [10000, 10100))
    add("read1 outside, the fragment reaches in", pair(b, 9900, 200, FR))
    add("the fragment abuts on the left", pair(b, 9800, 200, FR))
    add("the fragment abuts on the right", pair(b, 10100, 200, FR, left=False))
    add("read1 inside", pair(b, 10010, 150, RF))
    add("over size spans the region", pair(b, 9000, 70000, FR))
    add("inside chrA's merged regions", pair(a, 150045, 100, TANDEM))
    # references
    add("on chrC", pair(c, 1000, 222, FR))
    add("on chrC, reverse", pair(c, 1500, 223, FR, left=False))
    add("the last base of chrA", pair(a, 200000 - 250, 250, FR, left=False))
    add("the first base of chrB", pair(b, 0, 250, FR))
    add("past the end of chrB", pair(b, 49900, 300, FR))
    add("past the end of chrD", pair(3, 4900, 2000, RF))
    # record placement and the rest of the filter
    add("long CIGAR", pair(a, 8000, 333, FR)._replace(cigar=[("M", 20), ("I", 2), ("M", 14)], long=True))
    add("no query length", Rec(a, 8100, 30, 0x1 | 0x40 | 0x20, [], a, 8300, 236))
    add("low MAPQ", pair(a, 8200, 250, FR, mapq=MAPQ - 1))
    add("duplicate", pair(a, 8300, 250, FR, more=0x400))
    add("read2", pair(a, 8400, 250, FR, more=0x80)._replace(flag=0x1 | 0x80 | 0x10))
    add("unmapped", Rec(a, 8500, 0, 0x1 | 0x40 | 0x4, [], a, 8500, 0))
    add("no reference", Rec(-1, -1, 0, 0x1 | 0x40 | 0x4 | 0x8, [], -1, -1, 0))
    # SAM spellings of RNEXT
    add("RNEXT spelled out", pair(a, 9000, 260, FR, rnext="chrA"))
    add("RNEXT other name", Rec(a, 9100, 30, 0x1 | 0x40 | 0x20, [("M", READ)], b, 9100, 0, "chrB"))
    add("PNEXT 0 with =", Rec(a, 9200, 30, 0x1 | 0x40 | 0x20, [("M", READ)], a, -1, 0, "="))
    add("negative TLEN", pair(a, 9300, 270, FR, left=False))
    return out


def random_pairs(rng, n):
    out = []
    for _ in range(n):
        ref = rng.choice((0, 0, 0, 1, 1, 2))
        top = REFS[ref][1]
        x = rng.random()
        size = max(20, int(rng.gauss(200, 40))) if x < 0.96 else rng.randrange(1500, 5000) if x < 0.99 else rng.randrange(60000, 70000)
        start0 = rng.randrange(0, max(top - min(size, 5000), 1))
        o = FR if rng.random() < 0.9 else rng.choice((RF, TANDEM))
        left = rng.random() < 0.5 or size > 5000        # (every read lies inside its reference; a far mate is only a field)
        r = pair(ref, start0, size, o, left, rng.choice((0, 5, 10, 30, 60)), rng.choice((0, 0, 0, 0, 0x400, 0x2, 0x100)))
        y = rng.random()
        if y < 0.03:
            r = r._replace(flag=r.flag | 0x8)
        elif y < 0.06:
            r = r._replace(mref=(ref + 1) % 3)
        elif y < 0.08:
            r = r._replace(tlen=0)
        elif y < 0.15:
            r = r._replace(flag=r.flag & 0x10, mref=-1, mpos0=-1, tlen=0)      # single-end among the pairs
        out.append(r)
        if rng.random() < 0.3:          # its read2, which the run's filter drops
            out.append(r._replace(pos0=max(r.mpos0, 0), flag=(r.flag & ~0x40 & ~0x30) | 0x80, mpos0=r.pos0, tlen=-r.tlen))
    return out


def library(seed=11):
    """The whole library in coordinate order (unplaced records last): the planted cases, the pile of PILE FR rows at PILE_SIZE and
    about 20 000 random pairs."""
    rng = random.Random(seed)
    recs = [r for _label, r in planted()]
    recs += [pair(0, 20000 + (i % 997), PILE_SIZE, FR, i % 2 == 0) for i in range(PILE)]
    recs += random_pairs(rng, 20000)
    keyed = sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))
    return [r for _i, r in keyed]


def edge_library(n):
    """Exactly ``n`` rows (FR, sizes 100 .. 100 + n - 1 modulo 50) and two records that are none."""
    return ([pair(0, 100 + i, 100 + i % 50, FR) for i in range(n)]
            + [Rec(0, 90000, 30, 0, [("M", READ)], -1, -1, 0), pair(0, 90010, 200, FR, mapq=0)])


# ---- writers ----

def bam_record(r, name=b"p") -> bytes:
    """``io_writers.bam_record``'s struct with next_refID, next_pos and tlen given."""
    cigar = r.cigar
    tags = b""
    l_seq = sum(n for op, n in cigar if op in "MIS=X")
    if r.long:                           # the real CIGAR in CG:B,I behind the <l_seq>S<ref_len>N placeholder (SAM spec 4.2.2)
        real = b"".join(struct.pack("<I", (n << 4) | W.CIGAR_OPS.index(op)) for op, n in cigar)
        tags = b"CGBI" + struct.pack("<I", len(cigar)) + real
        cigar = [("S", l_seq), ("N", sum(n for op, n in r.cigar if op in "MDN=X"))]
    cig = b"".join(struct.pack("<I", (n << 4) | W.CIGAR_OPS.index(op)) for op, n in cigar)
    nm = name + b"\0"
    body = (struct.pack("<iiBBHHHiiii", r.ref, r.pos0, len(nm), r.mapq, 4680, len(cigar), r.flag, l_seq, r.mref, r.mpos0, r.tlen)
            + nm + cig + b"\x11" * ((l_seq + 1) // 2) + b"\x20" * l_seq + tags)
    return struct.pack("<i", len(body)) + body


def bam_records(recs):
    return [bam_record(r, b"p%d" % i) for i, r in enumerate(recs)]


def write_bam(path, recs, indexed=False, refs=REFS):
    if indexed:
        W.write_bam_indexed(path, refs, bam_records(recs), [r.ref for r in recs])
    else:
        W.write_bam(path, refs, bam_records(recs))


def sam_line(r, name, refs=REFS) -> str:
    cig = "".join("%d%s" % (n, op) for op, n in r.cigar) or "*"
    l_seq = sum(n for op, n in r.cigar if op in "MIS=X")
    rnext = r.rnext if r.rnext is not None else "*" if r.mref < 0 else "=" if r.mref == r.ref else refs[r.mref][0]
    return "\t".join([name, str(r.flag), refs[r.ref][0] if r.ref >= 0 else "*", str(r.pos0 + 1), str(r.mapq), cig, rnext,
                      str(r.mpos0 + 1), str(r.tlen), "A" * l_seq or "*", "I" * l_seq or "*"]) + "\n"


def sam_text(recs, refs=REFS) -> bytes:
    head = "@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:{}\tLN:{}\n".format(n, l) for n, l in refs)
    return (head + "".join(sam_line(r, "p%d" % i, refs) for i, r in enumerate(recs))).encode()


def straddles(recs, step, refs=REFS):
    """Pair records whose bytes lie across a multiple of ``step`` in the record area of the BAM stream."""
    at, n = 0, 0
    for r, b in zip(recs, bam_records(recs)):
        if r.flag & 0x1 and at // step != (at + len(b) - 1) // step:
            n += 1
        at += len(b)
    return n


# ---- the yardstick ----

def merged(regions, length):
    out = []
    for b, e in sorted((max(b, 0), min(e, length)) for b, e in regions):
        if b >= e:
            continue
        if out and b <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([b, e])
    return out


def restate(records, refs, use, max_size, mask=None):
    """(rows left as (ref_id, start1, size, orientation) in file order, the ten counters, H as three lists of max_size)."""
    c = dict.fromkeys(COUNTERS, 0)
    hist = [[0] * max_size for _ in range(3)]
    rows = []
    regions = {i: merged(mask.get(n, []), l) for i, (n, l) in enumerate(refs)} if mask else {}
    for r in records:
        qlen = sum(n for op, n in r.cigar if op in "MIS=X")
        if r.flag & EXCLUDE or r.mapq < MAPQ or r.ref < 0 or qlen == 0 or not use[r.ref]:
            continue
        c["reads"] += 1
        if not r.flag & 0x1:
            continue
        c["paired"] += 1
        if r.flag & 0x8:
            c["mate_unmapped"] += 1
            continue
        if r.mref != r.ref:
            c["mate_elsewhere"] += 1
            continue
        if r.tlen == 0 or r.tlen == -(1 << 31) or r.mpos0 < 0:
            c["no_size"] += 1
            continue
        size = abs(r.tlen)
        rev, mate_rev = bool(r.flag & 0x10), bool(r.flag & 0x20)
        if rev == mate_rev:
            o = TANDEM
        elif (not rev and r.tlen > 0) or (rev and r.tlen < 0):
            o = FR
        else:
            o = RF
        if size > max_size:
            c[("over_fr", "over_rf", "over_tandem")[o]] += 1
            continue
        c["rows"] += 1
        start1 = min(r.pos0, r.mpos0) + 1
        last = start1 + size - 1
        if any(b + 1 <= last and start1 <= e for b, e in regions.get(r.ref, [])):
            c["masked"] += 1
            continue
        rows.append((r.ref, start1, size, o))
        hist[o][size - 1] += 1
    return rows, [c[k] for k in COUNTERS], hist
