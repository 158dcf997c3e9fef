"""TEST INFRASTRUCTURE for the record chain of the device BAM reader (pymasc_amd/csrc/ingest/bam_device.hip, "The record chain";
DESIGN.md 7.1): small valid BAM record streams with DECOY records planted where the reader's speculative step looks first, the
truth of every stream as its builder wrote it down, and a plain-Python restatement of the rule (``model``).

The decoys.  A decoy is a byte-exact alignment record stored inside the ``XD:B:C`` tag of a true record (its HOST).  No reader that
follows the block_size fields from the first record ever sees one.  The device reader cuts the stream into 16-KB pieces and guesses
the first record of every piece: the first offset where two records in a row look like records.  Where a host's tag lies behind a
piece boundary, that offset is a decoy, the guess is wrong, and the repair rounds have to find it out from the neighbour's end.

Telling a leak.  True records lie on reference 0 (``true``): 36M, MAPQ 30, forward.  Decoys lie on reference 1 (``decoy``), which
holds no true record: 50M, MAPQ 60, reverse, position 7000 + i.  A decoy that reaches any consumer shows as a read on ``decoy``, a
length of 50, a reverse read, or a read that passes MAPQ 40.

``model`` shares no code with the product.  It restates ``rec_plausible``, the guess of ``k_bam_spec``, the walk of ``k_bam_walk``
with its four refusals (the stream ends inside the record, block_size < 32, a record shorter than its name and CIGAR, an unknown
reference id) and the repair loop of ``walk_chain`` as the comments in bam_device.hip state them.  IF THE PRODUCT'S PLAUSIBILITY
RULE EVER CHANGES, ``plausible`` BELOW CHANGES WITH IT: the wrong-guess figures of the cases depend on it, and
tests/test_chain_cases.py fails until they are derived again.

What the model gives for the cases (tests/test_chain_cases.py prints this table; ``wrong``: pieces whose guess is neither right
nor missing; rounds: launches of the repair pass, the last, empty one included, when every piece reads last round's ends / pieces
in ascending order see fresh ends / pieces in descending order):

    case          bytes  pieces records  wrong missing  rounds last/asc/desc  rewalks last/asc/desc
    rejoin        82020       6     850      1       1       2 / 2 / 2           2 / 2 / 2
    bad           82020       6     850      1       1       2 / 2 / 2           2 / 2 / 2
    overshoot    114788       8    1192      1       1       4 / 2 / 4           6 / 2 / 6
    fake_chain   147556      10     852      5       1       6 / 2 / 6           6 / 6 / 6
    every_piece  163845      11    1681      8       1       3 / 2 / 3           9 / 9 / 9
    to_the_end    49340       4     511      1       0       2 / 2 / 2           1 / 1 / 1
    saturated    541995      34    1500     13       0       2 / 2 / 2           13 / 13 / 13
    pairs        543435      34    1515     13       0       3 / 2 / 3           13 / 13 / 13

(The missing guess of the aligned cases is the last piece: the 100 or 5 bytes behind the last boundary hold no record start.
``fake_chain`` has five wrong guesses because its host's name is 201 bytes long, see ``_fake_chain``; ``to_the_end`` puts its
host 150 bytes before the boundary, see ``_to_the_end``.)
"""
import functools
import struct
from collections import namedtuple

from . import fragments_cases as FR
from . import io_writers as W

P = 16384                                        # WALK_PIECE
REFS = [("true", 2_000_000), ("decoy", 100_000)]
DEFAULT_EXCLUDE = 0x4 | 0x80 | 0x400             # PMX_BAM_DEFAULT_EXCLUDE
CASES = ("rejoin", "bad", "overshoot", "fake_chain", "every_piece", "to_the_end", "saturated", "pairs")
#: pieces whose guess is neither right nor missing; None: at least a quarter of the pieces
WRONG_GUESSES = {"rejoin": 1, "bad": 1, "overshoot": 1, "fake_chain": 5, "every_piece": 8, "to_the_end": 1, "saturated": None,
                 "pairs": None}
PAIR_SIZES = tuple(180 + k for k in range(15))   # the planted true pairs of ``pairs``, FR, one of each size


# ---- building blocks ----

def _with_block_size(rec: bytes, bs: int) -> bytes:
    return struct.pack("<I", bs) + rec[4:]


def _grown(rec: bytes, extra: int) -> bytes:
    """``rec`` with ``extra`` more tag bytes."""
    return _with_block_size(rec, len(rec) - 4 + extra) + b"\x05" * extra


def decoy(i: int, extra: int = 0) -> bytes:
    return _grown(W.bam_record(1, 7000 + i, 60, 0x10, [("M", 50)], b"d"), extra)


def pair_decoy(i: int, extra: int = 0) -> bytes:
    """A decoy that is one mate of a proper pair (read1 for even i, read2 for odd i; the mate 150 bases to the left, forward)."""
    flag = 0x1 | 0x2 | 0x10 | (0x80 if i & 1 else 0x40)
    return _grown(FR.bam_record(FR.Rec(1, 7000 + i, 60, flag, [("M", 50)], 1, 7000 + i - 150, -200), b"d"), extra)


DECOY_LEN = len(decoy(0))
assert len(pair_decoy(0)) == DECOY_LEN == 117


class _Builder:
    """A record stream under construction: ``records`` (bytes), ``truth`` (one tuple per record, written down here and never
    parsed back), ``size`` (bytes so far) and ``decoys`` (the stream offset of the first decoy of every host)."""

    def __init__(self):
        self.records, self.truth, self.decoys, self.size = [], [], [], 0

    def _add(self, rec: bytes, flag: int) -> None:
        self.records.append(rec)
        self.truth.append((0, 10 + 7 * len(self.truth) + 1, 36, False, 30, flag))
        self.size += len(rec)

    def true(self, tags: bytes = b"", name: bytes = b"t") -> None:
        self._add(W.bam_record(0, 10 + 7 * len(self.truth), 30, 0, [("M", 36)], name, tags=tags), 0)

    def true_pair(self, size: int) -> None:
        r = FR.pair(0, 10 + 7 * len(self.truth), size, FR.FR, left=True, mapq=30)
        assert not r.flag & 0x10
        self._add(FR.bam_record(r, b"t"), r.flag)

    def host(self, payload: bytes, name: bytes = b"t") -> None:
        self.true(b"XDBC" + struct.pack("<I", len(payload)) + payload, name)
        self.decoys.append(self.size - len(payload))

    def pad_to(self, n: int) -> None:
        """True records until the stream is exactly ``n`` bytes; the last one takes the slack in a tag of \\x02 bytes."""
        plain = len(W.bam_record(0, 0, 30, 0, [("M", 36)], b"t"))
        assert n - self.size >= plain + 8, (n, self.size)
        while n - self.size >= 2 * plain + 8:
            self.true()
        slack = n - self.size - plain
        self.true(b"XPBC" + struct.pack("<I", slack - 8) + b"\x02" * (slack - 8))
        assert self.size == n


HOST_PREFIX = 104                                # bytes of a host record (name "t") in front of its payload


def _rejoin(b):
    b.pad_to(2 * P - 20)
    b.host(decoy(0) + decoy(1) + decoy(2))       # the third decoy ends where the host ends: the wrong walk rejoins the chain
    b.pad_to(5 * P + 100)


def _bad(b):
    b.pad_to(2 * P - 20)
    b.host(decoy(0) + decoy(1) + struct.pack("<I", 7) + b"\0" * 60)
    b.pad_to(5 * P + 100)


def _overshoot(b):
    b.pad_to(2 * P - 20)
    b.host(decoy(0) + _with_block_size(decoy(1), 2 * P + 333))
    b.pad_to(7 * P + 100)


def _fake_chain(b):
    # (the host's name is 201 bytes long, so its payload of 4 P bytes begins 284 bytes into piece 2 and ends 284 bytes into piece 6:
    # room for two whole decoys there, and the guess of a fifth piece is wrong as well; the slack goes to the first decoy)
    name = b"h" * 200
    prefix = HOST_PREFIX + len(name) - 1
    n = (4 * P) // DECOY_LEN
    slack = 4 * P - n * DECOY_LEN
    assert prefix - 20 >= 2 * DECOY_LEN
    b.pad_to(2 * P - 20)
    b.host(decoy(0, slack) + b"".join(decoy(1 + k) for k in range(n - 1)), name)
    assert b.size == 6 * P + prefix - 20
    b.pad_to(9 * P + 100)


def _every_piece(b):
    for c in range(1, 9):
        b.pad_to(c * P - 20 - c % 3)
        b.host(decoy(2 * c) + decoy(2 * c + 1) + (b"\x03" * 17 if c % 2 == 0 else b""))
    b.pad_to(10 * P + 5)


def _to_the_end(b):
    # (the host starts 150 bytes before the boundary, not 20: its first decoy begins in piece 2, so the only offset of piece 3 that
    # looks like a record is the second decoy, whose end is the stream's: the nx == N arm of the guess)
    b.pad_to(3 * P - 150)
    b.host(decoy(0) + decoy(1))
    assert b.decoys[-1] < 3 * P < b.decoys[-1] + DECOY_LEN and b.size == b.decoys[-1] + 2 * DECOY_LEN


def _saturated(b, dec=decoy, pairs=False):
    for i in range(1500):
        if pairs and i % 100 == 50:
            b.true_pair(PAIR_SIZES[i // 100])
        tail = (b"", b"\x03" * 17, struct.pack("<I", 5) + b"\0" * 40)[i % 3]
        b.host(dec(i % 500) + dec((i + 1) % 500, i % 7) + tail)


def _pairs(b):
    _saturated(b, pair_decoy, True)


@functools.lru_cache(maxsize=None)
def _built(name: str) -> _Builder:
    b = _Builder()
    globals()["_" + name](b)
    assert len(b.records) == len(b.truth)
    return b


def case(name: str):
    """(refs, records, truth): ``truth`` the (ref, pos1, qlen, reverse, mapq, flag) of the true records, in file order."""
    b = _built(name)
    return list(REFS), list(b.records), list(b.truth)


def first_decoys(name: str):
    """The offset in the record stream of the first decoy of every host record."""
    return list(_built(name).decoys)


def kept(truth, mapq: int, flag_exclude: int = DEFAULT_EXCLUDE):
    """The (ref name, pos1, qlen, reverse) of the truth that pass a reader's filter."""
    return [(REFS[r][0], p, q, v) for r, p, q, v, m, f in truth if m >= mapq and not f & flag_exclude]


def to_the_end_cut():
    """``to_the_end`` with the host's block_size raised by 40: the stream ends inside the host record, the last true one, while its
    decoys still end exactly at the stream's end."""
    _refs, records, _truth = case("to_the_end")
    bs, = struct.unpack_from("<I", records[-1])
    return list(REFS), records[:-1] + [_with_block_size(records[-1], bs + 40)]


def every_piece_bs7():
    """``every_piece`` with a true record in the middle of piece 6 patched to block_size = 7; (refs, records, records in front)."""
    _refs, records, _truth = case("every_piece")
    at = 0
    for k, rec in enumerate(records):
        if at >= 6 * P + P // 2:
            assert at + len(rec) < 7 * P - 1000 and b"XD" not in rec
            return list(REFS), records[:k] + [_with_block_size(rec, 7)] + records[k + 1:], k
        at += len(rec)
    raise AssertionError("no record in piece 6")


# ---- the truth by a serial walk ----

def serial(stream: bytes):
    """(offsets, fields): every record a serial walk of the block_size fields meets, and its (ref, pos1, qlen, reverse, mapq,
    flag) with the query length summed over the CIGAR's M operations."""
    offsets, fields, s = [], [], 0
    while s < len(stream):
        bs, ref, pos, l_name, mapq, _bin, n_cig, flag = struct.unpack_from("<IiiBBHHH", stream, s)
        cig = struct.unpack_from("<%dI" % n_cig, stream, s + 36 + l_name)
        offsets.append(s)
        fields.append((ref, pos + 1, sum(v >> 4 for v in cig if v & 15 == 0), bool(flag & 0x10), mapq, flag))
        s += 4 + bs
    assert s == len(stream)
    return offsets, fields


def piece_starts(offsets, n: int):
    """The first record at or behind the start of every piece (``n``, the stream's size, where there is none)."""
    out, k = [], 0
    for c in range((n + P - 1) // P):
        while k < len(offsets) and offsets[k] < c * P:
            k += 1
        out.append(offsets[k] if k < len(offsets) else n)
    return out


# ---- the rule, restated ----

NONE, BAD = -1, -2                               # WALK_NONE, WALK_BAD
SCHEDULES = ("last_round", "ascending", "descending")
Model = namedtuple("Model", "guesses starts records rounds rewalks")


def plausible(D: bytes, o: int, N: int, nref: int) -> bool:
    if o + 36 > N:
        return False
    bs, ref, pos, l_name, _mapq, _bin, n_cig, _flag, l_seq, mref, mpos = struct.unpack_from("<IiiBBHHHiii", D, o)
    if bs < 32 or bs > 1 << 28 or o + 4 + bs > N:
        return False
    if ref < -1 or ref >= nref or pos < -1 or mref < -1 or mref >= nref or mpos < -1 or l_name == 0 or l_seq < 0:
        return False
    if 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > bs:
        return False
    return D[o + 36 + l_name - 1] == 0


def guess(D: bytes, N: int, nref: int, c: int) -> int:
    if c == 0:
        return 0
    for o in range(c * P, min((c + 1) * P, N)):
        if plausible(D, o, N, nref):
            nx = o + 4 + struct.unpack_from("<I", D, o)[0]
            if nx == N or plausible(D, nx, N, nref):
                return o
    return NONE


def walk(D: bytes, N: int, nref: int, s: int, c: int):
    """(where the walk of piece c from s ended, the records it counted)."""
    if s == NONE:
        return NONE, 0
    n = 0
    while s < (c + 1) * P and s < N:
        if s + 4 > N:
            return BAD, n
        bs, = struct.unpack_from("<I", D, s)
        if bs < 32 or s + 4 + bs > N:
            return BAD, n
        ref, _pos, l_name, _mapq, _bin, n_cig = struct.unpack_from("<iiBBHH", D, s + 4)
        if 32 + l_name + 4 * n_cig > bs or ref >= nref:
            return BAD, n
        n += 1
        s += 4 + bs
    return s, n


@functools.lru_cache(maxsize=None)
def _guesses(D: bytes, nref: int):
    return tuple(guess(D, len(D), nref, c) for c in range((len(D) + P - 1) // P))


def model(stream_bytes: bytes, nref: int, schedule: str = "last_round") -> Model:
    """The chain of ``stream_bytes`` as the rule closes it: the guesses, the closed piece starts, the record count, the launches
    of the repair pass (the last, empty one included) and the pieces walked again.  ``schedule``: what a piece sees of its
    neighbour in one launch -- ``last_round``: last round's end; ``ascending``: pieces run in ascending order and see fresh ends;
    ``descending``: in descending order."""
    assert schedule in SCHEDULES
    D, N = bytes(stream_bytes), len(stream_bytes)
    np_ = (N + P - 1) // P
    guesses = list(_guesses(D, nref))
    spec = list(guesses)
    end, cnt = [list(x) for x in zip(*(walk(D, N, nref, spec[c], c) for c in range(np_)))] if np_ else ([], [])
    rounds = rewalks = 0
    while True:
        if rounds > np_ + 1:
            raise AssertionError("record chain did not close")
        rounds += 1
        seen = list(end) if schedule == "last_round" else end
        nmis = 0
        for c in (range(np_ - 1, 0, -1) if schedule == "descending" else range(1, np_)):
            e = seen[c - 1]
            if e in (BAD, NONE) or e == spec[c]:
                continue
            spec[c] = e
            nmis += 1
            end[c], cnt[c] = walk(D, N, nref, e, c)
        rewalks += nmis
        if nmis == 0:
            break
    return Model(guesses, spec, sum(cnt), rounds, rewalks)


@functools.lru_cache(maxsize=None)
def summary(name: str):
    """What the tests need of a case's model: pieces, wrong and missing guesses, the pieces whose guess is not the true start (each
    is walked again at least once, whatever the schedule) and the model under every schedule."""
    refs, records, _truth = case(name)
    stream = b"".join(records)
    offsets, _fields = serial(stream)
    true_starts = piece_starts(offsets, len(stream))
    models = {s: model(stream, len(refs), s) for s in SCHEDULES}
    g = models["last_round"].guesses
    wrong = [c for c in range(len(g)) if g[c] != NONE and g[c] != true_starts[c]]
    missing = [c for c in range(len(g)) if g[c] == NONE]
    return dict(bytes=len(stream), pieces=len(g), records=len(records), true_starts=true_starts, wrong=wrong, missing=missing,
                off=len(wrong) + len(missing), models=models)
