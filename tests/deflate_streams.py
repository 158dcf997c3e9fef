"""TEST INFRASTRUCTURE: a bit-level DEFLATE writer (RFC 1951) and a model of what its symbols mean, for streams that no
encoder emits: explicit code lengths (any that the format allows, optimal or not), explicit headers and run-length coding of the
lengths, stored blocks at any bit offset, length 258 as symbol 284 with 31 extra bits, matches at chosen distances -- and
streams that a decoder must refuse.  It knows nothing about the readers: the expected output of a stream is `model(symbols)`,
and tests/test_deflate_streams.py holds every stream of this module against zlib's decoder.

A symbol is an int (a literal byte) or a tuple (length, distance[, length symbol]).  Streams that must be refused also use
("bits", value, n) for raw bits, ("L", symbol, extra) for any literal / length symbol and ("D", symbol, extra) for any distance
symbol."""
import struct
import zlib

import numpy as np

LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
         8193, 12289, 16385, 24577]
DEXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DL = [5] * 32
CL_DEFAULT = [4] * 13 + [5] * 6          # a complete code over all 19 code-length symbols (13/16 + 6/32)
INF_NEAR = 3774                          # the distance up to which the device decoder copies from its ring in LDS
MEMBER_CDATA_MAX = 65536 - 18 - 8        # DEFLATE bytes in a BGZF member that has only the BC subfield


def length_symbol(length):
    """The usual symbol of a match length (258 -> 285) and its extra bits' value."""
    s = max(i for i in range(29) if LBASE[i] <= length)
    return 257 + s, length - LBASE[s]


def distance_symbol(dist):
    s = max(i for i in range(30) if DBASE[i] <= dist)
    return s, dist - DBASE[s]


_LSYM = [None] * 259
for _l in range(3, 259):
    _LSYM[_l] = length_symbol(_l)
_DSYM_STEP = [distance_symbol(d) for d in range(1, 513)]


def _dsym(dist):
    if dist <= 512:
        return _DSYM_STEP[dist - 1]
    s = 2 * (dist - 1).bit_length() - 2 + (((dist - 1) >> ((dist - 1).bit_length() - 2)) & 1)
    return s, dist - DBASE[s]


def canonical(lens):
    """Canonical Huffman codes (RFC 1951 3.2.2) of a list of code lengths: [(code, length)], code MSB first.  An incomplete set
    gets the same codes a decoder gives it; an over-subscribed one gets codes cut to their length (no decoder reads them)."""
    cnt = [0] * 17
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * 17, 0
    for b in range(1, 16):
        code = (code + cnt[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lens:
        if l:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
        else:
            out.append(None)
    return out


def kraft(lens):
    """Sum of 2^-l over the non-zero lengths, in units of 2^-15: 32768 = complete."""
    return sum(1 << (15 - l) for l in lens if l)


_REV8 = [int("{:08b}".format(i)[::-1], 2) for i in range(256)]


def _rev(code, n):
    return ((_REV8[code & 255] << 8) | _REV8[(code >> 8) & 255]) >> (16 - n)


class BitWriter:
    """Bits into a bytearray, LSB first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, cl):            # a Huffman code: packed starting from its most significant bit
        self.bits(_rev(cl[0], cl[1]), cl[1])

    def align(self):
        if self.n:
            self.buf.append(self.acc & 255)
            self.acc = self.n = 0

    def raw(self, data):
        assert self.n == 0
        self.buf += data

    @property
    def bitpos(self):
        return 8 * len(self.buf) + self.n

    def getvalue(self):
        return bytes(self.buf) + (bytes([self.acc & 255]) if self.n else b"")


def model(symbols, prefix=b""):
    """The bytes a symbol list means: a literal appends, a match copies byte by byte from `distance` back.  (`prefix`: bytes in
    front of the stream that a match may reach -- what a decoder without a test of the distance would read.)"""
    out = bytearray(prefix)
    for s in symbols:
        if isinstance(s, int):
            out.append(s)
        else:
            length, dist = s[0], s[1]
            assert 3 <= length <= 258 and 1 <= dist <= len(out), (length, dist, len(out))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
    return bytes(out[len(prefix):])


def plain_rle(lens):
    return list(lens)


def greedy_rle(lens):
    """A run-length coding of the lengths as an encoder would choose it (16 / 17 / 18 with the longest count)."""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run = j - i
        if v == 0 and run >= 3:
            n = min(run, 138)
            ops.append((18, n) if n >= 11 else (17, n))
            i += n
        elif v and run >= 4:
            ops.append(v)
            n = min(run - 1, 6)
            ops.append((16, n))
            i += 1 + n
        else:
            ops.append(v)
            i += 1
    return ops


def expand_rle(ops):
    out = []
    for o in ops:
        if isinstance(o, int):
            out.append(o)
        elif o[0] == 16:
            out += [out[-1]] * o[1]
        else:
            out += [0] * o[1]
    return out


class Stream:
    """One DEFLATE stream under construction: the bits, and the symbols they mean (stored bytes count as literals)."""

    def __init__(self):
        self.w = BitWriter()
        self.symbols = []

    # -- blocks ----------------------------------------------------------------------------------------------------
    def stored(self, data, final=False, length=None, nlen=None):
        w = self.w
        w.bits(1 if final else 0, 1)
        w.bits(0, 2)
        w.align()
        length = len(data) if length is None else length
        w.bits(length, 16)
        w.bits((length ^ 0xffff) if nlen is None else nlen, 16)
        w.raw(data)
        self.symbols += list(data)
        return self

    def fixed(self, symbols, final=False, eob=True):
        self.w.bits(1 if final else 0, 1)
        self.w.bits(1, 2)
        self._symbols(symbols, canonical(FIXED_LL), canonical(FIXED_DL), eob)
        return self

    def dynamic(self, symbols, ll, dl, final=False, hlit=None, hdist=None, hclen=None, cl=None, rle=None, eob=True, check=True):
        """ll / dl: the literal / length and the distance code lengths (HLIT / HDIST default to their counts); cl: the 19 lengths
        of the code-length code; rle: how ll + dl are written, a list of lengths 0..15 and (16 | 17 | 18, count)."""
        w = self.w
        hlit = len(ll) if hlit is None else hlit
        hdist = len(dl) if hdist is None else hdist
        cl = list(CL_DEFAULT) if cl is None else list(cl)
        ops = plain_rle(list(ll) + list(dl)) if rle is None else rle
        if hclen is None:
            hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
        if check:
            assert expand_rle(ops) == list(ll) + list(dl), "the run-length coding does not give the lengths"
            assert all(cl[s] == 0 for s in CL_ORDER[hclen:]), "HCLEN cuts a code length off"
        w.bits(1 if final else 0, 1)
        w.bits(2, 2)
        w.bits(hlit - 257, 5)
        w.bits(hdist - 1, 5)
        w.bits(hclen - 4, 4)
        for s in CL_ORDER[:hclen]:
            w.bits(cl[s], 3)
        cc = canonical(cl)
        for o in ops:
            if isinstance(o, int):
                w.code(cc[o])
            else:
                w.code(cc[o[0]])
                if o[0] == 16:
                    w.bits(o[1] - 3, 2)
                elif o[0] == 17:
                    w.bits(o[1] - 3, 3)
                else:
                    w.bits(o[1] - 11, 7)
        self._symbols(symbols, canonical(list(ll) + [0] * (288 - len(ll))), canonical(list(dl) + [0] * (32 - len(dl))), eob)
        return self

    def _symbols(self, symbols, lc, dc, eob):
        w = self.w
        for s in symbols:
            if isinstance(s, int):
                w.code(lc[s])
                self.symbols.append(s)
            elif s[0] == "bits":
                w.bits(s[1], s[2])
            elif s[0] == "L":
                w.code(lc[s[1]])
                if 265 <= s[1] <= 284:
                    w.bits(s[2], LEXTRA[s[1] - 257])
            elif s[0] == "D":
                w.code(dc[s[1]])
                w.bits(s[2], (s[1] >> 1) - 1 if s[1] >= 4 else 0)
            else:
                length, dist = s[0], s[1]
                if len(s) > 2:
                    ls, le = s[2], length - LBASE[s[2] - 257]
                    assert 0 <= le < (1 << LEXTRA[ls - 257])
                else:
                    ls, le = _LSYM[length]
                w.code(lc[ls])
                if LEXTRA[ls - 257]:
                    w.bits(le, LEXTRA[ls - 257])
                ds, de = _dsym(dist)
                w.code(dc[ds])
                if DEXTRA[ds]:
                    w.bits(de, DEXTRA[ds])
                self.symbols.append(s)
        if eob:
            w.code(lc[256])

    # -- results ---------------------------------------------------------------------------------------------------
    def raw(self):
        return self.w.getvalue()

    def expected(self):
        return model(self.symbols)


# ---------------------------------------------------------------- wrappers ----------------------------------------------------
def bgzf_member(raw, payload=None, crc=None, isize=None, bsize=None, extra=None):
    """A BGZF member around a raw DEFLATE stream.  CRC32 / ISIZE default to those of `payload`, BSIZE to the member's size; `extra`
    (a number of bytes, or None) puts a subfield 'XX' of that many bytes in front of 'BC'."""
    sub = b"" if extra is None else b"XX" + struct.pack("<H", extra) + bytes(range(1, extra + 1))
    xlen = len(sub) + 6
    total = 12 + xlen + len(raw) + 8
    assert total <= 65536, "the stream does not fit a BGZF member (%d bytes)" % total
    crc = (zlib.crc32(payload) & 0xffffffff) if crc is None else crc
    isize = len(payload) if isize is None else isize
    return (b"\x1f\x8b\x08\x04" + b"\0\0\0\0" + b"\0\xff" + struct.pack("<H", xlen) + sub + b"BC"
            + struct.pack("<HH", 2, total - 1 if bsize is None else bsize) + raw + struct.pack("<II", crc, isize))


def extra_for_skew(member_off, skew):
    """The size of the extra subfield with which the DEFLATE stream of a member at file offset `member_off` starts at a file
    offset that is `skew` modulo 4 (None: no subfield does it)."""
    if (member_off + 18) & 3 == skew:
        return None
    return (skew - (member_off + 18 + 4)) & 3


def zlib_wrap(raw, payload):
    """RFC 1950: CMF / FLG in front, Adler-32 (big-endian) behind."""
    return b"\x78\x9c" + raw + struct.pack(">I", zlib.adler32(payload) & 0xffffffff)


# ---------------------------------------------------------------- code lengths --------------------------------------------------
def random_lengths(rng, n, long_share, long_lo, max_len=15):
    """n code lengths that satisfy Kraft's equality and are NOT chosen by frequency: a random full binary tree.  About
    `long_share` of the leaves end up `long_lo` bits or more deep (as far as n allows)."""
    if n == 0:
        return []
    if n == 1:
        return [1]
    want_long = int(round(long_share * n))
    depths = [1, 1]
    while len(depths) < n:
        room = n - len(depths)
        deep = [i for i, d in enumerate(depths) if d >= long_lo]
        cand = [i for i, d in enumerate(depths) if d < max_len]
        if len(deep) < want_long and room > 0:
            # go deeper along the deepest leaf that may still split
            i = max(cand, key=lambda k: (depths[k], rng.random()))
            if depths[i] >= long_lo and len(deep) + 1 > want_long:
                i = cand[int(rng.integers(0, len(cand)))]
        else:
            shallow = [i for i in cand if depths[i] < long_lo - 1] or cand
            i = shallow[int(rng.integers(0, len(shallow)))]
        depths[i] += 1
        depths.append(depths[i])
    assert kraft(depths) == 32768
    return [int(depths[i]) for i in rng.permutation(n)]


def spine(n):
    """1, 2, ..., n - 1, n - 1: the complete code with the longest codes n - 1 symbols can get."""
    return list(range(1, n)) + [n - 1]


def lengths_for(nsym, assign):
    """A list of nsym code lengths, zero except assign = {symbol: length}."""
    out = [0] * nsym
    for s, l in assign.items():
        out[s] = l
    return out


# ---------------------------------------------------------------- the seeded re-encoder --------------------------------------
def _common(data, a, p, limit):
    """Length of the common prefix of data[a:] and data[p:], at most limit (a < p; an overlap is what a match copies)."""
    if data[a:a + limit] == data[p:p + limit]:
        return limit
    lo, hi = 0, limit          # data[a:a+lo] equal, data[a:a+hi] not
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if data[a:a + mid] == data[p:p + mid]:
            lo = mid
        else:
            hi = mid
    return lo


def tokenise(payload, rng, literal_share=0.25, max_chain=6):
    """A symbol list whose model is `payload`, with the choices an encoder does not make: among the matches a hash chain finds,
    any candidate (the nearest, the farthest, one in between), any length from 3 to the longest, runs as overlapping matches,
    and a literal where a match exists."""
    n = len(payload)
    table = {}
    syms, p = [], 0
    rnd = rng.random(2 * n + 16).tolist()
    ri = 0

    def insert(q):
        if q + 3 <= n:
            table.setdefault(payload[q:q + 3], []).append(q)

    while p < n:
        cands = table.get(payload[p:p + 3]) if p + 3 <= n else None
        r0, r1 = rnd[ri], rnd[ri + 1]
        ri += 2
        step = 1
        if cands and r0 >= literal_share:
            lo = p - 32768
            pick = cands[-max_chain:] + cands[:2]
            pick = [c for c in pick if c >= lo]
            # an overlapping match: a period of 1..3 right behind the cursor
            for d in (1, 2, 3):
                if p >= d and payload[p - d:p - d + 3] == payload[p:p + 3]:
                    pick.append(p - d)
            if pick:
                a = pick[int(r1 * len(pick))]
                longest = _common(payload, a, p, min(258, n - p))
                if longest >= 3:
                    k = rnd[ri]
                    ri += 1
                    length = longest if k < 0.5 else 3 + int((k - 0.5) * 2 * (longest - 2))
                    if length == 258 and k < 0.25:
                        syms.append((258, p - a, 284))
                    else:
                        syms.append((length, p - a))
                    step = length
        if step == 1:
            syms.append(payload[p])
        for q in range(p, min(p + step, p + 8)):      # (not every position of a long match: the chains stay short)
            insert(q)
        p += step
        if ri > 2 * n:
            rnd = rng.random(2 * n + 16).tolist()
            ri = 0
    return syms


def _used(symbols):
    ls, ds = {256}, set()
    for s in symbols:
        if isinstance(s, int):
            ls.add(s)
        else:
            ls.add(s[2] if len(s) > 2 else _LSYM[s[0]][0])
            ds.add(_dsym(s[1])[0])
    return sorted(ls), sorted(ds)


def encode(payload, rng, long_lit=0.5, long_dist=0.5, literal_share=0.25, block_symbols=(1, 4000), stats=None):
    """`payload` as one DEFLATE stream no encoder would write: tokenise() cut into blocks of random type (dynamic mostly; fixed;
    stored, whose bytes are the model of the symbols they replace), every dynamic block with non-optimal complete code lengths, a
    share of them 12 to 15 bits (literal / length) and 9 to 15 bits (distance).  Returns (raw, symbols); `stats` (a dict) collects
    what the coverage conditions of tests/test_deflate_streams.py count."""
    syms = tokenise(payload, rng, literal_share)
    st = Stream()
    done_bytes = 0
    i = 0
    if stats is None:
        stats = {}
    for k in ("lit12", "len12", "dist9", "overlap", "band0", "band1", "band2", "band3", "blocks"):
        stats.setdefault(k, 0)
    while True:
        n = int(rng.integers(block_symbols[0], block_symbols[1] + 1))
        if rng.random() < 0.15:
            n = int(rng.integers(0, 12))
        blk = syms[i:i + n]
        i += len(blk)
        final = i >= len(syms)
        kind = rng.random()
        blk_bytes = len(model(blk, payload[:done_bytes]))
        stats["blocks"] += 1
        if kind < 0.12 and blk_bytes <= 65535:
            data = payload[done_bytes:done_bytes + blk_bytes]
            st.stored(data, final)
        else:
            if kind < 0.24:
                st.fixed(blk, final)
                ll, dl = FIXED_LL, FIXED_DL
            else:
                ls, ds = _used(blk)
                extra = [int(x) for x in rng.integers(0, 286, int(rng.integers(0, 4)))]      # codes that no symbol uses
                ls = sorted(set(ls) | set(extra))
                if len(ls) == 1:
                    ls = sorted(set(ls) | {0})
                if len(ds) == 1 and rng.random() < 0.5:
                    ds = sorted(set(ds) | {(ds[0] + 1) % 30})
                la = random_lengths(rng, len(ls), long_lit, 12)
                da = random_lengths(rng, len(ds), long_dist, 9)
                hlit = max(257, ls[-1] + 1, int(rng.integers(257, 287)))
                hdist = max(1, (ds[-1] + 1) if ds else 1, int(rng.integers(1, 31)))
                ll = lengths_for(hlit, dict(zip(ls, la)))
                dl = lengths_for(hdist, dict(zip(ds, da)))
                r = rng.random()
                rle = greedy_rle(ll + dl) if r < 0.7 else plain_rle(ll + dl)
                cl_used = sorted({o if isinstance(o, int) else o[0] for o in rle})
                ca = random_lengths(rng, len(cl_used), 0.3, 6, max_len=7) if len(cl_used) > 1 else [1]
                if len(cl_used) == 1:      # the code-length code must be complete: a second code nothing uses
                    cl_used = sorted(set(cl_used) | {(cl_used[0] + 1) % 19})
                    ca = [1, 1]
                cl = lengths_for(19, dict(zip(cl_used, ca)))
                st.dynamic(blk, ll, dl, final, cl=cl, rle=rle)
            for s in blk:
                if isinstance(s, int):
                    stats["lit12"] += ll[s] >= 12
                else:
                    lsym = s[2] if len(s) > 2 else _LSYM[s[0]][0]
                    stats["len12"] += ll[lsym] >= 12
                    stats["dist9"] += dl[_dsym(s[1])[0]] >= 9
            stats["len12"] += ll[256] >= 12
        for s in blk:
            if not isinstance(s, int):
                d = s[1]
                stats["overlap"] += d < s[0]
                stats["band0" if d <= 64 else "band1" if d <= INF_NEAR else "band2" if d <= 4096 else "band3"] += 1
        done_bytes += blk_bytes
        if final:
            break
    assert done_bytes == len(payload)
    return st.raw(), st.symbols


def encode_members(data, rng, chunk=24000, **kw):
    """`data` cut into pieces, each encoded by encode() so that it fits a BGZF member: [(raw, payload, symbols)]."""
    out, p = [], 0
    while p < len(data):
        n = int(rng.integers(chunk // 2, chunk + 1))
        while True:
            piece = data[p:p + n]
            raw, syms = encode(piece, rng, **kw)
            if len(raw) <= MEMBER_CDATA_MAX - 8:
                break
            n = n * 2 // 3
        out.append((raw, piece, syms))
        p += len(piece)
    return out


# ---------------------------------------------------------------- the case tables -----------------------------------------------
class Case:
    """name, family, the raw DEFLATE stream, the bytes it means (None: it must be refused).  For a stream that must be refused:
    `isize` / `crc` of its member, `error`: a pattern the device reader's message must match, `by`: 'zlib' (zlib's decoder raises)
    or 'member' (only the member's CRC32 / ISIZE / size refuse it); `prefix`: CRC32 and ISIZE are those of model(symbols) with the byte
    in front of the member as its window."""

    def __init__(self, name, family, raw, expected=None, symbols=None, isize=None, crc=None, error=None, by="zlib", prefix=False):
        self.name, self.family, self.raw, self.expected, self.symbols = name, family, raw, expected, symbols
        self.isize, self.crc, self.error, self.by, self.prefix = isize, crc, error, by, prefix

    def __repr__(self):
        return "Case(%s/%s)" % (self.family, self.name)


def _case(name, family, st, **kw):
    return Case(name, family, st.raw(), st.expected(), st.symbols, **kw)


def _noise(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def _long_codes():
    fam, out = "long_codes", []
    lits = [0x41 + i for i in range(10)]
    lsyms = [257, 264, 270, 284, 285]
    sp = spine(16)                                   # 10 literals, end-of-block, 5 length symbols: code lengths 1 .. 15, 15
    base = _noise(1, 300)
    for name, order in (("on_literals", [256] + lsyms + lits), ("on_end_of_block", lits[:5] + lsyms + lits[5:] + [256]),
                        ("on_length_symbols", lits + [256] + lsyms)):
        assign = dict(zip(order, sp))
        # the noise in front of it needs codes too: 256 more literals would not leave room for a 1-bit code, so the noise goes
        # into a stored block and the crafted block takes matches from it
        ll = lengths_for(286, assign)
        dl = lengths_for(30, dict(zip([0, 5, 6, 15], [1, 2, 3, 3])))
        body = []
        for k in range(6):
            body += lits + [(3, 1), (10, 10), (24, 200), (258, 7, 284), (258, 200), lits[k]] + lits[::-1]
        st = Stream().stored(base).dynamic(body, ll, dl, final=True)
        out.append(_case(name, fam, st))
    # a run of literals that all take the slow path: one lands on every 256-byte boundary, whatever the member's offset
    assign = dict(zip([256, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 0x61, 0x62], sp))
    ll = lengths_for(257, assign)
    st = Stream().dynamic([0x61, 0x62] * 400 + [1, 2, 0x61], ll, [0], final=True)
    out.append(_case("slow_literals_across_groups_and_last_byte", fam, st))
    st = Stream().dynamic([1, 2, 3, 0x62], ll, [0], final=True)
    out.append(_case("slow_literal_is_the_last_byte", fam, st))
    # distance codes of 1 to 15 bits
    dsyms = [0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 23, 24]
    for name, order in (("distance_long_far", dsyms), ("distance_long_near", dsyms[::-1])):
        dl = lengths_for(30, dict(zip(order, sp)))
        st = Stream().stored(_noise(2, 5000))
        body = []
        for j, s in enumerate(dsyms * 2):
            body.append((3 + 17 * j % 250, DBASE[s] + (j % (1 << DEXTRA[s]) if DEXTRA[s] else 0)))
        st.fixed([], False).dynamic(body, lengths_for(286, {**{s: 5 for s in range(257, 286)}, 256: 5, 0: 4}), dl, final=True)
        out.append(_case(name, fam, st))
    # a single distance code of one bit (incomplete, and allowed), and no distance code at all
    ll = lengths_for(286, {**{s: 6 for s in range(257, 286)}, **{c: 6 for c in range(64, 96)}, 256: 6, 0: 5})
    assert kraft(ll) == 32768
    st = Stream().dynamic([65, 66, 67, (258, 1), (258, 1, 284), (3, 1), 68, (4, 1)], ll, [1], final=True)
    out.append(_case("single_distance_code", fam, st))
    st = Stream().stored(_noise(3, 40)).dynamic([65, (5, 20), (200, 17), (30, 24), 66], ll, lengths_for(9, {8: 1}), final=True)
    out.append(_case("single_distance_code_symbol_8", fam, st))
    st = Stream().dynamic([65, 66, 67, 90, 0, 64], ll, [0], final=True)
    out.append(_case("no_distance_code", fam, st))
    return out


def _literal_runs():
    fam, out = "literal_runs", []
    for bits, total in ((1, 65000), (11, 65000), (12, 65000)):
        if bits == 1:
            ll = lengths_for(257, {0x41: 1, 0x42: 2, 256: 2})
            lit = 0x41
        else:
            # end-of-block 1 bit, literals 2 .. bits - 1, two of `bits`: the larger one has the code of all ones
            order = [256] + list(range(0x30, 0x30 + bits - 2)) + [0x7a, 0x7b]
            ll = lengths_for(257, dict(zip(order, list(range(1, bits)) + [bits, bits])))
            lit = 0x7b
        assert kraft(ll) == 32768 and (bits == 1 or canonical(ll)[lit] == ((1 << bits) - 1, bits))
        per = min(total, (MEMBER_CDATA_MAX - 200) * 8 // bits)
        nmem = -(-total // per)
        for k in range(nmem):
            n = total // nmem
            st = Stream().dynamic([lit] * n, ll, [0], final=True, rle=greedy_rle(ll + [0]))
            out.append(_case("%d_bit_code_x%d_part%d" % (bits, n, k), fam, st))
    return out


GEOM_LENGTHS = [3, 4, 63, 64, 65, 128, 129, 257, 258]
GEOM_DISTANCES = [1, 2, 3, 63, 64, 65, 3773, 3774, 3775, 4095, 4096, 4097, 32767, 32768]


def _match_geometry():
    fam, out = "match_geometry", []
    # every length at every distance; 258 both ways.  Noise in front so that a wrong source shows.
    near = [d for d in GEOM_DISTANCES if d <= 4097]
    st = Stream().stored(_noise(4, 4100))
    body = []
    for length in GEOM_LENGTHS:
        for d in near + [length - 1, length, length + 1]:
            if d >= 1:
                body.append((length, d))
                body.append(length & 255)
        body.append((258, 100, 284))
    body += [(258, d, 284) for d in near]
    st.fixed(body, final=True)
    out.append(_case("lengths_x_distances_to_4097", fam, st))
    st = Stream().stored(_noise(5, 32768))
    body = []
    for length in GEOM_LENGTHS:
        for d in (32767, 32768, 4097, 3775, 3774):
            body += [(length, d), 7]
    body += [(258, 32768, 284), (258, 32767, 284)]
    st.fixed(body, final=True)
    out.append(_case("lengths_x_distances_to_32768", fam, st))
    # a distance equal to the whole output so far, near and far, and again and again (every one reaches the member's first byte)
    body = [10, 20, 30]
    n = 3
    while n < 30000:
        length = min(258, n if n % 2 else max(3, n // 2))
        body.append((length, n))
        n += length
        body.append(n & 255)
        n += 1
    st = Stream().fixed(body, final=True)
    out.append(_case("distance_reaches_the_first_byte", fam, st))
    # far matches whose source is the member's first bytes (its first, partial 256-byte group)
    st = Stream().stored(_noise(6, 3800))
    body, n = [], 3800
    for k in range(12):
        body.append((20 + 19 * k, n - 3 * k))
        n += 20 + 19 * k
    st.fixed(body, final=True)
    out.append(_case("far_source_in_the_first_group", fam, st))
    # matches of 258 (and a literal) from every phase against the 256-byte groups: one that begins on a boundary, one that
    # completes a group, one that completes two; the last match ends the member
    st = Stream().stored(_noise(7, 260))
    body, n = [], 260
    ds = [1, 258, 259, 200, 3774, 3775, 4096, 257]
    for k in range(250):
        d = ds[k % len(ds)]
        body.append((258, d if d <= n else 260))
        n += 258
        if k < 249:
            body.append(k & 255)
            n += 1
    st.fixed(body, final=True)
    out.append(_case("every_phase_and_a_match_that_ends_the_member", fam, st))
    st = Stream().stored(_noise(8, 10))
    body = []
    for k in range(256):
        body += [(4, 5 + (k % 4)), k]
    st.fixed(body + [(3, 3)], final=True)
    out.append(_case("short_matches_from_every_phase", fam, st))
    return out


def _stored_blocks():
    fam, out = "stored_blocks", []
    noise = _noise(9, 70000)
    st, p = Stream(), 0
    st.stored(b"")
    for n in (1, 63, 64, 65, 255, 256, 257, 0, 4000, 2, 3):
        st.stored(noise[p:p + n])
        p += n
    st.fixed([(40, 5), (258, 100), (100, 3800), (258, 4700), (3, 1), (258, 4096, 284)])
    st.stored(noise[p:p + 300]).fixed([(258, 250), (258, 6000)]).stored(b"", final=True)
    out.append(_case("lengths_in_a_row_and_matches_into_them", fam, st))
    # behind a fixed block that ends at each of the 8 bit offsets: 3 + 9 k + 7 bits, k nine-bit literals
    st = Stream()
    for k in range(8):
        before = st.w.bitpos
        st.fixed([200 + k] * k)
        assert (st.w.bitpos - before) % 8 == (2 + k) % 8
        st.stored(noise[100 * k:100 * k + 5 + k])
    st.fixed([(30, 7)], final=True)
    out.append(_case("at_every_bit_offset", fam, st))
    big = MEMBER_CDATA_MAX - 7 - 5          # (room for the largest extra subfield the tests put in front)
    st = Stream().stored(noise[:big], final=True)
    out.append(_case("largest_len_of_a_member", fam, st))
    st = Stream().stored(noise[:40000]).stored(b"").stored(noise[1:300]).fixed([(258, 32768), (258, 4097), (100, 300)], final=True)
    out.append(_case("stored_then_far_matches", fam, st))
    return out


def _dynamic_headers():
    fam, out = "dynamic_headers", []
    body = [65, 66, 67, (10, 2), 68, (258, 3, 284), 0, 255, (5, 13)]
    # HCLEN 5 is the least a block can have: with HCLEN 4 only 16, 17, 18 and 0 have codes, every length is 0, and there is no
    # end-of-block code (INVALID has that stream).  Lengths 0 and 8 only: 256 codes of 8 bits.
    ll = [0] + [8] * 256
    st = Stream().dynamic([1, 2, 3, 255, 77], ll, [0], final=True, hclen=5, cl=lengths_for(19, {0: 1, 8: 1}))
    out.append(_case("hclen_5_hlit_257_hdist_1", fam, st))
    ll286 = lengths_for(286, {**{s: 9 for s in range(0, 256)}, **{s: 6 for s in range(257, 286)}, 256: 5})
    ll286[257] = 5
    assert kraft(ll286) == 32768, kraft(ll286)
    dl30 = [5] * 28 + [4] * 2
    assert kraft(dl30) == 32768
    cl19 = lengths_for(19, {s: 4 for s in range(13)})
    for s in range(13, 19):
        cl19[s] = 5
    st = Stream().stored(_noise(10, 20)).dynamic(body, ll286, dl30, final=True, hclen=19, cl=cl19)
    out.append(_case("hclen_19_hlit_286_hdist_30", fam, st))
    # a code-length code with 7-bit codes; every repeat code with its smallest and its largest count
    rle = [7, (16, 3), 8, (16, 6), (17, 3), 9, (17, 10), 8, (16, 3), (18, 11), 9, 9, 9, (18, 138), (18, 75),
           7, 1, 2, 3, 5, 8,          # end-of-block, 257 .. 261
           2, (16, 3)]
    seq = expand_rle(rle)
    ll, dl = seq[:262], seq[262:]
    assert len(dl) == 4 and kraft(ll) == 32768 and kraft(dl) == 32768
    cl = lengths_for(19, dict(zip([1, 2, 3, 5, 7, 8, 9, 16, 17, 18], [7, 7, 6, 5, 3, 2, 3, 2, 3, 4])))
    assert kraft(cl) == 32768
    sy = [0, 5, 14, 26, 41, (3, 1), (4, 2), (5, 3), (6, 4), (7, 1), 42, 3]
    st = Stream().dynamic(sy, ll, dl, final=True, cl=cl, rle=rle)
    out.append(_case("cl_code_of_7_bits_and_every_repeat_count", fam, st))
    # a run of 16 that crosses from the literal / length lengths into the distance lengths; a run of 18 that ends at HLIT + HDIST
    ll = [8] * 240 + [0] * 16 + [6] * 4
    dl = [6, 6, 1, 2, 3, 4, 5] + [0] * 12
    assert kraft(ll) == 32768 and kraft(dl) == 32768
    rle = [8, (16, 6)] * 34 + [8, 8, (18, 16), 6, (16, 5), 1, 2, 3, 4, 5, (18, 12)]
    sy = [0, 1, 239, 5, 6, 7, 8, 9, 10, (3, 1), (4, 2), (5, 3), (5, 4), (3, 5), (3, 7), (3, 9)]
    st = Stream().dynamic(sy, ll, dl, final=True, rle=rle)
    out.append(_case("run_16_across_hlit_and_run_18_to_the_end", fam, st))
    return out


def _many_blocks():
    fam, out = "many_blocks", []
    st = Stream()
    for _ in range(1000):
        st.fixed([])
    st.fixed(list(b"after a thousand empty blocks") + [(20, 5)], final=True)
    out.append(_case("thousand_empty_fixed_blocks", fam, st))
    # stored / fixed / dynamic every few bytes; the dynamic tables alternate between long and short codes, and between alphabets
    rng = np.random.default_rng(11)
    st = Stream()
    lits_a = list(range(0x41, 0x41 + 10))
    long_ll = lengths_for(286, dict(zip([256] + lits_a + [257, 258, 284, 285, 260], spine(16))))
    short_ll = lengths_for(270, dict(zip([0x41, 0x30, 256, 258], [2, 2, 2, 2])))
    long_dl = lengths_for(30, dict(zip([0, 1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 23, 24], spine(16))))
    short_dl = lengths_for(4, {0: 1, 3: 1})
    st.stored(_noise(12, 4200))
    for k in range(120):
        t = k % 4
        if t == 0:
            st.stored(bytes(rng.integers(0, 256, int(rng.integers(0, 9)), dtype=np.uint8)))
        elif t == 1:
            st.dynamic(lits_a + [(3, 4097), (258, 1, 284), (4, 24), lits_a[k % 10], (6, 3000)], long_ll, long_dl)
        elif t == 2:
            st.fixed([k, (3, 1), 255 - k])
        else:
            st.dynamic([0x41, 0x30, (4, 1), (4, 4), 0x30], short_ll, short_dl)
    st.fixed([], final=True)
    out.append(_case("alternating_block_types_and_tables", fam, st))
    return out


MEMBER_SIZES = [0, 1, 15, 16, 17, 255, 256, 257, 65535, 65536]


def _member_sizes():
    fam, out = "member_sizes", []
    rng = np.random.default_rng(13)
    piece = _noise(14, 700)
    for n in MEMBER_SIZES:
        data = (piece * (n // len(piece) + 1))[:n]
        if n == 0:
            st = Stream().fixed([], final=True)
            out.append(_case("isize_0", fam, st))
            continue
        raw, syms = encode(data, rng, long_lit=0.3, long_dist=0.4)
        assert len(raw) <= MEMBER_CDATA_MAX - 8
        out.append(Case("isize_%d" % n, fam, raw, data, syms))
    return out


def _valid():
    out = []
    for f in (_long_codes, _literal_runs, _match_geometry, _stored_blocks, _dynamic_headers, _many_blocks, _member_sizes):
        out += f()
    names = [(c.family, c.name) for c in out]
    assert len(set(names)) == len(names)
    return out


# messages of the device reader (the table in bam_device.hip)
E_ANY = "DEFLATE|BGZF block"
E_BTYPE = "reserved block type"
E_STORED = "LEN != ~NLEN"
E_TABLE = "malformed Huffman code lengths"
E_CODE = "no Huffman code of its block"
E_DIST = "match distance beyond the start"
E_OUTPUT = "more output than ISIZE"
E_ISIZE = "does not inflate to its recorded size"
E_CRC = "CRC32 mismatch"

LL_OK = lengths_for(286, {**{c: 6 for c in range(64, 96)}, **{s: 6 for s in range(257, 286)}, 256: 6, 0: 5})
DL_OK = [5] * 28 + [4] * 2


def _invalid():
    out = []

    def bad(name, st, error, isize=10, by="zlib", symbols=None, **kw):
        out.append(Case(name, "invalid", st.raw(), None, symbols, isize=isize, error=error, by=by, **kw))

    st = Stream()
    st.w.bits(1, 1)
    st.w.bits(3, 2)
    st.w.bits(0, 29)
    bad("reserved_block_type", st, E_BTYPE)
    bad("stored_len_is_not_nlen", Stream().stored(b"0123456789", final=True, nlen=0x1234), E_STORED)
    # over-subscribed: one code too many
    over = list(LL_OK)
    over[2] = 6
    bad("oversubscribed_literal_code", Stream().dynamic([65], over, DL_OK, final=True), E_TABLE)
    bad("oversubscribed_distance_code", Stream().dynamic([65], LL_OK, [4] * 3 + [5] * 27, final=True), E_TABLE)
    cl = list(CL_DEFAULT)
    cl[0] = 3
    bad("oversubscribed_code_length_code", Stream().dynamic([65], LL_OK, DL_OK, final=True, cl=cl), E_TABLE)
    # incomplete: one code missing.  The symbols that are used all have codes: a decoder that accepts the set decodes the
    # stream to 10 bytes, and the member's CRC32 and ISIZE are those of these bytes -- only the code lengths refuse it.
    ten = [65, 66, 67, 68, 69, (5, 5)]
    inc = list(LL_OK)
    inc[95] = 0
    bad("incomplete_literal_code", Stream().dynamic(ten, inc, DL_OK, final=True), E_TABLE, crc=zlib.crc32(model(ten)))
    bad("incomplete_distance_code", Stream().dynamic(ten, LL_OK, [5] * 27 + [0] + [4] * 2, final=True), E_TABLE,
        crc=zlib.crc32(model(ten)))
    bad("incomplete_distance_code_of_two_codes", Stream().dynamic(ten, LL_OK, lengths_for(8, {4: 2, 7: 2}), final=True), E_TABLE,
        crc=zlib.crc32(model(ten)))
    bad("incomplete_distance_code_of_one_2_bit_code", Stream().dynamic(ten, LL_OK, lengths_for(8, {4: 2}), final=True), E_TABLE,
        crc=zlib.crc32(model(ten)))
    cl = list(CL_DEFAULT)
    cl[18] = 0
    bad("incomplete_code_length_code", Stream().dynamic(ten, LL_OK, DL_OK, final=True, cl=cl), E_TABLE, crc=zlib.crc32(model(ten)))
    bad("repeat_16_first", Stream().dynamic([], LL_OK, DL_OK, final=True, rle=[(16, 3)] + LL_OK[3:] + DL_OK, check=False), E_TABLE)
    bad("repeat_beyond_hlit_hdist", Stream().dynamic([], LL_OK, DL_OK, final=True, rle=LL_OK + DL_OK[:-2] + [(16, 3)], check=False),
        E_TABLE)
    noeob = list(LL_OK)
    noeob[256] = 0
    noeob[2] = 5
    bad("no_end_of_block_code", Stream().dynamic([65], noeob, DL_OK, final=True, eob=False), E_TABLE)
    bad("hclen_4", Stream().dynamic([], [0] * 257, [0], final=True, hclen=4, cl=lengths_for(19, {0: 1, 18: 1}),
                                    rle=[(18, 138), (18, 120)], eob=False), E_TABLE)
    # allowed incomplete sets, and the bit pattern that is none of their codes
    one = lengths_for(257, {256: 1})
    bad("pattern_outside_a_single_literal_code", Stream().dynamic([("bits", 1, 1), ("bits", 0, 30)], one, [0], final=True, eob=False),
        E_CODE)
    bad("pattern_outside_a_single_distance_code",
        Stream().dynamic([65, 66, 67, ("L", 257, 0), ("bits", 1, 1), ("bits", 0, 30)], LL_OK, [1], final=True), E_CODE)
    bad("match_without_any_distance_code", Stream().dynamic([65, 66, 67, ("L", 257, 0), ("bits", 0, 30)], LL_OK, [0], final=True),
        E_CODE)
    for s in (30, 31):
        bad("fixed_distance_symbol_%d" % s, Stream().fixed([65] * 9 + [("L", 257, 0), ("D", s, 0)], final=True), E_DIST)
        bad("dynamic_hdist_%d" % (s + 1), Stream().dynamic([65], LL_OK, DL_OK + [0] * (s - 29), final=True, check=False), E_TABLE)
    for s in (286, 287):
        bad("fixed_length_symbol_%d" % s, Stream().fixed([65] * 9 + [("L", s, 0), ("D", 0, 0)], final=True), E_DIST)
    # a distance one byte beyond the member's start, in a member that is not the first: CRC32 and ISIZE are those of the bytes a
    # decoder without the test would produce (`prefix`: the byte in front of the member), so only the distance test refuses it
    bad("distance_one_beyond_the_member_start", Stream().fixed([65, 66, 67, ("L", 257, 0), ("D", 3, 0)], final=True), E_DIST,
        isize=6, prefix=True, symbols=[65, 66, 67, (3, 4)])
    # more output than ISIZE
    bad("literal_beyond_isize", Stream().fixed([65] * 11, final=True), E_OUTPUT, by="member")
    bad("match_beyond_isize", Stream().fixed([65] * 8 + [(3, 1)], final=True), E_OUTPUT, by="member")
    bad("stored_beyond_isize", Stream().fixed([65] * 8).stored(b"abc", final=True), E_OUTPUT, by="member")
    bad("many_literals_beyond_isize", Stream().fixed([65] * 2000, final=True), E_OUTPUT, by="member")
    bad("no_end_of_block_runs_into_the_trailer", Stream().fixed([65] * 10, final=True, eob=False), E_ANY, by="member")
    ok = Stream().fixed(list(b"0123456789"), final=True)
    good_crc = zlib.crc32(b"0123456789")
    bad("isize_too_small_crc_right", ok, E_OUTPUT, isize=9, by="member", crc=good_crc)
    bad("isize_too_large_crc_right", ok, E_ISIZE, isize=11, by="member", crc=good_crc)
    bad("crc_wrong_isize_right", ok, E_CRC, isize=10, by="member", crc=good_crc ^ 0x100)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return out


_CACHE = {}


def valid_cases():
    if "v" not in _CACHE:
        _CACHE["v"] = _valid()
    return _CACHE["v"]


def invalid_cases():
    if "i" not in _CACHE:
        _CACHE["i"] = _invalid()
    return _CACHE["i"]


def __getattr__(name):          # VALID / INVALID: built on first use (the literal runs take a second of Python)
    if name == "VALID":
        return valid_cases()
    if name == "INVALID":
        return invalid_cases()
    raise AttributeError(name)


# ---------------------------------------------------------------- files ---------------------------------------------------------
REFS = [("c1", 1 << 28)]


def carrier_record(pos0, payload_len, pad):
    """The front of a BAM record whose tail is `payload_len` bytes that follow in the stream (they count as the record's tags, which
    no reader parses): the inflated stream of a file of crafted members stays a chain of records, so that the host reader and the
    device reader's record walk read it too.  40 + pad bytes, 1 <= pad <= 255; the record reads as 10M at pos0, mapq 30."""
    assert 1 <= pad <= 255
    name = b"n" * (pad - 1) + b"\0"
    body = struct.pack("<iiBBHHHiiii", 0, pos0, len(name), 30, 4680, 1, 0, 0, -1, -1, 0) + name + struct.pack("<I", 10 << 4)
    return struct.pack("<i", len(body) + payload_len) + body


def header_member(level=6):
    from . import io_writers as W
    return W.bgzf_block(W.bam_header(REFS), level), W.bam_header(REFS)


def crafted_header_member(skew=None):
    """The BAM header as a member of its own whose stream holds a match that reaches the first byte of the FILE's output: the
    text's "BAM" is a copy of the magic, 12 bytes back."""
    from . import io_writers as W
    hbytes = W.bam_header(REFS, "@CO\tBAM\n@SQ\tSN:%s\tLN:%d\n" % REFS[0])
    assert hbytes[12:15] == b"BAM"
    st = Stream().fixed(list(hbytes[:12]) + [(3, 12)] + list(hbytes[15:]), final=True)
    assert st.expected() == hbytes
    return bgzf_member(st.raw(), hbytes, extra=None if skew is None else extra_for_skew(0, skew)), hbytes


def geometry(symbols, pstart):
    """What the matches of a member whose output starts at `pstart` modulo 256 do against the 256-byte groups of the output."""
    seen, pos = set(), pstart & 255
    for s in symbols:
        if isinstance(s, int):
            pos += 1
            continue
        if pos & 255 == 0:
            seen.add("begins_on_a_boundary")
        done = ((pos + s[0]) >> 8) - (pos >> 8)
        if done:
            seen.add("completes_%d" % done)
        if (pos + s[0]) & 255 == 0:
            seen.add("ends_on_a_boundary")
        if s[1] > INF_NEAR and pos - s[1] < 256:          # (positions count from the group the member starts in)
            seen.add("far_source_in_the_first_group")
        pos += s[0]
    if symbols and not isinstance(symbols[-1], int):
        seen.add("ends_the_member")
    return seen


class CraftedFile:
    """data: the file; want: its inflated stream; where: [(case, offset of its output in the stream)]; reads: the records of the
    stream as a reader's batches give them."""

    def __init__(self, data, want, where, reads):
        self.data, self.want, self.where, self.reads = data, want, where, reads

    def first_difference(self, got):
        """'' if `got` is the inflated stream, else which case's output differs first, and where."""
        if got == self.want:
            return ""
        n = min(len(got), len(self.want))
        first = next((i for i in range(n) if got[i] != self.want[i]), n)
        name = "the header or a carrier record"
        for c, off in self.where:
            if off <= first < off + max(len(c.expected), 1):
                name = "%s/%s, byte %d of its %d" % (c.family, c.name, first - off, len(c.expected))
        return "first difference at byte %d of %d / %d (%s)" % (first, len(got), len(self.want), name)


def build_file(cases, skew=None, phases=(0,), header=None):
    """header member, then for every case a carrier member (a zlib-written record front, whose length sets the case's output
    offset: phases[i % len] modulo 256) and the case's member (DEFLATE stream at `skew` modulo 4 in the file), then the EOF member."""
    from . import io_writers as W
    hm, hbytes = header if header is not None else header_member()
    parts, want, where, reads = [hm], [hbytes], [], []
    off, out_off = len(hm), len(hbytes)
    for i, c in enumerate(cases):
        exp = c.expected
        phase = phases[i % len(phases)]
        pad = (phase - (out_off + 40)) & 255
        if pad:
            front = carrier_record(1000 + i, len(exp), pad)
            reads.append((False, REFS[0][0], 1001 + i, 10))
        else:          # (256 bytes: two records)
            front = carrier_record(1000 + i, 0, 128) + carrier_record(1000 + i, len(exp), 128 - 40)
            reads += [(False, REFS[0][0], 1001 + i, 10)] * 2
        fm = W.bgzf_block(front)
        parts.append(fm)
        want.append(front)
        off += len(fm)
        out_off += len(front)
        assert (out_off & 255) == phase
        m = bgzf_member(c.raw, exp, extra=None if skew is None else extra_for_skew(off, skew))
        assert skew is None or (off + len(m) - 8 - len(c.raw)) & 3 == skew
        parts.append(m)
        want.append(exp)
        where.append((c, out_off))
        off += len(m)
        out_off += len(exp)
    return CraftedFile(b"".join(parts) + W.BGZF_EOF, b"".join(want), where, reads)


def build_invalid_file(c):
    """A header member, a carrier, the member that must be refused, the EOF member."""
    from . import io_writers as W
    hm, hbytes = header_member()
    front = carrier_record(7, c.isize, 20)
    payload = None
    crc = c.crc
    if c.prefix:
        payload = model(c.symbols, front[-1:])
        crc = zlib.crc32(payload)
    m = bgzf_member(c.raw, payload, crc=(crc if crc is not None else 0x12345678) & 0xffffffff, isize=c.isize)
    return hm + W.bgzf_block(front) + m + W.BGZF_EOF
