"""TEST INFRASTRUCTURE: a plain inflate (RFC 1950 / 1951) that keeps the structure of what it reads -- blocks, headers, the header's
operations as written, every token with its place and width in the stream -- and refuses what the format forbids.  It is the
oracle of the tests that look inside an encoder's streams (tests/test_gpu_deflate_dissect.py, tests/test_deflate_codes.py), so it
shares nothing with an encoder: the tables come from tests/deflate_streams.py, and tests/test_deflate_dissect.py holds it against
zlib's decoder.  Pure Python; 64 KB of literals take a few tenths of a second.

Behind it, the reference code lengths the same tests judge an encoder by: the Huffman optimum (a leaf wins a tie) and the optimum
under a length limit (package-merge), both as plain restatements over lists of counts."""
import heapq
import struct
import zlib

from .deflate_streams import (CL_ORDER, DBASE, DEXTRA, FIXED_DL, FIXED_LL, LBASE, LEXTRA, canonical, expand_rle, greedy_rle, kraft)


class Invalid(ValueError):
    """The stream is not one RFC 1950 / 1951 allows."""


class Block:
    """One DEFLATE block.  first_bit: where its BFINAL bit lies in the stream (bit 0 = the least significant bit of the stream's first
    byte); bits: from there to behind its end-of-block code (stored: behind its last byte).  tokens: (bit offset, bits, literal) or
    (bit offset, bits, (length, distance, length symbol, distance symbol)); eob: (bit offset, bits) of the end-of-block code.
    Dynamic: hlit, hdist, hclen, cl (19 lengths), ops (lengths 0 .. 15 and (16 | 17 | 18, count), as written), ll, dl (the declared
    lengths), header_bits (everything between the three block bits and the first token).  Stored: pad (the bits skipped), length."""

    def __init__(self, final, btype, first_bit):
        self.final, self.btype, self.first_bit = final, btype, first_bit
        self.bits = 0
        self.tokens, self.eob = [], None
        self.hlit = self.hdist = self.hclen = None
        self.cl = self.ops = self.ll = self.dl = None
        self.header_bits = 0
        self.pad = self.pad_value = 0
        self.length = None

    @property
    def token_bits(self):
        return sum(t[1] for t in self.tokens)


class Dissection:
    """cmf, flg, adler (None for a raw stream), blocks, data (the decoded bytes), pad / pad_value (the bits between the last block and
    the next byte boundary), end_bit (behind the last block)."""

    def __init__(self):
        self.cmf = self.flg = self.adler = None
        self.blocks, self.data = [], b""
        self.pad = self.pad_value = self.end_bit = 0

    @property
    def tokens(self):
        return [t for b in self.blocks for t in b.tokens]


def _rev(code, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (code & 1)
        code >>= 1
    return r


def _table(lens, what, single_ok):
    """(table, width): table[the next `width` bits of the stream] = symbol << 4 | length, or -1 where no code begins so.  Refuses an
    over-subscribed set, and an incomplete one unless it is a single code of one bit and `single_ok`.  No code at all: (None, 0)."""
    used = [l for l in lens if l]
    if not used:
        return None, 0
    k = kraft(lens)
    if k > 32768:
        raise Invalid("over-subscribed %s code" % what)
    if k < 32768 and not (single_ok and used == [1]):
        raise Invalid("incomplete %s code" % what)
    width = max(used)
    tab = [-1] * (1 << width)
    for sym, c in enumerate(canonical(lens)):
        if c is not None:
            code, l = c
            n = 1 << (width - l)
            tab[_rev(code, l)::1 << l] = [sym << 4 | l] * n
    return tab, width


_FIXED = []


def _fixed_tables():
    if not _FIXED:
        _FIXED.append((_table(FIXED_LL, "fixed", False), _table(FIXED_DL, "fixed distance", False)))
    return _FIXED[0]


def _inflate(buf, pos, limit, d):
    """The blocks of buf from bit `pos` on, none of them beyond bit `limit`, into d; returns the bit behind the last one."""
    data = bytes(buf) + b"\0" * 8
    out = bytearray()
    frm = int.from_bytes

    def take(n):
        nonlocal pos
        v = (frm(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << n) - 1)
        pos += n
        if pos > limit:
            raise Invalid("the stream ends inside a block")
        return v

    def sym(tab, width, what):
        nonlocal pos
        e = tab[(frm(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & ((1 << width) - 1)]
        if e < 0:
            raise Invalid("a bit pattern that is no %s code" % what)
        pos += e & 15
        if pos > limit:
            raise Invalid("the stream ends inside a block")
        return e >> 4

    while True:
        first = pos
        final = take(1)
        b = Block(bool(final), take(2), first)
        d.blocks.append(b)
        if b.btype == 3:
            raise Invalid("reserved block type")
        if b.btype == 0:
            b.pad = -pos & 7
            b.pad_value = take(b.pad)
            length, nlen = take(16), take(16)
            if length != nlen ^ 0xffff:
                raise Invalid("LEN != ~NLEN")
            if pos + 8 * length > limit:
                raise Invalid("the stream ends inside a stored block")
            b.length = length
            out += data[pos >> 3:(pos >> 3) + length]
            pos += 8 * length
            b.bits = pos - first
            if final:
                return pos, bytes(out)
            continue
        if b.btype == 1:
            (lt, lw), (dt, dw) = _fixed_tables()
        else:
            b.hlit, b.hdist, b.hclen = take(5) + 257, take(5) + 1, take(4) + 4
            if b.hlit > 286 or b.hdist > 30:
                raise Invalid("HLIT %d / HDIST %d: too many symbols" % (b.hlit, b.hdist))
            b.cl = [0] * 19
            for s in CL_ORDER[:b.hclen]:
                b.cl[s] = take(3)
            ct, cw = _table(b.cl, "code-length", False)
            if ct is None:
                raise Invalid("no code-length code at all")
            b.ops, n, total = [], 0, b.hlit + b.hdist
            last = None
            while n < total:
                s = sym(ct, cw, "code-length")
                if s < 16:
                    b.ops.append(s)
                    last = s
                    n += 1
                    continue
                if s == 16:
                    if last is None:
                        raise Invalid("a repeat with no length in front of it")
                    k = 3 + take(2)
                elif s == 17:
                    k = 3 + take(3)
                    last = 0
                else:
                    k = 11 + take(7)
                    last = 0
                b.ops.append((s, k))
                n += k
            if n > total:
                raise Invalid("a repeat beyond HLIT + HDIST")
            lens = expand_rle(b.ops)
            b.ll, b.dl = lens[:b.hlit], lens[b.hlit:]
            if not b.ll[256]:
                raise Invalid("no end-of-block code")
            lt, lw = _table(b.ll, "literal / length", True)
            dt, dw = _table(b.dl, "distance", True)
            b.header_bits = pos - first - 3
        tokens = b.tokens
        lmask = (1 << lw) - 1
        while True:
            at = pos
            e = lt[(frm(data[pos >> 3:(pos >> 3) + 4], "little") >> (pos & 7)) & lmask]
            if e < 0:
                raise Invalid("a bit pattern that is no literal / length code")
            pos += e & 15
            s = e >> 4
            if s < 256:
                out.append(s)
                tokens.append((at, e & 15, s))
                continue
            if pos > limit:
                raise Invalid("the stream ends inside a block")
            if s == 256:
                b.eob = (at, pos - at)
                break
            if s > 285:
                raise Invalid("length symbol %d" % s)
            length = LBASE[s - 257] + (take(LEXTRA[s - 257]) if LEXTRA[s - 257] else 0)
            if dt is None:
                raise Invalid("a match in a block without a distance code")
            ds = sym(dt, dw, "distance")
            if ds > 29:
                raise Invalid("distance symbol %d" % ds)
            dist = DBASE[ds] + (take(DEXTRA[ds]) if DEXTRA[ds] else 0)
            if dist > len(out):
                raise Invalid("a distance of %d with %d bytes of output" % (dist, len(out)))
            if dist >= length:
                out += out[len(out) - dist:len(out) - dist + length]
            else:
                for _ in range(length):
                    out.append(out[-dist])
            tokens.append((at, pos - at, (length, dist, s, ds)))
        if pos > limit:
            raise Invalid("the stream ends inside a block")
        b.bits = pos - first
        if final:
            return pos, bytes(out)


def dissect_raw(raw):
    """A raw DEFLATE stream (RFC 1951) from bit 0 on; what lies behind its last block's byte is not looked at."""
    d = Dissection()
    d.end_bit, d.data = _inflate(raw, 0, 8 * len(raw), d)
    d.pad = -d.end_bit & 7
    d.pad_value = (raw[d.end_bit >> 3] >> (d.end_bit & 7)) if d.pad else 0
    return d


def dissect(stream):
    """One zlib stream (RFC 1950), the whole of `stream`: header, blocks, padding to the byte, Adler-32 -- and nothing else."""
    stream = bytes(stream)
    if len(stream) < 6:
        raise Invalid("shorter than a header and an Adler-32")
    d = Dissection()
    d.cmf, d.flg = stream[0], stream[1]
    if d.cmf & 15 != 8 or d.cmf >> 4 > 7 or (d.cmf << 8 | d.flg) % 31 or d.flg & 0x20:
        raise Invalid("CMF / FLG %02x %02x" % (d.cmf, d.flg))
    d.end_bit, d.data = _inflate(stream[:-4], 16, 8 * (len(stream) - 4), d)
    d.pad = -d.end_bit & 7
    d.pad_value = (stream[d.end_bit >> 3] >> (d.end_bit & 7)) if d.pad else 0
    if (d.end_bit + d.pad) // 8 + 4 != len(stream):
        raise Invalid("%d bytes behind the last block, not the 4 of an Adler-32" % (len(stream) - (d.end_bit + d.pad) // 8))
    d.adler = struct.unpack(">I", stream[-4:])[0]
    if d.adler != zlib.adler32(d.data) & 0xffffffff:          # (the sum itself is RFC 1950's; the test holds it against the bytes)
        raise Invalid("Adler-32 mismatch")
    return d


def chained_rle(lens):
    """deflate_streams.greedy_rle with one rule changed, the rule of the device encoder's header: behind a length and its first
    (16, n), the rest of a run of that length goes on with (16, n) while 3 or more remain (code 16 repeats the PREVIOUS length,
    which still is that length), where greedy_rle writes the length again before every 16.  The two are the same list whenever no
    non-zero run is longer than 9; a longer run is never more operations this way."""
    ops, i = [], 0
    while i < len(lens):
        v, j = lens[i], i
        while j < len(lens) and lens[j] == v:
            j += 1
        run, i = j - i, j
        if v:
            ops.append(v)
            run -= 1
        while run:
            if v == 0 and run >= 3:
                n = min(run, 138)
                ops.append((18, n) if n >= 11 else (17, n))
            elif v and run >= 3:
                n = min(run, 6)
                ops.append((16, n))
            else:
                n = 1
                ops.append(v)
            run -= n
    return ops


# ---------------------------------------------------------------- reference code lengths ----------------------------------------
def huffman_lengths(freq):
    """The code lengths of a Huffman tree over the used symbols of freq (count > 0), with the two-queue rule that a leaf wins a
    tie against an inner node: among the optimal trees that is the one of least depth (and least variance).  One used symbol: 1."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    out = [0] * len(freq)
    if len(used) == 1:
        out[used[0][1]] = 1
    if len(used) < 2:
        return out
    # (weight, kind, serial): kind 0 = leaf, 1 = inner, so a leaf wins a tie; inner nodes among themselves in the order made
    heap = [(f, 0, i) for i, (f, _s) in enumerate(used)]
    heapq.heapify(heap)
    parent, serial = {}, len(used)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        parent[a[1:]] = parent[b[1:]] = (1, serial)
        heapq.heappush(heap, (a[0] + b[0], 1, serial))
        serial += 1
    for i, (_f, s) in enumerate(used):
        node, depth = (0, i), 0
        while node in parent:
            node, depth = parent[node], depth + 1
        out[s] = depth
    return out


def package_merge(freq, maxbits):
    """Optimal code lengths of at most maxbits for the used symbols of freq (Larmore and Hirschberg's package-merge, the plain
    list form): the lengths of a minimum-cost complete code under the limit.  One used symbol: 1."""
    used = sorted((f, s) for s, f in enumerate(freq) if f)
    out = [0] * len(freq)
    m = len(used)
    if m == 1:
        out[used[0][1]] = 1
    if m < 2:
        return out
    assert m <= 1 << maxbits
    leaves = [(f, (i,)) for i, (f, _s) in enumerate(used)]
    packages = []
    for _ in range(maxbits - 1):
        merged = sorted(leaves + packages, key=lambda x: x[0])
        packages = [(merged[k][0] + merged[k + 1][0], merged[k][1] + merged[k + 1][1]) for k in range(0, len(merged) - 1, 2)]
    merged = sorted(leaves + packages, key=lambda x: x[0])
    for _w, items in merged[:2 * m - 2]:
        for i in items:
            out[used[i][1]] += 1
    return out


def cost(freq, lens):
    return sum(f * l for f, l in zip(freq, lens))


def token_histograms(tokens):
    """(counts of the 286 literal / length symbols with the end-of-block symbol, counts of the 30 distance symbols, extra bits)."""
    lf, df, extra = [0] * 286, [0] * 30, 0
    for _at, _bits, t in tokens:
        if isinstance(t, int):
            lf[t] += 1
        else:
            lf[t[2]] += 1
            df[t[3]] += 1
            extra += LEXTRA[t[2] - 257] + DEXTRA[t[3]]
    lf[256] += 1
    return lf, df, extra


def fixed_bits(tokens):
    """The bits of one fixed block with these tokens: 3, the codes of RFC 1951 3.2.6, 5-bit distances, the extra bits."""
    lf, df, extra = token_histograms(tokens)
    return 3 + cost(lf, FIXED_LL) + 5 * sum(df) + extra


def best_dynamic_bits(tokens):
    """The bits of a dynamic block with these tokens as well as plain means build one: package-merge lengths for both alphabets
    (no encoder's data bits are fewer), the header of those lengths in the greedy run-length coding, package-merge lengths for
    the code-length alphabet."""
    lf, df, extra = token_histograms(tokens)
    ll = package_merge(lf, 15)
    dl = package_merge(df, 15)
    if sum(1 for f in lf if f) == 1:
        ll[0 if lf[0] == 0 else 1] = 1
    if not any(df):
        dl[0] = 1
    data = cost(lf, ll) + cost(df, dl) + extra
    hlit = max(257, max(s for s in range(286) if ll[s]) + 1)
    hdist = max(1, max(s for s in range(30) if dl[s]) + 1)
    ops = greedy_rle(ll[:hlit] + dl[:hdist])
    cf = [0] * 19
    xb = 0
    for o in ops:
        if isinstance(o, int):
            cf[o] += 1
        else:
            cf[o[0]] += 1
            xb += {16: 2, 17: 3, 18: 7}[o[0]]
    cl = package_merge(cf, 7)
    hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
    if sum(1 for f in cf if f) == 1:          # (a partner completes the code; it costs no bit)
        cl[0 if cf[0] == 0 else 1] = 1
        hclen = max([4] + [i + 1 for i, s in enumerate(CL_ORDER) if cl[s]])
    return 3 + 14 + 3 * hclen + cost(cf, cl) + xb + data
