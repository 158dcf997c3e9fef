"""tests/deflate_dissect.py against zlib (no GPU): the oracle of tests/test_gpu_deflate_dissect.py and tests/test_deflate_codes.py
decodes what zlib decodes, to the same bytes and the same Adler-32, accounts for every bit of a stream, and refuses what zlib
refuses."""
import struct
import zlib

import pytest

from tests import deflate_streams as DS
from tests import test_gpu_deflate_dissect as G
from tests.deflate_dissect import Invalid, best_dynamic_bits, chained_rle, dissect, dissect_raw, fixed_bits, huffman_lengths, package_merge

STRATEGIES = [("default", zlib.Z_DEFAULT_STRATEGY), ("fixed", zlib.Z_FIXED), ("huffman_only", zlib.Z_HUFFMAN_ONLY), ("rle", zlib.Z_RLE)]


def account(stream, d):
    """Every bit of the stream is the header's, a block's three, a header's, a token's, an end-of-block code's, padding or the
    Adler-32's; the blocks lie end to end."""
    at, total = 16, 16
    for b in d.blocks:
        assert b.first_bit == at
        if b.btype == 0:
            assert b.bits == 3 + b.pad + 32 + 8 * b.length and not b.tokens
        else:
            assert b.bits == 3 + b.header_bits + b.token_bits + b.eob[1]
            pos = b.first_bit + 3 + b.header_bits
            for off, bits, _t in b.tokens:
                assert off == pos
                pos += bits
            assert b.eob[0] == pos
        at += b.bits
        total += b.bits
    assert d.end_bit == at and [b.final for b in d.blocks] == [False] * (len(d.blocks) - 1) + [True]
    assert total + d.pad + 32 == 8 * len(stream)


def same_as_zlib(stream):
    d = dissect(stream)
    data = zlib.decompress(stream)
    assert d.data == data and d.adler == zlib.adler32(data) & 0xffffffff == struct.unpack(">I", stream[-4:])[0]
    assert (d.cmf, d.flg) == (stream[0], stream[1])
    account(stream, d)
    return d


@pytest.mark.parametrize("case", DS.valid_cases(), ids=lambda c: "%s-%s" % (c.family, c.name))
def test_the_crafted_streams(case):
    stream = DS.zlib_wrap(case.raw, case.expected)
    d = same_as_zlib(stream)
    assert d.data == case.expected
    # the tokens are the symbols the stream was written from (stored bytes count as literals there)
    want = [s if isinstance(s, int) else (s[0], s[1], s[2] if len(s) > 2 else DS.length_symbol(s[0])[0]) for s in case.symbols]
    got = []
    for b in d.blocks:
        if b.btype == 0:
            got += list(d.data[len(DS.model(got)):][:b.length])
        else:
            got += [t if isinstance(t, int) else t[:3] for _o, _n, t in b.tokens]
    assert got == want


def test_the_header_is_kept_as_written():
    case = next(c for c in DS.valid_cases() if c.name == "cl_code_of_7_bits_and_every_repeat_count")
    (b,) = dissect_raw(case.raw).blocks
    assert b.ops[:6] == [7, (16, 3), 8, (16, 6), (17, 3), 9] and (18, 138) in b.ops and max(b.cl) == 7
    assert (b.hlit, b.hdist) == (262, 4) and DS.expand_rle(b.ops) == b.ll + b.dl
    case = next(c for c in DS.valid_cases() if c.name == "hclen_19_hlit_286_hdist_30")
    b = dissect_raw(case.raw).blocks[1]
    assert (b.hlit, b.hdist, b.hclen) == (286, 30, 19) and b.ops == b.ll + b.dl          # (plain_rle: no repeat code)
    assert b.header_bits == 14 + 3 * 19 + sum(b.cl[o] for o in b.ops)


@pytest.mark.parametrize("name", sorted(G.inputs()))
def test_zlib_streams_of_the_encoder_cases(name):
    raw = G.inputs()[name]
    for level in (0, 1, 6, 9):
        for _sname, strategy in STRATEGIES:
            o = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
            stream = o.compress(raw) + o.flush()
            d = same_as_zlib(stream)
            assert d.data == raw
            if level and strategy == zlib.Z_FIXED:
                assert {b.btype for b in d.blocks} <= {0, 1}
                for b in d.blocks:
                    if b.btype == 1:
                        assert b.bits == fixed_bits(b.tokens)
            if level and strategy == zlib.Z_HUFFMAN_ONLY:
                assert all(isinstance(t, int) for _o, _n, t in d.tokens)


@pytest.mark.parametrize("case", [c for c in DS.invalid_cases() if c.by == "zlib"], ids=lambda c: c.name)
def test_what_zlib_refuses_is_refused(case):
    with pytest.raises(zlib.error):
        zlib.decompressobj(-15).decompress(case.raw + b"\0" * 8)
    with pytest.raises(Invalid):
        dissect_raw(case.raw + b"\0" * 8)


def test_the_wrapper_is_checked():
    """RFC 1950: the header's check bits, the method, no dictionary, the Adler-32, and nothing behind it."""
    good = zlib.compress(b"hello, hello, hello", 6)
    assert dissect(good).data == b"hello, hello, hello"
    wrong_sum = good[:-1] + bytes([good[-1] ^ 1])
    wrong_check = b"\x78\x9d" + good[2:]
    wrong_method = b"\x79\x9c" + good[2:]
    dictionary = b"\x78\xbb" + good[2:]
    short_sum = good[:-1]
    for bad in (wrong_sum, wrong_check, wrong_method, dictionary, short_sum):
        with pytest.raises(Invalid):
            dissect(bad)
        with pytest.raises(zlib.error):
            zlib.decompress(bad)
    with pytest.raises(Invalid):          # (zlib.decompress lets bytes behind the stream pass; one stream is one stream here)
        dissect(good + b"\0")


def test_the_reference_lengths():
    """huffman_lengths is optimal (it meets package_merge where the limit does not act) and package_merge is complete, within
    the limit, and optimal on the sets small enough to try every code."""
    import itertools
    import random
    rng = random.Random(1)
    for _ in range(300):
        m = rng.randrange(2, 40)
        f = [rng.choice((0, 1, 1, 2, 3, 5, 8, 100, 1000)) * rng.randrange(1, 4) for _ in range(m)]
        if sum(1 for x in f if x) < 2:
            continue
        h = huffman_lengths(f)
        assert DS.kraft(h) == 32768 and all((l > 0) == (x > 0) for l, x in zip(h, f))
        for limit in (max(h), max(h) + 1, 15):
            p = package_merge(f, limit)
            assert DS.kraft(p) == 32768 and sum(a * b for a, b in zip(f, p)) == sum(a * b for a, b in zip(f, h))
        limit = max(6, max(h) - 2)
        if limit < max(h):
            p = package_merge(f, limit)
            assert DS.kraft(p) == 32768 and max(p) <= limit and sum(a * b for a, b in zip(f, p)) >= sum(a * b for a, b in zip(f, h))
    # every complete code of 5 symbols within 3 bits
    f = [1, 1, 2, 3, 40]
    codes = [c for c in itertools.product(range(1, 4), repeat=5) if sum(8 >> l for l in c) == 8]
    assert sum(a * b for a, b in zip(f, package_merge(f, 3))) == min(sum(a * b for a, b in zip(f, c)) for c in codes)
    assert max(huffman_lengths(f)) == 4
    # a leaf wins a tie: 1 1 2 has one tree; 1 1 1 1 2 2 is 3 3 3 3 2 2 and not 4 4 3 2 2 2 ... of the same cost
    assert huffman_lengths([1, 1, 1, 1, 2, 2]) == [3, 3, 3, 3, 2, 2]
    assert chained_rle([5] * 9 + [0] * 12 + [3] * 10) == [5, (16, 6), 5, 5, (18, 12), 3, (16, 6), (16, 3)]
    assert chained_rle([5] * 9 + [0] * 12) == DS.greedy_rle([5] * 9 + [0] * 12)
    toks = [(0, 8, 65)] * 20 + [(0, 20, (10, 3, 264, 2))]
    assert fixed_bits(toks) == 3 + 20 * 8 + 7 + 5 + 7 and best_dynamic_bits(toks) > 17 + 12
