"""The DEFLATE encoder on the GPU (pmx_ddeflate).  The decoder of record is Python's ``zlib.decompress``, which
checks the header, every code, every distance and the Adler-32; nothing here is compared with the encoder's own output or with a
twin of it.  Every case is one call of a few chunks.

Measured on one MI355X (``test_both_halves_compress`` prints the figures it asserts on): the data sections of coverage_cases'
library at 1024 items per section and extend 0 / 200 / 1300, as a share of their raw bytes: device 0.317 / 0.328 / 0.341, zlib
level 6 0.276 / 0.284 / 0.290, level 1 0.311 / 0.312 / 0.321, Z_FIXED 0.413 / 0.421 / 0.429, Z_HUFFMAN_ONLY 0.515 / 0.528 / 0.543."""
import random
import zlib

import numpy as np
import pytest

from pymasc_amd import coverage
from pymasc_amd.native import PmxIOError, load_ingest_library
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC

pytestmark = pytest.mark.gpu

FC = CC.FC
MAX = coverage.DEFLATE_MAX_CHUNK


def bound(n):
    return n + 5 * max(1, -(-n // 65535)) + 6


def deflate(chunks):
    """One ``pmx_ddeflate`` call; asserts what holds for every call: the sizes, the bound, the tiling, and that zlib gives the bytes
    back.  Returns the streams."""
    L = load_ingest_library()
    offsets = np.zeros(len(chunks) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(c) for c in chunks], dtype=np.uint64)
    src = np.frombuffer(b"".join(chunks) + b"\0", dtype=np.uint8)
    cap = sum(bound(len(c)) for c in chunks)
    dst, sizes = np.full(cap + 8, 0xA5, dtype=np.uint8), np.zeros(len(chunks), dtype=np.uint32)
    got = L.pmx_ddeflate(0, src.ctypes.data, offsets.ctypes.data, len(chunks), dst.ctypes.data, cap, sizes.ctypes.data)
    assert got >= 0, L.pmx_dbam_last_error()
    assert got == int(sizes.sum()) <= cap and (dst[got:] == 0xA5).all()         # the streams tile dst and nothing lies behind them
    ends = np.cumsum(sizes.astype(np.int64))
    streams = [dst[int(z - n):int(z)].tobytes() for z, n in zip(ends, sizes)]
    for raw, stream in zip(chunks, streams):
        assert len(stream) <= bound(len(raw)) == L.pmx_ddeflate_bound(len(raw))
        assert zlib.decompress(stream) == raw
        assert stream[0] == 0x78 and not stream[1] & 0x20 and (stream[0] << 8 | stream[1]) % 31 == 0     # 32-KB window, no dictionary
    return streams


def rand(rng, n):
    return bytes(rng.getrandbits(8) for _ in range(n))


def test_tiny_chunks():
    streams = deflate([b"", b"a", b"ab", b"abc", b"abcd", b"abcde", b"\xff", b"zz"])
    assert len(streams[0]) <= 11


def test_the_match_length_ceiling():
    streams = deflate([b"\0" * 258, b"\0" * 259, b"\0" * 260, b"q" * 258, b"q" * 259, b"q" * 260, b"ab" * 130])
    assert all(len(s) <= 24 for s in streams)


def test_the_largest_chunk_of_zeros_and_of_noise():
    noise = rand(random.Random(5), MAX)
    zeros, stored = deflate([b"\0" * MAX, noise])
    assert len(zeros) < MAX // 100
    assert len(stored) <= bound(MAX)                    # (two stored blocks: 65535 + 1 bytes)


def test_a_zero_region_is_a_few_dozen_matches():
    (stream,) = deflate([b"\0" * 12312])
    assert 20 * len(stream) < 12312


@pytest.mark.parametrize("distance", [32768, 32769])
def test_the_window_ends_at_32768(distance):
    rng = random.Random(distance)
    head = rand(rng, 300)
    raw = head + rand(rng, distance - 300) + head
    (stream,) = deflate([raw])                          # (zlib refuses a distance beyond the window)
    if distance == 32768:
        assert len(stream) < len(raw)                   # the repeat was used: noise alone does not shrink
    else:
        assert len(stream) > len(raw)                   # nothing to use: stored


def test_degenerate_trees():
    rng = random.Random(9)
    once = list(range(256))
    rng.shuffle(once)
    # every value occurs, and no 3-gram repeats: a de Bruijn-like walk is not needed, 3000 distinct 3-grams out of 2^24 are easy
    seen, out = set(), bytearray(once)
    for i in range(len(out) - 2):
        seen.add(bytes(out[i:i + 3]))
    while len(out) < 3000:
        b = rng.getrandbits(8)
        gram = bytes(out[-2:]) + bytes([b])
        if gram not in seen:
            seen.add(gram)
            out.append(b)
    deflate([bytes(out), b"x", bytes(out[:1000])])


def test_the_length_limit_acts():
    fib = [1, 1]
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    raw = bytearray(b"".join(bytes([65 + i]) * c for i, c in enumerate(fib)))
    assert len(raw) == 46367 and fib[-1] == 17711
    random.Random(3).shuffle(raw)
    (stream,) = deflate([bytes(raw)])
    assert len(stream) < len(raw) // 2                  # about 2.4 bits per byte of entropy: the dynamic block was taken


@pytest.fixture(scope="module")
def sections():
    """The data sections of coverage_cases' library per (extend, items), made with HostParts once."""
    reads = FC.kept(CC.synthetic())
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)]
    out = {}
    for extend in CC.EXTENDS:
        c = coverage.count_host(*cols, BC.NAMES, BC.LENGTHS, CC.USES["all"], extend)
        parts = coverage.HostParts(c)
        for items in (1024, 4):
            secs = []
            for k in range(len(parts.refs)):
                for blob, table in parts.section_chunks(k, k, items):
                    ends = np.cumsum(table[:, 4].astype(np.int64))
                    secs += [blob[int(z - r):int(z)] for z, r in zip(ends, table[:, 4])]
            out[extend, items] = secs
    return out


@pytest.mark.parametrize("items", [1024, 4])
@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_the_section_sets(sections, extend, items):
    secs = sections[extend, items]
    assert len(secs) >= (21 if items == 1024 else 4000)
    deflate(secs)


def _zlib_total(secs, strategy):
    total = 0
    for raw in secs:
        o = zlib.compressobj(6, zlib.DEFLATED, 15, 8, strategy)
        total += len(o.compress(raw) + o.flush())
    return total


@pytest.mark.parametrize("extend", CC.EXTENDS)
def test_both_halves_compress(sections, extend):
    """The matcher and the dynamic codes both work: the device's total lies below zlib's level 6 with Z_FIXED (LZ77 without
    dynamic codes) and below its Z_HUFFMAN_ONLY (dynamic codes without LZ77) on the same sections."""
    secs = sections[extend, 1024]
    raw = sum(len(s) for s in secs)
    assert 21 <= len(secs) <= 22 and 200_000 < raw < 280_000
    dev = sum(len(s) for s in deflate(secs))
    fixed, huffman = _zlib_total(secs, zlib.Z_FIXED), _zlib_total(secs, zlib.Z_HUFFMAN_ONLY)
    level6, level1 = sum(len(zlib.compress(s, 6)) for s in secs), sum(len(zlib.compress(s, 1)) for s in secs)
    print("extend {}: raw {} device {:.4f} zlib-6 {:.4f} zlib-1 {:.4f} Z_FIXED {:.4f} Z_HUFFMAN_ONLY {:.4f}".format(
        extend, raw, dev / raw, level6 / raw, level1 / raw, fixed / raw, huffman / raw))
    assert dev < fixed and dev < huffman


def test_many_mixed_chunks_and_the_same_bytes_twice(sections):
    rng = random.Random(21)
    pool = sections[200, 1024]
    chunks = []
    for i in range(300):
        kind = i % 6
        n = rng.choice((0, 1, 7, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 12312))
        if kind == 0:
            chunks.append(rand(rng, min(n, 2000)))
        elif kind == 1:
            chunks.append(bytes([rng.getrandbits(8)]) * n)
        elif kind == 2:
            chunks.append(pool[i % len(pool)][:n])
        elif kind == 3:
            chunks.append((rand(rng, 1 + rng.getrandbits(4)) * (n + 1))[:n])
        elif kind == 4:
            chunks.append(bytes(rng.choice(b"ACGT\n") for _ in range(min(n, 3000))))
        else:
            chunks.append(pool[i % len(pool)][rng.getrandbits(6):][:n])
    chunks[17] = (pool[0] + pool[1])[:20000]            # a chunk of the 32-KB class
    chunks[18] = b"".join(pool[2:6])[:40000]            # and one of the 64-KB class
    first = deflate(chunks)
    assert deflate(chunks) == first                     # deterministic: the same bytes in, the same bytes out
    assert coverage.deflate_device(chunks) == first     # the Python door is the same call


def test_errors():
    L = load_ingest_library()
    src = np.zeros(MAX + 8, dtype=np.uint8)
    dst, sizes = np.zeros(2 * MAX, dtype=np.uint8), np.zeros(4, dtype=np.uint32)

    def fails(offsets, text, cap=dst.size, p_src=src.ctypes.data, p_dst=dst.ctypes.data, p_sizes=sizes.ctypes.data):
        off = np.array(offsets, dtype=np.uint64)
        rc = L.pmx_ddeflate(0, p_src, off.ctypes.data, len(offsets) - 1, p_dst, cap, p_sizes)
        assert rc == -3 and text in L.pmx_dbam_last_error().decode()

    fails([0, MAX + 1], "a chunk of more than 65536 bytes")
    fails([0, 10, 5], "the offsets descend")
    fails([0, 100, 200], "the buffer is too small", cap=20)
    fails([0, 100], "null pointer", p_sizes=None)
    fails([0, 100], "null pointer", p_dst=None)
    fails([0, 100], "null pointer", p_src=None)
    assert L.pmx_ddeflate(0, src.ctypes.data, None, 1, dst.ctypes.data, dst.size, sizes.ctypes.data) == -3
    with pytest.raises(PmxIOError, match="more than 65536"):
        coverage.deflate_device([b"\0" * (MAX + 1)])
    assert coverage.deflate_device([]) == []
