"""The streams of tests/deflate_streams.py against zlib's decoder and the host reader (libpymasc_io.so, zlib): every valid stream
inflates to what its symbols mean and ends at its last byte, every invalid one is refused, and the seeded re-encodings reach the
parts of a decoder that an encoder's output does not (counted on the symbol lists and code lengths themselves).  The GPU side
is tests/test_gpu_inflate_streams.py: the same files through libpymasc_ingest.so's k_bgzf_inflate."""
import gzip
import zlib

import numpy as np
import pytest

from pymasc_amd import bam as B
from . import deflate_streams as S
from . import io_writers as W
from .test_io_readers import BAM, _all_reads

SEEDS = (1, 2, 3)
FAMILIES = ("long_codes", "literal_runs", "match_geometry", "stored_blocks", "dynamic_headers", "many_blocks", "member_sizes")


def family(name):
    return [c for c in S.VALID if c.family == name]


def golden_stream() -> bytes:
    with gzip.open(BAM, "rb") as fp:
        return fp.read()


SYNTH_REFS = [("chrA", 50000), ("chrB_with_a_long_name" * 3, 30000), ("chrC", 999)]


def synthetic_stream():
    recs, meta = W.synth_bam_records(np.random.default_rng(17), SYNTH_REFS, 700)
    return W.bam_header(SYNTH_REFS) + b"".join(recs), meta


_CORPORA = {}


def corpus(name, seed):
    """(members [(raw, payload, symbols)], the coverage counts) of one seeded re-encoding; built once per session."""
    if (name, seed) not in _CORPORA:
        data = golden_stream() if name == "golden" else synthetic_stream()[0]
        stats = {}
        _CORPORA[(name, seed)] = (S.encode_members(data, np.random.default_rng(seed), stats=stats), stats, data)
    return _CORPORA[(name, seed)]


def corpus_file(name, seed, skew=None):
    """The re-encoding as a BAM file: its members in place of the ones an encoder wrote."""
    parts, off = [], 0
    for raw, piece, _s in corpus(name, seed)[0]:
        m = S.bgzf_member(raw, piece, extra=None if skew is None else S.extra_for_skew(off, skew))
        parts.append(m)
        off += len(m)
    return b"".join(parts) + W.BGZF_EOF


def _inflates_to(raw, expected, name):
    d = zlib.decompressobj(-15)
    got = d.decompress(raw)
    assert got == expected, name
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b"", "%s: the stream does not end at its last byte" % name
    # ... and not a byte sooner
    d = zlib.decompressobj(-15)
    d.decompress(raw[:-1])
    assert not d.eof, "%s: the stream ends before its last byte" % name


def test_the_tables_hold_what_the_issue_lists():
    assert sorted({c.family for c in S.VALID}) == sorted(FAMILIES)
    names = {c.name for c in S.INVALID}
    assert len(names) == len(S.INVALID) >= 30
    assert {"isize_%d" % n for n in S.MEMBER_SIZES} == {c.name for c in family("member_sizes")}
    assert [len(c.expected) for c in family("member_sizes")] == S.MEMBER_SIZES


@pytest.mark.parametrize("fam", FAMILIES)
def test_valid_streams_inflate_to_their_model(fam):
    cases = family(fam)
    assert cases
    for c in cases:
        assert S.model(c.symbols) == c.expected, c.name
        _inflates_to(c.raw, c.expected, "%s/%s" % (fam, c.name))


def test_what_the_crafted_streams_hold():
    """Read off the symbols and the bits written, not off a decoder: the properties the families are there for."""
    by = {c.name: c for c in S.VALID}
    long_syms = [s for c in family("match_geometry") for s in c.symbols if not isinstance(s, int)]
    assert {s[0] for s in long_syms} >= set(S.GEOM_LENGTHS)
    assert {s[1] for s in long_syms} >= set(S.GEOM_DISTANCES) | {l + d for l in S.GEOM_LENGTHS for d in (-1, 0, 1)} - {0}
    assert any(len(s) > 2 and s[2] == 284 for s in long_syms) and any(s[0] == 258 and len(s) == 2 for s in long_syms)
    for pstart in (0, 1, 255):
        g = S.geometry(by["every_phase_and_a_match_that_ends_the_member"].symbols, pstart)
        assert g >= {"completes_1", "completes_2", "ends_the_member"}, (pstart, g)
        assert S.geometry(by["short_matches_from_every_phase"].symbols, pstart) >= {"begins_on_a_boundary", "ends_on_a_boundary"}
        assert "far_source_in_the_first_group" in S.geometry(by["far_source_in_the_first_group"].symbols, pstart)
    c = by["distance_reaches_the_first_byte"]
    n, whole = 0, 0
    for s in c.symbols:
        if not isinstance(s, int):
            whole += s[1] == n
            n += s[0]
        else:
            n += 1
    assert whole > 100
    assert len(by["largest_len_of_a_member"].raw) == S.MEMBER_CDATA_MAX - 7
    assert sum(len(c.expected) for c in family("literal_runs") if c.name.startswith("12_bit")) == 65000


@pytest.mark.parametrize("name", ["golden", "synthetic"])
@pytest.mark.parametrize("seed", SEEDS)
def test_seeded_reencodings_inflate_and_cover(name, seed):
    members, st, data = corpus(name, seed)
    assert b"".join(p for _r, p, _s in members) == data
    for k, (raw, piece, syms) in enumerate(members):
        assert S.model(syms) == piece
        _inflates_to(raw, piece, "%s seed %d member %d" % (name, seed, k))
    print(name, seed, st)
    assert st["lit12"] >= 1000 and st["len12"] >= 200 and st["dist9"] >= 200, st
    assert min(st["band0"], st["band1"], st["band2"], st["band3"]) >= 50, st
    assert st["overlap"] >= 20, st


def test_invalid_streams_are_refused_by_zlib_and_by_the_host_reader(tmp_path):
    for c in S.INVALID:
        if c.by == "zlib":
            with pytest.raises(zlib.error):
                zlib.decompressobj(-15).decompress(c.raw)
        else:          # a stream zlib takes (or one that just stops): its member's CRC32 / ISIZE / end refuse it
            d = zlib.decompressobj(-15)
            out = d.decompress(c.raw)
            assert not d.eof or len(out) != c.isize or (zlib.crc32(out) & 0xffffffff) != c.crc, c.name
        p = tmp_path / "bad.bam"
        p.write_bytes(S.build_invalid_file(c))
        with pytest.raises(B.PmxIOError):
            with B.BamReader(p) as h:
                _all_reads(h, 0)
            pytest.fail("the host reader accepts " + c.name)


def test_the_member_that_reads_its_neighbour_is_refused_only_for_its_distance():
    """distance_one_beyond_the_member_start: with the byte in front of the member as a window, zlib inflates it to the bytes whose
    CRC32 and ISIZE the member carries -- no other test of a reader can refuse it."""
    c = next(c for c in S.INVALID if c.name == "distance_one_beyond_the_member_start")
    data = S.build_invalid_file(c)
    front = S.carrier_record(7, c.isize, 20)
    d = zlib.decompressobj(-15, zdict=front[-1:])
    out = d.decompress(c.raw)
    crc, isize = np.frombuffer(data[-len(W.BGZF_EOF) - 8:-len(W.BGZF_EOF)], dtype="<u4").tolist()
    assert d.eof and len(out) == isize == c.isize and (zlib.crc32(out) & 0xffffffff) == crc


@pytest.mark.parametrize("fam", FAMILIES)
def test_host_reader_reads_the_crafted_files(tmp_path, fam):
    """Host parity: the files the GPU tests open, through BamReader (zlib): every member passes its CRC32 against the model's bytes
    and the carrier records come back."""
    header = S.crafted_header_member(1) if fam == "match_geometry" else None
    for skew, phases in ((0, (0,)), (1, (1,)), (2, (255,)), (3, (0, 1, 255))):
        cf = S.build_file(family(fam), skew, phases, header=header if skew == 1 else None)
        p = tmp_path / "v.bam"
        p.write_bytes(cf.data)
        with B.BamReader(p) as h:
            assert _all_reads(h, 0) == cf.reads
        with gzip.open(p, "rb") as fp:
            assert fp.read() == cf.want


@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_host_reader_reads_the_reencodings(tmp_path, name):
    if name == "golden":
        with B.BamReader(BAM) as h:
            exp = _all_reads(h, 0)
    else:
        from .test_io_readers import _expected
        exp = _expected(synthetic_stream()[1], SYNTH_REFS, 0)
    for seed in SEEDS:
        p = tmp_path / "r.bam"
        p.write_bytes(corpus_file(name, seed, seed & 3))
        with B.BamReader(p) as h:
            assert _all_reads(h, 0) == exp
    assert len(exp) > 2000


def test_bigwig_writer_takes_another_compressor(tmp_path):
    """write_bigwig(compress=callable): data blocks in encode()'s streams, read by the host reader like zlib's."""
    from pymasc_amd.bigwig import BigWigReader
    from .test_io_readers import _tracks
    chromsizes = {"chr1": 200000, "chr2": 50000}
    tracks = _tracks(np.random.default_rng(3), chromsizes)
    rng = np.random.default_rng(4)

    def compress(payload):
        raw, _syms = S.encode(payload, rng)
        return S.zlib_wrap(raw, payload)

    assert zlib.decompress(compress(b"abcabcabc" * 50)) == b"abcabcabc" * 50
    a, b = tmp_path / "a.bw", tmp_path / "b.bw"
    W.write_bigwig(a, chromsizes, tracks, items_per_block=100)
    W.write_bigwig(b, chromsizes, tracks, items_per_block=100, compress=compress)
    with BigWigReader(a) as x, BigWigReader(b) as y:
        for c in chromsizes:
            for u, v in zip(x.fetch_arrays(0.5, c), y.fetch_arrays(0.5, c)):
                assert (u == v).all() and u.size == v.size
