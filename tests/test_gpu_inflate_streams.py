"""k_bgzf_inflate (libpymasc_ingest.so) on DEFLATE streams that no zlib encoder produces: the case tables and seeded
re-encodings of tests/deflate_streams.py, which tests/test_deflate_streams.py holds against zlib's decoder and the host reader.
Valid members are compared byte for byte with what their symbols mean (and their CRC32 / ISIZE are checked on the device), at
every skew of the compressed stream against a dword and at the output offsets where the flush and k_bgzf_crc take their edge
paths; invalid ones must be reported where zlib and the host reader report them, with the message of their cause."""
import numpy as np
import pytest

from pymasc_amd import bam as B
from pymasc_amd import bam_device as D
from . import deflate_streams as S
from . import io_writers as W
from .test_deflate_streams import FAMILIES, SEEDS, SYNTH_REFS, corpus, corpus_file, family, synthetic_stream
from .test_io_readers import BAM, _all_reads, _expected

pytestmark = pytest.mark.gpu

SKEWS = (0, 1, 2, 3)            # in_off & 3
PHASES = (0, 1, 255)            # out_off & 255: with them out_off & 15 is 0, 1 and 15


@pytest.mark.parametrize("fam", FAMILIES)
def test_crafted_members_inflate_to_their_model(tmp_path, fam):
    cases = family(fam)
    path = tmp_path / "v.bam"
    for skew in SKEWS:
        for phase in PHASES:
            header = S.crafted_header_member(skew) if fam == "match_geometry" else None      # (a match that reaches byte 0 of the file)
            cf = S.build_file(cases, skew, (phase,), header=header)
            path.write_bytes(cf.data)
            with D.DeviceBamReader(path) as r:
                c = r.counters()
                assert c["members"] == 2 * len(cases) + 2 and c["bytes_out"] == len(cf.want)
                diff = cf.first_difference(r.inflated())
                assert not diff, "%s at skew %d, output offset %d mod 256: %s" % (fam, skew, phase, diff)
                assert _all_reads(r, 0) == cf.reads
    # the three phases in one file: members of different alignment side by side
    cf = S.build_file(cases, 2, PHASES)
    path.write_bytes(cf.data)
    with D.DeviceBamReader(path) as r:
        diff = cf.first_difference(r.inflated())
        assert not diff, "%s, mixed offsets: %s" % (fam, diff)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", ["golden", "synthetic"])
def test_seeded_reencodings_read_like_the_original(tmp_path, name, seed):
    """The golden BAM's stream / synthetic records, re-encoded: same bytes, and the records of the device reader == the host
    reader's on the same file == the original's."""
    data = corpus(name, seed)[2]
    path = tmp_path / "r.bam"
    path.write_bytes(corpus_file(name, seed, seed & 3))
    if name == "golden":
        with B.BamReader(BAM) as h:
            original = [_all_reads(h, q) for q in (0, 10)]
    else:
        original = [_expected(synthetic_stream()[1], SYNTH_REFS, q) for q in (0, 10)]
    with B.BamReader(path) as h:
        host = [_all_reads(h, q) for q in (0, 10)]
    with D.DeviceBamReader(path) as r:
        got = r.inflated()
        if got != data:
            first = next((i for i in range(min(len(got), len(data))) if got[i] != data[i]), -1)
            raise AssertionError("%s seed %d: lengths %d / %d, first difference at byte %d" % (name, seed, len(got), len(data), first))
        dev = [_all_reads(r, q) for q in (0, 10)]
    assert dev == host == original and len(dev[0]) > 2000


def test_golden_reencoding_through_the_stream_reader(tmp_path):
    """... and in windows of a few KB (members inflated window by window): the same batches as the file reader."""
    from pymasc_amd.stream_device import DeviceStreamReader
    path = tmp_path / "s.bam"
    path.write_bytes(corpus_file("golden", SEEDS[0], 1))
    with D.DeviceBamReader(path) as f:
        exp = [np.concatenate(x) for x in zip(*f.batches(10))]
    with DeviceStreamReader(str(path), window_bytes=6000) as s:
        got = [np.concatenate(x) for x in zip(*s.batches(10))]
        assert s.stream_info()["windows"] > 1
    assert len(exp[0]) == 1292
    for a, b in zip(got, exp):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("seed", SEEDS)
def test_bigwig_blocks_in_crafted_streams(tmp_path, seed):
    """The same decoder behind open_size (BigWig data blocks, zlib-wrapped): blocks compressed by encode(); device == host reader ==
    the file zlib wrote."""
    from pymasc_amd.bigwig import BigWigReader
    from pymasc_amd.bigwig_device import DeviceBigWigReader
    from .test_gpu_ingest import _same_intervals
    from .test_io_readers import _tracks
    rng = np.random.default_rng(31)
    chromsizes = {"chr1": 500000, "chr2": 120000, "chrX_random_with_a_long_name": 40000, "chrM": 16571}
    tracks = _tracks(rng, chromsizes)
    erng = np.random.default_rng(seed)

    def compress(payload):
        raw, _syms = S.encode(payload, erng, block_symbols=(1, 300))
        return S.zlib_wrap(raw, payload)

    path, plain = tmp_path / "t.bw", tmp_path / "z.bw"
    W.write_bigwig(path, chromsizes, tracks, kind="bedgraph", compress=compress, items_per_block=37 * seed, rtree_block=3, bpt_block=2)
    W.write_bigwig(plain, chromsizes, tracks, kind="bedgraph", compress=True, items_per_block=37 * seed, rtree_block=3, bpt_block=2)
    with BigWigReader(path) as h, BigWigReader(plain) as z, DeviceBigWigReader(path) as d:
        assert d.chromsizes == h.chromsizes
        for thr in (1, 0, 0.25):
            for c in chromsizes:
                a = h.fetch_arrays(thr, c)
                assert _same_intervals(a, d.fetch_arrays(thr, c)), (thr, c)
                assert _same_intervals(a, z.fetch_arrays(thr, c)), (thr, c)
        _b, _e, n, in_order = d.fetch_device(1, "chr1")
        a = h.fetch_arrays(1, "chr1")
        assert n == a[0].size and in_order == bool((a[0] < a[1]).all() and (a[0][1:] >= a[1][:-1]).all())


def test_invalid_members_are_reported_with_their_cause(tmp_path):
    """One file per case: a valid header member, a carrier, the bad member, the EOF member.  The host reader refuses every one, and
    so does the device, with the message of the one test that can refuse it (the table in bam_device.hip)."""
    import re
    path = tmp_path / "bad.bam"
    wrong = []
    for c in S.INVALID:
        path.write_bytes(S.build_invalid_file(c))
        with pytest.raises(B.PmxIOError):
            with B.BamReader(path) as h:
                _all_reads(h, 0)
        try:
            with D.DeviceBamReader(path) as r:
                r.inflated()
                _all_reads(r, 0)
            wrong.append("%s: accepted" % c.name)
        except B.PmxIOError as e:
            if not (re.search("DEFLATE|BGZF block", str(e)) and re.search(c.error, str(e))):
                wrong.append("%s: reported as %r, not as %r" % (c.name, str(e), c.error))
    assert not wrong, "the device reader on %d of %d invalid members:\n" % (len(wrong), len(S.INVALID)) + "\n".join(wrong)
