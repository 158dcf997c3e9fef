"""The k-mer uniqueness track of a genome FASTA on the device (pymasc_amd.kmer_track.DeviceKmerTrackReader, pmx_dkm_open;
DESIGN.md 7.13) against the host generator, its checker, and the plain-Python oracle: every case of tests/kmer_cases.py, forced
hash collisions, several sort passes, a ~50 Mbp genome with planted repeat families, the error texts; then -m genome.fa end to
end (run_files, the command, precalc, two gloo ranks) against -m of the oracle's BED."""
import gzip
import os

import numpy as np
import pytest

from pymasc_amd import inputs, kmer_track, pipeline
from pymasc_amd.bam import PmxIOError
from . import io_writers as W
from . import kmer_cases as K
from .test_gpu_cli import _command, _tree

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return K.write_cases(str(tmp_path_factory.mktemp("fa")))


def track_of(reader):
    return {c: list(zip(*(a.tolist() for a in reader.fetch_arrays(0.0, c)[:2]))) for c in reader.chromsizes}


def arrays_of(reader):
    return {c: reader.fetch_arrays(1.0, c) for c in reader.chromsizes}


@pytest.mark.parametrize("k", K.KS)
def test_device_equals_host_and_oracle(cases, k):
    for path, recs in cases:
        exp = K.oracle(recs, k)
        with kmer_track.DeviceKmerTrackReader(path, k) as d, kmer_track.KmerTrackReader(path, k) as h:
            assert d.kind == "kmer"
            assert list(d.chromsizes.items()) == list(h.chromsizes.items())
            got = track_of(d)
            assert got == exp, (path, k)
            assert got == track_of(h)
            for c in d.chromsizes:
                b, e, v = d.fetch_arrays(1.0, c)
                assert b.dtype == np.uint32 and (v == 1.0).all() and d.sorted
                assert len(d.fetch_arrays(1.5, c)[0]) == 0


@pytest.mark.parametrize("bits", [8, 1])
def test_forced_collisions_are_resolved_exactly(cases, bits):
    for path, recs in cases[::3]:
        for k in (16, 36, 101):
            with kmer_track.DeviceKmerTrackReader(path, k, hash_bits=bits) as d:
                assert track_of(d) == K.oracle(recs, k), (path, k, bits)


def test_several_passes_equal_one(cases):
    for path, recs in cases[:6]:
        for k in (31, 36):
            with kmer_track.DeviceKmerTrackReader(path, k) as one, \
                    kmer_track.DeviceKmerTrackReader(path, k, budget_bytes=24 * 700) as many:
                assert track_of(many) == track_of(one) == K.oracle(recs, k)


def test_a_bin_larger_than_the_budget_is_an_error(cases):
    path, _recs = cases[0]
    with pytest.raises(PmxIOError) as e:
        kmer_track.DeviceKmerTrackReader(path, 36, hash_bits=1, budget_bytes=24 * 100)
    assert "does not fit the sort budget" in str(e.value)


def test_fifty_megabase_genome_device_equals_host(tmp_path):
    recs = K.big_genome(11, 50_000_000, nchrom=6)
    p = tmp_path / "big.fa"
    p.write_bytes(K.fasta_bytes(recs, width=60))
    for k in (36, 100):
        with kmer_track.DeviceKmerTrackReader(p, k) as d, \
                kmer_track.DeviceKmerTrackReader(p, k, budget_bytes=24 * 20_000_000) as d3:
            a = arrays_of(d)
            n = sum(len(x[0]) for x in a.values())
            assert n > 1000
            for c, (b, e, _v) in arrays_of(d3).items():
                np.testing.assert_array_equal(b, a[c][0])
                np.testing.assert_array_equal(e, a[c][1])
            if k == 36:
                with kmer_track.KmerTrackReader(p, k) as h:
                    for c, (b, e, _v) in arrays_of(h).items():
                        np.testing.assert_array_equal(b, a[c][0])
                        np.testing.assert_array_equal(e, a[c][1])


@pytest.mark.parametrize("name,text,msg", K.MALFORMED)
def test_device_error_texts_equal_the_hosts(tmp_path, name, text, msg):
    for data, fname in ((text, name), (gzip.compress(text), name + ".gz"), (W.bgzf_compress(text), name + ".bgz")):
        p = tmp_path / fname
        p.write_bytes(data)
        with pytest.raises(PmxIOError) as h:
            kmer_track.KmerTrackReader(p, 16)
        with pytest.raises(PmxIOError) as d:
            kmer_track.DeviceKmerTrackReader(p, 16)
        assert d.value.msg == h.value.msg
        assert d.value.msg.endswith(": " + msg)


# ---- end to end -------------------------------------------------------------------------------------------------------

def _genome_and_reads(d, seed=3):
    """A 3 x 100 kbp genome with repeats, its oracle BED at k = 36 and a coordinate-sorted BAM of 36-bp reads on it."""
    recs = K.big_genome(seed, 300_000, nchrom=3, families=12, copies=9, famlen=(40, 600))
    fa = os.path.join(d, "genome.fa")
    with open(fa, "wb") as fh:
        fh.write(K.fasta_bytes(recs, width=70))
    exp = K.oracle(recs, 36)
    bed = os.path.join(d, "oracle_k36.bed")
    with open(bed, "w") as fh:
        for n, _s in recs:
            for b, e in exp[n]:
                fh.write("{}\t{}\t{}\n".format(n, b, e))
    refs = [(n, len(s)) for n, s in recs]
    rng = np.random.default_rng(seed)
    records, _m = W.synth_bam_records(rng, refs, 4000, readlen=36)
    bam = os.path.join(d, "reads.bam")
    W.write_bam(bam, refs, records)
    return fa, bed, bam


def _tables(out):
    return {n: open(os.path.join(out, n), "rb").read() for n in sorted(os.listdir(out)) if n.endswith(".tab")}


def test_run_files_fasta_equals_the_oracle_bed(tmp_path):
    fa, bed, bam = _genome_and_reads(str(tmp_path))
    for track, out in ((fa, "fa"), (bed, "bed")):
        res = pipeline.run_files([bam], str(tmp_path / out), 200, read_len=36, mapq_criteria=10, mappability_path=track)
        assert res[0].error is None
    assert _tables(tmp_path / "fa") == _tables(tmp_path / "bed")
    assert (tmp_path / "genome_k36_mappability.json").exists()
    assert (tmp_path / "oracle_k36_mappability.json").read_bytes() == (tmp_path / "genome_k36_mappability.json").read_bytes()
    result, _w = pipeline.run(bam, str(tmp_path / "run"), 200, read_len=36, mapq_criteria=10, mappability_path=fa)
    assert _tables(tmp_path / "run") == _tables(tmp_path / "fa")


def test_command_mapgen_precalc_and_two_gloo_ranks(tmp_path):
    fa, bed, bam = _genome_and_reads(str(tmp_path), seed=5)
    common = ["reads.bam", "-d", "200", "-q", "10", "-r", "36", "--skip-plots"]
    rc, err = _command("pymasc_amd.mapgen", ["genome.fa", "-k", "36", "-o", "gen_k36.bed.gz"], tmp_path)
    assert rc == 0, err
    assert gzip.decompress((tmp_path / "gen_k36.bed.gz").read_bytes()) == open(bed, "rb").read()
    rc, err = _command("pymasc_amd.precalc", ["-m", "genome.fa", "-d", "200", "-r", "36"], tmp_path)
    assert rc == 0, err
    assert (tmp_path / "genome_k36_mappability.json").exists()
    rc, err = _command("pymasc_amd", common + ["-m", "genome.fa", "-o", "fa"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", common + ["-m", "gen_k36.bed.gz", "-o", "bed"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", common + ["-m", "genome.fa", "-o", "two", "-p", "2"], tmp_path, PMX_DIST_BACKEND="gloo")
    assert rc == 0, err
    assert _tables(tmp_path / "fa") == _tables(tmp_path / "bed")
    assert _tree(tmp_path / "two") == _tree(tmp_path / "fa")
