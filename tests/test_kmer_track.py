"""The k-mer uniqueness track of a genome FASTA on the host (pymasc_amd.kmer_track.KmerTrackReader, pmx_kmer_open; DESIGN.md
7.13): equal to the plain-Python oracle of tests/kmer_cases.py for every genome, layout, compression and k; the error texts;
the routing of -m by name; the _k<K>_ cache path; the precalc and mapgen argument errors; mapgen's bytes."""
import gzip
import os

import numpy as np
import pytest

from pymasc_amd import inputs, kmer_track, mapgen, precalc
from pymasc_amd.bam import PmxIOError
from pymasc_amd.mappability import default_stats_path
from . import kmer_cases as K


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    return K.write_cases(str(tmp_path_factory.mktemp("fa")))


def track_of(reader):
    return {c: list(zip(*(a.tolist() for a in reader.fetch_arrays(0.0, c)[:2]))) for c in reader.chromsizes}


@pytest.mark.parametrize("k", K.KS)
def test_host_generator_equals_the_oracle(cases, k):
    for path, recs in cases:
        exp = K.oracle(recs, k)
        with kmer_track.KmerTrackReader(path, k) as r:
            assert r.kind == "kmer"
            assert list(r.chromsizes.items()) == [(n, len(s)) for n, s in recs]
            assert track_of(r) == exp, (path, k)
            assert r.sorted


def test_the_cases_hold_every_kind_of_position():
    """The genomes are not trivial: at k = 36 there are unique runs, repeats and (at even k) palindromes."""
    recs = dict(K.genome_cases())["basic"]
    seqs = [s.upper() for _n, s in recs]
    pal = [s[p:p + 16] for s in seqs for p in range(len(s) - 15) if s[p:p + 16] == K.revcomp(s[p:p + 16])]
    assert pal
    runs = K.oracle(recs, 36)
    assert sum(len(v) for v in runs.values()) > 5 and runs["chrS"] == []


def test_values_and_thresholds(cases):
    path, recs = cases[0]
    with kmer_track.KmerTrackReader(path, 36) as r:
        b, e, v = r.fetch_arrays(1.0, "chr1")
        assert len(b) and (v == 1.0).all() and b.dtype == np.uint32
        assert len(r.fetch_arrays(1.5, "chr1")[0]) == 0
        with pytest.raises(KeyError):
            r.fetch_arrays(1.0, "nope")


@pytest.mark.parametrize("name,text,msg", K.MALFORMED)
def test_error_texts(tmp_path, name, text, msg):
    p = tmp_path / name
    p.write_bytes(text)
    with pytest.raises(PmxIOError) as e:
        kmer_track.KmerTrackReader(p, 16)
    assert str(e.value).endswith(": " + msg), str(e.value)
    gz = tmp_path / (name + ".gz")
    gz.write_bytes(gzip.compress(text))
    with pytest.raises(PmxIOError) as e:
        kmer_track.KmerTrackReader(gz, 16)
    assert str(e.value).endswith(": " + msg)


def test_bad_k(tmp_path):
    p = tmp_path / "g.fa"
    p.write_bytes(b">c\nACGTACGTACGTACGTACGT\n")
    for k in (None, 15, 1025):
        with pytest.raises(ValueError):
            kmer_track.KmerTrackReader(p, k)


def test_is_fasta_routing(tmp_path):
    for n in ("g.fa", "g.FASTA", "g.fna", "g.fas", "g.fa.gz", "g.Fa.BGZ", "dir.x/g.fasta.gz"):
        assert kmer_track.is_fasta(n), n
    for n in ("g.bw", "g.bb", "g.bedGraph", "g.bed", "g.wig.gz", "g.fa.bw", "g.fastq", "g.fa.txt", "fa"):
        assert not kmer_track.is_fasta(n), n
    p = tmp_path / "g.fa"
    p.write_bytes(b">c\n" + b"ACGT" * 10 + b"\n")
    with pytest.raises(ValueError):
        inputs.open_track(p, False)                # a FASTA needs k
    with inputs.open_track(p, False, k=16) as t:
        assert isinstance(t, kmer_track.KmerTrackReader) and t.chromsizes == {"c": 40}
    bg = tmp_path / "t.bedGraph"
    bg.write_bytes(b"c\t0\t10\t1\n")
    with inputs.open_track(bg, False, k=36) as t:   # other tracks ignore k
        assert type(t).__name__ == "TextTrackReader"
    assert inputs.track_on_device(bg, True) and not inputs.track_on_device(bg, False)


def test_cache_path_names_k():
    assert str(default_stats_path("/a/hg38.fa", 36)) == "/a/hg38_k36_mappability.json"
    assert str(default_stats_path("/a/hg38.fa.gz", 100)) == "/a/hg38_k100_mappability.json"
    assert str(default_stats_path("x.v2.FASTA.bgz", 50)) == "x.v2_k50_mappability.json"
    assert str(default_stats_path("/a/t.bw", 36)) == "/a/t_mappability.json"
    with pytest.raises(ValueError):
        default_stats_path("/a/hg38.fa")


def test_fasta_sizes_from_fai_or_headers(tmp_path):
    p = tmp_path / "g.fa"
    p.write_bytes(b">a desc\r\nACGT\r\nAC\r\n\r\n>b\tx\nNNNN\n")
    assert kmer_track.fasta_sizes(p) == {"a": 6, "b": 4}
    (tmp_path / "g.fa.fai").write_text("a\t6\t0\t4\t5\nb\t4\t20\t4\t5\n")
    assert kmer_track.fasta_sizes(p) == {"a": 6, "b": 4}


def test_precalc_fasta_needs_r(tmp_path, capsys):
    p = tmp_path / "g.fa"
    p.write_bytes(b">c\n" + b"ACGT" * 10 + b"\n")
    assert precalc.main(["-m", str(p), "-d", "100"]) == 2
    assert "-r/--max-readlen" in capsys.readouterr().err


def test_precalc_leaves_a_valid_k_cache_alone(tmp_path):
    """A valid _k36_ cache: no track is generated and no GPU touched (the sizes come from the headers)."""
    import json
    p = tmp_path / "g.fa"
    p.write_bytes(b">c\n" + b"ACGT" * 10 + b"\n")
    cache = tmp_path / "g_k36_mappability.json"
    d = 100
    need = d - 36 + 1 if d > 2 * 36 - 1 else 36
    stats = {"max_shift": need, "__whole__": [0] * (need + 1), "references": {"c": [0] * (need + 1)}}
    cache.write_text(json.dumps(stats))
    before = cache.read_bytes()
    assert precalc.main(["-m", str(p), "-d", str(d), "-r", "36"]) == 0
    assert cache.read_bytes() == before
    assert not (tmp_path / "g_mappability.json").exists()


def test_mapgen_argument_errors(tmp_path, capsys):
    p = tmp_path / "g.fa"
    p.write_bytes(b">c\n" + b"ACGT" * 10 + b"\n")
    assert mapgen.main([str(p), "-o", str(tmp_path / "o.bed")]) == 2
    assert mapgen.main([str(p), "-k", "8", "-o", str(tmp_path / "o.bed")]) == 2
    assert mapgen.main([str(p), "-k", "36"]) == 2
    assert mapgen.main([str(tmp_path / "missing.fa"), "-k", "36", "-o", str(tmp_path / "o.bed")]) == 1


def test_mapgen_bytes_from_the_host_generator(cases, tmp_path, monkeypatch):
    monkeypatch.setattr(inputs, "default_device_ingest", lambda world, context=None: False)
    path, recs = cases[0]
    exp = K.oracle(recs, 36)
    text = "".join("{}\t{}\t{}\n".format(n, b, e) for n, _s in recs for b, e in exp[n]).encode()
    out = tmp_path / "g_k36.bed"
    assert mapgen.main([path, "-k", "36", "-o", str(out)]) == 0
    assert out.read_bytes() == text
    gz = tmp_path / "g_k36.bed.gz"
    assert mapgen.main([path, "-k", "36", "-o", str(gz)]) == 0
    assert gzip.decompress(gz.read_bytes()) == text
    first = gz.read_bytes()
    assert mapgen.main([path, "-k", "36", "-o", str(gz)]) == 0
    assert gz.read_bytes() == first                   # mtime 0: equal tracks, equal bytes
    with inputs.open_track(out, False) as t:          # the BED read back is the same track
        assert {c: list(zip(*(a.tolist() for a in t.fetch_arrays(1.0, c)[:2]))) for c in t.chromsizes} == \
            {n: v for n, v in exp.items() if v}
