"""``--coverage-deflate`` / ``coverage_compress="device"`` without a GPU: the options, the settings, the writer's
third mode (streams a source hands are written as they are) pinned byte for byte against the host-zlib file, the refusals that
replace a silent fall-back to zlib, and the encoder's size bound."""
import os
import zlib

import numpy as np
import pytest

from pymasc_amd import cli, coverage, pipeline
from tests import bigwig_out_cases as BC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests.fake_context import FakeContext

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")


def test_options(monkeypatch):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert a.coverage_deflate is None and not a.coverage_compress
    a = cli.parse_args(base + ["--coverage-format", "bigwig", "--coverage-compress"])
    assert a.coverage_deflate is None and a.coverage_compress
    for where in ("host", "device"):
        for more in ([], ["--coverage-compress"]):
            a = cli.parse_args(base + ["--coverage-format", "bigwig", "--coverage-deflate", where] + more)
            assert a.coverage and a.coverage_format == "bigwig" and a.coverage_compress and a.coverage_deflate == where
    for bad in (["--coverage-deflate", "device"], ["--coverage", "--coverage-deflate", "host"],
                ["--coverage-format", "bedgraph", "--coverage-deflate", "device"], ["--coverage-format", "bigwig", "--coverage-deflate", "gpu"],
                ["--coverage-format", "bigwig", "--coverage-deflate"]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2 and cli.main(base + bad) == 2
    text = " ".join(cli.get_parser().format_help().split())
    assert "--coverage-deflate {host,device}" in text and "2048 items" in text and "differ from zlib's" in text
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bw = ["--coverage-format", "bigwig"]
    for more, want in ((bw + ["--coverage-compress"], True), (bw + ["--coverage-deflate", "host"], True),
                       (bw + ["--coverage-deflate", "device"], "device"), (bw + ["--coverage-compress", "--coverage-deflate", "device"], "device"),
                       (bw, None)):
        seen.clear()
        assert cli.main(["a.bam", "--skip-plots"] + more) == 0
        assert seen.get("coverage_compress") == want and seen["coverage_format"] == "bigwig"


def test_the_settings_take_device_and_refuse_what_cannot_have_it(tmp_path):
    assert coverage.check_format("bigwig", "device") == "bigwig" and coverage.check_format("bigwig", True) == "bigwig"
    assert coverage.check_compress("device") == "device" and coverage.check_compress(1) is True and coverage.check_compress(0) is False
    for fmt, compress in (("bedgraph", "device"), ("bigwig", "gpu"), ("bigwig", "host")):
        with pytest.raises(ValueError, match="coverage_"):
            coverage.check_format(fmt, compress)
    kw = dict(read_len=36, mapq_criteria=10, context=FakeContext(), coverage=True, coverage_extend=200)
    for bad in (dict(coverage_compress="device"), dict(coverage_format="bedgraph", coverage_compress="device"),
                dict(coverage_format="bigwig", coverage_compress="zlib")):
        with pytest.raises(ValueError, match="coverage_"):
            pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, device_ingest=False, **bad, **kw)
    # the host path cannot compress on the device, and says so before anything runs: no fall-back to zlib
    with pytest.raises(ValueError, match="device ingest"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, device_ingest=False, coverage_format="bigwig", coverage_compress="device", **kw)
    assert not (tmp_path / "bad").exists()


class _ZlibParts(coverage.HostParts):
    """``HostParts`` with the two calls a compressing source has, the streams made by host zlib: what ``compress=True`` writes."""

    @staticmethod
    def _z(blob, table):
        ends = np.cumsum(table[:, 4].astype(np.int64))
        parts = [zlib.compress(blob[int(z - r):int(z)]) for z, r in zip(ends, table[:, 4])]
        return b"".join(parts), table, np.array([len(p) for p in parts], dtype=np.uint32)

    def section_chunks_z(self, k, chrom_id, items):
        for blob, table in self.section_chunks(k, chrom_id, items):
            yield self._z(blob, table)

    def zoom_records_z(self, level, items):
        return self._z(*self.zoom_records(level, items))


def _host(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


@pytest.mark.parametrize("items", [1024, 4])
def test_the_writer_takes_streams_as_they_are(tmp_path, items):
    c = _host(FC.kept(CC.synthetic()), BC.REFS, CC.USES["all"], 200)
    files = {}
    for mode, src in ((True, coverage.HostParts(c)), ("device", _ZlibParts(c)), (False, coverage.HostParts(c))):
        with open(tmp_path / str(mode), "w+b") as fp:
            coverage.assemble_bigwig(fp, src, mode, items_per_section=items)
        files[mode] = (tmp_path / str(mode)).read_bytes()
    assert files["device"] == files[True] and len(files[True]) < len(files[False])
    got, raw = BC.read_file(tmp_path / "device"), BC.read_file(tmp_path / "False")
    assert got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in raw.items() if k != "compressed"}
    # no kept read: no section and no level, in every mode
    empty = _host([], BC.REFS, CC.USES["all"], 200)
    with open(tmp_path / "e1", "w+b") as a, open(tmp_path / "e2", "w+b") as b:
        coverage.assemble_bigwig(a, _ZlibParts(empty), "device", items_per_section=items)
        coverage.assemble_bigwig(b, coverage.HostParts(empty), True, items_per_section=items)
    assert (tmp_path / "e1").read_bytes() == (tmp_path / "e2").read_bytes()


def test_device_over_a_host_source_raises(tmp_path):
    c = _host(BC.small_reads(), BC.SMALL_REFS, BC.SMALL_USE, 0)
    with open(tmp_path / "x", "w+b") as fp:
        with pytest.raises(ValueError, match="section_chunks_z"):
            coverage.assemble_bigwig(fp, coverage.HostParts(c), "device")
        assert fp.tell() == 0
        with pytest.raises(ValueError, match="2048 items"):
            coverage.assemble_bigwig(fp, _ZlibParts(c), "device", items_per_section=2049)
        assert fp.tell() == 0
        coverage.assemble_bigwig(fp, _ZlibParts(c), "device", items_per_section=2048)
    with pytest.raises(ValueError, match="section_chunks_z"):
        coverage.write_bigwig(tmp_path / "y", "y", c, compress="device")
    assert sorted(os.listdir(tmp_path)) == ["x"]


def test_the_bound():
    assert [coverage.deflate_bound(n) for n in (0, 1, 65535, 65536)] == [11, 12, 65546, 65552]
    assert coverage.DEFLATE_MAX_CHUNK == 65536 and 32 * coverage.DEVICE_ITEMS == coverage.DEFLATE_MAX_CHUNK
