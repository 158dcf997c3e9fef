"""bigBed mappability tracks on the device (pymasc_amd.bigwig_device.DeviceBigWigReader with a bigBed file, k_bb_records; DESIGN.md
7.12) against the host reader, its checker: every input of tests/test_bigbed.py, a 2 M-record 24-chromosome file of many blocks,
the error texts; then the golden run with the bigBed twin of the golden BigWig, the pymasc and pymasc-precalc commands with it,
and two gloo ranks (the host reader on each) against one."""
import shutil

import numpy as np
import pytest

from pymasc_amd import bigwig, bigwig_device, inputs, pipeline
from pymasc_amd.bam import PmxIOError
from . import bigbed_writers as B
from . import text_track_cases as C
from .test_bigbed import THRESHOLDS, cases, corrupt_cases, host_error, write_golden_twin, zero_length_case
from .test_gpu_cli import GOLDEN_JSON, STEM, _command, _tree
from .test_gpu_run_files import GOLD, TABLES, _check_tables

pytestmark = pytest.mark.gpu


def _agree(path, thresholds=THRESHOLDS):
    """The device reader equals the host reader: kind, chromsizes, every chromosome's arrays at each threshold, sorted."""
    with bigwig.BigWigReader(path) as h, bigwig_device.DeviceBigWigReader(path) as d:
        assert d.kind == h.kind == "bigbed"
        assert d.chromsizes == h.chromsizes
        assert list(d.chromsizes) == list(h.chromsizes)
        n = 0
        for th in thresholds:
            for c in h.chromsizes:
                a, b = h.fetch_arrays(th, c), d.fetch_arrays(th, c)
                for x, y in zip(a, b):
                    assert x.dtype == y.dtype
                    np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))
                assert d.sorted == h.sorted, (c, th)
                n += a[0].size
        with pytest.raises(KeyError):
            d.fetch_arrays(1.0, "no-such-chromosome")
    return n


def test_every_input_agrees(tmp_path):
    for name, sizes, records, opts in cases() + [zero_length_case()]:
        p = tmp_path / (name + ".bb")
        B.write_bigbed(p, sizes, records, **opts)
        _agree(p)


def test_two_million_records_many_blocks(tmp_path):
    recs = B.random_records(0x2B1D, 2_000_000, ["chr%d" % i for i in range(1, 25)], rest_len=(4, 90))
    sizes = {n: int(v[1][-1]) + 1 for n, v in recs.items()}
    sizes["chr9"] = int(recs["chr9"][0][len(recs["chr9"][0]) // 3])      # records past the chromosome's end
    for compress in (True, False):
        p = tmp_path / ("big%d.bb" % compress)
        lay = B.write_bigbed(p, sizes, recs, compress=compress, items_per_block=512, rtree_block=64)
        assert len(lay["blocks"]) > 3000
        assert _agree(p, (0, 1.0)) > 2 * 1_900_000


def test_error_texts_equal_the_host_readers(tmp_path):
    for name, write, words in corrupt_cases():
        p = tmp_path / (name + ".bb")
        write(p)
        want = host_error(p)
        assert want is not None and words in want, name
        with bigwig_device.DeviceBigWigReader(p) as d:
            with pytest.raises(PmxIOError) as ed:
                for c in d.chromsizes:
                    d.fetch_arrays(0, c)
        assert ed.value.msg == want, name


def test_open_track_on_the_device(tmp_path):
    p = write_golden_twin(tmp_path / "twin.data")
    with inputs.open_track(p, True) as r:
        assert isinstance(r, bigwig_device.DeviceBigWigReader) and r.kind == "bigbed"
    with inputs.open_track(C.BIGWIG, True) as r:
        assert r.kind == "bigwig"


def _golden_bam(d):
    bam = d / (STEM + ".bam")
    shutil.copy(GOLD + ".bam", bam)
    shutil.copy(GOLD + ".bam.bai", str(bam) + ".bai")
    return bam


def test_golden_run_with_the_bigbed_twin(tmp_path):
    d = tmp_path / "in"
    d.mkdir()
    bam = _golden_bam(d)
    track = write_golden_twin(tmp_path / "hg19_36mer-test.bb")
    _result, written = pipeline.run(bam, tmp_path / "out", max_shift=300, read_len=36, mapq_criteria=10,
                                    mappability_path=track)
    assert [p.name for p in written] == [STEM + s for s in TABLES]
    _check_tables(written)


def test_command_tree_equals_the_bigwigs(tmp_path):
    bam = _golden_bam(tmp_path)
    for d in ("tbw", "tbb"):            # (each track's _mappability.json cache beside it, apart)
        (tmp_path / d).mkdir()
    shutil.copy(C.BIGWIG, tmp_path / "tbw" / "x.bigwig")
    write_golden_twin(tmp_path / "tbb" / "x.bb")
    common = [bam.name, "-d", "300", "-q", "10", "-r", "36", "--skip-plots"]
    rc, err = _command("pymasc_amd", common + ["-m", "tbw/x.bigwig", "-o", "bw"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", common + ["-m", "tbb/x.bb", "-o", "bb"], tmp_path)
    assert rc == 0, err
    assert _tree(tmp_path / "bb") == _tree(tmp_path / "bw")
    _check_tables([tmp_path / "bb" / (STEM + s) for s in TABLES])


def test_precalc_writes_the_golden_cache(tmp_path):
    write_golden_twin(tmp_path / "hg19_36mer-test.bb")
    rc, err = _command("pymasc_amd.precalc", ["-m", "hg19_36mer-test.bb", "-d", "300", "-r", "36"], tmp_path)
    assert rc == 0, err
    assert (tmp_path / "hg19_36mer-test_mappability.json").read_bytes() == open(GOLDEN_JSON, "rb").read()


def test_two_gloo_ranks_equal_one_with_a_bigbed(tmp_path):
    bam = _golden_bam(tmp_path)
    write_golden_twin(tmp_path / "x.bb")
    common = [bam.name, "-m", "x.bb", "-d", "300", "-q", "10", "-r", "36", "--skip-plots"]
    rc, err = _command("pymasc_amd", common + ["-o", "one"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", common + ["-o", "two", "-p", "2"], tmp_path, PMX_DIST_BACKEND="gloo")
    assert rc == 0, err
    assert _tree(tmp_path / "two") == _tree(tmp_path / "one")
    _check_tables([tmp_path / "one" / (STEM + s) for s in TABLES])
