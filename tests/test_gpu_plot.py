"""``python -m pymasc_amd`` on the GPU, then ``python -m pymasc_amd.plot`` on the tables it wrote, both as child processes:
the replot's ``_stats.tab`` equals the run's row for row, its ``_cc.tab`` / ``_mscc.tab`` equal the run's (the per-chromosome
columns exactly, ``whole`` to decimal=10), and its PDF has PyMaSC's pages.  The reference's golden run (``-d 300 -q 10``),
with both curves, with ``--skip-ncc`` and with ``-i chr1`` given to both commands."""
import os
import re
import shutil

import numpy as np
import pytest

from pymasc_amd import stats as S
from . import fixtures as fx
from .test_gpu_cli import _command

pytestmark = pytest.mark.gpu

STEM = "ENCFF000RMB-test"
GOLD = os.path.join(fx.GOLDEN, STEM)


@pytest.fixture
def golden(tmp_path):
    """Copies of the golden BAM (with its index) and the track: the cache is written beside the copy."""
    bam = tmp_path / (STEM + ".bam")
    shutil.copy(GOLD + ".bam", bam)
    shutil.copy(GOLD + ".bam.bai", str(bam) + ".bai")
    bw = tmp_path / "hg19_36mer-test.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    return bam, bw


def _rows(path):
    with open(path) as fh:
        return [line.rstrip("\n").split("\t") for line in fh]


def _pages(path) -> int:
    return len(re.findall(rb"/Type\s*/Page(?![A-Za-z])", open(path, "rb").read()))


@pytest.mark.parametrize("extra,tables,pages", [([], ["_cc.tab", "_mscc.tab"], 5),
                                                (["--skip-ncc"], ["_mscc.tab"], 3),
                                                (["-i", "chr1"], ["_cc.tab", "_mscc.tab"], 5)])
def test_replot_of_the_golden_run(tmp_path, golden, extra, tables, pages):
    bam, bw = golden
    rc, err = _command("pymasc_amd", [bam.name, "-m", bw.name, "-d", "300", "-q", "10", "--skip-plots", "-o", "out"] + extra,
                       tmp_path)
    assert rc == 0, err
    plot_extra = [] if extra == ["--skip-ncc"] else extra
    rc, err = _command("pymasc_amd.plot", ["out/" + STEM, "-s", bam.name, "-m", bw.name, "-o", "replot"] + plot_extra,
                       tmp_path)
    assert rc == 0, err
    out, rep = tmp_path / "out", tmp_path / "replot"
    assert sorted(os.listdir(rep)) == sorted([STEM + ".pdf", STEM + "_stats.tab"] + [STEM + t for t in tables])
    got, want = S.load_stats(rep / (STEM + "_stats.tab")), S.load_stats(out / (STEM + "_stats.tab"))
    assert list(got.items()) == list(want.items())
    if not extra:
        assert got["Genome length"] == S.load_stats(GOLD + "_stats.tab")["Genome length"]
    for t in tables:
        g, w = _rows(rep / (STEM + t)), _rows(out / (STEM + t))
        assert [r[0] for r in g] == [r[0] for r in w] and g[0] == w[0]
        assert [r[2:] for r in g] == [r[2:] for r in w]
        np.testing.assert_almost_equal([float(r[1]) for r in g[1:]], [float(r[1]) for r in w[1:]], decimal=10)
    assert _pages(rep / (STEM + ".pdf")) == pages
