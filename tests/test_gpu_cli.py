"""``python -m pymasc_amd`` and ``python -m pymasc_amd.precalc`` on the GPU, as child processes: the reference's golden run
(`-d 300 -q 10 -r 36 -m bigwig`) with the read length given and estimated, the BAM file and its BGZF SAM twin under two names,
the precalc cache, and ``-p 2`` (gloo on one GPU; nccl where there are two) against ``-p 1``."""
import os
import shutil
import signal
import subprocess
import sys

import pytest

from . import fixtures as fx
from . import sam_cases as SC
from .test_gpu_run_files import GOLD, TABLES, _check_tables
from .test_gpu_stats import _check_golden

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_JSON = os.path.join(fx.GOLDEN, "hg19_36mer-test_mappability.json")
STEM = "ENCFF000RMB-test"


def _command(module, argv, cwd, timeout=600, **env):
    """``python -m <module> argv`` in ``cwd`` under a time limit: on expiry SIGTERM, 10 s, then SIGKILL, and the test fails.
    Never retried.  Returns (exit status, stderr)."""
    e = dict(os.environ)
    e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE"):
        e.pop(k, None)
    e.update(env)
    p = subprocess.Popen([sys.executable, "-m", module] + list(argv), cwd=str(cwd), env=e, stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True)
    try:
        _out, err = p.communicate(timeout=timeout)
    except subprocess.TimeoutExpired:
        p.send_signal(signal.SIGTERM)
        try:
            p.communicate(timeout=10)
        except subprocess.TimeoutExpired:
            p.kill()
            p.communicate()
        pytest.fail("python -m {} {} did not finish in {} s".format(module, " ".join(argv), timeout))
    return p.returncode, err


@pytest.fixture
def inputs(tmp_path):
    """Copies of the golden BAM (with its index), its BGZF SAM twin and the track: no cache is written under tests/golden."""
    bam = tmp_path / (STEM + ".bam")
    shutil.copy(GOLD + ".bam", bam)
    shutil.copy(GOLD + ".bam.bai", str(bam) + ".bai")
    sam = tmp_path / "twin.sam.gz"
    shutil.copy(SC.GOLDEN_SAM_GZ, sam)
    bw = tmp_path / "hg19_36mer-test.bigwig"
    shutil.copy(os.path.join(fx.GOLDEN, "hg19_36mer-test.bigwig"), bw)
    return bam, sam, bw


def _tree(d):
    return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}


def _check_set(out, base):
    written = [out / (base + s) for s in TABLES]
    _check_tables(written)
    _check_golden(out / (base + "_stats.tab"), base)


def test_golden_run_read_length_given_and_estimated(tmp_path, inputs):
    bam, _sam, bw = inputs
    common = [bam.name, "-m", bw.name, "-d", "300", "-q", "10", "--skip-plots"]
    rc, err = _command("pymasc_amd", common + ["-o", "out", "-r", "36"], tmp_path)
    assert rc == 0, err
    out = tmp_path / "out"
    assert sorted(os.listdir(out)) == sorted(STEM + s for s in TABLES + ["_stats.tab"])
    _check_set(out, STEM)
    assert (tmp_path / "hg19_36mer-test_mappability.json").read_bytes() == open(GOLDEN_JSON, "rb").read()
    rc, err = _command("pymasc_amd", common + ["-o", "est"], tmp_path)
    assert rc == 0, err
    assert "Estimated read length = 36" in err
    assert _tree(tmp_path / "est") == _tree(out)


def test_bam_and_sam_twin_with_names(tmp_path, inputs):
    bam, sam, bw = inputs
    rc, err = _command("pymasc_amd", [str(bam), str(sam), "-m", str(bw), "-d", "300", "-q", "10", "-r", "36", "-n", "A",
                                      "B", "-o", "out"], tmp_path)
    assert rc == 0, err
    out = tmp_path / "out"
    assert sorted(os.listdir(out)) == sorted(b + s for b in "AB" for s in TABLES + ["_stats.tab"])
    for b in "AB":
        _check_set(out, b)
        assert "Skip output plots '{}'".format(os.path.join("out", b + ".pdf")) in err


def test_precalc_writes_the_golden_cache(tmp_path, inputs):
    _bam, _sam, bw = inputs
    rc, err = _command("pymasc_amd.precalc", ["-m", str(bw), "-d", "300", "-r", "36"], tmp_path)
    assert rc == 0, err
    assert (tmp_path / "hg19_36mer-test_mappability.json").read_bytes() == open(GOLDEN_JSON, "rb").read()
    st = os.stat(tmp_path / "hg19_36mer-test_mappability.json")
    rc, err = _command("pymasc_amd.precalc", ["-m", str(bw), "-d", "300", "-r", "36"], tmp_path)
    assert rc == 0, err
    assert "Mappability stats updating is not required." in err
    assert os.stat(tmp_path / "hg19_36mer-test_mappability.json").st_mtime_ns == st.st_mtime_ns


@pytest.mark.parametrize("backend", ["gloo", "nccl"])
def test_two_ranks_equal_one(tmp_path, inputs, backend):
    import torch
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip("two ranks over nccl need two GPUs")
    bam, _sam, bw = inputs
    common = [bam.name, "-m", bw.name, "-d", "300", "-q", "10", "-r", "36", "--skip-plots"]
    rc, err = _command("pymasc_amd", common + ["-o", "one"], tmp_path)
    assert rc == 0, err
    rc, err = _command("pymasc_amd", common + ["-o", "two", "-p", "2"], tmp_path, PMX_DIST_BACKEND=backend)
    assert rc == 0, err
    assert _tree(tmp_path / "two") == _tree(tmp_path / "one")
    _check_set(tmp_path / "two", STEM)
