"""The C-ABI library builds, loads and exports every symbol include/pymasc_amd.h declares; without a
GPU it must fail loudly (no CPU fallback)."""
import os
import re

import pytest

from pymasc_amd import build, ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name="pymasc_amd.h"):
    text = open(os.path.join(ROOT, "include", name)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pmx_[a-z_0-9]+)\s*\(", text)))


def _check_prototypes(table):
    """Every entry of a reader library's table states both a restype and an argtypes list (the functions without arguments an
    empty one)."""
    for name, proto in table.items():
        assert isinstance(proto, tuple) and len(proto) == 2, name
        restype, argtypes = proto
        assert restype is None or hasattr(restype, "from_param"), name
        assert isinstance(argtypes, list) and all(hasattr(a, "from_param") for a in argtypes), name
        assert (argtypes == []) == name.endswith(("_last_error", "_version")), name


def test_library_builds_for_gfx950():
    path = build.build()
    assert os.path.exists(path)
    blob = open(path, "rb").read()
    assert b"gfx950" in blob   # the code object target is embedded in the fat binary


def test_every_declared_symbol_is_exported():
    L = ffi.load_library()
    syms = header_symbols()
    assert len(syms) >= 20
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(ffi.EXPORTS) == syms
    assert L.pmx_version() >= 101


def test_io_library_builds_and_exports_its_header():
    """libpymasc_io.so (host readers, include/pymasc_amd_io.h): every declared symbol, nothing undeclared bound."""
    from pymasc_amd import bam, native
    path = build.build_io()
    assert os.path.exists(path)
    L = bam.load_io_library()
    syms = header_symbols("pymasc_amd_io.h")
    assert len(syms) >= 14
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(bam.IO_EXPORTS) == syms
    _check_prototypes(native.IO_PROTOTYPES)
    assert L.pmx_io_version() >= 1
    text = open(os.path.join(ROOT, "include", "pymasc_amd_io.h")).read()
    consts = dict(re.findall(r"#define\s+(PMX_BAM_FLAG_[A-Z0-9]+)\s+(0x[0-9a-fA-F]+)u", text))
    for k, v in consts.items():
        assert getattr(bam, k) == int(v, 16), k


def test_ingest_library_builds_and_exports_its_header(tmp_path):
    """libpymasc_ingest.so (device-side BGZF inflate + BAM decode, include/pymasc_amd_ingest.h): gfx950 code object, every
    declared symbol exported, nothing undeclared bound; without a GPU opening a file fails loudly (no host inflate in it)."""
    from pymasc_amd import bam, bam_device, native
    path = build.build_ingest()
    assert os.path.exists(path)
    assert b"gfx950" in open(path, "rb").read()
    L = bam_device.load_ingest_library()
    syms = header_symbols("pymasc_amd_ingest.h")
    assert len(syms) >= 12
    for s in syms:
        assert hasattr(L, s), s
    assert sorted(bam_device.INGEST_EXPORTS) == syms
    _check_prototypes(native.INGEST_PROTOTYPES)
    assert L.pmx_dbam_version() >= 1
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(bam.PmxIOError, match="GPU|device|HIP"):
            bam_device.DeviceBamReader(os.path.join(ROOT, "tests", "golden", "ENCFF000RMB-test.bam"))


def test_header_constants_match_binding():
    text = open(os.path.join(ROOT, "include", "pymasc_amd.h")).read()
    consts = dict(re.findall(r"#define\s+(PMX_[A-Z_0-9]+)\s+(-?\d+)u?\b", text))
    for name in ("PMX_ROW_NCC_CCBINS", "PMX_ROW_MSCC_FSUM", "PMX_ROW_MSCC_RSUM", "PMX_ROW_MSCC_CCBINS",
                 "PMX_ROW_MLEN", "PMX_ROW_SCALARS", "PMX_NROWS", "PMX_FLAG_SKIP_NCC", "PMX_FLAG_FORCE_DENSE", "PMX_FLAG_SKIP_MLEN",
                 "PMX_FLAG_FORCE_SPARSE", "PMX_FLAG_WINDOW_ONLY", "PMX_FLAG_DEEP_LISTS", "PMX_PATH_DENSE", "PMX_PATH_SPARSE", "PMX_KERNEL_CC_DENSE",
                 "PMX_KERNEL_CC_SPARSE", "PMX_KERNEL_AUTOCORR", "PMX_KERNEL_CC_EVENTS"):
        assert int(consts[name]) == getattr(ffi, name), name
    ledger = [name for name in consts if name.startswith("PMX_LEDGER_") and not name.endswith("_")]
    assert len(ledger) == int(consts["PMX_LEDGER_FAMILIES_"]) == len(ffi.ledger_sizes())
    for name in ledger:
        assert int(consts[name]) == getattr(ffi, name), name


def test_no_gpu_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    assert ffi.device_count() == 0
    with pytest.raises(ffi.PmxError) as ei:
        ffi.Context(0)
    assert ei.value.code == -4
    from pymasc_amd.calculator import CCHipCalculator
    with pytest.raises(ffi.PmxError):
        CCHipCalculator(100, 36, ["chr1"], [1000])


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "pymasc_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in src.lower() or f == "__init__.py" and False, os.path.join(dirpath, f)


def test_no_method_is_defined_twice_in_a_class():
    """A second `def` of the same name silently replaces the first (round 4: a new Context.bits_set_regions_dev for uint32 arrays
    shadowed the int64 one the benchmark's vector builder calls -- the bench's own end-to-end check caught it, no test did)."""
    import ast
    import glob
    for f in glob.glob(os.path.join(ROOT, "pymasc_amd", "*.py")):
        tree = ast.parse(open(f).read())
        for c in [n for n in ast.walk(tree) if isinstance(n, ast.ClassDef)]:
            names = [n.name for n in c.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))]
            props = {n.name for n in c.body if isinstance(n, ast.FunctionDef) and n.decorator_list}
            dup = {x for x in names if names.count(x) > 1 and x not in props}
            assert not dup, (f, c.name, dup)
