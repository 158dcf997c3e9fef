#!/usr/bin/env bash
# TEST INFRASTRUCTURE ONLY.  Builds the reference's own `successive` calculators (NCC and MSCC) from the
# sources where they lie in the reference tree (/root/reference, or $PYMASC_REFERENCE) into oracle/_ref/
# (git-ignored, never committed).  They are used by oracle/make_ref_vectors.py and
# oracle/make_ref_mscc_vectors.py to generate golden vectors in THIS container only; nothing of the
# reference tree (source, generated C, bytecode or otherwise) is copied, and nothing of it travels to the GPU box.
#
# Built, each with cython + numpy only:
#   PyMaSC/core/successive/ncc.pyx    the NCC calculator
#   PyMaSC/core/successive/mscc.pyx   the MSCC calculator; takes its feeder as a Python object
#   PyMaSC/core/mappability.pyx       BWFeederWithMappableRegionSum, that feeder (and the lag table)
#   PyMaSC/reader/bigwig.pyx          BigWigReader underneath it.  Its `import pyBigWig` is a plain Python-level
#                                     import resolved when the module is loaded: the generator puts
#                                     oracle/ref_shims/ (a JSON-backed stand-in of our own) on sys.path
# NOT built: core/bitarray/* (links the noporpoise/BitArray C library, an empty submodule in the reference
# tree) and core/readlen.pyx (not on this path).
set -euo pipefail
REF="${PYMASC_REFERENCE:-/root/reference}"
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/_ref"
[ -d "$REF/PyMaSC" ] || { echo "no reference tree at $REF: skipping oracle/_ref build"; exit 0; }
mkdir -p "$OUT"
PYINC=$(python3 -c 'import sysconfig; print(sysconfig.get_paths()["include"])')
NPINC=$(python3 -c 'import numpy; print(numpy.get_include())')
EXT=$(python3 -c 'import sysconfig; print(sysconfig.get_config_var("EXT_SUFFIX"))')
for pyx in core/successive/ncc core/successive/mscc core/mappability reader/bigwig; do
    mod=$(basename "$pyx")
    python3 -m cython -3 -I "$REF" -o "$OUT/$mod.c" "$REF/PyMaSC/$pyx.pyx"
    gcc -O2 -fPIC -shared -w -DNPY_NO_DEPRECATED_API=NPY_1_7_API_VERSION -I"$PYINC" -I"$NPINC" \
        -o "$OUT/$mod$EXT" "$OUT/$mod.c"
    rm -f "$OUT/$mod.c"
    echo "built $OUT/$mod$EXT"
done
