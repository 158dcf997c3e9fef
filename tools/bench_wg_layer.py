#!/usr/bin/env python3
"""Runs bench.py with every context it creates put at a layer width (pmx_debug_set_wg_layer: 0 the device's compute units,
1 the tile ranges in launch order -- the order before DESIGN.md 8.0.5) -- the third column of its A/B table.  bench.py itself
has no such switch and gets none; the library reads no environment.

usage: python tools/bench_wg_layer.py WIDTH [bench.py arguments ...]"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
width = int(sys.argv[1])
from pymasc_amd import ffi

_init = ffi.Context.__init__


def _init_with_width(self, *a, **k):
    _init(self, *a, **k)
    self.debug_set_wg_layer(width)


ffi.Context.__init__ = _init_with_width
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
