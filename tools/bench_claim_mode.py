#!/usr/bin/env python3
"""Runs bench.py with every context it creates put into a claim mode (pmx_debug_set_claim_mode: 0 claims + helping, 1 odd
workgroups help only, 2 the static walk) -- the third column of the A/B tables of DESIGN.md 8.0.3.  bench.py itself has no such
switch and gets none; the library reads no environment.

usage: python tools/bench_claim_mode.py MODE [bench.py arguments ...]"""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
mode = int(sys.argv[1])
from pymasc_amd import ffi

_init = ffi.Context.__init__


def _init_with_mode(self, *a, **k):
    _init(self, *a, **k)
    self.debug_set_claim_mode(mode)


ffi.Context.__init__ = _init_with_mode
sys.argv = [os.path.join(ROOT, "bench.py")] + sys.argv[2:]
runpy.run_path(sys.argv[0], run_name="__main__")
