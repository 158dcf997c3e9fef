#!/usr/bin/env python3
"""Read-length estimate benchmark: the histogram of pmx_dbam_readlen_hist on an already-open device reader, next to
that file's decode() and the host reader's pmx_bam_readlen_hist, for tools/bench_ingest.py's synthetic file (every read 36: the
contention case) and for a file of the same records whose CIGAR lengths are a trimmed mix (20..36).  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_ingest import synth_bam  # noqa: E402
from pymasc_amd import bam as B  # noqa: E402
from pymasc_amd import bam_device as D  # noqa: E402


def trimmed(seed):
    rng = np.random.default_rng(seed)
    lens = np.arange(20, 37)
    p = np.where(lens == 36, 40.0, 1.0) * np.exp((lens - 36) / 6.0)
    p /= p.sum()
    return lambda k: rng.choice(lens, size=k, p=p).astype(np.int64)


def measure(path, mapq, reps):
    out = {}
    with D.DeviceBamReader(path) as r:
        t0 = time.perf_counter()
        r.read_length_histogram(mapq)                 # on a fresh handle: the record chain is built first
        out["first_hist_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        dec, hist = [], []
        for i in range(reps):
            t0 = time.perf_counter()
            r.decode(mapq)
            dec.append(time.perf_counter() - t0)
            m = mapq + 1 + (i % 2)                    # another threshold each time: the kept result is not reused
            t0 = time.perf_counter()
            h = r.read_length_histogram(m)
            hist.append(time.perf_counter() - t0)
        out["decode_ms"] = [round(x * 1e3, 3) for x in sorted(dec)]
        out["hist_ms"] = [round(x * 1e3, 3) for x in sorted(hist)]
        out["records"] = r.counters()["records"]
        dev = r.read_length_histogram(mapq)
    host = []
    for _ in range(3):
        with B.BamReader(path, threads=16) as b:
            t0 = time.perf_counter()
            hh = b.read_length_histogram(mapq)
            host.append(time.perf_counter() - t0)
    out["host16_s"] = [round(x, 3) for x in sorted(host)]
    out["distinct"] = int(dev.lengths.size)
    out["median"] = dev.estimate("MEDIAN")
    out["device_equals_host"] = bool(dev.counters == hh.counters and dev.lengths.tolist() == hh.lengths.tolist()
                                     and dev.counts.tolist() == hh.counts.tolist() and dev.first.tolist() == hh.first.tolist())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--dir", default="/tmp")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    res = {"reads": a.reads}
    for tag, lens in (("one_length", None), ("trimmed_mix", trimmed(5))):
        path = os.path.join(a.dir, "pymasc_readlen_%s.bam" % tag)
        synth_bam(path, a.reads, cigar_lengths=lens)
        try:
            res[tag] = measure(path, a.mapq, a.reps)
        finally:
            os.remove(path)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
