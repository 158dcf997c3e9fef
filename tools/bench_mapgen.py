#!/usr/bin/env python3
"""k-mer track benchmark: a synthetic genome FASTA -> DeviceKmerTrackReader -> intervals in HBM.

Writes a FASTA of the hg38 chromosome sizes (pymasc_amd.synth.HG38; --bases scales them down) with repeat content: random
bases, families of exact copies on either strand, tandem repeats and N runs.  Then, with the file in the page cache, times
open -> intervals in HBM for each k (best of --repeat), reports the peak device memory of the open, and runs the host
generator on a smaller genome (--host-bases) for scale.  One JSON line per measurement.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pymasc_amd import kmer_track  # noqa: E402
from pymasc_amd.synth import HG38  # noqa: E402


def write_genome(path, bases, seed=1, width=60):
    """hg38-shaped chromosomes scaled to `bases` in all; returns the bases written."""
    rng = np.random.default_rng(seed)
    total = sum(n for _c, n in HG38)
    lut = np.frombuffer(b"ACGT", dtype=np.uint8)
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGTN")] = list(b"TGCAN")
    fams = [lut[rng.integers(0, 4, int(rng.integers(300, 6000)))] for _ in range(200)]
    written = 0
    with open(path, "wb") as fh:
        for name, n in HG38:
            n = max(1000, int(n * bases / total))
            a = lut[rng.integers(0, 4, n, dtype=np.uint8)]
            for _ in range(n // 20000):                     # ~15 % of the bases in repeat copies
                f = fams[int(rng.integers(0, len(fams)))]
                x = f if rng.random() < 0.5 else comp[f][::-1]
                p = int(rng.integers(0, max(1, n - len(x))))
                a[p:p + len(x)] = x[:n - p]
            for _ in range(max(1, n // 5_000_000)):         # tandem repeats and N runs
                unit = lut[rng.integers(0, 4, int(rng.integers(2, 200)))]
                L = min(n // 4, 50_000)
                p = int(rng.integers(0, n - L))
                a[p:p + L] = np.resize(unit, L)
                p = int(rng.integers(0, n - L))
                a[p:p + L // 2] = ord("N")
            fh.write(b">" + name.encode() + b"\n")
            rows = a[: (n // width) * width].reshape(-1, width)
            body = np.concatenate([rows, np.full((rows.shape[0], 1), 10, dtype=np.uint8)], axis=1).tobytes()
            fh.write(body)
            if n % width:
                fh.write(a[(n // width) * width:].tobytes() + b"\n")
            written += n
    return written


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=float, default=3.1e9, help="genome size in bases (default: hg38's)")
    ap.add_argument("--ks", default="36,100")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--host-bases", type=float, default=2e7, help="genome size of the host generator's run (0: none)")
    ap.add_argument("--dir", default="/tmp")
    args = ap.parse_args()
    import torch
    path = os.path.join(args.dir, "bench_mapgen.fa")
    t = time.perf_counter()
    n = write_genome(path, int(args.bases))
    print(json.dumps({"what": "write", "bases": n, "bytes": os.path.getsize(path), "s": round(time.perf_counter() - t, 2)}),
          flush=True)
    with open(path, "rb") as fh:                            # into the page cache
        while fh.read(1 << 26):
            pass
    for k in [int(x) for x in args.ks.split(",")]:
        best, intervals, peak = None, 0, 0
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            free0, _tot = torch.cuda.mem_get_info(0)
            low = [free0]
            stop = threading.Event()

            def poll():                                     # the lowest free memory seen during the open
                while not stop.is_set():
                    low[0] = min(low[0], torch.cuda.mem_get_info(0)[0])
                    time.sleep(0.002)
            th = threading.Thread(target=poll)
            th.start()
            t = time.perf_counter()
            try:
                r = kmer_track.DeviceKmerTrackReader(path, k)
                dt = time.perf_counter() - t
            finally:
                stop.set()
                th.join()
            with r:
                intervals = sum(len(r.fetch_arrays(1.0, c)[0]) for c in r.chromsizes)
            best = dt if best is None else min(best, dt)
            peak = max(peak, free0 - low[0])
        print(json.dumps({"what": "device", "k": k, "bases": n, "best_s": round(best, 3), "intervals": intervals,
                          "peak_device_GiB": round(peak / 2**30, 2), "free_before_GiB": round(free0 / 2**30, 1)}), flush=True)
    os.unlink(path)
    if args.host_bases:
        hp = os.path.join(args.dir, "bench_mapgen_host.fa")
        hn = write_genome(hp, int(args.host_bases), seed=2)
        for k in [int(x) for x in args.ks.split(",")]:
            t = time.perf_counter()
            with kmer_track.KmerTrackReader(hp, k, threads=16) as h:
                dh = time.perf_counter() - t
            t = time.perf_counter()
            with kmer_track.DeviceKmerTrackReader(hp, k) as d:
                dd = time.perf_counter() - t
            print(json.dumps({"what": "host_vs_device", "k": k, "bases": hn, "host_s": round(dh, 3), "device_s": round(dd, 3)}),
                  flush=True)
        os.unlink(hp)


if __name__ == "__main__":
    main()
