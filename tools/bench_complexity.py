"""Times pmx_dbam_complexity on the synthetic file of tools/bench_ingest.py beside reading that file (open + decode on the device)
and beside complexity.count_host on the fetched arrays: python tools/bench_complexity.py --reads 20000000 --out profiles/complexity.json

The times are wall-clock around the library calls (allocations and the result copy included), medians after one warm-up call."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import complexity  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from tools.bench_ingest import synth_bam  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_complexity_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(a.path):
        synth_bam(a.path, a.reads)
    opens, counts = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        with DeviceBamReader(a.path) as r:
            kept = r.decode(a.mapq, complexity.COMPLEXITY_EXCLUDE)
            opens.append(time.perf_counter() - t0)
    with DeviceBamReader(a.path) as r:
        kept = r.decode(a.mapq, complexity.COMPLEXITY_EXCLUDE)
        c = r.library_complexity(a.mapq)                    # warm-up
        for _ in range(a.reps):
            t0 = time.perf_counter()
            c = r.library_complexity(a.mapq)
            counts.append(time.perf_counter() - t0)
        cols = r._fetch(0, kept)
        t0 = time.perf_counter()
        per, hist = complexity.count_host(*cols, len(r.references))
        host_s = time.perf_counter() - t0
        assert int(per[:, 0].sum()) == c.reads == kept and int(per[:, 1].sum()) == c.distinct
        assert [int(x) for x in hist] == [int(x) for x in c.hist]
    res = dict(reads=a.reads, kept=kept, distinct=c.distinct, m1=c.m1, m2=c.m2, mapq=a.mapq,
               file_to_records_s=sorted(opens), complexity_call_s=sorted(counts), complexity_call_median_s=statistics.median(counts),
               count_host_s=host_s, peak_device_bytes_per_kept_read=40, library_version=int(r._L.pmx_dbam_version()))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
