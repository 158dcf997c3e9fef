"""Times the anchor profile behind --tss (pmx_dbam_tss_begin + add + copy) on the synthetic file of tools/bench_ingest.py beside the
peak count's add over the same reads (pmx_dbam_peakcount_add, the nearest comparable launch):
python tools/bench_tss.py --reads 20000000 --out profiles/tss.json

The anchors are synthetic: --anchors sites, one at the start of every line of tools/bench_peaks.py's synthetic peak set (spread over
the references in proportion to their lengths, shuffled), on a random strand; the peak count takes those lines themselves.  The times
are wall-clock around the library calls (allocations, the sort of the anchors and the result copies included), medians after one
warm-up round.  --reps 1 is the run to put under `rocprofv3 --kernel-trace --stats` for the split of the kernels; the trace is a
run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import peaks, tss  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE  # noqa: E402
from tools.bench_ingest import synth_bam  # noqa: E402
from tools.bench_peaks import synthetic_lines  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_complexity_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--anchors", type=int, default=60_000)
    ap.add_argument("--flank", type=int, default=2000)
    ap.add_argument("--extend", type=int, nargs="+", default=[0, 1])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(a.path):
        print("writing {} ...".format(a.path), file=sys.stderr, flush=True)
        synth_bam(a.path, a.reads)
    res = dict(reads=a.reads, mapq=a.mapq, flank=a.flank, runs=[])
    with DeviceBamReader(a.path) as r:
        res["kept"] = r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["library_version"] = int(r._L.pmx_dbam_version())
        lines = synthetic_lines(r.references, r.lengths, a.anchors)
        rng = np.random.default_rng(2)
        sites = {n: [(b + 1, "+-"[int(s)]) for (b, _e), s in zip(v, rng.integers(0, 2, size=len(v)))] for n, v in lines.items()}
        bound = tss.open_anchors(sites, r.references, r.lengths)
        for extend in a.extend:
            c = tss.count_device(r, bound, a.mapq, None, a.flank, extend)           # warm-up
            begins, adds, copies = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                acc = tss.DeviceCount(r, bound, a.mapq, None, a.flank, extend)
                t1 = time.perf_counter()
                acc.add(r)
                t2 = time.perf_counter()
                table = acc.copy(r)
                t3 = time.perf_counter()
                begins.append(t1 - t0)
                adds.append(t2 - t1)
                copies.append(t3 - t2)
            assert c.N <= res["kept"] and int(table.sum()) == int(c.total.sum()) and c.anchors == len(bound)
            pk = peaks.DeviceCount(r, lines, a.mapq, None, extend)
            pk.add(r)                                                               # warm-up
            pk_adds = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                pk.add(r)
                pk_adds.append(time.perf_counter() - t0)
            res["runs"].append(dict(extend=extend, anchors=c.anchors, reads=c.N, reads_near_anchors=c.n_near, pairs=c.pairs,
                                    bases=int(c.total.sum()), enrichment=c.enrichment, begin_s=sorted(begins), add_s=sorted(adds),
                                    copy_s=sorted(copies), begin_median_s=statistics.median(begins), add_median_s=statistics.median(adds),
                                    copy_median_s=statistics.median(copies), peakcount_lines=int(pk.layout.offsets[-1]),
                                    peakcount_add_s=sorted(pk_adds), peakcount_add_median_s=statistics.median(pk_adds)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
