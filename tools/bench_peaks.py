"""Times the peak count behind --peaks (pmx_dbam_peakcount_begin + add + totals) on the synthetic file of tools/bench_ingest.py beside
reading that file (open + decode on the device): python tools/bench_peaks.py --reads 20000000 --out profiles/peaks.json

The peak set is synthetic: --lines non-overlapping lines of 200 to 2000 bases, spread over the references in proportion to their
lengths and handed over in a shuffled order.  The times are wall-clock around the library calls (allocations, the sort of the lines
and the result copies included), medians after one warm-up round.  --reps 1 --no-open is the run to put under
`rocprofv3 --kernel-trace --stats` for the split of the kernels; the trace is a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import peaks  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE  # noqa: E402
from tools.bench_ingest import synth_bam  # noqa: E402


def synthetic_lines(references, lengths, n, seed=1):
    """``{name: [(start, end), ...]}``: about ``n`` lines that do not overlap, one per slot of equal width, shuffled."""
    rng = np.random.default_rng(seed)
    total = float(sum(lengths))
    out = {}
    for name, length in zip(references, lengths):
        k = int(n * length / total)
        slot = length // max(k, 1)
        if k == 0 or slot < 2001:
            continue
        width = rng.integers(200, 2001, size=k)
        start = np.arange(k) * slot + rng.integers(0, slot - width)
        order = rng.permutation(k)
        out[name] = list(zip(start[order].tolist(), (start + width)[order].tolist()))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_complexity_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--lines", type=int, default=100_000)
    ap.add_argument("--extend", type=int, nargs="+", default=[0, 200])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-open", action="store_true", help="skip the timing of open + decode")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(a.path):
        synth_bam(a.path, a.reads)
    opens = []
    for _ in range(0 if a.no_open else 3):
        t0 = time.perf_counter()
        with DeviceBamReader(a.path) as r:
            r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
            opens.append(time.perf_counter() - t0)
    res = dict(reads=a.reads, mapq=a.mapq, file_to_records_s=sorted(opens), runs=[])
    with DeviceBamReader(a.path) as r:
        res["kept"] = r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["library_version"] = int(r._L.pmx_dbam_version())
        lines = peaks.open_peaks(synthetic_lines(r.references, r.lengths, a.lines))
        for extend in a.extend:
            c = peaks.count_device(r, lines, a.mapq, None, extend)                # warm-up
            whole, begins, adds, reads_back = [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                acc = peaks.DeviceCount(r, lines, a.mapq, None, extend)
                t1 = time.perf_counter()
                acc.add(r)
                t2 = time.perf_counter()
                totals, _per_ref = acc.totals(r)
                t3 = time.perf_counter()
                whole.append(t3 - t0)
                begins.append(t1 - t0)
                adds.append(t2 - t1)
                reads_back.append(t3 - t2)
            assert c.N <= res["kept"] and [c.N, c.n_in, c.union_bases, c.n_lines] == totals.tolist()
            res["runs"].append(dict(extend=extend, lines=c.n_lines, reads=c.N, reads_in_peaks=c.n_in, peak_bases=c.union_bases,
                                    genome_bases=c.genome_bases, frip=c.frip, enrichment=c.enrichment,
                                    begin_add_totals_s=sorted(whole), begin_add_totals_median_s=statistics.median(whole),
                                    begin_median_s=statistics.median(begins), add_median_s=statistics.median(adds),
                                    totals_median_s=statistics.median(reads_back)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
