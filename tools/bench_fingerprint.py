"""Times the bin count behind --fingerprint (pmx_dbam_bincount_begin + add + hist) on the synthetic file of tools/bench_ingest.py
beside reading that file (open + decode on the device): python tools/bench_fingerprint.py --reads 20000000 --out profiles/fingerprint.json

The times are wall-clock around the library calls (allocations, the zeroing of the bins and the result copies included), medians
after one warm-up round.  --reps 1 --no-open is the run to put under `rocprofv3 --kernel-trace --stats` for the split of the two
kernels; the trace is a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import fingerprint  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE  # noqa: E402
from tools.bench_ingest import synth_bam  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_complexity_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--bin", type=int, default=500)
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
    res = dict(reads=a.reads, mapq=a.mapq, bin_size=a.bin, file_to_records_s=sorted(opens), runs=[])
    with DeviceBamReader(a.path) as r:
        res["kept"] = r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["library_version"] = int(r._L.pmx_dbam_version())
        for extend in a.extend:
            c = fingerprint.count_device(r, a.mapq, None, a.bin, extend)          # warm-up
            whole, begins, adds, hists = [], [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                acc = fingerprint.DeviceCount(r, a.mapq, None, a.bin, extend)
                t1 = time.perf_counter()
                acc.add(r)
                t2 = time.perf_counter()
                c = acc.result(r)
                t3 = time.perf_counter()
                whole.append(t3 - t0)
                begins.append(t1 - t0)
                adds.append(t2 - t1)
                hists.append(t3 - t2)
            assert c.reads <= res["kept"] and c.T >= c.reads
            res["runs"].append(dict(extend=extend, bins=c.B, reads=c.reads, total=c.T, largest_bin=c.kmax, mean=c.mean, auc=c.auc,
                                    synthetic_jsd=c.synthetic_jsd, begin_add_hist_s=sorted(whole),
                                    begin_add_hist_median_s=statistics.median(whole), begin_median_s=statistics.median(begins),
                                    add_median_s=statistics.median(adds), hist_median_s=statistics.median(hists)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
