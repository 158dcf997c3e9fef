"""Times the GC-bias count behind --gc-bias (pmx_dgc_open, pmx_dbam_gcbias_begin, _add, _tables) on the synthetic 3.1-Gbp genome of
tools/bench_mapgen.py and the synthetic file of tools/bench_ingest.py: python tools/bench_gcbias.py --out profiles/gcbias.json

The times are wall-clock around the library calls (allocations and the result copies included), each the median of --reps rounds
after one warm-up round.  `begin` holds k_gc_bits and k_gc_windows (the genome pass); the open is timed apart.  --reps 1 is the
run to put under `rocprofv3 --kernel-trace --stats` for the split of the kernels; the trace is a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import gcbias  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE  # noqa: E402
from pymasc_amd.synth import HG38  # noqa: E402
from tools.bench_ingest import synth_bam  # noqa: E402
from tools.bench_mapgen import write_genome  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_complexity_bench.bam")
    ap.add_argument("--genome", default="/tmp/pymasc_gcbias_bench.fa")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--window", type=int, nargs="+", default=[100, 1024])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(a.path):
        synth_bam(a.path, a.reads)
    if not os.path.exists(a.genome):        # (an int: every record gets exactly its hg38 length, the file's header's)
        write_genome(a.genome, sum(n for _c, n in HG38))
    res = dict(reads=a.reads, mapq=a.mapq, genome_bytes=os.path.getsize(a.genome), runs=[])
    opens = []
    for k in range(a.reps + 1):
        t0 = time.perf_counter()
        g = gcbias.DeviceGenome(a.genome)
        opens.append(time.perf_counter() - t0)
        if k < a.reps:
            g.close()
    res.update(open_s=sorted(opens[1:]), open_median_s=statistics.median(opens[1:]), records=len(g.names), bases=sum(g.lengths))
    with g, DeviceBamReader(a.path) as r:
        res["kept"] = r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["library_version"] = int(r._L.pmx_dbam_version())
        for window in a.window:
            c = gcbias.count_device(r, g, a.mapq, None, window)                 # warm-up
            begins, adds, tables = [], [], []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                acc = gcbias.DeviceCount(r, g, a.mapq, None, window)
                t1 = time.perf_counter()
                acc.add(r)
                t2 = time.perf_counter()
                c = acc.result(r)
                t3 = time.perf_counter()
                begins.append(t1 - t0)
                adds.append(t2 - t1)
                tables.append(t3 - t2)
            assert c.reads + c.off_end + c.blocked <= res["kept"]
            res["runs"].append(dict(window=window, windows=c.windows, reads=c.reads, off_end=c.off_end, blocked=c.blocked,
                                    window_gc=c.window_gc, read_gc=c.read_gc, at_dropout=c.at_dropout, gc_dropout=c.gc_dropout,
                                    distance=c.distance, begin_s=sorted(begins), begin_median_s=statistics.median(begins),
                                    add_median_s=statistics.median(adds), tables_median_s=statistics.median(tables)))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
