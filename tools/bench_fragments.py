"""Times the pair counts behind --fragments and --coverage-extend pair (pmx_dbam_fragments_add, pmx_dbam_coverage_add_fragments)
against the side counts that walk the same chain on the same handle (pmx_dbam_bincount_add, pmx_dbam_coverage_add), on a synthetic
coordinate-sorted paired-end file: python tools/bench_fragments.py --out profiles/fragments.json

The file is opened once.  The times are wall-clock around the library calls (allocations and the result copies included), --reps
samples each after one warm-up call, all in this process.  The yardstick of fragments_add is bincount_add: when its median exceeds
that one's by more than the spread between bincount_add's own fastest and slowest sample, the JSON says so and gives the split of
pmx_dbam_fragments_timings (the row filter by the wall clock, k_fr_hist by HIP events)."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import coverage, fingerprint, fragments  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE  # noqa: E402
from pymasc_amd.synth import HG38  # noqa: E402
from tests import io_writers as W  # noqa: E402


def synth_paired_bam(path, n_records, seed=1, readlen=36, chroms=4):
    """A coordinate-sorted file of ``n_records`` read1 records on the first ``chroms`` chromosomes of hg38, each with its mate
    fields: 92 % FR at a size of about N(200, 40), 3 % RF, 2 % TANDEM, 2 % with the mate elsewhere and 1 % of 3 to 60 kb."""
    rng = np.random.default_rng(seed)
    refs = [(n, l) for n, l in HG38][:chroms]
    total = sum(l for _, l in refs)
    name_len = 12
    rec_dtype = np.dtype([("block_size", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"),
                          ("bin", "<u2"), ("n_cig", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"),
                          ("npos", "<i4"), ("tlen", "<i4"), ("name", "S%d" % name_len), ("cigar", "<u4"),
                          ("seq", "u1", ((readlen + 1) // 2,)), ("qual", "u1", (readlen,))])
    with open(path, "wb") as fp, ThreadPoolExecutor(8) as pool:
        def flush(data):
            blocks = [data[i:i + 0xff00] for i in range(0, len(data), 0xff00)]
            for z in pool.map(lambda b: W.bgzf_block(b, 1), blocks):
                fp.write(z)
        pending = W.bam_header(refs)
        for rid, (_n, ln) in enumerate(refs):
            mine = int(round(n_records * ln / total))
            for done in range(0, mine, 2_000_000):      # (in slices of the chromosome's length, each sorted: memory stays bounded)
                k = min(mine - done, 2_000_000)
                lo, hi = int(ln * done / mine), int(ln * (done + k) / mine)
                rec = np.zeros(k, dtype=rec_dtype)
                size = np.maximum(rng.normal(200, 40, size=k).astype(np.int64), readlen)
                far = rng.random(k) < 0.01
                size[far] = rng.integers(3000, 60000, size=int(far.sum()))
                start = np.sort(rng.integers(lo, max(hi - 70000, lo + 1), size=k))
                is_left = rng.random(k) < 0.5
                kind = rng.random(k)
                rev = np.where(kind < 0.92, ~is_left, np.where(kind < 0.95, is_left, False))
                mate_rev = np.where(kind < 0.95, ~rev, rev)
                rec["block_size"] = rec_dtype.itemsize - 4
                rec["ref"] = rid
                rec["pos"] = np.where(is_left, start, start + size - readlen)
                rec["l_name"] = name_len
                rec["mapq"] = rng.integers(0, 61, size=k)
                rec["bin"] = 4680
                rec["n_cig"] = 1
                rec["flag"] = 0x41 | np.where(rev, 0x10, 0) | np.where(mate_rev, 0x20, 0) | np.where(rng.random(k) < 0.03, 0x400, 0)
                rec["l_seq"] = readlen
                rec["nref"] = np.where(kind < 0.98, rid, (rid + 1) % len(refs))
                rec["npos"] = np.where(is_left, start + size - readlen, start)
                rec["tlen"] = np.where(is_left, size, -size)
                rec["name"] = b"pair0000000"
                rec["cigar"] = (readlen << 4) | 0
                rec["seq"] = rng.integers(0, 256, size=(k, (readlen + 1) // 2), dtype=np.uint8)
                rec["qual"] = rng.integers(20, 41, size=(k, readlen), dtype=np.uint8)
                order = np.argsort(rec["pos"], kind="stable")
                pending += rec[order].tobytes()
                cut = len(pending) - len(pending) % 0xff00
                flush(pending[:cut])
                pending = pending[cut:]
        flush(pending)
        fp.write(W.BGZF_EOF)
    return refs


def timed(call, reps):
    call()                                  # warm-up
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        out.append(time.perf_counter() - t0)
    return dict(median_s=statistics.median(out), samples_s=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_fragments_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    t0 = time.perf_counter()
    if not os.path.exists(a.path):
        synth_paired_bam(a.path, a.records)
    res = dict(records=a.records, mapq=a.mapq, file_bytes=os.path.getsize(a.path), write_s=time.perf_counter() - t0, reps=a.reps)
    t0 = time.perf_counter()
    with DeviceBamReader(a.path) as r:
        res["open_s"] = time.perf_counter() - t0
        res["kept"] = r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["library_version"] = int(r._L.pmx_dbam_version())
        fp = fingerprint.DeviceCount(r, a.mapq, None, 500, 0)
        res["bincount_add"] = timed(lambda: fp.add(r), a.reps)
        for max_size in (2000, 65536):
            fr = fragments.DeviceCount(r, a.mapq, None, max_size)
            key = "fragments_add_{}".format(max_size)
            res[key] = timed(lambda: fr.add(r), a.reps)
            sec = (ctypes.c_double * 2)()
            r._L.pmx_dbam_fragments_timings(r._h, sec)
            c = fr.result(r)
            res[key].update(rows=c.counters["rows"] // (a.reps + 1), over=sum(c.over) // (a.reps + 1),
                            row_filter_s=sec[0] / (a.reps + 1), k_fr_hist_s=sec[1] / (a.reps + 1))
            if max_size == 2000:
                st = c.stats(fragments.FR)
                res["fr"] = {k: st[k] for k in ("n", "mean", "sd", "median", "mad", "mode")}
        cv = coverage.DeviceCount(r, a.mapq, None, 200)
        res["coverage_add_200"] = timed(lambda: cv.add(r), a.reps)
        pair = coverage.DeviceCount(r, a.mapq, None, "pair", 2000)
        res["coverage_add_fragments"] = timed(lambda: pair.add(r), a.reps)
    b = res["bincount_add"]
    spread = max(b["samples_s"]) - min(b["samples_s"])
    res["yardstick"] = dict(bincount_add_median_s=b["median_s"], bincount_add_spread_s=spread)
    for max_size in (2000, 65536):
        f = res["fragments_add_{}".format(max_size)]
        res["yardstick"]["fragments_add_{}_above".format(max_size)] = bool(f["median_s"] - b["median_s"] > spread)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
