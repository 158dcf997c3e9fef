"""Times the fragment pileup behind --coverage (pmx_dbam_coverage_begin + add + finish + the whole text pull) on the synthetic file of
tools/bench_ingest.py, beside reading that file (open + decode on the device) in the same process and beside coverage.count_host on
the same reads: python tools/bench_coverage.py --reads 20000000 --out profiles/coverage.json

The times are wall-clock around the library calls (allocations, the zeroing of the table and the result copies included), medians
after one warm-up round, split per call.  --reps 1 --no-open --no-host is the run to put under `rocprofv3 --kernel-trace --stats`
for the split of the kernels; the trace is a run of its own.

--format bigwig [--compress [host|device]] also writes the bigWig file of the same runs in every round, behind the
text pull, and splits its time into the section pulls, zoom begin (the fill and the folds), the record pulls and the rest, which is
the host's assembly (R-trees, the file writes and, with --compress host, zlib); with --compress device the pulls
are the compressed ones, pmx_dbam_coverage_sections_z / _zoom_records_z.  profiles/coverage_bigwig.json is
python tools/bench_coverage.py --reads 20000000 --format bigwig --no-host --out profiles/coverage_bigwig.json

--bin N / --normalize none|cpm|rpgc: with a bin above 1 or a normalisation every round also makes the signal track
behind finish (pmx_dbam_coverage_signal, timed as "signal"), and the text pull and the bigWig file are the signal's.

--control FILE [--compare log2|ratio|subtract]: a second synthetic file (made with another seed and
--control-reads reads when it does not exist) is decoded once; every round then piles it up on its own handle behind the signal (begin
+ add + finish, timed as "control") and makes the compared track (pmx_dbam_coverage_compare, timed as "compare") in place of the
signal, so "compare" stands beside "signal" on the same pileup, and the text pull and the bigWig file are the compared track's.

--call X [--call-gap N] [--call-length N]: every round also calls the peaks of the track the text pull read
(pmx_dbam_coverage_call, timed as "call") and pulls their narrowPeak lines (timed as "call_text"), behind the text pull and outside
"whole"; the depth track is first made a signal at bin 1 and scale 1.0 (timed as "call_signal").  The totals and the longest peak, in
runs and in bases, are recorded under "call".  profiles/coverage_call.json is
python tools/bench_coverage.py --reads 20000000 --format bigwig --bin 50 --normalize cpm --control /tmp/pymasc_coverage_control.bam \
    --control-reads 10000000 --call 1 --no-host --no-open --reps 3 --out profiles/coverage_call.json

--poisson [--lambda S L] (needs --control): every round also makes the p-score track behind the compared one on the
same two pileups (pmx_dbam_coverage_poisson, timed as "poisson", so it stands beside "compare"), and the text pull, the peaks and the
bigWig file are the p-score track's.  Recorded under "poisson": its totals, the bytes the call holds per bin (24 per bin, 12 per 256
bins, 8 per entry of F, 20 per boundary, 16 per run), and -- from the two pileups pulled to the host once, outside the timing -- the
longest series of a run.  profiles/coverage_poisson.json is
python tools/bench_coverage.py --reads 20000000 --format bigwig --bin 50 --control /tmp/pymasc_coverage_control.bam \
    --control-reads 10000000 --poisson --no-host --no-open --reps 3 --out profiles/coverage_poisson.json

--qvalue [--call-q X] (needs --poisson): every round also builds the q-score table of the p-score track behind the text
pull (pmx_dbam_coverage_qvalue, timed as "qvalue"), takes pcut(X) on the device (timed as "qvalue_cutoff"; X defaults to 2, q <= 0.01)
and calls the peaks at it (at --call's cutoff when that is given), so "qvalue" stands beside "poisson" and "call" of the same run, and
the narrowPeak lines carry column 9.  Recorded under "qvalue": the four totals, the runs, pcut, the 8-bit digits in which the keys
differ (the radix passes that ran) and the bytes the call holds (40 per run, 3072 per 8192 runs, 64, 32 per row, the table's 16 per
row among them).  profiles/coverage_qvalue.json is
python tools/bench_coverage.py --reads 20000000 --format bigwig --bin 50 --control /tmp/pymasc_coverage_control.bam \
    --control-reads 10000000 --poisson --qvalue --no-host --no-open --reps 3 --out profiles/coverage_qvalue.json"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pymasc_amd import coverage  # noqa: E402
from pymasc_amd.bam_device import DeviceBamReader  # noqa: E402
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE  # noqa: E402
from tools.bench_ingest import synth_bam  # noqa: E402


class _Timed:
    """A source of coverage.assemble_bigwig that adds up the time spent in each of its three kinds of calls."""

    def __init__(self, src):
        self.src, self.refs, self.totals, self.bin = src, src.refs, src.totals, getattr(src, "bin", None)
        self.t = dict(sections=0.0, zoom_begin=0.0, zoom_records=0.0)
        self.pulled = dict(sections=0, zoom_records=0)      # bytes copied from the device
        self.raw = dict(sections=0, zoom_records=0)         # raw bytes of the sections they hold

    def section_chunks(self, k, chrom_id, items, z=False):
        it = iter((self.src.section_chunks_z if z else self.src.section_chunks)(k, chrom_id, items))
        while True:
            t0 = time.perf_counter()
            got = next(it, None)
            self.t["sections"] += time.perf_counter() - t0
            if got is None:
                return
            self.pulled["sections"] += len(got[0]) + sum(x.nbytes for x in got[1:])
            self.raw["sections"] += int(got[1][:, 4].sum(dtype="int64"))
            yield got

    def zoom_begin(self, z0, levels, ids):
        t0 = time.perf_counter()
        out = self.src.zoom_begin(z0, levels, ids)
        self.t["zoom_begin"] += time.perf_counter() - t0
        self.z0, self.levels = z0, levels
        return out

    def zoom_records(self, level, items, z=False):
        t0 = time.perf_counter()
        out = (self.src.zoom_records_z if z else self.src.zoom_records)(level, items)
        self.t["zoom_records"] += time.perf_counter() - t0
        self.pulled["zoom_records"] += len(out[0]) + sum(x.nbytes for x in out[1:])
        self.raw["zoom_records"] += int(out[1][:, 4].sum(dtype="int64"))
        return out

    def section_chunks_z(self, k, chrom_id, items):
        return self.section_chunks(k, chrom_id, items, True)

    def zoom_records_z(self, level, items):
        return self.zoom_records(level, items, True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_complexity_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--extend", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-open", action="store_true", help="skip the timing of open + decode")
    ap.add_argument("--no-host", action="store_true", help="skip coverage.count_host on the same reads")
    ap.add_argument("--format", choices=coverage.FORMATS, default="bedgraph", help="bigwig: also time the bigWig file of the same runs")
    ap.add_argument("--compress", nargs="?", const="host", default=None, choices=("host", "device"),
                    help="the sections of the bigWig file compressed: host (the bare flag): zlib on the host; device: on the GPU")
    ap.add_argument("--bin", type=int, default=1, help="the signal track's bin (1 .. 65536)")
    ap.add_argument("--normalize", choices=coverage.NORMALIZE, default="none", help="the signal track's normalisation")
    ap.add_argument("--control", default=None, help="a control file: every round also makes the treatment against it")
    ap.add_argument("--control-reads", type=int, default=None, help="the reads of a control made here (default: half of --reads)")
    ap.add_argument("--compare", choices=coverage.COMPARE, default="log2", help="the operation with --control")
    ap.add_argument("--poisson", action="store_true", help="with --control: every round also makes the p-score track, behind the compared one")
    ap.add_argument("--lambda", dest="windows", type=int, nargs=2, default=list(coverage.LAMBDA_WINDOWS), help="the two windows of --poisson")
    ap.add_argument("--qvalue", action="store_true", help="with --poisson: every round also builds the q-score table and calls the peaks with it")
    ap.add_argument("--call-q", type=float, default=2.0, help="with --qvalue and no --call: the peaks are called at pcut(X)")
    ap.add_argument("--call", type=float, default=None, help="a cutoff: every round also calls the peaks of the track and pulls their lines")
    ap.add_argument("--call-gap", type=int, default=coverage.CALL_GAP, help="the largest gap inside a peak")
    ap.add_argument("--call-length", type=int, default=coverage.CALL_LENGTH, help="the smallest peak")
    ap.add_argument("--bigwig-path", default="/tmp/pymasc_coverage_bench.bw")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.poisson and (a.control is None or a.normalize != "none"):
        ap.error("--poisson needs --control and --normalize none")
    if a.qvalue and not a.poisson:
        ap.error("--qvalue needs --poisson")
    if not os.path.exists(a.path):
        synth_bam(a.path, a.reads)
    if a.control is not None and not os.path.exists(a.control):
        synth_bam(a.control, a.control_reads or a.reads // 2, seed=2)
    opens = []
    for _ in range(0 if a.no_open else 3):
        t0 = time.perf_counter()
        with DeviceBamReader(a.path) as r:
            r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
            opens.append(time.perf_counter() - t0)
    res = dict(file_reads=a.reads, mapq=a.mapq, extend=a.extend, file_to_records_s=sorted(opens))
    signal = a.bin != 1 or a.normalize != "none" or a.control is not None
    with contextlib.ExitStack() as stack:
        r = stack.enter_context(DeviceBamReader(a.path))
        rc = None if a.control is None else stack.enter_context(DeviceBamReader(a.control))
        if rc is not None:
            res["control_kept"] = rc.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["kept"] = n = r.decode(a.mapq, PMX_BAM_DEFAULT_EXCLUDE)
        res["library_version"] = int(r._L.pmx_dbam_version())
        res["table_bytes"] = 4 * (sum(r.lengths) + len(r.lengths))
        split = dict(begin=[], add=[], finish=[], signal=[], text=[], whole=[])
        versus = dict(control=[], compare=[], poisson=[]) if a.poisson else dict(control=[], compare=[])
        called = dict(call_signal=[], call=[], call_text=[])
        qtimes = dict(qvalue=[], qvalue_cutoff=[])
        bw = dict(sections=[], zoom_begin=[], zoom_records=[], assembly=[], whole=[])
        for rep in range(a.reps + 1):               # (the first round warms up)
            t = [time.perf_counter()]
            acc = coverage.DeviceCount(r, a.mapq, None, a.extend)
            t.append(time.perf_counter())
            acc.add(r)
            t.append(time.perf_counter())
            totals = acc.finish(r)
            t.append(time.perf_counter())
            if signal:
                scale = coverage.scale_of(a.normalize, totals["reads"], totals["fragment_bases"], [l for _n, l in acc.refs])
                res["signal"] = dict(acc.signal(r, a.bin, scale, a.normalize), bin=a.bin, normalize=a.normalize, scale=scale)
            t.append(time.perf_counter())
            if rc is not None:                      # the control's pileup on its own handle, then the compared track in the signal's place
                cacc = coverage.DeviceCount(rc, a.mapq, None, a.extend)
                cacc.add(rc)
                ctotals = cacc.finish(rc)
                t1 = time.perf_counter()
                a_t, a_c = coverage.factors_of(a.normalize, totals, ctotals, [l for _n, l in acc.refs])
                res["compare"] = dict(acc.compare(r, cacc, rc, a.bin, a.compare, a_t, a_c, 1.0, a.normalize, a.control), bin=a.bin, op=a.compare,
                                      normalize=a.normalize, a_t=a_t, a_c=a_c, control_totals=ctotals)
                t2 = time.perf_counter()
                if a.poisson:                       # on the same two pileups, in the compared track's place
                    res["poisson"] = dict(acc.poisson(r, cacc, rc, a.bin, a_c, *a.windows, a.control), bin=a.bin, a_c=a_c, windows=a.windows)
                t3 = time.perf_counter()
                if rep:
                    versus["control"].append(t1 - t[4])
                    versus["compare"].append(t2 - t1)
                    if a.poisson:
                        versus["poisson"].append(t3 - t2)
            size = sum(len(chunk) for chunk in acc.text_chunks(r, signal=signal))
            t.append(time.perf_counter())
            cutoff = a.call
            if a.qvalue:                            # the table of the p-score track, and the cutoff from it
                tq = [time.perf_counter()]
                qtot = acc.qvalue(r)
                tq.append(time.perf_counter())
                pcut = acc.qvalue_cutoff(r, a.call_q)
                tq.append(time.perf_counter())
                cutoff = pcut if a.call is None else a.call
                if rep:
                    qtimes["qvalue"].append(tq[1] - tq[0])
                    qtimes["qvalue_cutoff"].append(tq[2] - tq[1])
                res["qvalue"] = dict(qtot, call_q=a.call_q, pcut=pcut, cutoff=cutoff, runs=acc.sig["totals"]["runs"])
            if cutoff is not None:                  # the peaks of the track the text pull read, and their lines
                tc = [time.perf_counter()]
                if acc.sig is None:
                    acc.signal(r, 1, 1.0)
                tc.append(time.perf_counter())
                ctotals = acc.call(r, cutoff, a.call_gap, a.call_length)
                tc.append(time.perf_counter())
                csize = sum(len(chunk) for chunk in acc.call_text_chunks(r))
                tc.append(time.perf_counter())
                if rep:
                    for k, name in enumerate(called):
                        called[name].append(tc[k + 1] - tc[k])
                rows = acc.call_rows(r)
                res["call"] = dict(ctotals, cutoff=cutoff, max_gap=a.call_gap, min_length=a.call_length, text_bytes=csize,
                                   signal_runs=acc.sig["totals"]["runs"], longest_peak_runs=int(rows[5].max()) if rows[5].size else 0,
                                   longest_peak_bases=int((rows[2] - rows[1]).max()) if rows[5].size else 0)
            if a.format == "bigwig":
                src = _Timed(coverage.bigwig_source(acc, r, signal))
                t0 = time.perf_counter()
                with open(a.bigwig_path, "w+b") as fp:
                    coverage.assemble_bigwig(fp, src, {None: False, "host": True, "device": "device"}[a.compress])
                whole = time.perf_counter() - t0
                if rep:
                    for name in ("sections", "zoom_begin", "zoom_records"):
                        bw[name].append(src.t[name])
                    bw["assembly"].append(whole - sum(src.t.values()))
                    bw["whole"].append(whole)
                    res["bigwig"] = dict(bytes=os.path.getsize(a.bigwig_path), compress=a.compress, z0=src.z0, levels=src.levels,
                                         section_bytes_pulled=src.pulled["sections"], record_bytes_pulled=src.pulled["zoom_records"],
                                         section_bytes_raw=src.raw["sections"], record_bytes_raw=src.raw["zoom_records"])
            if rep:
                for k, name in enumerate(("begin", "add", "finish", "signal", "text")):
                    split[name].append(t[k + 1] - t[k])
                split["whole"].append(t[5] - t[0])
                if rc is not None:                  # (the text pull begins behind compare)
                    split["text"][-1] -= sum(v[-1] for v in versus.values())
        if rc is not None:
            split.update(versus)
        if a.call is not None or a.qvalue:
            split.update(called)
        if a.qvalue:
            split.update(qtimes)
            n_runs, m = res["qvalue"]["runs"], res["qvalue"]["rows"]
            keys = ~acc.qvalue_rows(r)[0].view("uint32")            # (the distinct values' keys differ where the runs' do)
            differ = int(np.bitwise_or.reduce(keys) ^ np.bitwise_and.reduce(keys)) if m else 0
            held = 40 * n_runs + 3072 * (-(-n_runs // 8192)) + 64 + 32 * m if n_runs else 0
            res["qvalue"].update(radix_passes=[d for d in range(8) if (differ >> (8 * d)) & 255], held_bytes=held, table_bytes=16 * m)
        res.update(totals, text_bytes=size, text_chunk_runs=coverage.TEXT_CHUNK,
                   **{k + "_s": v for k, v in split.items()},              # (every round, in the order they ran)
                   **{k + "_median_s": statistics.median(v) for k, v in split.items()})
        if a.format == "bigwig":
            res["bigwig"].update(**{k + "_s": v for k, v in bw.items()}, **{k + "_median_s": statistics.median(v) for k, v in bw.items()})
            os.unlink(a.bigwig_path)
        if a.poisson:                               # what the call held, and the longest series: from the pileups, outside the timing
            t_host, c_host = acc.result(r), cacc.result(rc)
            nb = sum(-(-l // a.bin) for _n, l in acc.refs)
            ne = runs = longest = 0
            lengths = dict(acc.refs)
            seen = set()
            for name, s0, e0, k, lam in t_host.poisson_pairs(c_host, a.bin, res["poisson"]["a_c"], *a.windows):
                gaps = int((s0[1:] > e0[:-1]).sum()) + int(s0[0] > 0) + int(e0[-1] < lengths[name])
                ne, runs = ne + int(s0.size) + gaps, runs + int(s0.size)
                seen.add(name)
                up = k.astype("float64") > lam
                if up.any():
                    longest = max(longest, int(coverage.poisson_series(k[up], lam[up])[1].max()))
            ne += sum(1 for name, l in acc.refs if name not in seen and l > 0)
            assert runs == res["poisson"]["runs"]
            held = 24 * nb + 12 * (-(-nb // 256)) + 8 * (totals["max_depth"] + 1) + 20 * ne + 16 * runs
            res["poisson"].update(bins=nb, boundaries=ne, longest_series=longest, held_bytes=held, held_bytes_per_bin=held / nb)
        if not a.no_host:
            cols = r._fetch(0, n)
            t0 = time.perf_counter()
            c = coverage.count_host(*cols, r.references, r.lengths, [1] * len(r.references), a.extend)
            res["count_host_s"] = time.perf_counter() - t0
            t0 = time.perf_counter()
            host_size = sum(len(chunk) for chunk in c.text_chunks())
            res["host_text_s"] = time.perf_counter() - t0
            assert c.totals == tuple(totals[k] for k in coverage.TOTALS) and (signal or host_size == size)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
            fp.write("\n")


if __name__ == "__main__":
    main()
