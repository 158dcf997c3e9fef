#!/usr/bin/env python3
"""Ingest benchmark: synthetic coordinate-sorted BAM -> native reader -> calculator.

Writes a BAM of N single-end reads over hg38-sized chromosomes (vectorised numpy record layout, BGZF level 1),
then reports
  * reader only: records/s and GB/s of uncompressed BAM for 1..T threads (libpymasc_io.so, no GPU involved),
  * end to end with --gpu: feed_bam into CCHipCalculator (NCC, max_shift 1000) wall-clock, split into ingest and
    device time.
pysam is not installed, so the reference's own per-read loop cannot be timed here; the comparable CPU figure is a
pure-Python loop over the decoded arrays calling feed_forward_read / feed_reverse_read per read (--pyloop), which
is what handler/calc.py:140-153 does minus pysam's own decode cost.
"""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from pymasc_amd import bam as B  # noqa: E402
from pymasc_amd.synth import HG38  # noqa: E402
from tests import io_writers as W  # noqa: E402


def synth_bam(path, n_reads, seed=1, readlen=36, chroms=None, cigar_lengths=None, index=False):
    """cigar_lengths(k): query lengths of the next k records' one M operation (default: all readlen; the record layout, sequence
    and qualities stay those of readlen bases, so the file has the same size and records either way).  index: also write
    <path>.bai (one chunk per reference and the pseudo-bin 37450, as samtools puts it)."""
    rng = np.random.default_rng(seed)
    refs = [(n, l) for n, l in HG38] if chroms is None else [(n, l) for n, l in HG38][:chroms]
    total = sum(l for _, l in refs)
    name_len = 12
    # one fixed-size record layout: 32-byte core + name + 1 CIGAR op + seq + qual
    rec_dtype = np.dtype([("block_size", "<i4"), ("ref", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"),
                          ("bin", "<u2"), ("n_cig", "<u2"), ("flag", "<u2"), ("l_seq", "<i4"), ("nref", "<i4"),
                          ("npos", "<i4"), ("tlen", "<i4"), ("name", "S%d" % name_len), ("cigar", "<u4"),
                          ("seq", "u1", ((readlen + 1) // 2,)), ("qual", "u1", (readlen,))])
    header = W.bam_header(refs)
    t0 = time.time()
    zsizes, spans, u = [], {}, len(header)      # (for the index: compressed block sizes, uncompressed [beg, end) per reference)
    with open(path, "wb") as fp, ThreadPoolExecutor(8) as pool:
        def flush(data):
            blocks = [data[i:i + 0xff00] for i in range(0, len(data), 0xff00)]
            for z in pool.map(lambda b: W.bgzf_block(b, 1), blocks):
                fp.write(z)
                zsizes.append(len(z))
        pending = header
        for rid, (_n, ln) in enumerate(refs):
            k = int(round(n_reads * ln / total))
            if k == 0:
                continue
            spans[rid] = (u, u + k * (rec_dtype.itemsize))
            u += k * rec_dtype.itemsize
            rec = np.zeros(k, dtype=rec_dtype)
            rec["block_size"] = rec_dtype.itemsize - 4
            rec["ref"] = rid
            rec["pos"] = np.sort(rng.integers(0, ln - readlen - 1, size=k))
            rec["l_name"] = name_len
            rec["mapq"] = rng.integers(0, 61, size=k)
            rec["bin"] = 4680
            rec["n_cig"] = 1
            fl = np.where(rng.random(k) < 0.5, 16, 0)
            fl = np.where(rng.random(k) < 0.03, fl | 0x400, fl)
            rec["flag"] = fl
            rec["l_seq"] = readlen
            rec["nref"] = -1
            rec["npos"] = -1
            rec["name"] = b"read0000000"
            rec["cigar"] = ((readlen if cigar_lengths is None else cigar_lengths(k)) << 4) | 0
            rec["seq"] = rng.integers(0, 256, size=(k, (readlen + 1) // 2), dtype=np.uint8)
            rec["qual"] = rng.integers(20, 41, size=(k, readlen), dtype=np.uint8)
            pending += rec.tobytes()
            cut = len(pending) - len(pending) % 0xff00
            flush(pending[:cut])
            pending = pending[cut:]
        flush(pending)
        fp.write(W.BGZF_EOF)
    if index:
        import struct
        coff = np.concatenate(([0], np.cumsum(zsizes))).tolist()

        def voff(x):      # (a position at a block end belongs to the next block)
            k, r = divmod(x, 0xff00)
            return (coff[k] << 16) | r
        out = [b"BAI\1", struct.pack("<i", len(refs))]
        for rid in range(len(refs)):
            if rid not in spans:
                out.append(struct.pack("<ii", 0, 0))
                continue
            vb, ve = voff(spans[rid][0]), voff(spans[rid][1])
            n = (spans[rid][1] - spans[rid][0]) // rec_dtype.itemsize
            out.append(struct.pack("<iIiQQ", 2, 4681, 1, vb, ve) + struct.pack("<IiQQQQ", 37450, 2, vb, ve, n, 0)
                       + struct.pack("<i", 0))
        with open(path + ".bai", "wb") as fp:
            fp.write(b"".join(out))
    return refs, time.time() - t0


def time_subsets(path, refs, mapq, reps=5):
    """Indexed device reads (DeviceBamReader(references=...): pmx_dbam_open_indexed + pmx_dbam_select) against the whole-file
    open: open + decode wall-clock and the compressed bytes read, for the whole file, the largest chromosome alone and one LPT
    share of 8 ranks.  The kept records of every case are checked against the host reader's per-chromosome counts."""
    from pymasc_amd import bam_device as D
    from pymasc_amd.sharding import lpt_assign
    names = [n for n, _ in refs]
    with B.BamReader(path, threads=16) as r:
        per = np.zeros(len(names), dtype=np.int64)
        for ref, _pos, _rl, _rev in r.batches(mapq):
            per += np.bincount(ref, minlength=len(names))
    largest = max(refs, key=lambda x: x[1])[0]
    share = [names[i] for i in sorted(lpt_assign([l for _, l in refs], 8)[0])]
    cases = [("whole_file", None), ("largest_chromosome", [largest]), ("lpt_share_of_8", share)]
    out = {}
    for label, sel in cases:
        want = int(per.sum()) if sel is None else int(sum(per[names.index(n)] for n in sel))
        runs = []
        for rep in range(reps + 1):      # (rep 0: warm-up, not in the statistics)
            t0 = time.time()
            with D.DeviceBamReader(path, references=sel) as r:
                t1 = time.time()
                kept = r.decode(mapq)
                t2 = time.time()
                c = r.counters()
            assert kept == want, (label, kept, want)
            if rep:
                runs.append((t1 - t0, t2 - t0, c["bytes_in"], c["members"]))
        tot = np.array([x[1] for x in runs])
        out[label] = {"chromosomes": len(names) if sel is None else len(sel), "kept": want, "bytes_in": runs[0][2],
                      "members": runs[0][3], "file_bytes": os.path.getsize(path),
                      "open_s": [round(x[0], 4) for x in runs], "open_decode_s": [round(x, 4) for x in tot.tolist()],
                      "open_decode_median_s": round(float(np.median(tot)), 4), "open_decode_min_s": round(float(tot.min()), 4),
                      "open_decode_max_s": round(float(tot.max()), 4)}
        print(json.dumps({label: out[label]}), flush=True)
    return out


def time_reader(path, threads, mapq):
    t0 = time.time()
    n = 0
    with B.BamReader(path, threads=threads) as r:
        for ref, _pos, _rl, _rev in r.batches(mapq):
            n += ref.size
        c = r.counters()
    dt = time.time() - t0
    return {"threads": threads, "seconds": round(dt, 3), "records_per_s": round(c["records"] / dt),
            "kept": n, "records": c["records"], "uncompressed_GBps": round(c["bytes_out"] / dt / 1e9, 3),
            "compressed_GBps": round(c["bytes_in"] / dt / 1e9, 3)}


def time_device_reader(path, mapq, check=None):
    """The device path (libpymasc_ingest.so): file -> HBM -> inflate + CRC32 -> record chain -> filtered arrays IN HBM (what a
    device-side feed consumes), and the same + the copy of the arrays to the host (what BamReader.batches hands out)."""
    from pymasc_amd import bam_device as D
    out = []
    for rep in range(3):      # the first open also page-locks the staging buffers and loads the code object
        t0 = time.time()
        with D.DeviceBamReader(path) as r:
            t1 = time.time()
            kept = r.decode(mapq)
            t2 = time.time()
            n = 0
            cs = 0
            for ref, pos, _rl, rev in r.batches(mapq):
                n += ref.size
                cs += int(pos.astype(np.int64).sum()) + int(rev.sum())
            t3 = time.time()
            c, tm = r.counters(), r.timings()
        assert n == kept
        if check is not None:
            assert (n, cs) == check, ((n, cs), check)
        out.append({"rep": rep, "open_s": round(t1 - t0, 4), "decode_s": round(t2 - t1, 4), "resident_total_s": round(t2 - t0, 4),
                    "decode_again_and_copy_to_host_s": round(t3 - t2, 4), "kept": kept, "records": c["records"], "members": c["members"],
                    "pieces_rewalked": c["rewalked"], "phases_s": {k: round(v, 4) for k, v in tm.items()},
                    "records_per_s": round(c["records"] / (t2 - t0)), "uncompressed_GBps": round(c["bytes_out"] / (t2 - t0) / 1e9, 3),
                    "compressed_GBps": round(c["bytes_in"] / (t2 - t0) / 1e9, 3)})
        print(json.dumps(out[-1]), flush=True)
    return out


def synth_sam(path, n_reads, bgzf=False, seed=1, readlen=36):
    """The synthetic file of synth_bam as SAM text (bgzf: BGZF-compressed at level 1, as `bgzip -l 1` writes it), one fixed-width
    layout per reference built with numpy (zero-padded decimals are decimals): flags 0 / 16 with 2 % duplicates, MAPQ 0..60."""
    rng = np.random.default_rng(seed)
    refs = [(n, l) for n, l in HG38]
    total = sum(l for _, l in refs)
    header = ("@HD\tVN:1.0\tSO:coordinate\n" + "".join("@SQ\tSN:{}\tLN:{}\n".format(n, l) for n, l in refs)).encode()
    t0 = time.time()

    def digits(v, w):
        return (np.asarray(v, dtype=np.int64)[:, None] // (10 ** np.arange(w - 1, -1, -1, dtype=np.int64)) % 10 + 48).astype(np.uint8)

    with open(path, "wb") as fp, ThreadPoolExecutor(8) as pool:
        def flush(data, last=False):
            if not bgzf:
                fp.write(data)
                return b""
            n = len(data) if last else len(data) // 0xff00 * 0xff00
            for z in pool.map(lambda i: W.bgzf_block(data[i:i + 0xff00], 1), range(0, n, 0xff00)):
                fp.write(z)
            return data[n:]

        rest = flush(header)
        k0 = 0
        for _name, ln in refs:
            k = int(round(n_reads * ln / total))
            for a in range(0, k, 1 << 20):
                m = min(1 << 20, k - a)
                cols = [b"r", digits(np.arange(k0, k0 + m), 9), b"\t", None, b"\t" + _name.encode() + b"\t", None, b"\t", None,
                        ("\t%dM\t*\t0\t0\t" % readlen).encode() + b"A" * readlen + b"\t" + b"I" * readlen + b"\n"]
                flag = np.where(rng.random(m) < 0.5, 16, 0) | np.where(rng.random(m) < 0.02, 1024, 0)
                cols[3] = digits(flag, 4)
                cols[5] = digits(np.sort(rng.integers(1, ln - readlen, size=m)), 9)
                cols[7] = digits(rng.integers(0, 61, size=m), 2)
                parts = [np.broadcast_to(np.frombuffer(c, np.uint8), (m, len(c))) if isinstance(c, bytes) else c for c in cols]
                rest = flush(rest + np.concatenate(parts, axis=1).tobytes())
                k0 += m
        if bgzf:
            flush(rest, last=True)
            fp.write(W.BGZF_EOF)
    return refs, time.time() - t0


def time_sam(path, threads, mapq):
    """SamReader (host, threads) against DeviceSamReader (open + decode + runs, resident in HBM); the same records either way."""
    from pymasc_amd import sam as S
    out = {"sam_bytes": os.path.getsize(path), "host": [], "device": []}
    check = None
    for t in threads:
        t0 = time.time()
        with S.SamReader(path, threads=t) as r:
            t1 = time.time()
            n = cs = 0
            for _ref, pos, _rl, rev in r.batches(mapq):
                n += pos.size
                cs += int(pos.astype(np.int64).sum()) + int(rev.sum())
            c = r.counters()
        dt = time.time() - t0
        check = (n, cs)
        out["host"].append({"threads": t, "open_s": round(t1 - t0, 3), "seconds": round(dt, 3), "records": c["records"], "kept": n,
                            "text_GBps": round(c["bytes_out"] / dt / 1e9, 3)})
        print(json.dumps(out["host"][-1]), flush=True)
    for rep in range(3):      # the first open also page-locks the staging buffers and loads the code object
        t0 = time.time()
        with S.DeviceSamReader(path) as r:
            t1 = time.time()
            kept = r.decode(mapq)
            runs = r.device_runs()
            t2 = time.time()
            n = cs = 0
            for _ref, pos, _rl, rev in r.batches(mapq):
                n += pos.size
                cs += int(pos.astype(np.int64).sum()) + int(rev.sum())
            c, tm = r.counters(), r.timings()
        assert (n, cs) == check and kept == n, ((n, cs), check)
        out["device"].append({"rep": rep, "open_s": round(t1 - t0, 4), "decode_and_runs_s": round(t2 - t1, 4),
                              "resident_total_s": round(t2 - t0, 4), "runs": len(runs), "records": c["records"], "kept": kept,
                              "members": c["members"], "phases_s": {k: round(v, 4) for k, v in tm.items()},
                              "text_GBps": round(c["bytes_out"] / (t2 - t0) / 1e9, 3)})
        print(json.dumps(out["device"][-1]), flush=True)
    best_dev = min(x["resident_total_s"] for x in out["device"])
    best_host = min(x["seconds"] for x in out["host"])
    out["device_vs_host"] = {"device_resident_s": best_dev, "host_best_s": best_host, "speedup": round(best_host / best_dev, 2)}
    print(json.dumps(out["device_vs_host"]), flush=True)
    return out


def time_bigwig(path_bw, chroms_per_call=None):
    """A synthetic hg38-shaped mappability track (runs of ~500 bp every ~1250 bp, bedGraph sections of 1024 items, zlib) read
    chromosome by chromosome: the host reader (zlib on threads) against the device reader (intervals left in HBM), same intervals."""
    from pymasc_amd.bigwig import BigWigReader
    from pymasc_amd.bigwig_device import DeviceBigWigReader
    rng = np.random.default_rng(3)
    sizes = {n: l for n, l in HG38}
    tracks = {}
    t0 = time.time()
    for n, l in sizes.items():
        k = l // 1250
        starts = np.arange(k, dtype=np.int64) * 1250 + rng.integers(0, 600, k)
        ends = starts + rng.integers(200, 640, k)
        tracks[n] = list(zip(starts.tolist(), ends.tolist(), [1.0] * k))
    W.write_bigwig(path_bw, sizes, tracks, items_per_block=1024, rtree_block=256)
    out = {"intervals": sum(map(len, tracks.values())), "file_bytes": os.path.getsize(path_bw), "generate_s": round(time.time() - t0, 1)}
    del tracks
    host = []
    for _ in range(3):
        t0 = time.time()
        with BigWigReader(path_bw) as bw:
            chk = [(a.size, int(a.sum()) + int(b.sum())) for a, b, _v in (bw.fetch_arrays(1, c) for c in sizes)]
        host.append(round(time.time() - t0, 4))
    dev, dev_open = [], []
    for _ in range(3):
        t0 = time.time()
        with DeviceBigWigReader(path_bw) as bw:
            t1 = time.time()
            ns = [bw.fetch_device(1, c)[2] for c in sizes]
            dev.append(round(time.time() - t0, 4))
            dev_open.append(round(t1 - t0, 4))
    with DeviceBigWigReader(path_bw) as bw:     # parity of the whole track
        chk2 = [(a.size, int(a.sum()) + int(b.sum())) for a, b, _v in (bw.fetch_arrays(1, c) for c in sizes)]
    assert chk == chk2 and ns == [c[0] for c in chk]
    out.update({"host_reader_s": host, "device_reader_s": dev, "device_open_s": dev_open, "speedup": round(min(host) / min(dev), 2)})
    os.unlink(path_bw)
    return out


def synth_text_track(path, kind, compress, nlines, seed=7):
    """A seeded hg38-shaped text track of about `nlines` lines: alternating unmappable / mappable runs drawn from the golden
    track's run and gap lengths (pymasc_amd.synth.fixture_run_lengths), over the 24 chromosomes in proportion to their length.
    bedgraph: "chrom start end 0|1" for every run and gap; bed: the mappable runs; wig: one variableStep block per chromosome,
    a "pos 1" line per mappable run (span 36: the read length of a Umap-style k36 track)."""
    import gzip
    from pymasc_amd import synth
    runs, gaps = synth.fixture_run_lengths()
    rng = np.random.default_rng(seed)
    total = sum(l for _n, l in HG38)
    out = []
    t0 = time.time()
    for n, l in HG38:
        per = max(1, int(nlines * l / total) // (2 if kind == "bedgraph" else 1))
        r = rng.choice(runs, per)
        g = rng.choice(gaps, per)
        b = int(rng.integers(0, 10000)) + np.cumsum(g + r) - r          # starts of the mappable runs
        e = b + r
        if kind == "bedgraph":
            gb = np.concatenate(([0], e[:-1]))
            z = np.char.add(np.char.add(n + "\t", gb.astype(str)), np.char.add("\t", b.astype(str)))
            o = np.char.add(np.char.add(n + "\t", b.astype(str)), np.char.add("\t", e.astype(str)))
            lines = np.empty(2 * per, dtype=object)
            lines[0::2] = np.char.add(z, "\t0")
            lines[1::2] = np.char.add(o, "\t1")
            lines = lines[1:] if b[0] == 0 else lines
        elif kind == "bed":
            lines = np.char.add(np.char.add(n + "\t", b.astype(str)), np.char.add("\t", e.astype(str)))
        else:
            out.append("variableStep chrom={} span=36\n".format(n))
            lines = np.char.add((b + 1).astype(str), " 1")
        out.append("\n".join(lines.tolist()) + "\n")
    data = "".join(out).encode()
    if compress == "gzip":
        data = gzip.compress(data, 6)
    elif compress == "bgzf":
        data = W.bgzf_compress(data)
    with open(path, "wb") as fp:
        fp.write(data)
    return time.time() - t0


def time_text_track(path, reps=3):
    """Open + fetch of every chromosome at 1.0: the host reader against the device reader (intervals left in HBM)."""
    from pymasc_amd.text_track import DeviceTextTrackReader, TextTrackReader
    host = []
    for _ in range(reps):
        t0 = time.time()
        with TextTrackReader(path) as r:
            chk = [(a.size, int(a.sum()) + int(b.sum())) for a, b, _v in (r.fetch_arrays(1, c) for c in r.chromsizes)]
            names = list(r.chromsizes)
        host.append(round(time.time() - t0, 4))
    dev, dev_open = [], []
    for _ in range(reps):
        t0 = time.time()
        with DeviceTextTrackReader(path) as r:
            t1 = time.time()
            ns = [r.fetch_device(1, c)[2] for c in names]
            dev.append(round(time.time() - t0, 4))
            dev_open.append(round(t1 - t0, 4))
    with DeviceTextTrackReader(path) as r:      # parity of the whole track
        chk2 = [(a.size, int(a.sum()) + int(b.sum())) for a, b, _v in (r.fetch_arrays(1, c) for c in names)]
    assert chk == chk2 and ns == [c[0] for c in chk]
    return {"intervals_at_1": sum(c[0] for c in chk), "host_reader_s": host, "device_reader_s": dev, "device_open_s": dev_open,
            "speedup": round(min(host) / min(dev), 2)}


def synth_bigbed(path, nrec, seed=13):
    """A seeded hg38-shaped bigBed of about `nrec` BED6 records over the 24 chromosomes (in proportion to their length), with
    Umap-like rests (a name, a score, a strand: 20-30 bytes a record) in zlib blocks of 512 items (tests/bigbed_writers.py)."""
    from tests import bigbed_writers as BB
    t0 = time.time()
    total = sum(l for _n, l in HG38)
    recs = {}
    for i, (n, l) in enumerate(HG38):
        per = max(1, int(nrec * l / total))
        recs[n] = BB.random_records(seed + i, per, [n])[n]
    sizes = {n: max(l, int(recs[n][1][-1]) + 1) for n, l in HG38}
    BB.write_bigbed(path, sizes, recs, items_per_block=512, rtree_block=256)
    return sum(len(v[0]) for v in recs.values()), time.time() - t0


def time_bigbed(path, reps=3):
    """Open + fetch of every chromosome at 1.0: the host reader (zlib on threads) against the device reader (k_bb_records,
    intervals left in HBM); the device arrays are compared with the host's, element for element."""
    from pymasc_amd.bigwig import BigWigReader
    from pymasc_amd.bigwig_device import DeviceBigWigReader
    host = []
    for _ in range(reps):
        t0 = time.time()
        with BigWigReader(path) as r:
            assert r.kind == "bigbed"
            arrays = {c: r.fetch_arrays(1, c) for c in r.chromsizes}
        host.append(round(time.time() - t0, 4))
    dev, dev_open = [], []
    for _ in range(reps):
        t0 = time.time()
        with DeviceBigWigReader(path) as r:
            t1 = time.time()
            ns = [r.fetch_device(1, c)[2] for c in arrays]
            dev.append(round(time.time() - t0, 4))
            dev_open.append(round(t1 - t0, 4))
    with DeviceBigWigReader(path) as r:         # parity of the whole track
        for c, want in arrays.items():
            for x, y in zip(r.fetch_arrays(1, c), want):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), c
    assert ns == [a[0].size for a in arrays.values()]
    return {"intervals_at_1": sum(ns), "host_reader_s": host, "device_reader_s": dev, "device_open_s": dev_open,
            "speedup": round(min(host) / min(dev), 2)}


BED_FILES = [(order, comp) for order in ("sorted", "shuffled") for comp in ("none", "gzip", "bgzf")]


def bed_file_name(directory, order, comp):
    return os.path.join(directory, "reads.{}.tagAlign{}".format(order, {"none": "", "gzip": ".gz", "bgzf": ".bgz"}[comp]))


def synth_bed_reads(directory, nlines, seed=11):
    """A seeded tagAlign file of `nlines` 36-bp reads over the hg38 chromosomes in proportion to their length (ENCODE's layout:
    "chrom start end N 1000 strand"), sorted and `shuf`-shuffled, each plain, gzip and BGZF: the six files of BED_FILES (made
    once, reused when present).  Returns (sizes, seconds)."""
    import gzip
    t0 = time.time()
    if all(os.path.exists(bed_file_name(directory, o, c)) for o, c in BED_FILES):
        return HG38, 0.0
    os.makedirs(directory, exist_ok=True)
    rng = np.random.default_rng(seed)
    total = sum(l for _n, l in HG38)
    lines = []
    for n, l in HG38:
        per = max(1, int(nlines * l / total))
        b = np.sort(rng.integers(0, l - 36, per))
        strand = np.where(rng.integers(0, 2, per) == 1, "\tN\t1000\t-", "\tN\t1000\t+")
        lines.append(np.char.add(np.char.add(np.char.add(n + "\t", b.astype(str)), np.char.add("\t", (b + 36).astype(str))), strand))
    lines = np.concatenate(lines)
    for order in ("sorted", "shuffled"):
        if order == "shuffled":
            lines = lines[rng.permutation(lines.size)]
        data = ("\n".join(lines.tolist()) + "\n").encode()
        for comp in ("none", "gzip", "bgzf"):
            out = data if comp == "none" else gzip.compress(data, 1) if comp == "gzip" else W.bgzf_compress(data, level=1)
            with open(bed_file_name(directory, order, comp), "wb") as fp:
                fp.write(out)
    return HG38, time.time() - t0


def time_bed_reads(path, sizes, mapq, reps=3, host=True):
    """Open + decode at `mapq`: BedReadsReader on 16 threads against DeviceBedReadsReader (records left in HBM), best of `reps`
    (the file is in the page cache after the first read); the same records from both."""
    from pymasc_amd.bed_reads import BedReadsReader, DeviceBedReadsReader
    names, lens = [n for n, _ in sizes], [l for _, l in sizes]
    out = {}
    if host:
        hs = []
        for _ in range(reps):
            t0 = time.time()
            with BedReadsReader(path, names, lens, threads=16) as r:
                kept = r.decode(mapq)
                ref, pos, _rl, rev = r._fetch(0, kept)
            hs.append(round(time.time() - t0, 4))
        out["host_reader_s"] = hs
    ds, phases = [], None
    for _ in range(reps):
        t0 = time.time()
        with DeviceBedReadsReader(path, names, lens) as r:
            dk = r.decode(mapq)
            ds.append(round(time.time() - t0, 4))
            phases = r.timings()
            if host and _ == 0:
                dref, dpos, _drl, drev = r._fetch(0, dk)
                assert dk == kept and (dref == ref).all() and (dpos == pos).all() and (drev == rev).all()
    out.update({"kept": dk, "device_reader_s": ds, "device_phases_s": phases})
    if host:
        out["speedup"] = round(min(out["host_reader_s"]) / min(ds), 2)
    return out


def time_region_mask(path, refs, mapq, nmask, reps, seed=17):
    """Open + decode + feed of the device reader with and without a mask of ``nmask`` random regions of 0.5-20 kb laid over the
    references in proportion to their length: seconds of every repetition, the medians, the reads dropped."""
    from pymasc_amd import bam_device as D
    from pymasc_amd import region_mask
    from pymasc_amd.calculator import CCHipCalculator
    rng = np.random.default_rng(seed)
    total = sum(l for _n, l in refs)
    lines = {}
    for name, length in refs:
        k = max(1, round(nmask * length / total))
        b = rng.integers(0, max(length - 20000, 1), k)
        lines[name] = list(zip(b.tolist(), (b + rng.integers(500, 20000, k)).tolist()))
    mask = region_mask.open_mask(lines)
    out = {"regions": sum(len(v) for v in lines.values()), "unmasked_s": [], "masked_s": []}
    for rep in range(reps + 1):             # (the first pair warms up: pinned staging buffers, code objects)
        for key in ("unmasked_s", "masked_s"):
            calc = CCHipCalculator(1000, 36, [n for n, _ in refs], [l for _, l in refs])
            t0 = time.time()
            with D.DeviceBamReader(path) as r:
                if key == "masked_s":
                    r.set_exclude(mask.resolve(r.references, r.lengths))
                fed = r.feed(calc, mapq)
                dropped = r.excluded()
            dt = time.time() - t0
            calc.close()
            if rep:
                out[key].append(round(dt, 4))
                out["fed_" + key[:-2]] = fed
                out["dropped_" + key[:-2]] = dropped
    out["unmasked_median_s"] = float(np.median(out["unmasked_s"]))
    out["masked_median_s"] = float(np.median(out["masked_s"]))
    out["masked_over_unmasked"] = round(out["masked_median_s"] / out["unmasked_median_s"], 4)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--path", default="/tmp/pymasc_ingest_bench.bam")
    ap.add_argument("--mapq", type=int, default=10)
    ap.add_argument("--threads", type=int, nargs="*", default=[1, 2, 4, 8, 16])
    ap.add_argument("--chroms", type=int, default=None)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--device", action="store_true", help="time the device-side reader (BGZF inflate + decode as HIP kernels)")
    ap.add_argument("--bigwig", action="store_true", help="also time the mappability track: host reader against device reader")
    ap.add_argument("--pyloop", type=int, default=0, help="time a per-read Python feeding loop over this many reads")
    ap.add_argument("--subsets", action="store_true", help="write a .bai and time indexed device reads of chromosome subsets")
    ap.add_argument("--sam", choices=["plain", "bgzf"], default=None,
                    help="write the synthetic reads as SAM text (plain or BGZF) and time SamReader against DeviceSamReader")
    ap.add_argument("--track-text", choices=["bedgraph", "bed", "wig"], default=None,
                    help="write a seeded hg38-shaped text track and time TextTrackReader against DeviceTextTrackReader")
    ap.add_argument("--compress", choices=["none", "bgzf", "gzip"], default="none", help="compression of the --track-text file")
    ap.add_argument("--lines", type=int, default=20_000_000, help="about how many lines the --track-text file has")
    ap.add_argument("--bed", action="store_true",
                    help="write a seeded tagAlign file of --lines reads, sorted and shuffled, plain / gzip / BGZF, and time "
                         "BedReadsReader (16 threads) against DeviceBedReadsReader")
    ap.add_argument("--bed-dir", default="/tmp/pymasc_bed_bench", help="where the --bed files are made (and kept)")
    ap.add_argument("--bed-only", default=None, help="--bed: time only ORDER-COMP (e.g. shuffled-none), on the device only")
    ap.add_argument("--bigbed", action="store_true",
                    help="time a bigBed track of about --lines BED6 records: host reader against device reader (DESIGN.md 7.12)")
    ap.add_argument("--mask", type=int, default=0, metavar="N",
                    help="time open + decode + feed of the device reader with and without N random excluded regions "
                         "(--exclude-regions, DESIGN.md 7.15), --reps times each on the same file, and nothing else")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    if a.bed:
        sizes, gen_s = synth_bed_reads(a.bed_dir, a.lines)
        res = {"lines": a.lines, "generate_s": round(gen_s, 1), "mapq": a.mapq, "files": []}
        for order, comp in BED_FILES:
            if a.bed_only and a.bed_only != "{}-{}".format(order, comp):
                continue
            path = bed_file_name(a.bed_dir, order, comp)
            r = {"order": order, "compress": comp, "file_bytes": os.path.getsize(path)}
            r.update(time_bed_reads(path, sizes, a.mapq, a.reps, host=a.bed_only is None))
            res["files"].append(r)
            print(json.dumps(r), flush=True)
        if a.out:
            with open(a.out, "w") as fp:
                json.dump(res, fp, indent=1)
        return

    if a.bigbed:
        path = a.path + ".bb"
        nrec, gen_s = synth_bigbed(path, a.lines)
        res = {"kind": "bigbed", "records": nrec, "items_per_block": 512, "file_bytes": os.path.getsize(path),
               "generate_s": round(gen_s, 1)}
        try:
            res.update(time_bigbed(path, a.reps))
        finally:
            os.unlink(path)
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as fp:
                json.dump(res, fp, indent=1)
        return

    if a.track_text:
        path = a.path + "." + a.track_text + {"none": "", "bgzf": ".gz", "gzip": ".gz"}[a.compress]
        gen_s = synth_text_track(path, a.track_text, a.compress, a.lines)
        res = {"kind": a.track_text, "compress": a.compress, "file_bytes": os.path.getsize(path), "generate_s": round(gen_s, 1)}
        if a.compress == "none":
            res["lines"] = sum(1 for _ in open(path, "rb"))
        try:
            res.update(time_text_track(path))
        finally:
            os.unlink(path)
        print(json.dumps(res), flush=True)
        if a.out:
            with open(a.out, "w") as fp:
                json.dump(res, fp, indent=1)
        return

    if a.sam:
        path = a.path + (".sam" if a.sam == "plain" else ".sam.gz")
        _refs, gen_s = synth_sam(path, a.reads, bgzf=(a.sam == "bgzf"))
        res = {"reads": a.reads, "format": a.sam, "generate_s": round(gen_s, 1)}
        try:
            res.update(time_sam(path, [t for t in a.threads if t <= (os.cpu_count() or 1)], a.mapq))
        finally:
            os.unlink(path)
        if a.out:
            with open(a.out, "w") as fp:
                json.dump(res, fp, indent=1)
        return

    refs, gen_s = synth_bam(a.path, a.reads, chroms=a.chroms, index=a.subsets)
    res = {"reads": a.reads, "bam_bytes": os.path.getsize(a.path), "generate_s": round(gen_s, 1), "reader": []}
    if a.mask:
        res["region_mask"] = time_region_mask(a.path, refs, a.mapq, a.mask, a.reps)
        if a.out:
            with open(a.out, "w") as fp:
                json.dump(res, fp, indent=1)
        os.unlink(a.path)
        return
    for t in a.threads:
        if t <= (os.cpu_count() or 1):
            res["reader"].append(time_reader(a.path, t, a.mapq))
            print(json.dumps(res["reader"][-1]), flush=True)

    if a.device:
        with B.BamReader(a.path, threads=16) as r:       # the checker: same records, same fields
            n = cs = 0
            for ref, pos, _rl, rev in r.batches(a.mapq):
                n += ref.size
                cs += int(pos.astype(np.int64).sum()) + int(rev.sum())
        res["device_reader"] = time_device_reader(a.path, a.mapq, check=(n, cs))
        best = min(x["resident_total_s"] for x in res["device_reader"])
        host = min(x["seconds"] for x in res["reader"]) if res["reader"] else None
        res["device_vs_host_reader"] = {"device_resident_s": best, "host_best_s": host, "speedup": round(host / best, 2) if host else None}
        print(json.dumps(res["device_vs_host_reader"]), flush=True)

    if a.pyloop:
        from tests.fake_context import FakeContext     # host-only stand-in: the loop never reaches a flush here
        from pymasc_amd.calculator import CCHipCalculator
        with B.BamReader(a.path) as r:
            ref, pos, rl, rev = next(r.batches(a.mapq, batch=a.pyloop))
        calc = CCHipCalculator(1000, 36, [n for n, _ in refs], [l for _, l in refs], context=FakeContext())
        same = ref == ref[0]
        pos, rl, rev = pos[same].tolist(), rl[same].tolist(), rev[same].tolist()
        name = refs[int(ref[0])][0]
        t0 = time.time()
        for p, l, v in zip(pos, rl, rev):
            if v:
                calc.feed_reverse_read(name, p, l)
            else:
                calc.feed_forward_read(name, p, l)
        dt = time.time() - t0
        res["python_per_read_loop"] = {"reads": len(pos), "reads_per_s": round(len(pos) / dt)}
        print(json.dumps(res["python_per_read_loop"]), flush=True)

    if a.gpu:
        from pymasc_amd.calculator import CCHipCalculator
        calc = CCHipCalculator(1000, 36, [n for n, _ in refs], [l for _, l in refs])
        t0 = time.time()
        with B.BamReader(a.path) as r:
            fed = B.feed_bam(calc, r, a.mapq)
        dt = time.time() - t0
        whole = calc.get_whole_result()
        res["end_to_end"] = {"seconds": round(dt, 3), "reads_fed": fed, "reads_per_s": round(fed / dt),
                             "forward_sum": int(whole.forward_sum), "reverse_sum": int(whole.reverse_sum)}
        calc.close()
        print(json.dumps(res["end_to_end"]), flush=True)
        if a.device:      # the same file, inflated + decoded + filtered on the GPU, records handed to the feeders in HBM
            from pymasc_amd import bam_device as D
            res["end_to_end_device"] = []
            for rep in range(3):
                calc = CCHipCalculator(1000, 36, [n for n, _ in refs], [l for _, l in refs])
                t0 = time.time()
                with D.DeviceBamReader(a.path) as r:
                    fed2 = r.feed(calc, a.mapq)
                dt2 = time.time() - t0
                w2 = calc.get_whole_result()
                assert (fed2, int(w2.forward_sum), int(w2.reverse_sum)) == (fed, int(whole.forward_sum), int(whole.reverse_sum))
                calc.close()
                res["end_to_end_device"].append({"seconds": round(dt2, 3), "reads_fed": fed2, "reads_per_s": round(fed2 / dt2)})
                print(json.dumps(res["end_to_end_device"][-1]), flush=True)
    if a.subsets:
        res["subsets"] = time_subsets(a.path, refs, a.mapq)
    if a.bigwig:
        res["bigwig"] = time_bigwig(a.path + ".bw")
        print(json.dumps(res["bigwig"]), flush=True)
    if a.out:
        with open(a.out, "w") as fp:
            json.dump(res, fp, indent=1)
    os.unlink(a.path)
    if a.subsets:
        os.unlink(a.path + ".bai")


if __name__ == "__main__":
    main()
