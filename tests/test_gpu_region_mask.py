"""Excluded regions on the GPU: a masked run of the golden reads against the existing code on inputs the test
filters itself, table for table, through every reader; the device filter against the host reader and brute force; the device merge
against the host merge; pmx_bits_clear_regions_dev_ex against numpy.

The golden file holds reads on chr1 only, so the golden mask meets its conditions there (overlapping, abutting and out-of-order
lines, a line past the chromosome's end, both edge cases of the overlap rule, a name absent from the BAM); the same conditions on
several chromosomes with reads are met by the synthetic pipeline equivalence and the device-against-host case below."""
import csv
import os
import shutil
import threading

import numpy as np
import pytest
import torch

from pymasc_amd import ffi, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from tests import bed_reads_cases as BC
from tests import io_writers as W
from tests import sam_writers as SW

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STEM = "ENCFF000RMB-test"
L, SHIFT, MAPQ = 36, 300, 10


def golden_reads():
    with open(os.path.join(GOLD, STEM + ".reads.tsv"), newline="") as fh:
        return [dict(flag=int(r["flag"]), rname=r["rname"], pos=int(r["pos"]), mapq=int(r["mapq"]), qlen=int(r["qlen"]))
                for r in csv.DictReader(fh, dialect="excel-tab")]


def golden_track():
    return [(c, int(b), int(e), float(v)) for c, b, e, v in (ln.split() for ln in open(os.path.join(GOLD, "hg19_36mer-test.bedGraph")))]


def golden_mask(reads):
    """The mask's lines, chosen from the reads: (lines by chromosome, index of the read that must stay, of the one that must go)."""
    live = [i for i, r in enumerate(reads) if r["mapq"] >= MAPQ]
    stay, go = live[len(live) // 3], live[2 * len(live) // 3]
    s, g = reads[stay], reads[go]
    first, last = reads[live[0]]["pos"], reads[live[-1]]["pos"]
    span = last - first
    lines = {"chr1": [
        (s["pos"] + s["qlen"] - 1, s["pos"] + s["qlen"] + 3),       # begins exactly one base after the read's last base: not dropped
        (g["pos"] - 40, g["pos"]),                                  # ends exactly at the read's first base: dropped
        (first + span // 2, first + span // 2 + 4000),              # overlapping lines, out of order
        (first + span // 2 - 1500, first + span // 2 + 100),
        (first + span // 8, first + span // 8 + 900),               # abutting lines
        (first + span // 8 + 900, first + span // 8 + 2000),
        (249250000, 249400000),                                     # past the end of chr1 (249250621), which has the reads
    ], "chr20": [(600, 5000)],                                      # past the end of a chromosome without reads too
        "chrNotInTheBam": [(0, 1000)]}
    return lines, stay, go


def dropped_by_rule(r, lines, sizes):
    length = sizes[r["rname"]]
    last = r["pos"] + max(r["qlen"], 1) - 1
    return any(b < min(e, length) and b + 1 <= last and r["pos"] <= min(e, length) for b, e in lines.get(r["rname"], []))


@pytest.fixture(scope="module")
def golden(tmp_path_factory):
    d = tmp_path_factory.mktemp("region_mask")
    reads = golden_reads()
    sizes = dict(BC.golden_sizes())
    lines, stay, go = golden_mask(reads)
    drop = [dropped_by_rule(r, lines, sizes) for r in reads]
    assert not drop[stay] and drop[go]
    for rev in (0, 16):        # some but not all reads of each strand, among those the read filter keeps
        n = [x for r, x in zip(reads, drop) if r["flag"] & 16 == rev and r["mapq"] >= MAPQ]
        assert 0 < sum(n) < len(n)
    bed = d / "blacklist.bed"
    bed.write_text("".join("{}\t{}\t{}\tregion\n".format(c, b, e) for c, iv in lines.items() for b, e in iv))
    # (B)'s inputs: the SAM without the overlapping reads, the bedGraph with max(1, b + 2 - L) .. e cut out of every interval
    refs = BC.golden_sizes()
    kept = [SW.rec("r%d" % i, r["flag"], r["rname"], r["pos"], r["mapq"], [("M", r["qlen"])]) for i, (r, x) in enumerate(zip(reads, drop))
            if not x]
    fsam = d / "filtered.sam"
    fsam.write_bytes(SW.sam_text(refs, kept))
    out = []
    for c, b, e, v in golden_track():
        pieces = [(b, e)]
        for xb, xe in lines.get(c, []):
            cb, ce = max(1, xb + 2 - L) - 1, xe
            pieces = [q for pb, pe in pieces for q in ((pb, min(pe, cb)), (max(pb, ce), pe)) if q[0] < q[1]]
        out += ["{}\t{}\t{}\t{}\n".format(c, pb, pe, v) for pb, pe in pieces]
    fbg = d / "filtered.bedGraph"
    fbg.write_text("".join(out))
    for name in (STEM + ".bam", STEM + ".bam.bai", "hg19_36mer-test.bedGraph"):
        shutil.copy(os.path.join(GOLD, name), d / name)
    sam_gz = d / (STEM + ".sam.gz")
    shutil.copy(os.path.join(GOLD, STEM + ".sam.gz"), sam_gz)
    tag = d / (STEM + ".tagAlign")
    tag.write_text("".join(BC.golden_lines()))
    sizes_file = d / "chrom.sizes"
    BC.write_sizes(sizes_file, refs)
    return dict(dir=d, bed=str(bed), fsam=str(fsam), fbg=str(fbg), bam=str(d / (STEM + ".bam")), sam_gz=str(sam_gz), tag=str(tag),
                sizes=str(sizes_file), track=str(d / "hg19_36mer-test.bedGraph"), lines=lines)


def tables(written):
    return {os.path.basename(str(p)).rsplit("_", 1)[-1]: open(p).read() for p in written}


_B = {}


def run_b(golden, **kw):
    key = repr(sorted(kw.items()))
    if key not in _B:
        out = golden["dir"] / ("b%d" % len(_B))
        _r, w = pipeline.run(golden["fsam"], out, SHIFT, read_len=L, mapq_criteria=MAPQ, mappability_path=golden["fbg"],
                             save_mappability_stats=False, **kw)
        _B[key] = (_r, tables(w))
    return _B[key]


def plain_tables(golden):
    if "plain" not in _B:
        _r, w = pipeline.run(golden["bam"], golden["dir"] / "plain", SHIFT, read_len=L, mapq_criteria=MAPQ, mappability_path=golden["track"],
                             save_mappability_stats=False)
        _B["plain"] = (_r, tables(w))
    return _B["plain"]


def mlen0(result):
    """mappable_len[0] of chr1 (the chromosome with reads)."""
    chroms = getattr(result, "mappable_chroms", None) or result.chroms
    return chroms["chr1"].mappable_len[0]


def assert_equal_tables(a, b):
    assert set(a) == set(b)
    for k in a:
        if k == "complexity.tab":
            assert a[k].split("\n", 1)[1] == b[k].split("\n", 1)[1]        # (the first row is the file's name)
        else:
            assert a[k] == b[k], k                                         # every integer and every float column


CASES = {
    "bam": (lambda g: g["bam"], {}, {}),
    "indexed_bam_chromfilter": (lambda g: g["bam"], {"chromfilter": [(True, ["chr1"])]}, {"chromfilter": [(True, ["chr1"])]}),
    "sam_gz": (lambda g: g["sam_gz"], {}, {}),
    "tagalign": (lambda g: g["tag"], {"chrom_sizes": "SIZES"}, {}),
    "host": (lambda g: g["bam"], {"device_ingest": False}, {}),
    "skip_ncc": (lambda g: g["bam"], {"skip_ncc": True}, {"skip_ncc": True}),
    "complexity": (lambda g: g["bam"], {"complexity": True}, {"complexity": True}),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_masked_run_equals_the_existing_code_on_filtered_inputs(golden, case):
    path, kw_a, kw_b = CASES[case]
    kw_a = {k: (golden["sizes"] if v == "SIZES" else v) for k, v in kw_a.items()}
    ra, wa = pipeline.run(path(golden), golden["dir"] / ("a_" + case), SHIFT, read_len=L, mapq_criteria=MAPQ,
                          mappability_path=golden["track"], exclude_regions=golden["bed"], save_mappability_stats=False, **kw_a)
    rb, tb = run_b(golden, **kw_b)
    assert_equal_tables(tables(wa), tb)
    r0, t0 = plain_tables(golden)
    assert mlen0(ra) == mlen0(rb) != mlen0(r0)      # the mask changes the track
    if not kw_b:
        assert tables(wa)["nreads.tab"] != t0["nreads.tab"]


def test_synthetic_chromosomes_masked_run_equals_filtered_inputs(tmp_path):
    """Three chromosomes with reads, each with unsorted, overlapping and abutting lines and lines past its end, on the real
    context: run (A) with the mask against run (B) on a SAM and a bedGraph the test filters itself."""
    rng = np.random.default_rng(21)
    refs = [("c1", 400_000), ("c2", 250_000), ("c3", 120_000)]
    recs = SW.synth_records(rng, refs, 6000)
    for r in recs[::3]:
        r["flag"] |= 16
    sizes = dict(refs)
    lines = {}
    for name, length in refs:
        b = rng.integers(0, length - 3000, 30)
        iv = list(zip(b.tolist(), (b + rng.integers(1, 2500, 30)).tolist()))
        iv += [(iv[0][1], iv[0][1] + 700), iv[1], (length - 900, length + 10_000_000), (length + 5, length + 50)]
        lines[name] = [iv[i] for i in rng.permutation(len(iv))]
    lines["absent"] = [(0, 100)]
    reads = [dict(flag=r["flag"], rname=r["rname"], pos=r["pos"], mapq=r["mapq"], qlen=r["seq_len"]) for r in recs]
    drop = [dropped_by_rule(r, lines, sizes) for r in reads]
    for name, _l in refs:
        for rev in (0, 16):
            n = [x for r, x in zip(reads, drop) if r["rname"] == name and r["flag"] & 16 == rev and r["mapq"] >= 1]
            assert 0 < sum(n) < len(n)
    sam, bam = SW.write_twins(tmp_path, "lib", refs, recs)
    fsam = tmp_path / "filtered.sam"
    fsam.write_bytes(SW.sam_text(refs, [r for r, x in zip(recs, drop) if not x]))
    track = [(c, s, s + 900) for c, length in refs for s in range(50, length - 1000, 1700)]
    bg, fbg, bed = tmp_path / "track.bedGraph", tmp_path / "cut.bedGraph", tmp_path / "mask.bed"
    bg.write_text("".join("{}\t{}\t{}\t1\n".format(*t) for t in track))
    out = []
    for c, b, e in track:
        pieces = [(b, e)]
        for xb, xe in lines.get(c, []):
            xe = min(xe, sizes[c])                              # clipped to the chromosome, as the rule says
            if xb >= xe:
                continue
            cb, ce = max(1, xb + 2 - L) - 1, xe
            pieces = [q for pb, pe in pieces for q in ((pb, min(pe, cb)), (max(pb, ce), pe)) if q[0] < q[1]]
        out += ["{}\t{}\t{}\t1\n".format(c, pb, pe) for pb, pe in pieces]
    fbg.write_text("".join(out))
    bed.write_text("".join("{}\t{}\t{}\n".format(c, b, e) for c, iv in lines.items() for b, e in iv))
    kw = dict(read_len=L, mapq_criteria=1, save_mappability_stats=False, complexity=True)
    rb, wb = pipeline.run(str(fsam), tmp_path / "b", SHIFT, mappability_path=str(fbg), **kw)
    r0, w0 = pipeline.run(bam, tmp_path / "plain", SHIFT, mappability_path=str(bg), **kw)
    for tag, path, more in (("bam", bam, {}), ("sam", sam, {}), ("host", bam, {"device_ingest": False}),
                            ("cached", bam, {"save_mappability_stats": True})):
        ra, wa = pipeline.run(path, tmp_path / tag, SHIFT, mappability_path=str(bg), exclude_regions=str(bed), **{**kw, **more})
        assert_equal_tables(tables(wa), tables(wb))
        assert tables(wa)["mscc.tab"] != tables(w0)["mscc.tab"] and tables(wa)["nreads.tab"] != tables(w0)["nreads.tab"]


def test_masked_stream_equals_the_existing_code_on_filtered_inputs(golden, tmp_path):
    fifo = tmp_path / (STEM + ".bam")
    os.mkfifo(fifo)
    data = open(golden["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(data)
    t = threading.Thread(target=writer)
    t.start()
    try:
        _r, wa = pipeline.run(str(fifo), tmp_path / "a", SHIFT, read_len=L, mapq_criteria=MAPQ, mappability_path=golden["track"],
                              exclude_regions=golden["bed"], save_mappability_stats=False)
    finally:
        t.join()
    assert_equal_tables(tables(wa), run_b(golden)[1])


def test_masked_and_unmasked_caches_live_side_by_side(golden, tmp_path):
    track = tmp_path / "track.bedGraph"
    shutil.copy(golden["track"], track)
    kw = dict(read_len=L, mapq_criteria=MAPQ, mappability_path=str(track))
    _r, wa = pipeline.run(golden["bam"], tmp_path / "a", SHIFT, exclude_regions=golden["bed"], **kw)
    _r, w0 = pipeline.run(golden["bam"], tmp_path / "u", SHIFT, **kw)
    assert sorted(p.name for p in tmp_path.glob("*.json")) == ["track_blacklist_mappability.json", "track_mappability.json"]
    assert_equal_tables(tables(wa), run_b(golden)[1])
    assert tables(w0) == plain_tables(golden)[1]
    _r, wa2 = pipeline.run(golden["bam"], tmp_path / "a2", SHIFT, exclude_regions=golden["bed"], **kw)      # both caches are loaded now
    _r, w02 = pipeline.run(golden["bam"], tmp_path / "u2", SHIFT, **kw)
    assert tables(wa2) == tables(wa) and tables(w02) == tables(w0)


# ---- the device filter against the host reader and brute force ---------------------------------------------------------------
def test_device_reader_equals_host_reader_and_brute_force(tmp_path):
    rng = np.random.default_rng(11)
    refs = [("c1", 3_000_000), ("c2", 2_000_000), ("c3", 1_000_000), ("empty", 5000)]
    recs = SW.synth_records(rng, refs[:3], 34000)                   # about 10^5 reads
    bam = str(tmp_path / "big.bam")
    W.write_bam(bam, refs, SW.bam_bytes(refs, recs))
    lines = {}
    for name, length in refs[:3]:
        b = rng.integers(0, length, 340)
        lines[name] = list(zip(b.tolist(), (b + rng.integers(1, 3000, 340)).tolist()))
    lines["c2"] += [lines["c2"][0], (lines["c2"][1][1], lines["c2"][1][1] + 50), (1_999_990, 2_100_000)]      # duplicate, abutting, past the end
    mask = region_mask.open_mask(lines)
    with BamReader(bam) as host, DeviceBamReader(bam) as dev:
        plain = [np.concatenate(c) for c in zip(*host.batches(1))]
        res = mask.resolve(host.references, host.lengths)
        host.set_exclude(res)
        dev.set_exclude(res)
        want = [np.concatenate(c) for c in zip(*host.batches(1))]
        got = [np.concatenate(c) for c in zip(*dev.batches(1))]
        for g, w in zip(got, want):
            assert g.shape == w.shape and (g == w).all()
        # brute force: a coverage vector per reference
        ref, pos, rlen, _rev = plain
        ndrop = 0
        for i, (name, length) in enumerate(refs):
            cov = np.zeros(length + 4000, dtype=np.int64)
            for b, e in lines.get(name, []):
                cov[b + 1:min(e, length) + 1] = 1
            csum = np.concatenate(([0], np.cumsum(cov)))
            sel = ref == i
            ndrop += int((csum[pos[sel] + rlen[sel]] - csum[pos[sel]] > 0).sum())
        assert 0 < ndrop < ref.size
        assert dev.excluded() == host.excluded() == ndrop == ref.size - want[0].size
        # the device merge against the host merge: unsorted, overlapping, abutting and duplicate lines, a reference with none
        for g, w in zip(dev.exclude_intervals(), res.merged_table()):
            assert (g == w).all()
        assert not (dev.exclude_intervals()[0] == 3).any()
        # the runs are those of the compacted arrays, and the complexity counts the same reads
        runs = dev.device_runs()
        assert [r[0] for r in runs] == [0, 1, 2] and sum(r[2] for r in runs) == want[0].size
        from pymasc_amd import complexity
        assert complexity.from_reader(dev, 1).reads == complexity.from_reader(host, 1).reads
        dev.set_exclude(None)
        assert dev.decode(1) == ref.size and dev.excluded() == 0


def test_no_name_in_common_is_a_value_error(golden, tmp_path):
    with pytest.raises(ValueError, match="references"):
        pipeline.run(golden["bam"], tmp_path / "o", SHIFT, read_len=L, exclude_regions={"1": [(700000, 800000)]})
    assert not (tmp_path / "o").exists() or not os.listdir(tmp_path / "o")


# ---- pmx_bits_clear_regions_dev_ex against numpy ------------------------------------------------------------------------------
def numpy_clear(bits, first, last, first_offset, left_pad):
    out = bits.copy()
    n = out.size
    for a, b in zip((np.asarray(first, np.int64) + first_offset).tolist(), np.asarray(last, np.int64).tolist()):
        if b < a:
            continue
        a, b = max(a, 0), min(b, n - 1)
        if b < a:
            continue
        a = max(a - left_pad, min(a, 1))
        out[a:b + 1] = False
    return out


@pytest.mark.parametrize("sorted_disjoint", [False, True])
@pytest.mark.parametrize("nbits", [1, 64, 1000, 65536, 200_003])
def test_clear_regions_against_numpy(nbits, sorted_disjoint):
    rng = np.random.default_rng(nbits + int(sorted_disjoint))
    with ffi.Context(0) as ctx:
        for n, pad in ((0, 0), (1, 0), (7, 35), (300, 35), (300, 5000), (40, 0)):
            bits = rng.random(nbits) < 0.7
            words = np.packbits(np.concatenate((bits, np.zeros(-nbits % 64, bool))), bitorder="little").view(np.uint64).copy()
            b = np.sort(rng.integers(0, nbits + 50, n)).astype(np.uint32)
            e = (b + rng.integers(0, max(2, nbits // 50), n)).astype(np.uint32)
            if n >= 7:      # word-aligned and unaligned ends, a start the pad takes below position 1, an end at and beyond nbits
                b[0], e[0] = 0, 3
                b[1], e[1] = 63, 127
                b[2], e[2] = 64, 64
                e[-1] = nbits + 40
            if sorted_disjoint and n:      # merged intervals: b_i + 1 <= e_i < b_(i+1) + 1
                e = np.maximum(e, b + 1)
                keep = np.ones(n, bool)
                top = -1
                for i in range(n):
                    keep[i] = int(b[i]) >= top
                    top = max(top, int(e[i]) + 1) if keep[i] else top
                b, e = b[keep], e[keep]
            elif n:
                order = rng.permutation(n)
                b, e = b[order], e[order]
            n = int(b.size)
            d_m = ctx.bits_alloc(nbits)
            d_state = ctx.bits_alloc(ffi.PMX_FEED_WORDS * 64)
            try:
                ctx.bits_upload(d_m, words, nbits)
                ctx.bits_clear(d_state, ffi.PMX_FEED_WORDS * 64)
                tb = torch.from_numpy(b.astype(np.int64)).to("cuda:0").to(torch.int32) if n else None     # (uint32 values as int32 bits)
                te = torch.from_numpy(e.astype(np.int64)).to("cuda:0").to(torch.int32) if n else None
                torch.cuda.synchronize()
                ctx.bits_clear_regions_dev_ex(d_m, nbits, tb.data_ptr() if n else 0, te.data_ptr() if n else 0, n, 1, pad, d_state,
                                              sorted_disjoint=sorted_disjoint)
                got = ctx.bits_download(d_m, nbits)
                state = ctx.bits_download(d_state, ffi.PMX_FEED_WORDS * 64)
            finally:
                ctx.bits_free(d_m)
                ctx.bits_free(d_state)
            got_bits = np.unpackbits(got.view(np.uint8), bitorder="little")[:nbits].astype(bool)
            assert (got_bits == numpy_clear(bits, b, e, 1, pad)).all(), (n, pad)
            assert int(state[ffi.PMX_FEED_REGIONS_UNSORTED]) == 0
            out_of_range = bool(n) and bool(((b.astype(np.int64) + 1 <= e) & (e.astype(np.int64) >= nbits)).any())
            assert bool(state[ffi.PMX_FEED_FIRST_OUT_OF_RANGE]) == out_of_range
