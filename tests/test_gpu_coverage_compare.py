"""Treatment against control on the GPU: pmx_dbam_coverage_compare and the signal consumers over its runs against
the loop restatement of tests/compare_cases and against the host path -- runs, totals, text bytes and the whole bigWig file with
compression off, byte for byte: everything is an integer or has one stated order.  The treatment through every device reader, with a
mask, a stream window by window, the pair pileup, compare and signal in turn on one pileup, a pileup against itself, the compressed
doors, the error paths, the stream's peak and up to the run's file."""
import os
import random
import threading

import numpy as np
import pytest

from pymasc_amd import coverage, pipeline, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.bed_reads import DeviceBedReadsReader
from pymasc_amd.native import PmxIOError
from pymasc_amd.sam import DeviceSamReader
from pymasc_amd.stream_device import DeviceStreamReader
from tests import bigwig_out_cases as BC
from tests import compare_cases as PC
from tests import coverage_cases as CC
from tests import fixtures as fx
from tests import fragments_cases as FR
from tests import io_writers as W
from tests import sam_writers as SW
from tests import signal_cases as SC

pytestmark = pytest.mark.gpu

FC = CC.FC
GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")
STEM = "ENCFF000RMB-test"
WINDOW = 8 << 10                    # compressed bytes per stream window: the file is cut into tens of windows
ALL = CC.USES["all"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """coverage_cases' library under the renamed references of bigwig_out_cases as every kind of input (the treatment), and a second
    draw of it as a BAM file (the control)."""
    d = tmp_path_factory.mktemp("gpu_coverage_compare")
    rows = CC.synthetic()
    recs = FC.alignment_records(rows, BC.REFS)
    _sam, bam, gz = SW.write_twins(d, "cv", BC.REFS, recs, bgzf_block=60_000)
    ids = {n: i for i, n in enumerate(BC.NAMES)}
    indexed = str(d / "indexed.bam")
    W.write_bam_indexed(indexed, BC.REFS, SW.bam_bytes(BC.REFS, recs), [ids[r["rname"]] for r in recs])
    tag = str(d / "cv.tagAlign")
    with open(tag, "w") as fp:
        fp.write("".join(FC.tagalign_lines(rows, BC.REFS)))
    crows = CC.synthetic(seed=23, n=9_000)
    control = SW.write_twins(d, "input", BC.REFS, FC.alignment_records(crows, BC.REFS))[1]
    t, c = FC.kept(rows), FC.kept(crows)
    return dict(dir=d, bam=bam, gz=gz, indexed=indexed, tag=tag, control=control, t=t, c=c, t_less=FC.masked(t, BC.REFS, BC.MASK),
                c_less=FC.masked(c, BC.REFS, BC.MASK), pile={}, sums={})


def _host_count(reads, refs, use, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    return coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)


def _pile(case, which, extend, masked=False, use="all"):
    """(the host pileup, the per-base depth lists of the restated runs), computed once per parameter set and left unchanged."""
    key = which, extend, masked, use
    if key not in case["pile"]:
        reads = case[which + "_less" if masked else which]
        want = CC.restate(reads, BC.REFS, CC.USES[use], extend)
        case["pile"][key] = _host_count(reads, BC.REFS, CC.USES[use], extend), BC.depth_lists(want, BC.REFS, CC.USES[use])
    return case["pile"][key]


def _sums(case, which, extend, B):
    if (which, extend, B) not in case["sums"]:
        case["sums"][which, extend, B] = SC.bin_sums(_pile(case, which, extend)[1], B)
    return case["sums"][which, extend, B]


def _factors(t, c, normalize):
    lengths = [l for _n, l in t.refs]
    return coverage.factors_of(normalize, dict(zip(coverage.TOTALS, t.totals)), dict(zip(coverage.TOTALS, c.totals)), lengths)


def _totals(tot):
    return tuple(tot[k] for k in coverage.SIGNAL_TOTALS)


@pytest.mark.parametrize("B", PC.BINS)
@pytest.mark.parametrize("extend", [0, 200])
def test_the_device_against_the_restatement(case, tmp_path, extend, B):
    t, c = _pile(case, "t", extend)[0], _pile(case, "c", extend)[0]
    with DeviceBamReader(case["bam"]) as r, DeviceBamReader(case["control"]) as rc:
        assert r._L.pmx_dbam_version() >= 20
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, extend), coverage.device_count_of(rc, FC.MAPQ, None, extend)
        for op, normalize in zip(PC.OPS, coverage.NORMALIZE):
            a_t, a_c = _factors(t, c, normalize)
            want = PC.restate(_sums(case, "t", extend, B), _sums(case, "c", extend, B), op, a_t, a_c, 1.0)
            assert _totals(acc.compare(r, cacc, rc, B, op, a_t, a_c, 1.0, normalize, case["control"])) == PC.totals(want)
            g = acc.signal_result(r)
            host = t.compare(c, B, op, a_t, a_c, 1.0, normalize, case["control"])
            assert PC.rows_got(g) == PC.rows_of(want) and g == host and g.tail == host.tail
            assert acc.text(r, signal=True) == PC.text_of(want) == b"".join(acc.text_chunks(r, 1000, signal=True))
            assert want["min"] < 0 or op == "ratio"
            if op != "ratio":                               # the whole file, where the values have both signs
                dev = coverage.write_bigwig(tmp_path / "dev", "dev", acc, r, signal=True)
                assert dev.read_bytes() == coverage.write_bigwig(tmp_path / "host", "host", host).read_bytes()
                PC.check_file(BC.read_file(dev), want, BC.REFS, B)
            assert coverage.write_coverage(tmp_path / "dev", "dev", acc, r, signal=True).read_bytes() == \
                coverage.write_coverage(tmp_path / "host", "dev", host).read_bytes()
        assert acc.result(r) == t and cacc.result(rc) == c  # the depth runs of both stay as they are


def _compare_files(reader, case, base, mask, extend, B, op, normalize, references=None):
    """(text, file bytes, totals) of the device's compared track of ``reader`` against the control file."""
    with DeviceBamReader(case["control"]) as rc:
        for x in (reader, rc):
            if mask is not None:
                x.set_exclude(mask.resolve(x.references, x.lengths))
        acc, cacc = coverage.device_count_of(reader, FC.MAPQ, references, extend), coverage.device_count_of(rc, FC.MAPQ, references, extend)
        return _pull(acc, reader, cacc, rc, case, base, B, op, normalize)


def _pull(acc, reader, cacc, rc, case, base, B, op, normalize):
    a_t, a_c = coverage.factors_of(normalize, acc.finish(reader), cacc.finish(rc), [l for _n, l in acc.refs])
    tot = acc.compare(reader, cacc, rc, B, op, a_t, a_c, 0.5, normalize, case["control"])
    track = coverage.write_coverage(base, "dev", acc, reader, signal=True).read_bytes()
    return track, coverage.write_bigwig(base, "dev", acc, reader, signal=True).read_bytes(), _totals(tot)


def _host_files(t, c, case, base, B, op, normalize):
    a_t, a_c = _factors(t, c, normalize)
    g = t.compare(c, B, op, a_t, a_c, 0.5, normalize, case["control"])
    return coverage.write_coverage(base, "dev", g).read_bytes(), coverage.write_bigwig(base, "dev", g).read_bytes(), g.totals


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("extend,B,op,normalize", [(0, 50, "log2", "none"), (200, 7, "subtract", "rpgc")])
def test_every_reader_makes_the_host_paths_track(case, tmp_path, extend, B, op, normalize, masked):
    mask = region_mask.open_mask(BC.MASK) if masked else None
    whole = _host_files(_pile(case, "t", extend, masked)[0], _pile(case, "c", extend, masked)[0], case, tmp_path / "host", B, op, normalize)
    assert b" control=input.bam compare=%s pseudocount=0.5\n" % op.encode() in whole[0][:400] and whole[2][0] > 500 and whole[2][2] < 0
    with DeviceBamReader(case["bam"]) as r:
        assert _compare_files(r, case, tmp_path / "bam", mask, extend, B, op, normalize) == whole
    with DeviceSamReader(case["gz"]) as r:
        assert _compare_files(r, case, tmp_path / "gz", mask, extend, B, op, normalize) == whole
    with DeviceBedReadsReader(case["tag"], BC.NAMES, BC.LENGTHS) as r:
        assert _compare_files(r, case, tmp_path / "tag", mask, extend, B, op, normalize) == whole
    chosen = [n for n, u in zip(BC.NAMES, CC.USES["no middle"]) if u]
    with DeviceBamReader(case["indexed"], references=chosen) as r:
        assert r.indexed
        part = _compare_files(r, case, tmp_path / "indexed", mask, extend, B, op, normalize, chosen)
    assert part == _host_files(_pile(case, "t", extend, masked, "no middle")[0], _pile(case, "c", extend, masked, "no middle")[0], case,
                               tmp_path / "host2", B, op, normalize)
    # a FIFO cut into windows
    fifo = tmp_path / "fifo"
    os.mkfifo(fifo)
    blob = open(case["bam"], "rb").read()

    def writer():
        with open(fifo, "wb") as fp:
            fp.write(blob)
    th = threading.Thread(target=writer)
    th.start()
    try:
        with DeviceStreamReader(str(fifo), window_bytes=WINDOW) as r, DeviceBamReader(case["control"]) as rc:
            for x in (r, rc):
                if mask is not None:
                    x.set_exclude(mask.resolve(x.references, x.lengths))
            acc = r.arm_coverage(FC.MAPQ, None, extend)
            for _ in r._windows():
                pass
            streamed = _pull(acc, r, coverage.device_count_of(rc, FC.MAPQ, None, extend), rc, case, tmp_path / "fifo_out", B, op, normalize)
            assert r.stream_info()["windows"] >= 10
    finally:
        th.join(60)
    assert streamed == whole


def _bam_of(d, name, refs, reads):
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(reads)]
    return SW.write_twins(d, name, refs, recs)[1]


def _planted_want(rt, rc, B, op, a_t, a_c, p):
    use = [1] * 4
    sums = [SC.bin_sums(BC.depth_lists(CC.restate(x, PC.P_REFS, use, 0), PC.P_REFS, use), B) for x in (rt, rc)]
    return PC.restate(*sums, op, a_t, a_c, p)


@pytest.mark.parametrize("op,a_t,a_c,p", [("log2", 1.0, 1.0, 1.0), ("ratio", 1.0, 1.0, 1.0), ("subtract", 1.0, 1.0, 1.0), ("subtract", PC.TINY, PC.TINY, 1.0),
                                          ("subtract", 1 / 128, 1 / 128, 1.0), ("log2", 0.37, 1.9, 0.5)])
def test_the_planted_situations(tmp_path, op, a_t, a_c, p):
    rt, rc_rows = PC.planted_treatment(), PC.planted_control()
    want = _planted_want(rt, rc_rows, PC.P_B, op, a_t, a_c, p)
    PC.check_planted(want, op, a_t, a_c, p)
    kw = dict(items_per_section=2, index_block=2, zoom_base=PC.P_ZOOM)
    with DeviceBamReader(_bam_of(tmp_path, "t", PC.P_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PC.P_REFS, rc_rows)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert _totals(acc.compare(r, cacc, rc, PC.P_B, op, a_t, a_c, p)) == PC.totals(want)
        assert PC.rows_got(acc.signal_result(r)) == PC.rows_of(want) and acc.text(r, signal=True) == PC.text_of(want)
        dev = coverage.write_bigwig(tmp_path / "p", "p", acc, r, signal=True, **kw)
        got = BC.read_file(dev, 2)
        PC.check_file(got, want, PC.P_REFS, PC.P_B, PC.P_ZOOM, 2)
        if op == "subtract":
            PC.check_planted_zoom(got, want)                # a zoom bin whose values are all negative
        # the compressed doors: the file decodes to the same sections
        z = BC.read_file(coverage.write_bigwig(tmp_path / "z", "p", acc, r, compress="device", signal=True, **kw), 2)
        assert z["compressed"] and {k: v for k, v in z.items() if k != "compressed"} == {k: v for k, v in got.items() if k != "compressed"}
        # compare, then signal, then compare on one pileup, with other bins: each replaces the one before, the depth runs serve all
        depths = BC.depth_lists(CC.restate(rt, PC.P_REFS, [1] * 4, 0), PC.P_REFS, [1] * 4)
        plain = SC.restate(SC.bin_sums(depths, 7), 0.37)
        assert _totals(acc.signal(r, 7, 0.37)) == SC.totals(plain) and acc.text(r, signal=True) == SC.text_of(plain)
        for B in (1, 7, 65536):
            other = _planted_want(rt, rc_rows, B, op, a_t, a_c, p)
            assert _totals(acc.compare(r, cacc, rc, B, op, a_t, a_c, p)) == PC.totals(other)
            assert PC.rows_got(acc.signal_result(r)) == PC.rows_of(other) and acc.text(r, signal=True) == PC.text_of(other)
        # the other way round: the control's handle takes the track, the treatment's keeps its own
        back = _planted_want(rc_rows, rt, PC.P_B, op, a_c, a_t, p)
        assert _totals(cacc.compare(rc, acc, r, PC.P_B, op, a_c, a_t, p)) == PC.totals(back) and cacc.text(rc, signal=True) == PC.text_of(back)
        assert acc.text(r, signal=True) == PC.text_of(other)
        # a pileup against itself: c == b
        for same in PC.OPS:
            mine = _planted_want(rt, rt, PC.P_B, same, 0.5, 0.5, 1.0)
            PC.check_self(mine, same)
            assert _totals(acc.compare(r, acc, r, PC.P_B, same, 0.5, 0.5, 1.0)) == PC.totals(mine) and acc.text(r, signal=True) == PC.text_of(mine)
        assert acc.text(r) == CC.text_of(CC.restate(rt, PC.P_REFS, [1] * 4, 0))


def test_a_reference_with_reads_in_one_file_only(tmp_path):
    rt, lone = PC.planted_treatment(), PC.planted_lonely()
    want, back = _planted_want(rt, lone, PC.P_B, "log2", 1.0, 1.0, 1.0), _planted_want(lone, rt, PC.P_B, "log2", 1.0, 1.0, 1.0)
    with DeviceBamReader(_bam_of(tmp_path, "t", PC.P_REFS, rt)) as r, DeviceBamReader(_bam_of(tmp_path, "c", PC.P_REFS, lone)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, None, 0)
        assert _totals(acc.compare(r, cacc, rc, PC.P_B)) == PC.totals(want) and PC.rows_got(acc.signal_result(r)) == PC.rows_of(want)
        assert _totals(cacc.compare(rc, acc, r, PC.P_B)) == PC.totals(back) and PC.rows_got(cacc.signal_result(rc)) == PC.rows_of(back)
        # a control without a kept read, and both without one
        none = coverage.device_count_of(rc, 255, None, 0)
        assert none.finish(rc)["reads"] == 0
        alone = _planted_want(rt, [], PC.P_B, "subtract", 1.0, 1.0, 1.0)
        assert _totals(acc.compare(r, none, rc, PC.P_B, "subtract")) == PC.totals(alone) and acc.text(r, signal=True) == PC.text_of(alone)
        assert _totals(none.compare(rc, none, rc, PC.P_B)) == (0, 0, 0.0, 0.0) and none.text(rc, signal=True) == b""
        assert none.ranges(rc, signal=True).tolist() == [0] * 5


def test_subtracting_an_empty_control_makes_the_signal_track(tmp_path):
    """compare with "subtract" against a control without a run on the chosen references is signal, bit for bit: t - 0.0 is t, and
    with S_c = 0 everywhere compare's runs begin where signal's do.  On the host classes too, over an empty pileup."""
    refs = [("s0", 1000), ("s1", 257), ("s2", 64)]
    rnd = random.Random(11)
    reads = []
    for k, (_n, length) in enumerate(refs):
        for _ in range((240, 80, 30)[k]):
            l = rnd.randint(1, 40)
            reads.append((k, rnd.randint(1, length - l + 1), l, rnd.randint(0, 1)))
    reads.sort(key=lambda x: (x[0], x[1]))
    crefs = refs + [("s3", 500)]
    creads = sorted((3, rnd.randint(1, 460), 36, 0) for _ in range(50))
    names = [n for n, _l in refs]
    t, none = _host_count(reads, refs, [1] * 3, 0), _host_count(creads, crefs, [1, 1, 1, 0], 0)
    assert t.n_runs > 100 and none.n_runs == 0 and none.reads == 0 and none.refs == t.refs
    scales = (1.0, 0.37, 2.0 ** -64)
    for B in (1, 2, 7, 50, 64, 65536):
        for s in scales:
            assert t.compare(none, B, "subtract", s, 1.0, 1.0) == t.signal(B, s)
    with DeviceBamReader(_bam_of(tmp_path, "t", refs, reads)) as r, DeviceBamReader(_bam_of(tmp_path, "c", crefs, creads)) as rc:
        acc, cacc = coverage.device_count_of(r, FC.MAPQ, None, 0), coverage.device_count_of(rc, FC.MAPQ, names, 0)
        assert cacc.finish(rc)["runs"] == 0 and acc.result(r) == t
        for B in (1, 2, 7, 64):
            for s in scales:
                want = acc.signal(r, B, s)
                plain = acc.signal_result(r)
                assert plain == t.signal(B, s) and want["runs"] > 0
                assert acc.compare(r, cacc, rc, B, "subtract", s, 1.0, 1.0) == want
                assert acc.signal_result(r) == plain


def test_the_pair_pileup(tmp_path):
    def pairs(seed, n):
        recs = [r for _l, r in FR.planted()] + FR.random_pairs(random.Random(seed), n)
        return [r for _i, r in sorted(enumerate(recs), key=lambda t: (t[1].ref < 0, t[1].ref, t[1].pos0, t[0]))]
    bam, control = str(tmp_path / "pe.bam"), str(tmp_path / "input.bam")
    FR.write_bam(bam, pairs(3, 3000))
    FR.write_bam(control, pairs(5, 2000))
    with BamReader(bam) as h, BamReader(control) as hc:
        t, c = coverage.from_reader(h, FR.MAPQ, None, "pair", 2000), coverage.from_reader(hc, FR.MAPQ, None, "pair", 2000)
    a_t, a_c = _factors(t, c, "cpm")
    g = t.compare(c, 50, "log2", a_t, a_c, 1.0, "cpm", control)
    assert t.reads > 500 and c.reads > 300 and g.n_runs > 100 and g.min < 0 < g.max
    with DeviceBamReader(bam) as r, DeviceBamReader(control) as rc:
        acc, cacc = coverage.device_count_of(r, FR.MAPQ, None, "pair", 2000), coverage.device_count_of(rc, FR.MAPQ, None, "pair", 2000)
        assert _totals(acc.compare(r, cacc, rc, 50, "log2", a_t, a_c, 1.0, "cpm", control)) == g.totals and acc.signal_result(r) == g
        assert coverage.write_coverage(tmp_path / "dev", "x", acc, r, signal=True).read_bytes() == coverage.write_coverage(tmp_path / "host", "x", g).read_bytes()
        assert coverage.write_bigwig(tmp_path / "dev", "x", acc, r, signal=True).read_bytes() == coverage.write_bigwig(tmp_path / "host", "x", g).read_bytes()


def test_the_error_paths(tmp_path):
    rt = PC.planted_treatment()
    bam = _bam_of(tmp_path, "t", PC.P_REFS, rt)
    other = _bam_of(tmp_path, "o", [(n, l + 1) for n, l in PC.P_REFS], rt)
    fewer = _bam_of(tmp_path, "f", PC.P_REFS[:3], [x for x in rt if x[0] < 3])
    deep = _bam_of(tmp_path, "d", PC.P_REFS, [(0, 1, 36, 0)] * 1024)
    with DeviceBamReader(bam) as r, DeviceBamReader(bam) as rc, DeviceBamReader(other) as ro, DeviceBamReader(fewer) as rf, DeviceBamReader(deep) as rd:
        L, h, tot = r._L, r._h, np.zeros(4, dtype=np.float64)
        stem = "pmx_dbam_coverage_compare: "

        def fails(rc_, text, code=-3):
            assert rc_ == code
            with pytest.raises(PmxIOError, match=text):
                r._raise(rc_)

        def call(hc, B=50, op=0, a_t=1.0, a_c=1.0, p=1.0, hb=None, out=tot):
            return L.pmx_dbam_coverage_compare(hb or h, hc, B, op, a_t, a_c, p, None if out is None else out.ctypes.data)
        fails(call(rc._h), stem + "no runs: call pmx_dbam_coverage_finish first")          # nothing begun
        acc = coverage.DeviceCount(r, FC.MAPQ, None, 0)
        acc.add(r)
        fails(call(rc._h), stem + "no runs: call pmx_dbam_coverage_finish first")          # a table, no runs yet
        acc.finish(r)
        fails(call(rc._h), stem + "the control has no runs")                               # the control: nothing begun
        cacc = coverage.DeviceCount(rc, FC.MAPQ, None, 0)
        cacc.add(rc)
        fails(call(rc._h), stem + "the control has no runs")                               # the control: a table
        cacc.finish(rc)
        fails(L.pmx_dbam_coverage_compare(None, rc._h, 50, 0, 1.0, 1.0, 1.0, tot.ctypes.data), "null handle")
        fails(L.pmx_dbam_coverage_compare(h, None, 50, 0, 1.0, 1.0, 1.0, tot.ctypes.data), "null handle")
        fails(call(rc._h, out=None), stem + "null output")
        coverage.device_count_of(ro, FC.MAPQ, None, 0)
        coverage.device_count_of(rf, FC.MAPQ, None, 0)
        fails(call(ro._h), stem + "the chosen references of the control differ")            # other lengths
        fails(call(rf._h), stem + "the chosen references of the control differ")            # fewer references
        part = coverage.device_count_of(rc, FC.MAPQ, ["p0", "p2"], 0)
        fails(call(rc._h), stem + "the chosen references of the control differ")            # another choice of the same header
        with pytest.raises(ValueError, match="the chosen references of the control differ"):
            acc.compare(r, part, rc, 50)
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 0)
        for bad in (0, 65537):
            fails(call(rc._h, B=bad), stem + "a bin of 1 to 65536 bases")
        for bad in (-1, 3):
            fails(call(rc._h, op=bad), stem + "the operation is 0 \\(log2\\), 1 \\(ratio\\) or 2 \\(subtract\\)")
        for bad in (2.0 ** -65, 0.0, -1.0, float("nan"), float("inf")):
            fails(call(rc._h, a_t=bad), stem + "a factor is a finite number of at least 2\\^-64")
            fails(call(rc._h, a_c=bad), stem + "a factor is a finite number of at least 2\\^-64")
            for op in (0, 1):
                fails(call(rc._h, op=op, p=bad), stem + "the pseudocount is a finite number of at least 2\\^-64")
            assert call(rc._h, op=2, p=bad) == 0                                            # subtract ignores it
        assert acc.finish(r)["max_depth"] == 5
        fails(call(rc._h, a_t=2.0 ** 39), stem + "factor \\* max_depth is 2\\^40 or more")
        fails(call(rc._h, a_c=2.0 ** 39), stem + "factor \\* max_depth is 2\\^40 or more")
        assert call(rc._h, a_t=2.0 ** 37, op=2) == 0 and tot[3] == 3 * 2.0 ** 37
        dacc = coverage.device_count_of(rd, FC.MAPQ, None, 0)                               # each factor against its own track's depth
        assert dacc.finish(rd)["max_depth"] == 1024
        fails(call(rd._h, a_c=2.0 ** 30), stem + "factor \\* max_depth is 2\\^40 or more")
        assert call(rd._h, a_t=2.0 ** 30) == 0
        for op in (0, 1):
            fails(call(rc._h, op=op, p=2.0 ** 40), stem + "the pseudocount is 2\\^40 or more")
        fails(call(rc._h, op=1, p=2.0 ** -39), stem + "\\(factor \\* max_depth \\+ pseudocount\\) / pseudocount is 2\\^40 or more")
        assert call(rc._h, op=0, p=2.0 ** -39) == 0 and call(rc._h, op=1, p=2.0 ** -37) == 0 and tot[2] == tot[3] == 1.0      # (the same file: every ratio is 1)
        # the host's checks say the same before the call
        for kw, text in ((dict(a_t=2.0 ** 39), "2\\^40"), (dict(pseudo=0.0), "coverage_pseudocount"), (dict(op="ratio", pseudo=2.0 ** -39), "pseudocount\\) / pseudocount"),
                         (dict(op="divide"), "coverage_compare"), (dict(bin=0), "coverage_bin"), (dict(a_c=float("nan")), "finite")):
            with pytest.raises(ValueError, match=text):
                acc.compare(r, cacc, rc, **dict(dict(bin=50), **kw))
        assert acc.compare(r, cacc, rc, 50)["runs"] > 0
        acc.begin(r)                                                                        # a new table: runs and track are gone
        fails(call(rc._h), stem + "no runs: call pmx_dbam_coverage_finish first")


def test_the_stream_peak_counts_the_bin_tables(case):
    """Few reads on long references: finish holds the table of 4 bytes per base and 24 bytes per tile of 4096 slots; compare at
    B = 2 holds two tables of that size together (16 bytes per bin of 2 bases), so its peak is about twice finish's -- but only if
    the tables are counted."""
    refs = [("long0", 3_000_000), ("long1", 1_000_001)]
    reads = [(0, 1000 * i + 1, 36, 0) for i in range(40)] + [(1, 999_990, 36, 0)]
    bam, control = _bam_of(case["dir"], "long", refs, reads), _bam_of(case["dir"], "long_input", refs, reads[::2])
    with DeviceStreamReader(bam, window_bytes=WINDOW) as r, DeviceBamReader(control) as rc:
        acc = r.arm_coverage(FC.MAPQ, None, 0)
        for _ in r._windows():
            pass
        assert acc.finish(r)["runs"] == 41
        cacc = coverage.device_count_of(rc, FC.MAPQ, None, 0)
        before = r.stream_info()["peak_device_bytes"]
        bases = sum(l for _n, l in refs)
        bins = sum(-(-l // 2) for _n, l in refs)
        assert 4 * bases < before < 16 * bins
        tot = acc.compare(r, cacc, rc, 2, "log2")
        after = r.stream_info()["peak_device_bytes"]
        assert tot["runs"] == 43 and 16 * bins <= after < 16 * bins + (before - 4 * bases) + (1 << 20)
        acc.compare(r, cacc, rc, 4, "log2")                 # (half the tables: the peak stays)
        assert r.stream_info()["peak_device_bytes"] == after


def test_the_run_against_a_control(tmp_path):
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, [int(x) for x in b.lengths]))
        cols = [np.concatenate(x) for x in zip(*b.batches(10))]
    rows = [(int(r), int(p) + 17, int(l), int(s)) for r, p, l, s in list(zip(*cols))[::3] if int(p) + 17 + int(l) <= refs[int(r)][1]]
    recs = [SW.rec("c%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(rows)]
    control = SW.write_twins(tmp_path, "input", refs, recs)[1]
    use = [1] * len(refs)
    t = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, 200)
    c = _host_count(rows, refs, use, 200)
    kw = dict(read_len=36, mapq_criteria=10, mappability_path=None, save_mappability_stats=False, coverage_extend=200, coverage_bin=50)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "text"), 300, coverage_control=control, **kw)
    g = t.compare(c, 50, "log2", 1.0, t.reads / c.reads, 1.0, "none", control)
    assert w1[-1].name == STEM + "_coverage.bedGraph" and w1[-1].read_bytes() == coverage.write_coverage(tmp_path / "host", STEM, g).read_bytes()
    assert g.n_runs > 50 and g.min < 0 < g.max and sorted(os.listdir(tmp_path / "text")) == sorted(p.name for p in w1)
    a_t, a_c = _factors(t, c, "cpm")
    g2 = t.compare(c, 50, "subtract", a_t, a_c, 1.0, "cpm", control)
    more = dict(coverage_control=control, coverage_compare="subtract", coverage_normalize="cpm", coverage_format="bigwig")
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "bw"), 300, **more, **kw)
    assert w2[-1].name == STEM + "_coverage.bw" and w2[-1].read_bytes() == coverage.write_bigwig(tmp_path / "host", STEM, g2).read_bytes()
    _r3, w3 = pipeline.run(GOLDEN_BAM, str(tmp_path / "z"), 300, coverage_compress="device", **more, **kw)
    got, want = BC.read_file(w3[-1]), BC.read_file(w2[-1])
    assert got["compressed"] and {k: v for k, v in got.items() if k != "compressed"} == {k: v for k, v in want.items() if k != "compressed"}
    assert sorted(os.listdir(tmp_path / "z")) == sorted(p.name for p in w3)                # (the temporary file is gone)
    # "auto": the control is piled up with the treatment's estimate, on one more read of both files
    _r4, w4 = pipeline.run(GOLDEN_BAM, str(tmp_path / "auto"), 300, coverage_control=control, stats=True, **dict(kw, coverage_extend="auto"))
    rows4 = dict(ln.rstrip("\n").split("\t") for ln in open(w4[-2]))
    extend = int(rows4["Estimated library length"])
    t4 = coverage.count_host(*cols, [n for n, _l in refs], [l for _n, l in refs], use, extend)
    c4 = _host_count(rows, refs, use, extend)
    g4 = t4.compare(c4, 50, "log2", 1.0, t4.reads / c4.reads, 1.0, "none", control)
    assert w4[-1].read_bytes() == coverage.write_coverage(tmp_path / "host4", STEM, g4).read_bytes()
