"""Excluded regions without a GPU: the rules of pymasc_amd.region_mask against brute force, the host readers with a
mask, name resolution, the dict form, the cache-path rule, both command lines, and the whole host path -- a masked run against the
existing code on inputs the test filters itself -- on the fake context."""
import json
import os

import numpy as np
import pytest

from pymasc_amd import cli, mappability, pipeline, precalc, region_mask
from pymasc_amd.bam import BamReader
from pymasc_amd.sam import SamReader
from tests import sam_writers as SW
from tests.fake_context import FakeContext

REFS = [("c1", 60000), ("c2", 45000), ("c3", 30000)]
L = 36


class ClearingFakeContext(FakeContext):
    """The fake context with pmx_bits_clear_regions_dev_ex restated bit by bit."""

    def bits_clear_regions_dev_ex(self, p, nbits, d_first, d_last, n, first_offset=0, left_pad=0, d_state=None, sorted_disjoint=False):
        w = self._mem[p]
        first = self._mem[d_first].view(np.uint32)[:n].astype(np.int64) + first_offset
        last = self._mem[d_last].view(np.uint32)[:n].astype(np.int64)
        for a, b in zip(first.tolist(), last.tolist()):
            if b < a:
                continue
            a, b = max(a, 0), min(b, nbits - 1)
            a = max(a - left_pad, min(a, 1))
            for j in range(a, b + 1):
                w[j >> 6] &= ~(np.uint64(1) << np.uint64(j & 63))


def brute_merge(lines, length):
    covered = np.zeros(length + 2, dtype=bool)
    for b, e in lines:
        covered[b:min(e, length)] = True
    d = np.diff(np.concatenate(([0], covered.astype(np.int8), [0])))
    return list(zip(np.flatnonzero(d == 1).tolist(), np.flatnonzero(d == -1).tolist()))


def brute_drop(pos, rlen, lines, length):
    covered = np.zeros(length + 200, dtype=bool)           # 1-based positions b + 1 .. e
    for b, e in lines:
        covered[b + 1:min(e, length) + 1] = True
    return np.array([covered[p:p + max(l, 1)].any() for p, l in zip(pos, rlen)], dtype=bool)


def random_lines(rng, n, length):
    b = rng.integers(0, length, n)
    e = b + rng.integers(1, 400, n)
    lines = list(zip(b.tolist(), e.tolist()))
    lines += [(lines[0][1], lines[0][1] + 10), lines[1], (length - 5, length + 500), (length + 10, length + 20), (7, 7)]
    return [lines[i] for i in rng.permutation(len(lines))]


def test_merge_against_brute_force():
    rng = np.random.default_rng(1)
    for n in (0, 2, 40, 300):
        lines = random_lines(rng, n, 20000) if n else []
        b, e = region_mask.merge([x for x, _ in lines], [y for _, y in lines], 20000)
        assert list(zip(b.tolist(), e.tolist())) == brute_merge(lines, 20000)
    b, e = region_mask.merge([10, 20, 5], [20, 30, 6], 100)            # abutting lines join, separate ones stay
    assert list(zip(b.tolist(), e.tolist())) == [(5, 6), (10, 30)]


def test_overlap_rule_against_brute_force_and_its_edges():
    rng = np.random.default_rng(2)
    lines = random_lines(rng, 60, 20000)
    mb, me = region_mask.merge([x for x, _ in lines], [y for _, y in lines], 20000)
    pos = rng.integers(1, 20000, 5000)
    rlen = rng.integers(1, 80, 5000)
    assert (region_mask.overlaps(pos, rlen, mb, me) == brute_drop(pos, rlen, lines, 20000)).all()
    mb, me = region_mask.merge([1035], [1100])
    # the read 1000..1035 ends one base before the interval's first position 1036: kept; 1001..1036 touches it: dropped
    assert region_mask.overlaps([1000, 1001], [36, 36], mb, me).tolist() == [False, True]
    # an interval that ends exactly at a read's first base drops it; one base earlier does not
    assert region_mask.overlaps([1100, 1101], [36, 36], mb, me).tolist() == [True, False]


def test_cut_intervals_against_bits():
    rng = np.random.default_rng(3)
    tb = np.sort(rng.integers(0, 30000, 200))
    te = tb + rng.integers(1, 300, 200)
    lines = random_lines(rng, 30, 30000)
    mb, me = region_mask.merge([x for x, _ in lines], [y for _, y in lines])
    pb, pe = region_mask.cut_intervals(tb, te, mb, me, L)
    want = np.zeros(31000, dtype=bool)
    for b, e in zip(tb, te):
        want[b:e] = True
    for b, e in zip(mb.tolist(), me.tolist()):
        want[max(1, b + 2 - L) - 1:e] = False                   # 1-based positions max(1, b + 2 - L) .. e
    got = np.zeros(31000, dtype=bool)
    for b, e in zip(pb, pe):
        assert b < e
        got[b:e] = True
    assert (got == want).all()


def test_names_are_resolved_against_the_references(caplog):
    mask = region_mask.open_mask({"c1": [(5, 9)], "chrUn": [(1, 2)], "other": [(3, 4)]})
    with caplog.at_level("WARNING"):
        r = mask.resolve([n for n, _ in REFS], [l for _, l in REFS])
    assert sum("2 chromosome name(s)" in m for m in caplog.messages) == 1
    assert r.merged(0)[0].tolist() == [5] and r.merged(1)[0].size == 0
    with pytest.raises(ValueError, match="chr1"):
        region_mask.open_mask({"1": [(5, 9)]}).resolve(["chr1"], [1000])
    with pytest.raises(ValueError):
        region_mask.open_mask({}).resolve(["chr1"], [1000])


def test_dict_and_file_masks_agree(tmp_path):
    lines = {"c1": [(50, 90), (10, 20), (85, 120)], "c3": [(0, 5)]}
    bed = tmp_path / "mask.bed"
    bed.write_text("".join("{}\t{}\t{}\tname\t0\t+\n".format(c, b, e) for c, iv in lines.items() for b, e in iv))
    a = region_mask.open_mask(lines).resolve(*zip(*REFS))
    b = region_mask.open_mask(bed).resolve(*zip(*REFS))
    for x, y in zip(a.merged_table(), b.merged_table()):
        assert x.tolist() == y.tolist()
    assert a.merged_table()[1].tolist() == [10, 50, 0]
    with pytest.raises(FileNotFoundError):
        region_mask.open_mask(tmp_path / "none.bed")


def test_cache_path_rule(tmp_path):
    assert region_mask.stats_path("/d/hg19_36mer.bw", "/x/blacklist.v2.bed.gz").name == "hg19_36mer_blacklist.v2_mappability.json"
    assert region_mask.stats_path("/d/t.bedGraph", "/x/bl.bed") != mappability.default_stats_path("/d/t.bedGraph")
    assert region_mask.stats_path("/d/t.bw", {"c1": [(1, 2)]}) is None


def _records(rng, per_ref=1500):
    recs = SW.synth_records(rng, REFS, per_ref)
    for r in recs[::7]:
        r["flag"] |= 16
    return recs


def _mask_lines(rng):
    return {"c1": random_lines(rng, 25, 60000), "c3": random_lines(rng, 10, 30000), "absent": [(1, 50)]}


def test_host_readers_against_brute_force(tmp_path):
    rng = np.random.default_rng(4)
    recs = _records(rng)
    sam, bam = SW.write_twins(tmp_path, "lib", REFS, recs)
    lines = _mask_lines(rng)
    from pymasc_amd.bed_reads import BedReadsReader
    tag = tmp_path / "lib.tagAlign"
    tag.write_text("".join("{}\t{}\t{}\tN\t{}\t{}\n".format(r["rname"], r["pos"] - 1, r["pos"] - 1 + r["seq_len"], r["mapq"],
                                                            "-" if r["flag"] & 16 else "+") for r in recs if r["seq_len"]))
    names, lens = [n for n, _ in REFS], [l for _, l in REFS]
    for cls, path in ((BamReader, bam), (SamReader, sam), (lambda p: BedReadsReader(p, names, lens), str(tag))):
        with cls(path) as plain, cls(path) as masked:
            ref, pos, rlen, rev = (np.concatenate(c) for c in zip(*plain.batches(1)))
            masked.set_exclude(region_mask.open_mask(lines).resolve(masked.references, masked.lengths))
            got = [np.concatenate(c) for c in zip(*masked.batches(1, batch=512))]
            drop = np.zeros(ref.size, dtype=bool)
            for i, (name, length) in enumerate(REFS):
                sel = ref == i
                drop[sel] = brute_drop(pos[sel], rlen[sel], lines.get(name, []), length)
            assert 0 < drop.sum() < ref.size
            for g, w in zip(got, (ref, pos, rlen, rev)):
                assert (g == w[~drop]).all()
            assert masked.excluded() == int(drop.sum())


def _filtered_inputs(d, recs, track, lines, read_len):
    """What the existing code is given in place of a mask: the SAM without the overlapping reads, the bedGraph with
    max(1, b + 2 - L) .. e cut out of every interval."""
    keep = []
    for r in recs:
        length = dict(REFS)[r["rname"]]
        hit = any(b + 1 <= r["pos"] + max(r["seq_len"], 1) - 1 and r["pos"] <= min(e, length) and b < min(e, length)
                  for b, e in lines.get(r["rname"], []))
        if not hit:
            keep.append(r)
    sam = d / "filtered.sam"
    sam.write_bytes(SW.sam_text(REFS, keep))
    out = []
    for c, b, e in track:
        pieces = [(b, e)]
        for xb, xe in lines.get(c, []):
            cb, ce = max(1, xb + 2 - read_len) - 1, xe              # 0-based half-open
            pieces = [q for pb, pe in pieces for q in ((pb, min(pe, cb)), (max(pb, ce), pe)) if q[0] < q[1]]
        out += [(c, pb, pe) for pb, pe in pieces]
    bg = d / "filtered.bedGraph"
    bg.write_text("".join("{}\t{}\t{}\t1\n".format(*t) for t in out))
    return str(sam), str(bg), len(recs) - len(keep)


def _tables(written):
    return {os.path.basename(str(p)).split("_")[-1]: open(p).read() for p in written}


def test_host_path_equals_the_existing_code_on_filtered_inputs(tmp_path, caplog):
    rng = np.random.default_rng(5)
    recs = _records(rng, 800)
    sam = tmp_path / "lib.sam"
    sam.write_bytes(SW.sam_text(REFS, recs))
    track = [(c, s, s + 700) for c, length in REFS for s in range(100, length - 1000, 1500)]
    bg = tmp_path / "track.bedGraph"
    bg.write_text("".join("{}\t{}\t{}\t1\n".format(*t) for t in track))
    lines = _mask_lines(rng)
    bed = tmp_path / "bl.bed"
    bed.write_text("".join("{}\t{}\t{}\n".format(c, b, e) for c, iv in lines.items() for b, e in iv if b < e))   # (a BED line is not empty)
    fsam, fbg, ndrop = _filtered_inputs(tmp_path, recs, track, lines, L)
    assert 0 < ndrop < len(recs)
    kw = dict(max_shift=120, read_len=L, mapq_criteria=1, device_ingest=False, complexity=True)
    with caplog.at_level("INFO"):
        ra, wa = pipeline.run(str(sam), tmp_path / "a", mappability_path=str(bg), exclude_regions=str(bed),
                              context=ClearingFakeContext(), **kw)
    assert any("reads of" in m and "left out" in m for m in caplog.messages)
    rb, wb = pipeline.run(fsam, tmp_path / "b", mappability_path=fbg, context=ClearingFakeContext(), **kw)
    r0, w0 = pipeline.run(str(sam), tmp_path / "c", mappability_path=str(bg), context=ClearingFakeContext(), **kw)
    ta, tb, t0 = _tables(wa), _tables(wb), _tables(w0)
    assert set(ta) == set(tb) == {"cc.tab", "mscc.tab", "nreads.tab", "complexity.tab"}
    for k in ("cc.tab", "mscc.tab", "nreads.tab"):
        assert ta[k] == tb[k], k
        assert ta[k] != t0[k], k                                    # the mask is felt
    assert ta["complexity.tab"].split("\n", 1)[1] == tb["complexity.tab"].split("\n", 1)[1]      # (the first row is the name)
    # the cache: the masked run wrote its own file and left the unmasked one alone, each valid for its run
    masked_cache, plain_cache = tmp_path / "track_bl_mappability.json", tmp_path / "track_mappability.json"
    assert json.load(open(masked_cache))["exclude_read_len"] == L
    assert "exclude_read_len" not in json.load(open(plain_cache))
    before = plain_cache.read_bytes()
    pipeline.run(str(sam), tmp_path / "a2", mappability_path=str(bg), exclude_regions=str(bed), context=ClearingFakeContext(), **kw)
    r1, w1 = pipeline.run(str(sam), tmp_path / "c2", mappability_path=str(bg), context=ClearingFakeContext(), **kw)
    assert plain_cache.read_bytes() == before and _tables(w1) == t0
    # a dict mask computes the same tables and writes no cache of its own
    os.remove(masked_cache)
    rd, wd = pipeline.run(str(sam), tmp_path / "d", mappability_path=str(bg), context=ClearingFakeContext(),
                          exclude_regions={c: iv for c, iv in lines.items()}, **kw)
    assert {k: v for k, v in _tables(wd).items() if k != "complexity.tab"} == {k: v for k, v in ta.items() if k != "complexity.tab"}
    assert not masked_cache.exists() and plain_cache.read_bytes() == before
    # no name in common: ValueError, and no table
    with pytest.raises(ValueError, match="references"):
        pipeline.run(str(sam), tmp_path / "e", exclude_regions={"chr1": [(1, 5)]}, context=ClearingFakeContext(), **kw)
    assert not (tmp_path / "e").exists() or not os.listdir(tmp_path / "e")


def test_command_lines(tmp_path, capsys):
    bed = tmp_path / "bl.bed"
    bed.write_text("c1\t1\t5\n")
    args = cli.parse_args(["x.bam", "--exclude-regions", str(bed)])
    assert args.exclude_regions == bed and cli.parse_args(["x.bam"]).exclude_regions is None
    assert precalc.get_parser().parse_args(["-m", "t.bw", "--exclude-regions", str(bed)]).exclude_regions == bed
    assert cli.main(["x.bam", "--exclude-regions", str(tmp_path / "none.bed")]) == 2
    assert precalc.main(["-m", "t.bw", "--exclude-regions", str(tmp_path / "none.bed")]) == 2
    assert "--exclude-regions" in capsys.readouterr().err


def test_dropped_count_through_the_index_covers_every_chromosome(tmp_path):
    from pymasc_amd.bam import feed_bam
    from tests import io_writers as W
    rng = np.random.default_rng(6)
    recs = _records(rng)
    ids = {n: i for i, (n, _l) in enumerate(REFS)}
    bam = str(tmp_path / "indexed.bam")
    W.write_bam_indexed(bam, REFS, SW.bam_bytes(REFS, recs), [ids[r["rname"]] for r in recs])
    lines = _mask_lines(rng)

    class Sink:
        references = ["c1", "c3"]
        fed = 0

        def feed_reads(self, chrom, pos, rlen, rev):
            self.fed += len(pos)

        def finishup_calculation(self):
            pass
    with BamReader(bam) as plain, BamReader(bam) as masked:
        assert masked.has_index()
        masked.set_exclude(region_mask.open_mask(lines).resolve(masked.references, masked.lengths))
        a, b = Sink(), Sink()
        feed_bam(a, plain, 1)
        feed_bam(b, masked, 1)
        per = [sum(r.size for r, *_ in masked.fetch(n, 1)) for n in ("c1", "c3")]
        assert masked.excluded() > 0                    # (the last fetch alone: one chromosome)
        feed_bam(b, masked, 1)
        assert a.fed - b.fed // 2 == masked.excluded() > 0 and b.fed // 2 == sum(per)
