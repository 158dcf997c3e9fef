"""Library complexity (NRF, PBC1, PBC2) without a GPU: the host checker, the host readers end to end, the table,
the option.  The yardstick is tests/complexity_cases.restate (a Counter over tuples), never the code under test."""
import math
import os

import numpy as np
import pytest

from pymasc_amd import cli, complexity, pipeline
from pymasc_amd.bam import BamReader
from pymasc_amd.bed_reads import BedReadsReader
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PMX_COMPLEXITY_BINS
from pymasc_amd.sam import SamReader
from tests import bed_reads_cases as BC
from tests import complexity_cases as CC
from tests import fixtures as fx
from tests import sam_writers as SW
from tests.fake_context import FakeContext

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")


def _host(ref, pos, ln, rev, nref):
    per, hist = complexity.count_host(ref, pos, ln, rev, nref)
    return [tuple(int(x) for x in row) for row in per], [int(x) for x in hist]


def test_bins_constant():
    assert PMX_COMPLEXITY_BINS == CC.BINS == 32
    assert complexity.COMPLEXITY_EXCLUDE == CC.EXCLUDE_KEEP_DUP == PMX_BAM_DEFAULT_EXCLUDE & ~0x400


@pytest.mark.parametrize("seed,nref,n", [(1, 3, 3000), (2, 1, 800), (3, 40, 5000)])
def test_count_host_equals_the_restatement(seed, nref, n):
    cols = CC.synthetic(np.random.default_rng(seed), nref=nref, n=n)
    CC.assert_sees_duplicates(*cols, above_bins=True)
    assert _host(*cols, nref) == CC.restate(*cols, nref)
    order = np.random.default_rng(seed + 100).permutation(len(cols[0]))          # the order of the reads does not matter
    assert _host(*[c[order] for c in cols], nref) == CC.restate(*cols, nref)


EDGES = {
    "no reads": ([], [], [], [], 2),
    "one read": ([1], [5], [36], [0], 2),
    "all on one key": ([0] * 7, [9] * 7, [36] * 7, [1] * 7, 1),
    "one field differs": ([0, 1, 0, 0, 0], [5, 5, 6, 5, 5], [36, 36, 36, 37, 36], [0, 0, 0, 0, 1], 2),
    "above the last bin": ([0] * 100 + [0] * 31 + [0] * 30, [3] * 100 + [4] * 31 + [5] * 30, [36] * 161, [0] * 161, 1),
    "read_len above bit 28": ([0, 0, 0, 0], [1, 1, 1, 1], [36, 36 + (1 << 28), 36 + (1 << 29), 36 + (1 << 30)], [0, 0, 0, 0], 1),
    "two references share every pos1": ([0, 1] * 6, [10, 10, 10, 10, 20, 20, 30, 30, 30, 30, 30, 30], [36] * 12, [0] * 12, 2),
}


@pytest.mark.parametrize("case", sorted(EDGES))
def test_count_host_edge_cases(case):
    *cols, nref = EDGES[case]
    want = CC.restate(*cols, nref)
    assert _host(*cols, nref) == want
    N, D, M1, M2 = CC.totals(want[0])
    if case == "one field differs":
        assert (N, D, M1) == (5, 5, 5)
    if case == "above the last bin":
        assert want[1][31] == 2 and want[1][30] == 1 and want[1][0] == 100
    if case == "read_len above bit 28":
        assert D == 4
    if case == "two references share every pos1":
        assert want[0][0] == want[0][1] == (6, 3, 1, 1)


def test_golden_file_has_no_duplicates():
    """The shipped file cannot show a duplicate: it is the NRF = PBC1 = 1, PBC2 = inf case only."""
    with BamReader(GOLDEN_BAM) as b:
        cols = [np.concatenate(x) for x in zip(*b.batches(1, CC.EXCLUDE_KEEP_DUP))]
        per, hist = CC.restate(*cols, len(b.references))
        assert CC.totals(per) == (2486, 2486, 2486, 0)
        c = b.library_complexity(1)
    assert CC.as_tables(c, b.references) == (per, hist)
    assert (c.reads, c.distinct, c.m1, c.m2, c.max_multiplicity) == (2486, 2486, 2486, 0, 1)
    assert c.nrf == 1.0 and c.pbc1 == 1.0 and c.pbc2 == math.inf


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """A BAM file, its SAM twin and a tagAlign file (sorted and shuffled) of one synthetic library with duplicates."""
    d = tmp_path_factory.mktemp("complexity")
    rng = np.random.default_rng(7)
    refs = CC.references(3)
    cols = CC.synthetic(rng, nref=3, n=2500)
    recs = CC.alignment_records(rng, refs, *cols)
    sam, bam = SW.write_twins(d, "lib", refs, recs)
    lines = CC.tagalign_lines(refs, *cols, rng)
    sizes = str(d / "sizes.txt")
    BC.write_sizes(sizes, refs)
    bed, shuf = str(d / "lib.tagAlign"), str(d / "shuffled.tagAlign")
    open(bed, "w").write("".join(lines))
    open(shuf, "w").write("".join(BC.shuffled(lines, seed=3)))
    return dict(refs=refs, recs=recs, sam=sam, bam=bam, lines=lines, bed=bed, shuffled=shuf, sizes=sizes, dir=d)


@pytest.mark.parametrize("mapq", [0, 1, 30])
@pytest.mark.parametrize("kind", ["bam", "sam"])
def test_host_alignment_readers(files, kind, mapq):
    refs, recs = files["refs"], files["recs"]
    names = [n for n, _l in refs]
    kept = CC.kept_columns(refs, recs, mapq)
    CC.assert_sees_duplicates(*kept, above_bins=True)
    want = CC.restate(*kept, len(refs))
    default = CC.restate(*CC.kept_columns(refs, recs, mapq, PMX_BAM_DEFAULT_EXCLUDE), len(refs))
    assert want != default                                  # the flagged duplicates are in the file and they are counted
    assert any(r["flag"] & 0x80 for r in recs) and any(r["flag"] & 0x4 for r in recs)
    assert any(r["mapq"] < 30 for r in recs) and any(r["mapq"] == 0 for r in recs)
    with (BamReader(files["bam"]) if kind == "bam" else SamReader(files["sam"])) as r:
        assert CC.as_tables(r.library_complexity(mapq), names) == want
        use = [1, 0, 1]
        part = complexity.from_reader(r, mapq, [names[0], names[2]])
        assert list(part.per_reference) == [names[0], names[2]]
        assert CC.as_tables(part, names) == CC.restate(*kept, len(refs), use)


@pytest.mark.parametrize("mapq", [0, 30])
def test_host_bed_reader_counts_encodes_lines(files, mapq):
    refs = files["refs"]
    names = [n for n, _l in refs]
    want = CC.restate_lines(files["lines"], refs, mapq)
    N, D, M1, M2 = CC.totals(want[0])
    assert D < N and M2 > 0 and want[1][0] > CC.BINS
    lengths = [l for _n, l in refs]
    for path in (files["bed"], files["shuffled"]):
        with BedReadsReader(path, names, lengths) as r:
            assert CC.as_tables(r.library_complexity(mapq), names) == want


def _some(seed=5):
    cols = CC.synthetic(np.random.default_rng(seed), nref=3, n=1500)
    names = ["c0", "c1", "c2"]
    per, hist = complexity.count_host(*cols, 3)
    return cols, names, complexity.LibraryComplexity({n: per[i] for i, n in enumerate(names)}, hist)


def test_table_round_trip(tmp_path):
    cols, names, c = _some()
    want = CC.restate(*cols, 3)
    assert CC.as_tables(c, names) == want
    N, D, M1, M2 = CC.totals(want[0])
    assert (c.reads, c.distinct, c.m1, c.m2, c.max_multiplicity) == (N, D, M1, M2, want[1][0])
    assert (c.nrf, c.pbc1, c.pbc2) == (D / N, M1 / D, M1 / M2)
    path = complexity.write_complexity(tmp_path / "x.y", "x.y", c)
    assert path.name == "x.y_complexity.tab" and sorted(os.listdir(tmp_path)) == ["x.y_complexity.tab"]
    name, back, ratios = complexity.read_complexity(path)
    assert name == "x.y" and back == c
    assert ratios == {"NRF": c.nrf, "PBC1": c.pbc1, "PBC2": c.pbc2}            # repr: they read back exactly
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert [r[0] for r in rows[:9]] == ["Name", "Reads", "Distinct positions", "Positions with one read",
                                        "Positions with two reads", "Largest multiplicity", "NRF", "PBC1", "PBC2"]
    assert rows[9] == ["chrom", "reads", "distinct", "one", "two"]
    assert rows[10:13] == [[n] + [str(x) for x in want[0][i]] for i, n in enumerate(names)]
    assert rows[13] == ["multiplicity", "positions"]
    assert rows[14:] == [[">=31" if k == 31 else str(k), str(want[1][k])] for k in range(1, 32) if want[1][k]]
    assert rows[-1][0] == ">=31"


def test_zero_denominators(tmp_path):
    empty = complexity.LibraryComplexity({"c0": (0, 0, 0, 0)}, np.zeros(32, dtype=np.int64))
    assert math.isnan(empty.nrf) and math.isnan(empty.pbc1) and math.isnan(empty.pbc2)
    hist = np.zeros(32, dtype=np.int64)
    hist[0], hist[1] = 1, 3
    unique = complexity.LibraryComplexity({"c0": (3, 3, 3, 0)}, hist)
    assert unique.pbc2 == math.inf and unique.nrf == 1.0
    text = {}
    for name, c in (("empty", empty), ("unique", unique)):
        p = complexity.write_complexity(tmp_path / name, name, c)
        text[name] = dict(ln.rstrip("\n").split("\t")[:2] for ln in open(p) if ln.count("\t") == 1)
        _n, back, ratios = complexity.read_complexity(p)
        assert back == c
    assert (text["empty"]["NRF"], text["empty"]["PBC1"], text["empty"]["PBC2"]) == ("nan", "nan", "nan")
    assert (text["unique"]["NRF"], text["unique"]["PBC2"]) == ("1.0", "inf")


def test_add_over_a_split_by_reference():
    cols, names, whole = _some(seed=9)
    ref = np.asarray(cols[0])
    parts = []
    for chosen in ([0, 2], [1]):
        m = np.isin(ref, chosen)
        per, hist = complexity.count_host(*[np.asarray(c)[m] for c in cols], 3)
        parts.append(complexity.LibraryComplexity({names[i]: per[i] for i in chosen}, hist))
    total = parts[0] + parts[1]
    assert CC.as_tables(total, names) == CC.as_tables(whole, names) == CC.restate(*cols, 3)
    assert total.max_multiplicity == whole.max_multiplicity


def test_option_parses():
    assert cli.parse_args(["a.bam", "-d", "100"]).complexity is False
    assert cli.parse_args(["a.bam", "-d", "100", "--complexity"]).complexity is True
    assert "_complexity.tab" in cli.get_parser().format_help()


def test_pipeline_writes_the_table_and_nothing_else_changes(files, tmp_path):
    refs, recs = files["refs"], files["recs"]
    names = [n for n, _l in refs]
    kw = dict(read_len=36, mapq_criteria=30, device_ingest=False, stats=True)
    res0, w0 = pipeline.run(files["bam"], str(tmp_path / "plain"), 120, context=FakeContext(), **kw)
    res1, w1 = pipeline.run(files["bam"], str(tmp_path / "with"), 120, context=FakeContext(), complexity=True, **kw)
    assert [p.name for p in w1] == [p.name for p in w0] + ["lib_complexity.tab"]
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, _ratios = complexity.read_complexity(w1[-1])
    kept = CC.kept_columns(refs, recs, 30)
    assert name == "lib" and CC.as_tables(c, names) == CC.restate(*kept, len(refs))
    # the chosen chromosomes only
    _r, w2 = pipeline.run(files["bam"], str(tmp_path / "two"), 120, context=FakeContext(), complexity=True,
                          references=[names[0], names[1]], **kw)
    _n, c2, _ = complexity.read_complexity(w2[-1])
    assert list(c2.per_reference) == names[:2]
    assert CC.as_tables(c2, names) == CC.restate(*kept, len(refs), [1, 1, 0])
    # several files, with names
    out = pipeline.run_files([files["bam"], files["sam"]], str(tmp_path / "files"), 120, context=FakeContext(), names=["A", "B"],
                             complexity=True, **kw)
    for f in out:
        assert f.written[-1].name == f.basename + "_complexity.tab"
        assert CC.as_tables(complexity.read_complexity(f.written[-1])[1], names) == CC.restate(*kept, len(refs))
