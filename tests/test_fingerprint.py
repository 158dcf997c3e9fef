"""The fingerprint and the Jensen-Shannon distance without a GPU: the host checker against the loop restatement of
tests/fingerprint_cases, the metrics on hand-made tables, the table file, the options, and the host path of the run."""
import math
import os

import numpy as np
import pytest

from pymasc_amd import cli, fingerprint, pipeline
from pymasc_amd.bam import BamReader
from pymasc_amd.fingerprint import BinCounts
from tests import fingerprint_cases as FC
from tests import fixtures as fx
from tests import io_writers as W
from tests import sam_writers as SW
from tests.fake_context import FakeContext

GOLDEN_BAM = os.path.join(fx.GOLDEN, "ENCFF000RMB-test.bam")


@pytest.fixture(scope="module")
def reads():
    return FC.kept(FC.synthetic())


def _host(reads, refs, use, bin_size, extend):
    cols = [np.array(c, dtype=np.int64) for c in zip(*reads)] if reads else [np.zeros(0, dtype=np.int64)] * 4
    counts, added = fingerprint.count_host(*cols, [l for _n, l in refs], use, bin_size, extend)
    return [int(x) for x in counts], added


@pytest.mark.parametrize("use", sorted(FC.USES))
@pytest.mark.parametrize("bin_size,extend", FC.PARAMS)
def test_count_host_equals_the_restatement(reads, bin_size, extend, use):
    use = FC.USES[use]
    assert FC.wanted_situations(FC.REFS, use, bin_size, extend) <= FC.situations(reads, FC.REFS, use, bin_size, extend)
    want = FC.restate(reads, FC.REFS, use, bin_size, extend)
    have = dict(FC.table(want[0]))
    assert 4095 in have and 4096 in have and 5000 in have           # either side of the exact table's edge, and the tail
    assert 0 < want[1] <= len(reads)
    assert _host(reads, FC.REFS, use, bin_size, extend) == want


def test_count_host_small_cases():
    refs = [("a", 10), ("b", 3), ("c", 7)]
    rows = [(0, 1, 4, 0), (0, 4, 4, 1), (0, 9, 5, 0), (0, 10, 1, 1), (1, 1, 3, 0), (2, 5, 4, 0), (2, 7, 1, 1), (2, 1, 2, 1), (2, 30, 5, 0)]
    # bins of 4: a has two (1..4, 5..8) and a tail of two bases, b has none, c has one (1..4) and a tail of three
    assert FC.restate(rows, refs, [1, 1, 1], 4, 0) == ([2, 1, 1], 3)
    assert _host(rows, refs, [1, 1, 1], 4, 0) == ([2, 1, 1], 3)
    # six bases from the 5' end: the reverse read at 4..7 reaches back to 2, the one at c:1..2 would begin below 1
    assert FC.restate(rows, refs, [1, 1, 1], 4, 6) == ([2, 3, 2], 5)
    for bin_size, extend in ((4, 6), (1, 0), (3, 2), (7, 0)):
        for use in ([1, 1, 1], [0, 1, 1], [1, 0, 0]):
            assert _host(rows, refs, use, bin_size, extend) == FC.restate(rows, refs, use, bin_size, extend)
    assert _host([], refs, [1, 1, 1], 4, 0) == ([0, 0, 0], 0)


def test_layout_errors():
    with pytest.raises(ValueError, match="no chosen reference is as long as one bin"):
        fingerprint.layout([100, 50], [1, 1], 101)
    with pytest.raises(ValueError, match="no chosen reference is as long as one bin"):
        fingerprint.layout([100, 500], [1, 0], 200)
    with pytest.raises(ValueError, match="the bin size is 0"):
        fingerprint.layout([100], [1], 0)
    with pytest.raises(ValueError, match="2\\^31 bins or more"):
        fingerprint.layout([1 << 30, 1 << 30], [1, 1], 1)
    first, nb = fingerprint.layout([100_003, 499, 70_001], [1, 1, 1], 500)
    assert first.tolist() == [0, 200, 200] and nb.tolist() == [200, 0, 140]


def _table(pairs, bin_size=500, extend=0):
    values, bins = zip(*pairs)
    return BinCounts(bin_size, extend, {"c": sum(bins)}, values, bins, reads=sum(v * b for v, b in pairs))


def test_metrics_on_hand_made_tables():
    even = _table([(7, 40)])
    assert (even.B, even.T, even.mean) == (40, 280, 7.0)
    assert even.auc == 0.5 and even.x_intercept == 0.0 and even.elbow == 1.0
    half = _table([(0, 20), (3, 20)])
    assert half.x_intercept == 0.5 and half.elbow == 0.5 and half.auc == 0.25
    # three groups by hand: X = .5, .75, 1; Y = 0, 1/7, 1; auc = .25 * (1/7) / 2 + .25 * (8/7) / 2; elbow at max(X - Y) = .75 - 1/7
    three = _table([(0, 2), (1, 1), (6, 1)])
    assert three.auc == pytest.approx(0.25 / 14 + 0.25 * 8 / 14, abs=1e-15) and three.elbow == 0.75
    assert 0.0 < even.synthetic_auc < 0.5 and 0.0 < even.synthetic_jsd < 1.0


def test_poisson_model():
    c = _table([(0, 30), (1, 50), (2, 15), (40, 5)])
    k, q = c.poisson()
    lam = c.mean
    assert k[0] == 0 and k[-1] == max(40, math.ceil(lam + 10 * math.sqrt(lam) + 20)) and abs(q.sum() - 1) < 1e-12
    want = np.array([math.exp(-lam) * lam ** i / math.factorial(i) for i in range(len(k))])
    np.testing.assert_allclose(q, want / want.sum(), rtol=1e-12, atol=1e-300)
    # a table that IS Poisson-shaped is close to its model, a pile-up is far from it
    n = 10 ** 6
    lam = 2.5
    shaped = _table([(i, round(n * math.exp(-lam) * lam ** i / math.factorial(i))) for i in range(14)])
    assert shaped.synthetic_jsd < 1e-3 and abs(shaped.synthetic_auc - shaped.auc) < 1e-3
    # 99 % empty bins against a Poisson model with q(0) = exp(-2.5): total variation >= 0.99 - 0.083 = 0.907, and by Pinsker's
    # inequality on both halves the divergence is at least TV^2 / (2 ln 2) bits = 0.593, the distance at least 0.77
    assert _table([(0, 990), (250, 10)]).synthetic_jsd > 0.77


def test_jsd_rules():
    a, b = _table([(0, 1), (2, 3)]), _table([(0, 2), (1, 1), (2, 1)])
    assert a.jsd_to(a) == 0.0 and b.jsd_to(b) == 0.0
    assert a.jsd_to(b) == b.jsd_to(a) and 0.0 < a.jsd_to(b) < 1.0
    m = [(0.25 + 0.5) / 2, 0.25 / 2, (0.75 + 0.25) / 2]
    want = math.sqrt(0.5 * (0.25 * math.log2(0.25 / m[0]) + 0.75 * math.log2(0.75 / m[2]))
                     + 0.5 * (0.5 * math.log2(0.5 / m[0]) + 0.25 * math.log2(0.25 / m[1]) + 0.25 * math.log2(0.25 / m[2])))
    assert a.jsd_to(b) == pytest.approx(want, abs=1e-15)
    assert _table([(1, 1), (3, 3)]).jsd_to(_table([(2, 4), (5, 4)])) == 1.0         # disjoint supports
    assert a.jsd_to(_table([(0, 10), (2, 30)], bin_size=64)) == 0.0                 # shares of bins, not numbers of bins


def test_no_reads_gives_nan(tmp_path):
    empty = _table([(0, 12)])
    assert (empty.B, empty.T, empty.mean, empty.x_intercept) == (12, 0, 0.0, 1.0)
    for v in (empty.auc, empty.elbow, empty.synthetic_auc, empty.synthetic_jsd, empty.jsd_to(_table([(1, 2)])),
              _table([(1, 2)]).jsd_to(empty)):
        assert math.isnan(v)
    p = fingerprint.write_fingerprint(tmp_path / "e", "e", empty)
    _n, back, block = fingerprint.read_fingerprint(p)
    assert back == empty and math.isnan(block["AUC"]) and block["Mean"] == 0.0


def test_bin_counts_equality_and_checks():
    a = _table([(0, 2), (3, 1)])
    assert a == _table([(3, 1), (0, 2)]) and a != _table([(0, 2), (3, 2)]) and a != _table([(0, 2), (3, 1)], extend=5)
    assert a != BinCounts(500, 0, {"c": 3}, [0, 3], [2, 1], reads=2)
    with pytest.raises(ValueError):
        BinCounts(500, 0, {"c": 3}, [0, 0], [2, 1], reads=0)
    assert BinCounts.from_counts(500, 0, {"c": 5}, [0, 7, 0, 7, 9], 3) == BinCounts(500, 0, {"c": 5}, [0, 7, 9], [2, 2, 1], 3)


def test_table_round_trip(tmp_path):
    c = BinCounts(64, 200, {"f0": 1562, "f2": 1093}, [0, 1, 2, 5000, 70000], [2000, 500, 150, 4, 1], reads=123456)
    control = _table([(0, 5), (1, 5)])
    path = fingerprint.write_fingerprint(tmp_path / "x.y", "x.y", c)
    assert path.name == "x.y_fingerprint.tab" and sorted(os.listdir(tmp_path)) == ["x.y_fingerprint.tab"]
    name, back, block = fingerprint.read_fingerprint(path)
    assert name == "x.y" and back == c
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    labels = ["Name", "Bin size", "Extend", "Bins", "Reads", "Mean", "X-intercept", "AUC", "Synthetic AUC", "Elbow",
              "Synthetic JS distance"]
    assert [r[0] for r in rows[:11]] == labels
    assert rows[1:5] == [["Bin size", "64"], ["Extend", "200"], ["Bins", "2655"], ["Reads", "123456"]]
    assert (block["Mean"], block["X-intercept"], block["AUC"], block["Synthetic AUC"], block["Elbow"], block["Synthetic JS distance"]) \
        == (c.mean, c.x_intercept, c.auc, c.synthetic_auc, c.elbow, c.synthetic_jsd)        # repr: they read back exactly
    assert rows[11:14] == [["chrom", "bins"], ["f0", "1562"], ["f2", "1093"]]
    assert rows[14:] == [["count", "bins"], ["0", "2000"], ["1", "500"], ["2", "150"], ["5000", "4"], ["70000", "1"]]
    path = fingerprint.write_fingerprint(tmp_path / "x.y", "x.y", c, control, "input.bam")
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)]
    assert [r[0] for r in rows[:14]] == labels + ["Control", "Control mean", "JS distance"]
    name, back, block = fingerprint.read_fingerprint(path)
    assert back == c and (block["Control"], block["Control mean"], block["JS distance"]) == ("input.bam", 0.5, c.jsd_to(control))


def test_options(tmp_path, capsys):
    base = ["a.bam", "-d", "100"]
    a = cli.parse_args(base)
    assert (a.fingerprint, a.fingerprint_bin, a.fingerprint_extend, a.fingerprint_control) == (False, None, None, None)
    assert cli.parse_args(base + ["--fingerprint"]).fingerprint is True
    a = cli.parse_args(base + ["--fingerprint-bin", "64"])
    assert a.fingerprint is True and a.fingerprint_bin == 64
    a = cli.parse_args(base + ["--fingerprint-extend", "200"])
    assert a.fingerprint is True and a.fingerprint_extend == 200
    control = tmp_path / "input.bam"
    control.write_bytes(b"")
    a = cli.parse_args(base + ["--fingerprint-control", str(control)])
    assert a.fingerprint is True and a.fingerprint_control == control
    for bad in (["--fingerprint-bin", "0"], ["--fingerprint-extend", "0"], ["--fingerprint-bin", "-3"], ["--fingerprint-bin", "x"],
                ["--fingerprint-control", str(tmp_path / "none.bam")]):
        with pytest.raises(SystemExit) as ei:
            cli.parse_args(base + bad)
        assert ei.value.code == 2
        assert cli.main(base + bad) == 2
    assert "no such file" in capsys.readouterr().err
    assert "_fingerprint.tab" in cli.get_parser().format_help()


def test_options_reach_run_files(tmp_path, monkeypatch):
    seen = {}

    def run_files(paths, outdir, max_shift, **kw):
        seen.update(kw)
        return [pipeline.FileResult(p, "b", None, [], None) for p in paths]
    monkeypatch.setattr(pipeline, "run_files", run_files)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    control = tmp_path / "input.bam"
    control.write_bytes(b"")
    assert cli.main(["a.bam", "--skip-plots"]) == 0
    assert not any(k.startswith("fingerprint") for k in seen)
    seen.clear()
    assert cli.main(["a.bam", "--skip-plots", "--fingerprint-extend", "150", "--fingerprint-control", str(control)]) == 0
    assert {k: v for k, v in seen.items() if k.startswith("fingerprint")} == dict(fingerprint=True, fingerprint_extend=150,
                                                                                  fingerprint_control=str(control))


def _golden_want(mapq, bin_size, extend, names=None):
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, b.lengths))
        cols = [np.concatenate(x).tolist() for x in zip(*b.batches(mapq))]
    use = [1 if names is None or n in names else 0 for n, _l in refs]
    counts, added = FC.restate(list(zip(cols[0], cols[1], cols[2], [int(x) for x in cols[3]])), refs, use, bin_size, extend)
    return refs, use, FC.table(counts), added


def test_pipeline_writes_the_table_and_nothing_else_changes(tmp_path):
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, stats=True, complexity=True)
    _r0, w0 = pipeline.run(GOLDEN_BAM, str(tmp_path / "plain"), 120, context=FakeContext(), **kw)
    _r1, w1 = pipeline.run(GOLDEN_BAM, str(tmp_path / "with"), 120, context=FakeContext(), fingerprint=True, **kw)
    stem = "ENCFF000RMB-test"
    assert [p.name for p in w1] == [p.name for p in w0] + [stem + "_fingerprint.tab"] and len(w0) == 4
    for p in w0:
        assert p.read_bytes() == (tmp_path / "with" / p.name).read_bytes()
    assert sorted(os.listdir(tmp_path / "with")) == sorted(p.name for p in w1)
    name, c, block = fingerprint.read_fingerprint(w1[-1])
    refs, use, want, added = _golden_want(10, 500, 0)
    assert name == stem and (c.bin_size, c.extend, c.reads) == (500, 0, added) and added > 0
    assert list(zip(c.values.tolist(), c.bins.tolist())) == want
    assert c.per_reference == {n: l // 500 for n, l in refs}
    assert "Control" not in block and 0 < block["AUC"] < 0.5 and block["X-intercept"] > 0.9
    # other parameters, the chosen chromosomes, a control (the file itself: distance 0)
    chosen = [refs[0][0], refs[2][0]]
    _r2, w2 = pipeline.run(GOLDEN_BAM, str(tmp_path / "two"), 120, context=FakeContext(), references=chosen, fingerprint_bin=100_000,
                           fingerprint_extend=200, fingerprint_control=GOLDEN_BAM, **kw)
    _n, c2, block2 = fingerprint.read_fingerprint(w2[-1])
    refs, use, want2, added2 = _golden_want(10, 100_000, 200, chosen)
    assert list(c2.per_reference) == chosen and list(zip(c2.values.tolist(), c2.bins.tolist())) == want2 and c2.reads == added2
    assert (block2["Control"], block2["JS distance"], block2["Control mean"]) == (GOLDEN_BAM, 0.0, c2.mean)
    with BamReader(GOLDEN_BAM) as b:
        assert b.bin_counts(10, chosen, 100_000, 200) == c2
    with pytest.raises(ValueError):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, context=FakeContext(), fingerprint_bin=0, **kw)
    with pytest.raises(ValueError, match="no chosen reference is as long as one bin"):
        pipeline.run(GOLDEN_BAM, str(tmp_path / "bad"), 120, context=FakeContext(), fingerprint=True, fingerprint_bin=1 << 30, **kw)


def test_a_control_with_another_length_skips_the_sample(tmp_path, caplog):
    with BamReader(GOLDEN_BAM) as b:
        refs = list(zip(b.references, b.lengths))
        cols = [np.concatenate(x).tolist() for x in zip(*b.batches(10))]
    recs = [SW.rec("q%d" % i, 16 if s else 0, refs[r][0], p, 40, (("M", l),)) for i, (r, p, l, s) in enumerate(zip(*cols))]
    other = [(n, l + 1 if i == 0 else l) for i, (n, l) in enumerate(refs)]
    (tmp_path / "in").mkdir()
    _sam, same = SW.write_twins(tmp_path / "in", "same", refs, recs)
    _sam, longer = SW.write_twins(tmp_path / "in", "longer", other, recs)
    kw = dict(read_len=36, mapq_criteria=10, device_ingest=False, context=FakeContext(), fingerprint_control=GOLDEN_BAM)
    out = pipeline.run_files([longer, same], str(tmp_path / "out"), 120, **kw)
    assert isinstance(out[0].error, ValueError) and "fingerprint control" in str(out[0].error) and out[0].written == []
    assert out[1].error is None and out[1].written[-1].name == "same_fingerprint.tab"
    assert sorted(os.listdir(tmp_path / "out")) == sorted(p.name for p in out[1].written)       # the skipped file gets no table
    block = fingerprint.read_fingerprint(out[1].written[-1])[2]
    assert block["JS distance"] == 0.0 and block["Control"] == GOLDEN_BAM
    # the first chromosome left out: the chosen references match again
    rest = [n for n, _l in refs[1:]]
    out = pipeline.run_files([longer], str(tmp_path / "rest"), 120, references=rest, **kw)
    assert out[0].error is None and out[0].written[-1].name == "longer_fingerprint.tab"
    with pytest.raises(ValueError, match="fingerprint control"):
        pipeline.run(longer, str(tmp_path / "one"), 120, **kw)
