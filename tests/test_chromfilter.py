"""PyMaSC's -i / -e chromosome filter (utils/calc.py filter_chroms, reader/bam.py apply_chromfilter) as
pymasc_amd.chromfilter.filter_references.  The expected values are worked out by hand from those semantics: consecutive
groups of one kind act as one, an include group narrows the current set, an exclude group keeps the current names it does not
match and continues with the ones it does, a final include group keeps the current set; header order."""
import pytest

from pymasc_amd.chromfilter import NoTargetChromosomesError, filter_references

HEADER = ["chr1", "chr2", "chr10", "chr11", "chrX", "chrY", "chrM", "chr1_random", "chrUn_gl000220"]


def test_no_filter_keeps_everything_in_header_order():
    assert filter_references(HEADER, None) == HEADER
    assert filter_references(HEADER, []) == HEADER


def test_include_only_narrows():
    assert filter_references(HEADER, [(True, ["chr1*"])]) == ["chr1", "chr10", "chr11", "chr1_random"]
    assert filter_references(HEADER, [(True, ["chrX", "chr2"])]) == ["chr2", "chrX"]      # header order, not pattern order


def test_exclude_only_removes():
    assert filter_references(HEADER, [(False, ["*_*", "chrM"])]) == ["chr1", "chr2", "chr10", "chr11", "chrX", "chrY"]


def test_include_then_exclude():
    # include chr1*: {chr1, chr10, chr11, chr1_random}; exclude *_random keeps the three others
    assert filter_references(HEADER, [(True, ["chr1*"]), (False, ["*_random"])]) == ["chr1", "chr10", "chr11"]


def test_exclude_then_include_takes_some_back():
    # exclude chr1*: keeps every other name; the include group then takes chr10 back from the excluded ones
    got = filter_references(HEADER, [(False, ["chr1*"]), (True, ["chr10"])])
    assert got == ["chr2", "chr10", "chrX", "chrY", "chrM", "chrUn_gl000220"]


def test_consecutive_groups_of_one_kind_are_merged():
    one = filter_references(HEADER, [(True, ["chrX"]), (True, ["chrY"]), (False, ["chrY"])])
    assert one == ["chrX"]
    assert one == filter_references(HEADER, [(True, ["chrX", "chrY"]), (False, ["chrY"])])
    # two exclude groups in a row are one exclude group (not exclude, take back nothing, exclude again)
    assert filter_references(HEADER, [(False, ["chrM"]), (False, ["chrY"])]) == filter_references(HEADER, [(False, ["chrM", "chrY"])])


def test_three_alternating_groups():
    # include chr?: {chr1, chr2, chrX, chrY, chrM}; exclude chr[XYM]: keeps {chr1, chr2}, continues with {chrX, chrY, chrM};
    # include chrX: {chrX} is kept too
    got = filter_references(HEADER, [(True, ["chr?"]), (False, ["chr[XYM]"]), (True, ["chrX"])])
    assert got == ["chr1", "chr2", "chrX"]


def test_glob_forms_and_case():
    assert filter_references(HEADER, [(True, ["chr[!0-9]"])]) == ["chrX", "chrY", "chrM"]
    assert filter_references(HEADER, [(True, ["chr1?"])]) == ["chr10", "chr11"]
    with pytest.raises(NoTargetChromosomesError):
        filter_references(HEADER, [(True, ["CHR1"])])                 # case-sensitive


def test_empty_result_raises_value_error():
    with pytest.raises(ValueError):
        filter_references(HEADER, [(True, ["nothing*"])])
    with pytest.raises(NoTargetChromosomesError):
        filter_references(HEADER, [(False, ["*"])])


def test_run_sharded_refuses_references_and_filter_together(tmp_path):
    from pymasc_amd import sharding
    with pytest.raises(ValueError):
        sharding.run_sharded(str(tmp_path / "none.bam"), 50, 36, 10, references=["c1"], chromfilter=[(True, ["c1"])])


def test_filter_on_host_run_equals_references(tmp_path):
    """The filter picks the chromosomes; the run is the one of ``references`` set to them (host stand-in, no GPU)."""
    import numpy as np
    from pymasc_amd import sharding, tables
    from . import io_writers as W
    from .fake_context import FakeContext
    rng = np.random.default_rng(3)
    refs = [("c1", 20000), ("c2", 15000), ("x1", 12000)]
    recs, meta = W.synth_bam_records(rng, refs, 300)
    path = str(tmp_path / "f.bam")
    W.write_bam_indexed(path, refs, recs, [int(x) for x in meta[:, 0]], block=0x1000)
    a = sharding.run_sharded(path, 60, 36, 10, chromfilter=[(True, ["c*"]), (False, ["c2"])], context=FakeContext())
    b = sharding.run_sharded(path, 60, 36, 10, references=["c1"], context=FakeContext())
    assert list(a.chroms) == ["c1"]
    pa = tables.write_tables(tmp_path / "a.bam", a)
    pb = tables.write_tables(tmp_path / "b.bam", b)
    assert [open(p, "rb").read() for p in pa] == [open(p, "rb").read() for p in pb]
    with pytest.raises(ValueError):
        sharding.run_sharded(path, 60, 36, 10, chromfilter=[(False, ["*"])], context=FakeContext())
