"""The host SAM reader opened for its header only (pmx_sam_open_header): the references, lengths and header text of the full
open, from plain and BGZF text -- a header that spans many BGZF members and more than the first inflated megabyte included --
the same header errors, and no record: the calls that read records refuse such a handle."""
import os

import numpy as np
import pytest

from pymasc_amd import inputs
from pymasc_amd.bam import PmxIOError
from pymasc_amd.sam import SamReader
from tests import io_writers as W
from tests import sam_cases as SC
from tests import sam_writers as SW


def _same(path):
    with SamReader(path) as full, SamReader(path, header_only=True) as head:
        assert head.references == full.references and head.lengths == full.lengths
        assert head.header_text == full.header_text
        with pytest.raises(PmxIOError, match="header only"):
            head.read_length_histogram(0)
        with pytest.raises(PmxIOError, match="header only"):
            next(iter(head.batches(0)))
    return head.references


@pytest.mark.parametrize("block", [300, 0xff00])
def test_header_only_equals_the_full_open(tmp_path, block):
    refs = [("c%d" % i, 10000 + i) for i in range(1, 6)]
    recs = SW.synth_records(np.random.default_rng(1), refs, 200)
    paths = SW.write_twins(tmp_path, "s", refs, recs, bgzf_block=block)
    assert _same(paths[0]) == tuple(n for n, _l in refs)
    assert _same(paths[2]) == tuple(n for n, _l in refs)


def test_golden_sam_gz():
    assert len(_same(SC.GOLDEN_SAM_GZ)) > 1


def test_a_header_longer_than_the_first_inflated_megabyte(tmp_path):
    """40,000 @SQ lines (about 1.3 MB of header) in 4-KB BGZF members: the prefix grows until the first record line."""
    refs = [("chrUn_%06d" % i, 1000 + i) for i in range(40000)]
    recs = [SW.rec(rname=refs[-1][0], pos=5)]
    _sam, _bam, gz = SW.write_twins(tmp_path, "big", refs, recs, bgzf_block=4096)
    assert len(SW.sam_header(refs)) > 1 << 20
    assert len(_same(gz)) == 40000
    # a file that is all header (no record line)
    whole = str(tmp_path / "only.sam.gz")
    with open(whole, "wb") as fh:
        fh.write(W.bgzf_compress(SW.sam_header(refs).encode(), 4096))
    assert len(_same(whole)) == 40000


@pytest.mark.parametrize("name", ["no_sq", "sq_without_ln", "sq_without_sn", "sq_ln_zero", "sq_ln_big", "sq_duplicate"])
@pytest.mark.parametrize("gz", [False, True])
def test_header_errors_are_those_of_the_full_open(tmp_path, name, gz):
    text = SC.malformed_cases()[name][0].encode()
    path = str(tmp_path / ("bad.sam.gz" if gz else "bad.sam"))
    with open(path, "wb") as fh:
        fh.write(W.bgzf_compress(text) if gz else text)
    with pytest.raises(PmxIOError) as full:
        SamReader(path)
    with pytest.raises(PmxIOError) as head:
        SamReader(path, header_only=True)
    assert (head.value.code, str(head.value)) == (full.value.code, str(full.value))


def test_a_record_error_is_not_seen_by_the_header(tmp_path):
    text, _line, _word = SC.malformed_cases()["error_in_last_of_many"]
    path = str(tmp_path / "late.sam")
    with open(path, "wb") as fh:
        fh.write(text.encode())
    with pytest.raises(PmxIOError):
        SamReader(path)
    with SamReader(path, header_only=True) as head:
        assert head.references == ("c1", "c2")


def test_open_header_takes_the_header_only_reader_for_sam(tmp_path, monkeypatch):
    refs = [("c1", 5000)]
    sam, bam, gz = SW.write_twins(tmp_path, "t", refs, [SW.rec(pos=5)], bgzf_block=0xff00)
    for p in (sam, gz):
        with inputs.open_header(p) as r:
            assert isinstance(r, SamReader) and r.references == ("c1",)
            with pytest.raises(PmxIOError, match="header only"):
                r.read_length_histogram(0)
    with inputs.open_header(bam) as r:
        assert r.references == ("c1",) and not os.path.exists(bam + ".bai")
