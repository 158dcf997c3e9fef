"""The lifecycle of the side counts' state in a device handle: pmx_dbam_bincount_*, _peakcount_*, _coverage_*,
_gcbias_* and _fragments_* through the C ABI on a file handle and on a stream handle.  A begin that refuses its argument leaves
its own family without a table and the other four as they were; a begin after it starts from zero; a stream's peak counts the
tables the header documents; a handle is closed with all five tables held."""
import ctypes
import struct

import numpy as np
import pytest

from pymasc_amd.bam_device import DeviceBamReader
from pymasc_amd.gcbias import DeviceGenome
from pymasc_amd.native import PMX_BAM_DEFAULT_EXCLUDE, PMX_BINCOUNT_HIST, PmxIOError
from pymasc_amd.stream_device import DeviceStreamReader
from tests import io_writers as W

pytestmark = pytest.mark.gpu

REFS = [("sA", 5000), ("sB", 3001)]
FAMILIES = ("bincount", "peakcount", "coverage", "gcbias", "fragments")
BIN, GC_WINDOW, MAX_SIZE = 100, 50, 300
PEAKS = [[(100, 400), (350, 900), (4000, 5000)], [(0, 10), (1500, 1600)]]       # per reference, 0-based and half-open
INVALID = -3                                                                    # PMX_DBAM_ERR_INVALID
X = PMX_BAM_DEFAULT_EXCLUDE


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    d = tmp_path_factory.mktemp("gpu_side_state")
    rng = np.random.default_rng(11)
    recs, _meta = W.synth_bam_records(rng, REFS, 180, mapq_lo=20)
    for i in range(0, len(recs), 3):                # every third record becomes the read1 of an FR pair of 150 bases
        r = bytearray(recs[i])
        ref, pos0 = struct.unpack_from("<ii", r, 4)
        struct.pack_into("<H", r, 18, 0x1 | 0x2 | 0x20 | 0x40)
        struct.pack_into("<iii", r, 24, ref, pos0 + 114, 150)
        recs[i] = bytes(r)
    bam, fasta = str(d / "reads.bam"), str(d / "genome.fa")
    W.write_bam(bam, REFS, recs, block=4096)
    with open(fasta, "w") as fh:
        for name, length in REFS:
            fh.write(">{}\n{}\n".format(name, "".join("ACGT"[k] for k in rng.integers(0, 4, size=length))))
    return dict(bam=bam, fasta=fasta)


@pytest.fixture(scope="module")
def genome(case):
    with DeviceGenome(case["fasta"]) as g:
        yield g


class Calls:
    """begin / add / total of every family on one handle, straight through the library."""

    def __init__(self, reader, genome):
        self.r, self.L, self.h, self.genome = reader, reader._L, reader._h, genome
        self.nref = self.L.pmx_dbam_nref(self.h)
        self.offsets = np.cumsum([0] + [len(p) for p in PEAKS]).astype(np.int64)
        self.pb = np.array([b for p in PEAKS for b, _e in p], dtype=np.uint32)
        self.pe = np.array([e for p in PEAKS for _b, e in p], dtype=np.uint32)
        self.none = np.zeros(self.nref, dtype=np.uint8)

    def begin(self, family, valid=True):
        L, h = self.L, self.h
        if family == "bincount":
            return L.pmx_dbam_bincount_begin(h, BIN if valid else 0, 0, None)
        if family == "peakcount":
            return L.pmx_dbam_peakcount_begin(h, self.nref if valid else self.nref + 1, self.offsets.ctypes.data, self.pb.ctypes.data,
                                              self.pe.ctypes.data, 0, None)
        if family == "coverage":
            return L.pmx_dbam_coverage_begin(h, 0, None if valid else self.none.ctypes.data)
        if family == "gcbias":
            return L.pmx_dbam_gcbias_begin(h, self.genome._h, GC_WINDOW if valid else 0, None)
        return L.pmx_dbam_fragments_begin(h, MAX_SIZE if valid else 0, None)

    def add(self, family):
        """(return code, the reads or rows the call counted)"""
        out = (ctypes.c_uint64 * 3)()
        rc = getattr(self.L, "pmx_dbam_{}_add".format(family))(self.h, 0, X, out)
        return rc, int(out[0])

    def total(self, family):
        """What the family has counted since its begin (coverage: by finish, which ends its table)."""
        L, h = self.L, self.h
        t = np.zeros(max(PMX_BINCOUNT_HIST, 3 * MAX_SIZE, GC_WINDOW + 1), dtype=np.uint64)
        tot = np.zeros(10, dtype=np.uint64)
        if family == "bincount":
            rc, k = L.pmx_dbam_bincount_hist(h, t.ctypes.data, tot.ctypes.data, 0, None), 2
        elif family == "peakcount":
            rc, k = L.pmx_dbam_peakcount_totals(h, tot.ctypes.data, t.ctypes.data), 0
        elif family == "coverage":
            rc, k = L.pmx_dbam_coverage_finish(h, tot.ctypes.data), 0
        elif family == "gcbias":
            rc, k = L.pmx_dbam_gcbias_tables(h, t.ctypes.data, t.ctypes.data, 0, tot.ctypes.data), 1       # (sum F: the reads placed)
        else:
            rc, k = L.pmx_dbam_fragments_tables(h, t.ctypes.data, tot.ctypes.data), 8       # (`rows`)
        assert rc >= 0, self.L.pmx_dbam_last_error()
        return int(tot[k])

    def no_table(self, family):
        rc, _n = self.add(family)
        assert rc == INVALID
        with pytest.raises(PmxIOError, match="pmx_dbam_{0}_add: no table: call pmx_dbam_{0}_begin first".format(family)):
            self.r._raise(rc)


def documented_bytes():
    """The device bytes the header documents for the five tables begun by Calls.begin, a lower bound."""
    bins = sum(length // BIN for _n, length in REFS)
    lines = sum(len(p) for p in PEAKS)
    slots = sum(length + 1 for _n, length in REFS)
    return 4 * bins + 28 * lines + 4 * slots + 16 * ((slots + 63) // 64) + 24 * MAX_SIZE


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("kind", ["file", "stream"])
def test_a_refused_begin_clears_its_own_family_only(case, genome, kind, family):
    reader = DeviceBamReader(case["bam"]) if kind == "file" else DeviceStreamReader(case["bam"], window_bytes=4096)
    with reader as r:
        c = Calls(r, genome)
        if kind == "stream":
            assert c.L.pmx_dbam_stream_next(c.h) > 0
            before = r.stream_info()["peak_device_bytes"]
        for f in FAMILIES:
            c.no_table(f)
        # 1. begin, then add
        first = {}
        for f in FAMILIES:
            assert c.begin(f) == 0, c.L.pmx_dbam_last_error()
            rc, first[f] = c.add(f)
            assert rc == 0 and first[f] > 0
        if kind == "stream":                        # 4. the peak counts the five tables
            assert r.stream_info()["peak_device_bytes"] >= before + documented_bytes()
        # 2. a begin that refuses its argument: no table of its own, the other four as they were
        assert c.begin(family, valid=False) == INVALID
        c.no_table(family)
        others = [f for f in FAMILIES if f != family]
        for f in others:
            assert c.add(f) == (0, first[f])
            assert c.total(f) == 2 * first[f]
        assert c.begin("coverage") == 0             # (its total is read by finish)
        # 3. begin again: the totals start from zero
        assert c.begin(family) == 0
        assert c.total(family) == 0
        if family == "coverage":
            assert c.begin(family) == 0
        assert c.add(family) == (0, first[family])
        if kind == "stream":                        # the tables outlive the window they were begun in
            assert c.L.pmx_dbam_stream_next(c.h) > 0
            for f in FAMILIES:
                assert c.add(f)[0] == 0
        # 5. closed with all five tables held
        for f in FAMILIES:
            assert c.add(f)[0] == 0
