"""The fixtures of tests/chain_cases.py bite: for every case the rule of the device reader's record chain, restated in Python,
starts from wrong guesses and still closes to the true chain under every schedule, and the host reader (serial by construction)
returns the truth.  No GPU; tests/test_gpu_record_chain.py runs the same files through the device reader."""
import pytest

from pymasc_amd import bam as B
from tests import chain_cases as CC
from tests import io_writers as W


def _reads(reader, mapq, **kw):
    out = []
    for ref, pos, rl, rev in reader.batches(mapq, **kw):
        out += [(reader.references[a], int(p), int(l), bool(v)) for a, p, l, v in zip(ref, pos, rl, rev)]
    return out


@pytest.mark.parametrize("name", CC.CASES)
def test_the_serial_walk_finds_the_builders_truth(name):
    _refs, records, truth = CC.case(name)
    stream = b"".join(records)
    offsets, fields = CC.serial(stream)
    assert fields == truth
    at = 0
    for o, rec in zip(offsets, records):
        assert o == at
        at += len(rec)
    assert all(t[0] == 0 and t[2] == 36 and not t[3] and t[4] == 30 for t in truth)
    assert (len(stream) + CC.P - 1) // CC.P <= (34 if name in ("saturated", "pairs") else 11)
    if name == "pairs":
        assert [t[5] & 0x1 for t in truth].count(1) == len(CC.PAIR_SIZES)


def test_the_building_blocks():
    refs, records, _truth = CC.case("rejoin")
    assert sum(map(len, records)) == 5 * CC.P + 100
    host = CC.first_decoys("rejoin")[0] - CC.HOST_PREFIX
    assert host == 2 * CC.P - 20                           # a host record starts 20 bytes before a piece boundary
    stream = b"".join(records)
    for k in range(3):                                     # its decoys are byte-exact records, and they look like records
        at = host + CC.HOST_PREFIX + k * CC.DECOY_LEN
        assert stream[at:at + CC.DECOY_LEN] == CC.decoy(k) and CC.plausible(stream, at, len(stream), len(refs))
    for maker in (CC.decoy, CC.pair_decoy):
        (ref, pos1, qlen, rev, mapq, flag), = CC.serial(maker(3, 5))[1]
        assert (ref, pos1, qlen, rev, mapq) == (1, 7004, 50, True, 60) and bool(flag & 0x1) == (maker is CC.pair_decoy)
    for name in CC.CASES:                                  # decoy positions lie inside the header's reference
        assert 7000 + 500 + 50 <= dict(CC.case(name)[0])["decoy"]


@pytest.mark.parametrize("name", CC.CASES)
def test_the_model_closes_to_the_truth_from_wrong_guesses(name):
    refs, records, _truth = CC.case(name)
    s = CC.summary(name)
    line = "%-11s %7d %7d %7d %6d %7d" % (name, s["bytes"], s["pieces"], s["records"], len(s["wrong"]), len(s["missing"]))
    for schedule in CC.SCHEDULES:
        m = s["models"][schedule]
        assert m.starts == s["true_starts"], schedule
        assert m.records == len(records), schedule
        assert m.rounds <= s["pieces"] + 1, schedule
        assert m.rewalks >= s["off"], schedule             # every piece whose guess is not the true start is walked again
    print(line + "       %s           %s" % (" / ".join(str(s["models"][k].rounds) for k in CC.SCHEDULES),
                                             " / ".join(str(s["models"][k].rewalks) for k in CC.SCHEDULES)))
    want = CC.WRONG_GUESSES[name]
    if want is None:
        assert 4 * len(s["wrong"]) >= s["pieces"]
    else:
        assert len(s["wrong"]) == want
    assert s["off"] > 0


def test_each_wrong_walk_ends_as_its_case_says():
    """rejoin: on the chain, with a wrong count; bad: in WALK_BAD; overshoot: off the chain, two pieces on; fake_chain: the guesses
    agree with each other's wrong ends; every_piece: WALK_BAD behind the even pieces; to_the_end: the guess's next record is the
    stream's end."""
    def parts(name):
        refs, records, _t = CC.case(name)
        stream = b"".join(records)
        return stream, len(stream), len(refs), CC.summary(name), set(CC.serial(stream)[0]) | {len(stream)}

    D, N, nref, s, chain = parts("rejoin")
    g = s["models"]["last_round"].guesses
    end, n = CC.walk(D, N, nref, g[2], 2)
    true_end, true_n = CC.walk(D, N, nref, s["true_starts"][2], 2)
    assert g[2] == CC.first_decoys("rejoin")[0] and end == true_end and n == true_n + 3

    D, N, nref, s, chain = parts("bad")
    assert CC.walk(D, N, nref, s["models"]["last_round"].guesses[2], 2) == (CC.BAD, 2)

    D, N, nref, s, chain = parts("overshoot")
    end, n = CC.walk(D, N, nref, s["models"]["last_round"].guesses[2], 2)
    assert n == 2 and end // CC.P == 4 and end not in chain

    D, N, nref, s, chain = parts("fake_chain")
    g = s["models"]["last_round"].guesses
    assert s["wrong"] == [2, 3, 4, 5, 6]
    for c in (2, 3, 4, 5):
        assert CC.walk(D, N, nref, g[c], c)[0] == g[c + 1] and g[c + 1] not in chain
    assert s["models"]["last_round"].rounds >= 5           # repaired one piece per round

    D, N, nref, s, chain = parts("every_piece")
    g = s["models"]["last_round"].guesses
    assert s["wrong"] == list(range(1, 9))
    for c in range(1, 9):
        assert (CC.walk(D, N, nref, g[c], c)[0] == CC.BAD) == (c % 2 == 0)

    D, N, nref, s, chain = parts("to_the_end")
    g = s["models"]["last_round"].guesses
    assert g[3] == CC.first_decoys("to_the_end")[0] + CC.DECOY_LEN and g[3] + CC.DECOY_LEN == N

    for name in ("saturated", "pairs"):
        D, N, nref, s, chain = parts(name)
        g = s["models"]["last_round"].guesses
        ends = [CC.walk(D, N, nref, g[c], c)[0] for c in s["wrong"]]
        assert ends.count(CC.BAD) >= 2 and sum(e in chain for e in ends) >= 2


@pytest.mark.parametrize("name", CC.CASES)
def test_the_host_reader_returns_the_truth(tmp_path, name):
    refs, records, truth = CC.case(name)
    path = tmp_path / (name + ".bam")
    W.write_bam(path, refs, records, block=257 if name == "rejoin" else 0xff00)
    with B.BamReader(path) as h:
        assert list(zip(h.references, h.lengths)) == refs
        for mapq in (0, 40):
            got = _reads(h, mapq)
            assert got == CC.kept(truth, mapq)
            assert not any(r[0] == "decoy" or r[2] == 50 or r[3] for r in got)
        assert CC.kept(truth, 0) and not CC.kept(truth, 40)
    with B.BamReader(path) as h:
        assert len(_reads(h, 0)) == len(truth) and h.counters()["records"] == len(records)
        hist = h.read_length_histogram(0)
        assert hist.lengths.tolist() == [36] and hist.counters["nreads"] == len(records)


def test_the_broken_streams_break_where_they_should(tmp_path):
    refs, records = CC.to_the_end_cut()
    whole = b"".join(CC.case("to_the_end")[1])
    assert len(b"".join(records)) == len(whole)
    path = tmp_path / "cut.bam"
    W.write_bam(path, refs, records)
    with B.BamReader(path) as h:
        with pytest.raises(B.PmxIOError, match="file ends inside an alignment record"):
            _reads(h, 0)
    refs, records, k = CC.every_piece_bs7()
    assert sum(map(len, records[:k])) // CC.P == 6
    path = tmp_path / "bs7.bam"
    W.write_bam(path, refs, records)
    with B.BamReader(path) as h:
        with pytest.raises(B.PmxIOError, match="block_size < 32"):
            _reads(h, 0)
