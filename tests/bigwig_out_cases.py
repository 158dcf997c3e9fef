"""Cases and the two yardsticks of the bigWig output tests (tests/test_coverage_bigwig.py, tests/test_gpu_coverage_bigwig.py;
DESIGN.md 7.18.1).

``read_file`` is a reader of the written file in ``struct`` and nothing else: it shares no code with tests/io_writers.py, with the
package's writer or with the project's readers, and asserts the file's structure while it reads.  ``restate_zoom`` and
``restate_summary`` state the zoom levels and the total summary as Python loops over a per-base depth list, which ``depth_lists``
fills base by base from the runs of ``coverage_cases.restate``; no numpy reduction and not the package's numpy twin.  An integer
becomes a float32 by ``np.float32(np.uint64(x))`` (round to nearest even).

The definitions: level ``k`` has the reduction ``z_k = z_0 * 4^k``; bin ``j`` of a reference covers ``[j * z, min((j + 1) * z, len))``;
a bin with a covered base (depth > 0) gives the record (id, start, end, covered bases, min, max, sum, sum of squares of the depth over
those bases); ``z_0`` is ``zoom_base`` or the smallest power of two that is at least ``10 * covered_bases / runs`` and 32; levels
exist for ``k < 10`` while ``z_k <= longest chosen length / 2``; no run: no level.  A chromosome's id is the rank of its name in
bytewise order.
"""
import struct
import zlib

import numpy as np

from tests import coverage_cases as CC

FC = CC.FC
# coverage_cases' library under names whose bytewise order (c, chr10, chr2, chrX_alt) is not the header's, of several lengths
RENAME = {"f0": "chr2", "f1": "chr10", "f2": "chrX_alt", "f3": "c"}
REFS = [(RENAME[n], l) for n, l in CC.REFS]
MASK = {RENAME[n]: v for n, v in CC.MASK.items()}
NAMES = [n for n, _l in REFS]
LENGTHS = [l for _n, l in REFS]

# The small case: written with 4 items per section and 3 per index node, and zoom_base 32 where the bin counts below matter.
SMALL_ITEMS, SMALL_BLOCK, SMALL_Z = 4, 3, 32
SMALL_REFS = [("s4", 128), ("s5x", 150), ("a3", 200), ("m12", 3000), ("B13long", 5000), ("tiny", 20), ("z_empty", 700), ("left_out", 300)]
SMALL_USE = [1, 1, 1, 1, 1, 1, 1, 0]


def small_reads():
    """Rows (ref, pos1, read_len, reverse), forward and apart, so that every read is a run ``[pos1 - 1, pos1 - 1 + read_len)``."""
    rows = [(0, 1, 10, 0), (0, 23, 10, 0), (0, 65, 8, 0), (0, 91, 10, 0)]               # s4: 4 runs; ends on 31, begins on 64, crosses 96
    rows += [(1, 6, 10, 0), (1, 21, 10, 0), (1, 41, 10, 0), (1, 71, 10, 0), (1, 141, 10, 0)]   # s5x: 5 runs, the last on its last base
    rows += [(2, 31, 100, 0), (2, 151, 10, 0), (2, 191, 10, 0)]                         # a3: 3 runs; [30, 130) holds bins 1, 2 and 3 whole
    rows += [(3, 51 + 60 * i, 20, 0) for i in range(48)]                                # m12: 48 runs = 12 sections of 4
    for i in range(49):                                                                 # B13long: 49 runs = 13 sections, depth 2 on every fifth
        rows += [(4, 8 + 100 * i, 30, 0)] * (2 if i % 5 == 0 else 1)
    rows += [(5, 4, 10, 0), (7, 11, 36, 0)]                                             # tiny; left_out (not chosen)
    return sorted(rows)


def check_small(want, z0=SMALL_Z):
    """The planted situations of the small case, asserted from the restatement of its runs."""
    runs = want["runs"]
    assert [len(runs[n]) for n in ("s4", "s5x", "a3")] == [4, 5, 3]
    assert len(runs["m12"]) == SMALL_ITEMS * SMALL_BLOCK * 4 and len(runs["B13long"]) == SMALL_ITEMS * SMALL_BLOCK * 4 + 1
    assert -(-len(runs["m12"]) // SMALL_ITEMS) == 4 * SMALL_BLOCK and -(-len(runs["B13long"]) // SMALL_ITEMS) == 4 * SMALL_BLOCK + 1
    assert (22, z0, 1) in runs["s4"] and (2 * z0, 72, 1) in runs["s4"]                  # ends on a bin's last base; begins on a bin's first
    assert (90, 100, 1) in runs["s4"] and 90 < 3 * z0 < 100                             # across one bin edge
    s, e, _d = runs["a3"][0]
    assert s < z0 and e > 4 * z0 and (e - 1) // z0 - s // z0 == 4                       # bins 1, 2 and 3 whole
    lengths = dict(SMALL_REFS)
    assert lengths["tiny"] < z0                                                         # its one bin is clipped to its length
    assert [-(-lengths[n] // z0) for n in ("tiny", "s4", "s5x", "a3")] == [1, 4, 5, 7]  # the fold's short last groups
    assert runs["s5x"][-1][1] == lengths["s5x"] and runs["a3"][-1][1] == lengths["a3"]  # a run on the last base
    assert "z_empty" not in runs and "left_out" not in runs
    assert {d for _s, _e, d in runs["B13long"]} == {1, 2}


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------------------------------------------

def depth_lists(want, refs, use):
    """{name: [depth of base 0, 1, ...]} of the chosen references, filled base by base from the restated runs."""
    out = {}
    for (name, length), u in zip(refs, use):
        if not u:
            continue
        row = [0] * length
        for s, e, d in want["runs"].get(name, []):
            for p in range(s, e):
                row[p] = d
        out[name] = row
    return out


def chrom_ids(names):
    """{name: id}: the rank in bytewise order."""
    return {n: i for i, n in enumerate(sorted(names, key=lambda n: n.encode()))}


def reductions(depths, zoom_base=None):
    """[z_0, z_1, ...] of the levels that exist."""
    covered = sum(1 for row in depths.values() for d in row if d > 0)
    runs = sum(1 for row in depths.values() for p, d in enumerate(row) if d > 0 and (p == 0 or row[p - 1] != d))
    if not runs:
        return []
    z0 = zoom_base
    if z0 is None:
        z0 = 32
        while z0 * runs < 10 * covered:
            z0 *= 2
    longest = max(len(row) for row in depths.values())
    return [z0 * 4 ** k for k in range(10) if z0 * 4 ** k <= longest / 2]


def f32(x) -> bytes:
    return np.float32(np.uint64(x)).tobytes()


def restate_zoom(depths, z):
    """The records of the level of reduction ``z`` in file order, each as the 32 bytes the file holds."""
    ids = chrom_ids(depths)
    out = []
    for name in sorted(depths, key=lambda n: ids[n]):
        row = depths[name]
        for lo in range(0, len(row), z):
            hi = min(lo + z, len(row))
            n = total = squares = high = 0
            low = None
            for p in range(lo, hi):
                d = row[p]
                if d > 0:
                    n += 1
                    total += d
                    squares += d * d
                    high = max(high, d)
                    low = d if low is None else min(low, d)
            if n:
                out.append(struct.pack("<IIII", ids[name], lo, hi, n) + f32(low) + f32(high) + f32(total) + f32(squares))
    return out


def restate_summary(depths) -> bytes:
    """The 40 bytes of the total summary."""
    n = total = squares = high = 0
    low = None
    for row in depths.values():
        for d in row:
            if d > 0:
                n += 1
                total += d
                squares += d * d
                high = max(high, d)
                low = d if low is None else min(low, d)
    return struct.pack("<Qdddd", n, float(low or 0), float(high), float(total), float(squares))


# ---------------------------------------------------------------------------------------------------------------------------------
# the reader
# ---------------------------------------------------------------------------------------------------------------------------------

MAGIC, CHROM_MAGIC, INDEX_MAGIC = 0x888FFC26, 0x78CA8C91, 0x2468ACE0


def _chrom_tree(blob, at):
    magic, block, key, val, count, _r = struct.unpack_from("<IIIIQQ", blob, at)
    assert magic == CHROM_MAGIC and block == 256 and val == 8 and count >= 1
    items, last = [], [at + 32]

    def walk(node, depth):
        assert depth < 8 and at < node < len(blob)
        leaf, _r, n = struct.unpack_from("<BBH", blob, node)
        assert 1 <= n <= block
        p = node + 4
        for _ in range(n):
            name = blob[p:p + key]
            if leaf:
                items.append((name,) + struct.unpack_from("<II", blob, p + key))
            else:
                child, = struct.unpack_from("<Q", blob, p + key)
                assert child > node                         # children after parents
                before = len(items)
                walk(child, depth + 1)
                assert items[before][0] == name             # an inner key is its child's first
            p += key + 8
        last[0] = max(last[0], p)
    walk(at + 32, 0)
    end = last[0]
    assert len(items) == count
    keys = [k for k, _i, _l in items]
    assert all(a < b for a, b in zip(keys, keys[1:]))       # strictly ascending, bytewise
    assert [i for _k, i, _l in items] == list(range(count))
    assert key == max(len(k.rstrip(b"\0")) for k in keys) and all(k.rstrip(b"\0") + b"\0" * (key - len(k.rstrip(b"\0"))) == k for k in keys)
    return [(k.rstrip(b"\0").decode(), i, l) for k, i, l in items], end


def _index(blob, at, block_want):
    """The leaf items (c0, s0, c1, e1, offset, size) of the R-tree at ``at``, in order; the header; where the index ends."""
    magic, block, count, c0, s0, c1, e1, end_off, per_slot, _r = struct.unpack_from("<IIQIIIIQII", blob, at)
    assert magic == INDEX_MAGIC and block == block_want
    leaves = []
    last = [at + 48]

    def walk(node, depth):
        """Returns the node's bounds ((c0, s0), (c1, e1)) from its items."""
        assert depth < 16 and at < node < len(blob)
        leaf, _r, n = struct.unpack_from("<BBH", blob, node)
        assert n <= block and (n >= 1 or (leaf and count == 0))
        p = node + 4
        lo, hi = None, (0, 0)
        for _ in range(n):
            a, b, c, d, off = struct.unpack_from("<IIIIQ", blob, p)
            if leaf:
                size, = struct.unpack_from("<Q", blob, p + 24)
                leaves.append((a, b, c, d, off, size))
                p += 32
            else:
                assert off > node                           # children after parents
                got = walk(off, depth + 1)
                assert got == ((a, b), (c, d))              # an inner item's bounds cover its children, and tightly
                p += 24
            lo = (a, b) if lo is None else lo
            assert lo <= (a, b)
            hi = max(hi, (c, d))
        last[0] = max(last[0], p)
        return lo or (0, 0), hi
    lo, hi = walk(at + 48, 0)
    assert len(leaves) == count and (lo, hi) == ((c0, s0), (c1, e1))
    assert all(a[:2] < b[:2] for a, b in zip(leaves, leaves[1:]))       # (id, start) order
    return leaves, per_slot, last[0]


def _sections(blob, leaves, first, end, inflate):
    """The raw bytes of every section, which together tile ``[first, end)`` of the file: each is reached exactly once."""
    at = first
    out = []
    for _a, _b, _c, _d, off, size in leaves:
        assert off == at and size > 0
        at += size
        raw = blob[off:off + size]
        if inflate:
            raw = zlib.decompress(raw)
            assert len(raw) <= inflate
        out.append(raw)
    assert at == end
    return out


def read_file(path, index_block=256):
    """dict(chroms=[(name, id, length)], runs={name: [(start0, end0, depth float)]}, sections=[items per data section],
    zooms=[(reduction, [32-byte records])], summary=40 bytes, compressed, largest=the largest raw section)."""
    blob = open(path, "rb").read()
    (magic, version, levels, tree_at, data_at, index_at, fields, defined, sql_at, summary_at, inflate, ext_at) = struct.unpack_from(
        "<IHHQQQHHQQIQ", blob, 0)
    assert magic == MAGIC and version == 4 and struct.unpack_from("<I", blob, len(blob) - 4)[0] == MAGIC
    assert (fields, defined, sql_at, ext_at) == (0, 0, 0, 0) and levels <= 10
    heads = [struct.unpack_from("<IIQQ", blob, 64 + 24 * k) for k in range(levels)]
    assert summary_at == 64 + 24 * levels and tree_at == summary_at + 40
    chroms, tree_end = _chrom_tree(blob, tree_at)
    assert tree_end == data_at                              # the layout: nothing between the parts
    order = [summary_at, tree_at, data_at, index_at] + [x for _z, _r, d, i in heads for x in (d, i)] + [len(blob) - 4]
    assert all(a < b for a, b in zip(order, order[1:])) and all(_r == 0 for _z, _r, _d, _i in heads)
    name_of = {i: n for n, i, _l in chroms}
    length_of = {i: l for _n, i, l in chroms}
    n_sections, = struct.unpack_from("<Q", blob, data_at)
    leaves, _per, index_end = _index(blob, index_at, index_block)
    assert len(leaves) == n_sections
    runs, counts, largest = {}, [], 0
    for leaf, raw in zip(leaves, _sections(blob, leaves, data_at + 8, index_at, inflate)):
        cid, start, end, step, span, kind, _r, n = struct.unpack_from("<IIIIIBBH", raw, 0)
        assert (step, span, kind, _r) == (0, 0, 1, 0) and len(raw) == 24 + 12 * n and n >= 1
        assert leaf[:4] == (cid, start, cid, end)           # the leaf's bounds are its section's header
        items = [struct.unpack_from("<IIf", raw, 24 + 12 * k) for k in range(n)]
        assert items[0][0] == start and items[-1][1] == end and end <= length_of[cid]
        assert all(a[1] <= b[0] for a, b in zip(items, items[1:])) and all(s < e for s, e, _v in items)
        runs.setdefault(name_of[cid], []).extend(items)
        counts.append(n)
        largest = max(largest, len(raw))
    at = index_end
    zooms = []
    for z, _r, zdata, zindex in heads:
        assert zdata == at                                  # a level begins where the part in front of it ends
        n_rec, = struct.unpack_from("<I", blob, zdata)
        zleaves, _per, at = _index(blob, zindex, index_block)
        recs = []
        for leaf, raw in zip(zleaves, _sections(blob, zleaves, zdata + 4, zindex, inflate)):
            assert len(raw) % 32 == 0
            part = [raw[a:a + 32] for a in range(0, len(raw), 32)]
            a, b = struct.unpack_from("<III", part[0]), struct.unpack_from("<III", part[-1])
            assert leaf[:4] == (a[0], a[1], b[0], b[2])
            recs += part
            largest = max(largest, len(raw))
        assert len(recs) == n_rec
        keys = [struct.unpack_from("<III", r) for r in recs]
        assert all(x[:2] < y[:2] for x, y in zip(keys, keys[1:]))
        assert all(s % z == 0 and e == min(s + z, length_of[c]) for c, s, e in keys)
        zooms.append((z, recs))
    assert at == len(blob) - 4
    assert all(a[0] * 4 == b[0] for a, b in zip(zooms, zooms[1:]))
    assert inflate == 0 or inflate == largest
    return dict(chroms=chroms, runs=runs, sections=counts, zooms=zooms, summary=blob[summary_at:summary_at + 40], compressed=inflate > 0,
                largest=largest)


def check_file(got, want, refs, use, depths, zoom_base=None, items=1024):
    """What ``read_file`` read against the restatement: the chromosomes, every run, the packing, the zoom levels and the total
    summary, the last two as bytes."""
    chosen = [(n, l) for (n, l), u in zip(refs, use) if u]
    ids = chrom_ids([n for n, _l in chosen])
    assert got["chroms"] == sorted(((n, ids[n], l) for n, l in chosen), key=lambda x: x[1])
    assert got["runs"] == {n: [(s, e, float(d)) for s, e, d in v] for n, v in sorted(want["runs"].items(), key=lambda x: ids[x[0]])}
    assert list(got["runs"]) == sorted(want["runs"], key=lambda n: ids[n])
    packing = [min(items, len(v) - a) for _n, v in sorted(want["runs"].items(), key=lambda x: ids[x[0]]) for a in range(0, len(v), items)]
    assert got["sections"] == packing                       # full sections, a reference's last one shorter, none with two references
    zs = reductions(depths, zoom_base)
    assert [z for z, _r in got["zooms"]] == zs
    for z, recs in got["zooms"]:
        assert recs == restate_zoom(depths, z)
    assert got["summary"] == restate_summary(depths)
