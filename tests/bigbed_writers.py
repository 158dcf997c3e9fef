"""TEST INFRASTRUCTURE: a bigBed writer from the published bbi layout (Kent et al. 2010, Bioinformatics 26:2204, supplement),
for the bigBed reader tests and the ingest benchmark (bedToBigBed is not installed).  The chromosome B+ tree is
io_writers._bpt's; records are packed with numpy so that inputs of millions of records build in seconds.  It knows nothing
about the readers.

A record is  chromId u32, chromStart u32, chromEnd u32, rest of the BED line (tab-separated, no chrom/start/end), NUL.
"""
import struct
import zlib

import numpy as np

from . import io_writers as W

BIGBED_MAGIC = 0x8789F2EB


def _rests(rests, n):
    """(lengths, blob) of the rest strings: one bytes for every record, a list of bytes, or (lengths, blob) already."""
    if isinstance(rests, (bytes, bytearray)):
        return np.full(n, len(rests), dtype=np.int64), bytes(rests) * n
    if isinstance(rests, tuple):
        lens, blob = rests
        return np.asarray(lens, dtype=np.int64), bytes(blob)
    rests = list(rests)
    assert len(rests) == n
    return np.fromiter((len(r) for r in rests), dtype=np.int64, count=n), b"".join(rests)


def pack_records(cid, starts, ends, rests) -> tuple:
    """The records as one byte string and the offset of each record in it (plus the end): (bytes, offsets[n + 1])."""
    n = len(starts)
    lens, blob = _rests(rests, n)
    assert int(lens.sum()) == len(blob)
    assert b"\0" not in blob
    size = 13 + lens
    offs = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(size, out=offs[1:])
    buf = np.zeros(int(offs[-1]), dtype=np.uint8)
    head = np.empty((n, 3), dtype="<u4")
    head[:, 0] = cid
    head[:, 1] = starts
    head[:, 2] = ends
    hb = head.view(np.uint8).reshape(n, 12)
    idx = offs[:-1, None] + np.arange(12)
    buf[idx.ravel()] = hb.ravel()
    if len(blob):
        rstart = np.zeros(n, dtype=np.int64)
        np.cumsum(lens[:-1], out=rstart[1:])
        pos = np.repeat(offs[:-1] + 12 - rstart, lens) + np.arange(len(blob))
        buf[pos] = np.frombuffer(blob, dtype=np.uint8)
    return buf.tobytes(), offs


def _rtree(leaves, index_off, rtree_block, items_per_block):
    """R-tree index bytes (48-byte header + nodes laid out top-down, children after parents), as bedToBigBed writes it."""
    levels = [[leaves[i:i + rtree_block] for i in range(0, len(leaves), rtree_block)] or [[]]]
    while len(levels[-1]) > 1:
        prev = levels[-1]
        levels.append([list(range(i, min(i + rtree_block, len(prev)))) for i in range(0, len(prev), rtree_block)])

    def bounds(li, ni):
        if li == 0:
            items = levels[0][ni]
            if not items:
                return (0, 0, 0, 0)
            return (items[0][0], items[0][1], items[-1][2], max(x[3] for x in items if x[2] == items[-1][2]))
        kids = [bounds(li - 1, k) for k in levels[li][ni]]
        return (kids[0][0], kids[0][1], kids[-1][2], kids[-1][3])

    order, sizes = [], {}
    for li in range(len(levels) - 1, -1, -1):
        for ni, node in enumerate(levels[li]):
            sizes[(li, ni)] = 4 + len(node) * (32 if li == 0 else 24)
            order.append((li, ni))
    offs, p = {}, index_off + 48
    for k in order:
        offs[k] = p
        p += sizes[k]
    rt = []
    for li, ni in order:
        node = levels[li][ni]
        if li == 0:
            rt.append(struct.pack("<BBH", 1, 0, len(node)))
            rt.extend(struct.pack("<IIIIQQ", *x) for x in node)
        else:
            rt.append(struct.pack("<BBH", 0, 0, len(node)))
            for k in node:
                rt.append(struct.pack("<IIIIQ", *bounds(li - 1, k), offs[(li - 1, k)]))
    top = bounds(len(levels) - 1, 0)
    hdr = struct.pack("<IIQIIIIQII", 0x2468ACE0, rtree_block, len(leaves), top[0], top[1], top[2], top[3], index_off,
                      items_per_block, 0)
    return hdr + b"".join(rt), len(levels)


def write_bigbed(path, chromsizes, records, compress=True, items_per_block=512, rtree_block=256, bpt_block=256,
                 field_count=None, split_chroms=True, raw_hook=None, block_hook=None):
    """Writes a bigBed file and returns its layout: {"data_off", "index_off", "blocks": [(offset, size)], "levels"}.

    chromsizes: {name: size}; chromosome ids follow the names' sorted order, as bedToBigBed numbers them.
    records: {name: (starts, ends, rests)} -- rests: one bytes for every record, a list of bytes, or (lengths, blob).  Records
    are written chromosome by chromosome in id order, each chromosome's in the order given (nothing is checked or sorted).
    A data block holds items_per_block records and, with split_chroms, never two chromosomes.  field_count: 3 + the fields of
    the rests (default: counted from the first rest).  raw_hook(i, payload) / block_hook(i, stored) may alter block i before /
    after compression (corrupt files)."""
    names = sorted(chromsizes)
    cid = {n: i for i, n in enumerate(names)}
    parts = []
    first_rest = None
    for n in names:
        if n not in records:
            continue
        s, e, r = records[n]
        s = np.asarray(s, dtype=np.int64)
        if not len(s):
            continue
        buf, offs = pack_records(cid[n], s, np.asarray(e, dtype=np.int64), r)
        if first_rest is None:
            first_rest = buf[offs[0] + 12:offs[1] - 1]
        parts.append((cid[n], s, np.asarray(e, dtype=np.int64), buf, offs))
    if field_count is None:
        field_count = 3 + (first_rest.count(b"\t") + 1 if first_rest else 0)
    # data blocks: (chrom of the first record, first start, chrom of the last record, largest end of it, payload)
    blocks = []
    if split_chroms:
        for c, s, e, buf, offs in parts:
            for i in range(0, len(s), items_per_block):
                j = min(i + items_per_block, len(s))
                blocks.append((c, int(s[i]), c, int(e[i:j].max()), buf[offs[i]:offs[j]]))
    else:
        flat = [(c, int(s[k]), int(e[k]), buf[offs[k]:offs[k + 1]]) for c, s, e, buf, offs in parts for k in range(len(s))]
        for i in range(0, len(flat), items_per_block):
            chunk = flat[i:i + items_per_block]
            last = chunk[-1][0]
            blocks.append((chunk[0][0], chunk[0][1], last, max(x[2] for x in chunk if x[0] == last),
                           b"".join(x[3] for x in chunk)))
    raw_max = 0
    chroms = [(n, cid[n], int(chromsizes[n])) for n in names]
    bpt_hdr, bpt_nodes, _ = W._bpt(chroms, bpt_block)
    chrom_tree_off = 64
    key = max(len(n) for n in names) + 1

    def shift_offsets(nodes: bytes) -> bytes:
        out, p = bytearray(nodes), 0
        while p < len(nodes):
            leaf, _r, cnt = struct.unpack_from("<BBH", nodes, p)
            p += 4
            for _ in range(cnt):
                if not leaf:
                    off, = struct.unpack_from("<Q", nodes, p + key)
                    struct.pack_into("<Q", out, p + key, off + chrom_tree_off)
                p += key + 8
        return bytes(out)

    bpt = bpt_hdr + shift_offsets(bpt_nodes)
    data_off = chrom_tree_off + len(bpt)
    data = [struct.pack("<Q", sum(len(p[1]) for p in parts))]
    pos = data_off + 8
    leaves, spans = [], []
    for i, (c0, s0, c1, e1, payload) in enumerate(blocks):
        if raw_hook is not None:
            payload = raw_hook(i, payload)
        raw_max = max(raw_max, len(payload))
        z = zlib.compress(payload) if compress else payload
        if block_hook is not None:
            z = block_hook(i, z)
        leaves.append((c0, s0, c1, e1, pos, len(z)))
        spans.append((pos, len(z)))
        data.append(z)
        pos += len(z)
    index_off = pos
    rtree, nlevels = _rtree(leaves, index_off, rtree_block, items_per_block)
    header = struct.pack("<IHHQQQHHQQIQ", BIGBED_MAGIC, 4, 0, chrom_tree_off, data_off, index_off, field_count, field_count,
                         0, 0, (raw_max if compress else 0), 0)
    assert len(header) == 64
    with open(path, "wb") as fp:
        fp.write(header + bpt + b"".join(data) + rtree + struct.pack("<I", BIGBED_MAGIC))
    return {"data_off": data_off, "index_off": index_off, "blocks": spans, "levels": nlevels}


def random_records(seed, nrec, names, rest_len=(8, 24)):
    """{name: (starts, ends, rests)}: about nrec / len(names) ascending, disjoint records per chromosome with Umap-like BED6
    rests (a name, a score, a strand; rest_len bounds the name's length) -- the arrays and (lengths, blob) built with numpy."""
    rng = np.random.default_rng(seed)
    per = -(-nrec // len(names))
    out = {}
    for n in names:
        gaps = rng.integers(0, 60, per)
        runs = rng.integers(1, 400, per)
        starts = int(rng.integers(0, 5000)) + np.cumsum(gaps + np.concatenate(([0], runs[:-1])))
        ends = starts + runs
        nl = rng.integers(rest_len[0], rest_len[1] + 1, per)
        letters = rng.integers(97, 123, int(nl.sum()), dtype=np.uint8)
        # each rest: <name letters>\t<score digit>\t<strand>
        lens = nl + 4
        blob = np.empty(int(lens.sum()), dtype=np.uint8)
        rstart = np.zeros(per, dtype=np.int64)
        np.cumsum(lens[:-1], out=rstart[1:])
        pos = np.repeat(rstart, nl) + (np.arange(int(nl.sum())) - np.repeat(np.cumsum(nl) - nl, nl))
        blob[pos] = letters
        tail = rstart + nl
        blob[tail] = 9
        blob[tail + 1] = rng.integers(48, 58, per, dtype=np.uint8)
        blob[tail + 2] = 9
        blob[tail + 3] = np.where(rng.integers(0, 2, per) == 1, 43, 45).astype(np.uint8)
        out[n] = (starts, ends, (lens, blob.tobytes()))
    return out
