"""Multi-GPU layer: chromosome jobs -> ranks, and the result exchange.

The reference parallelises over chromosomes with one worker process per chromosome task
(PyMaSC/handler/calc.py:163-235, utils/calc.py:95-145) and ships each per-chromosome result to the
parent over a multiprocessing.Queue (handler/worker.py:234).  Here: one process per GPU, chromosome
jobs assigned longest-processing-time-first, no collective on the data path, and ONE exchange at the
end: an all-gather of the per-chromosome result rows (the genome-wide curve is a Fisher-z merge of
per-chromosome cc, PyMaSC/utils/calc.py:172-241, so the rows must be kept) plus an all-reduce(sum)
of the genome-wide integer totals (mscc.pyx:238-239, stats.py:515-517).  Backend "nccl" is RCCL over
xGMI on the GPU box; the same code runs on "gloo" with CPU tensors in the tests.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple  # noqa: F401

import torch
import torch.distributed as dist


def lpt_assign(costs: Sequence[float], world_size: int) -> List[List[int]]:
    """Longest-processing-time-first: job indices per rank, deterministic on every rank."""
    order = sorted(range(len(costs)), key=lambda i: (-costs[i], i))
    loads = [0.0] * world_size
    out: List[List[int]] = [[] for _ in range(world_size)]
    for i in order:
        r = min(range(world_size), key=lambda k: (loads[k], k))
        out[r].append(i)
        loads[r] += costs[i]
    return out


def tile_range_assign(nbits: Sequence[int], world_size: int, tile_bits: int = 65536) -> List[List[Tuple[int, int, int]]]:
    """Equal shares of the genome's TILES, not of its chromosomes (round 4): the tiles of all jobs laid end to end are cut into
    world_size contiguous stretches; rank r gets [(job, first tile, tile count), ...] -- whole chromosomes in the middle of
    its stretch, a share of one at either end.  Every sum of the hot path is owned by one tile, so the ranks' partial
    result blocks ADD UP to the chromosome's (pmx_cc_batch_ranges_dev) and ONE all-reduce(sum) of the per-chromosome rows
    is the whole exchange -- BASELINE.json's north star.  LPT over whole chromosomes leaves 3.6 % imbalance on hg38 at 8
    ranks; this leaves less than one tile.  Deterministic on every rank."""
    ntiles = [max(1, (int(b) + tile_bits - 1) // tile_bits) for b in nbits]
    total = sum(ntiles)
    out: List[List[Tuple[int, int, int]]] = [[] for _ in range(world_size)]
    start = 0                                     # first global tile of the current job
    for j, nt in enumerate(ntiles):
        for r in range(world_size):
            lo, hi = total * r // world_size, total * (r + 1) // world_size      # rank r's stretch of the global sequence
            a, b = max(lo, start), min(hi, start + nt)
            if b > a:
                out[r].append((j, a - start, b - a))
        start += nt
    return out


def exchange_partial_rows(partial: torch.Tensor, group=None, force_collectives: bool = False) -> torch.Tensor:
    """partial: int64 [njobs, nrows, stride] -- this rank's SHARE of every chromosome's result block (zeros where it holds
    nothing).  Returns the complete blocks on every rank: one all-reduce(sum) over RCCL / xGMI."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    if world > 1 or (force_collectives and dist.is_initialized()):
        dist.all_reduce(partial, op=dist.ReduceOp.SUM, group=group)
    return partial


def owner_table(assignment: List[List[int]], njobs: int) -> List[Tuple[int, int]]:
    """job -> (rank, slot on that rank)."""
    table = [(-1, -1)] * njobs
    for r, jobs in enumerate(assignment):
        for s, j in enumerate(jobs):
            table[j] = (r, s)
    return table


_INDEX_CACHE: Dict[tuple, Tuple[torch.Tensor, torch.Tensor]] = {}


def _owner_index(assignment: List[List[int]], njobs: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
    """(rank, slot) index tensors of every job, built once per assignment (no per-step host->device copies)."""
    key = (tuple(tuple(a) for a in assignment), njobs, str(device))
    hit = _INDEX_CACHE.get(key)
    if hit is None:
        table = owner_table(assignment, njobs)
        hit = (torch.tensor([t[0] for t in table], device=device), torch.tensor([t[1] for t in table], device=device))
        _INDEX_CACHE[key] = hit
    return hit


def exchange_results(local_rows: torch.Tensor, assignment: List[List[int]], njobs: int,
                     group=None, force_collectives: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """local_rows: int64 [max_slots, nrows, stride], this rank's jobs in slot order (unused slots zero).

    Returns (rows[njobs, nrows, stride] in job order on every rank, totals[nrows, stride] = sum over
    all jobs, computed by all-reduce so it can be cross-checked against rows.sum(0)).
    force_collectives: run the all-gather / all-reduce even in a group of one rank (the one-GPU boxes' way to put the
    RCCL code path under test and to time its fixed cost)."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    max_slots = max(len(a) for a in assignment)
    assert local_rows.shape[0] == max_slots
    totals = local_rows.sum(dim=0)
    if world == 1 and not (force_collectives and dist.is_initialized()):
        gathered = local_rows.unsqueeze(0)
    else:
        flat = torch.empty((world * max_slots,) + tuple(local_rows.shape[1:]), dtype=local_rows.dtype,
                           device=local_rows.device)
        dist.all_gather_into_tensor(flat, local_rows.contiguous(), group=group)   # rank-major concatenation
        gathered = flat.view((world,) + tuple(local_rows.shape))
        dist.all_reduce(totals, op=dist.ReduceOp.SUM, group=group)
    idx_r, idx_s = _owner_index(assignment, njobs, local_rows.device)
    rows = gathered[idx_r, idx_s]
    return rows, totals


# ---------------------------------------------------------------------------------------------------------------
# From the input files: the reference's `-p N` flow (handler/calc.py:163-235, handler/worker.py:68-234), one
# process per GPU instead of one per chromosome task.
# ---------------------------------------------------------------------------------------------------------------

def rank_and_world(group=None) -> Tuple[bool, int, int]:
    """(is torch.distributed initialised, this rank in ``group``, the number of ranks in it); (False, 0, 1) without it."""
    on = dist.is_available() and dist.is_initialized()
    return on, (dist.get_rank(group) if on else 0), (dist.get_world_size(group) if on else 1)


def _collective_device_setup(device, group=None):
    """With a GPU backend (nccl = RCCL) object collectives stage their payload on torch's CURRENT device, which is
    cuda:0 in every fresh process: bind it to this rank's GPU first, or two ranks collide on one device."""
    if not (dist.is_available() and dist.is_initialized()) or device is None:
        return
    try:
        backend = str(dist.get_backend(group))
    except Exception:
        return
    if "nccl" in backend and torch.cuda.is_available():
        torch.cuda.set_device(int(device))


def on_rank0(fn, group, what: str):
    """``fn()`` computed on rank 0 alone and its value returned on every rank.  One rank: ``fn()``, its exception propagates.
    Several: rank 0 broadcasts the value or its error, re-raises its own exception (type kept), and every other rank raises
    ``RuntimeError("<what> failed on rank 0 [...]")`` -- none waits for a value that never comes.  A GPU backend needs
    ``_collective_device_setup`` first."""
    _on, rank, world = rank_and_world(group)
    if world == 1:
        return fn()
    box = [None, None]              # [value, error message]
    err = None
    if rank == 0:
        try:
            box[0] = fn()
        except Exception as e:      # every rank must learn about it (no hang below)
            err = e
            box[1] = "{}: {}".format(type(e).__name__, e)
    dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
    if err is not None:
        raise err
    if box[1] is not None:
        raise RuntimeError("{} failed on rank 0 [{}]".format(what, box[1]))
    return box[0]


def gather_chromosome_results(local: Dict[str, object], order: Sequence[str], group=None,
                              error: BaseException = None) -> Dict[str, object]:
    """Every rank's {chromosome: BothChromResult} -> the union on every rank, in ``order``.

    The payload is a few KB of integers per chromosome (what the reference pushes through a multiprocessing.Queue,
    worker.py:234); the fixed-shape tensor exchange used by the benchmark is ``exchange_results`` above.
    ``error``: this rank failed -- every rank learns about it from the same collective and raises, instead of the
    healthy ranks waiting for a peer that never arrives (the reference's '__ERROR__' report, worker.py:91-99 ->
    handler/calc.py:205-206).  Several ranks: the exception raised on every rank -- the failing rank's own, a RuntimeError
    on the others -- carries ``failed_ranks``, the same list ``[(rank, exception type name, message), ...]`` on every rank,
    so that callers can take one decision on all of them without another collective."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        if error is not None:
            raise error
        parts = [(None, local, None)]
    else:
        parts = [None] * dist.get_world_size(group)
        mine = (None, local, None) if error is None else (str(error), None, type(error).__name__)
        dist.all_gather_object(parts, mine, group=group)
    failed = [(r, p[2], p[0]) for r, p in enumerate(parts) if p[2] is not None]
    if failed:
        if error is None:
            error = RuntimeError("Worker error on rank(s): " + "; ".join("{} [{}: {}]".format(*f) for f in failed))
        error.failed_ranks = failed
        raise error                                        # the failing rank re-raises its own exception (type kept)
    merged: Dict[str, object] = {}
    for _err, p, _type in parts:
        for chrom, res in p.items():
            if chrom in merged:
                raise RuntimeError("chromosome {} was calculated by two ranks".format(chrom))
            merged[chrom] = res
    return {c: merged[c] for c in order if c in merged}


def reconcile_chromosome_sizes(bam_sizes: Dict[str, int], external_sizes: Dict[str, int]) -> Dict[str, int]:
    """The reference's rule when a mappability track is given (reader/bam.py:217-255 via handler/calc.py:100-115):
    for chromosomes present in both, a mismatch is warned about and the LONGER length is used."""
    import logging
    log = logging.getLogger(__name__)
    out = {}
    for ref, bam_size in bam_sizes.items():
        ext = external_sizes.get(ref)
        if ext is None:
            log.debug("External size for '%s' not found", ref)
            out[ref] = bam_size
            continue
        if ext != bam_size:
            log.warning("'%s' reference length mismatch: SAM/BAM -> %s, External -> %s", ref, format(bam_size, ","),
                        format(ext, ","))
            if bam_size < ext:
                log.warning("Use longer length '%d' for '%s' anyway", ext, ref)
        out[ref] = max(bam_size, ext)
    return out


def run_sharded(bam_path, max_shift: int, read_len: int, mapq_criteria: int, bigwig_path=None,
                references: Sequence[str] = None, skip_ncc: bool = False, device: int = None, context=None,
                chrom2mappable_len=None, group=None, device_ingest: Optional[bool] = None, bam=None, chromfilter=None,
                track=None, chrom_sizes=None, reader_hook=None, exclude_regions=None):
    """BAM (+ BigWig) -> genome-wide result on every rank; chromosomes LPT-sharded over the ranks by length.

    Launch: one process per GPU under ``torch.distributed`` (torchrun, or pymasc_amd.launch.spawn_ranks), the process
    group initialised BEFORE this call; ``device`` = this rank's GPU (default LOCAL_RANK).
    Every rank reads its own chromosomes through the .bai index when there is one (the reference requires it for
    its multi-process mode, reader/bam.py:246-262), otherwise it streams the whole BAM through the native reader
    (~30 M records/s on 16 host threads) and keeps its share; the kernels see only the rank's chromosomes; one object
    all-gather at the end, then the reference's aggregation (result.py:301-464 -> pymasc_amd.result.aggregate_results).
    A rank that fails reports through that same all-gather, so every rank raises instead of hanging.
    ``device_ingest``: inflate, walk and filter the BAM file on the GPU and hand the records to the feeders in HBM
    (pymasc_amd.bam_device) -- default: when this is the only rank and it runs on a real GPU; with several
    ranks each takes its own chromosomes through the host reader and the .bai instead of inflating the whole file N times.
    ``bam``: a reader of ``bam_path`` the caller has already opened (pipeline.run opens the device reader to estimate the read
    length on it, so that the file is inflated once per run); it is used instead of opening one and is left open.  A
    device reader implies ``device_ingest``.
    A SAM file (plain or BGZF, ``pymasc_amd.sam.detect_format``) is read whole, as a BAM file without an index: through the
    device SAM reader with ``device_ingest``, else the host one (pymasc_amd.inputs.open_alignments); ``bam`` may be an open
    reader of either.
    ``chromfilter``: PyMaSC's -i / -e chromosome filter, an ordered list of ``(include, [patterns])``
    (pymasc_amd.chromfilter); not together with ``references``.  A filter that leaves nothing raises on every rank.
    With the device reader and a .bai next to the BAM file, a rank of several -- or the only rank when ``references`` or
    ``chromfilter`` choose the chromosomes -- reads the header, takes its share and reads, copies and inflates only the BGZF
    members of that share (the device reader's ``select``); without an index, or with a ``bam`` given, the path
    is the whole-file one above.
    ``track``: a reader of ``bigwig_path`` the caller has already opened (pipeline.run_files opens the track once for all its
    files), used instead of opening one and left open, like ``bam``.
    ``chrom_sizes``: the references of a BED read file (``pymasc_amd.bed_reads``; a path or an ordered ``{name: length}``),
    which is read whole like SAM text -- by every rank of several through the host reader -- and is a ValueError without them.
    With a ``context`` given, the calculator still gives its bit-vectors back to the context's pool and frees its result arena
    before this returns (``CCHipCalculator.close`` never closes a context it does not own).
    ``reader_hook``: ``reader_hook(reader, names)`` is called with the open alignment reader and this rank's chromosomes just
    before they are fed; what it returns, when not None, is called without arguments once the feed has succeeded, while the
    reader is still open (pipeline.run counts the library complexity there: the file is inflated once).
    ``exclude_regions``: a BED file, an ordered ``{name: [(start, end), ...]}``, a ``region_mask.ExcludeMask`` or a ``ResolvedMask``
    of this file's references:
    the reads that overlap a region are left out by the reader (``set_exclude``, attached before ``reader_hook``; on the GPU with
    the device reader) and every chromosome's mappability vector is cleared where a read of ``read_len`` would touch one.  Names
    that are not references are skipped with one warning; none matching is a ValueError.  The count of the reads left out is
    logged at INFO.  A caller's ``bam`` reader keeps the mask afterwards."""
    from .calculator import CCHipCalculator
    from .chromfilter import kept_references
    from .inputs import (check_bed_sizes, default_device_ingest, find_index, open_alignments, open_track, reader_device,
                         track_on_device)
    from .result import aggregate_results
    from .bed_reads import is_bed_reads
    from .sam import is_sam

    if bam is None:
        check_bed_sizes(bam_path, chrom_sizes)
    on, rank, world = rank_and_world(group)
    if device is None and context is None and on:
        import os
        device = int(os.environ.get("LOCAL_RANK", "0"))
    _collective_device_setup(device, group)
    local: Dict[str, object] = {}
    names: List[str] = []
    error = None
    if bam is not None:
        from .bam_device import DeviceBamReader
        device_ingest = isinstance(bam, DeviceBamReader)
    elif device_ingest is None:
        device_ingest = default_device_ingest(world, context)
    if references is not None and chromfilter is not None:
        raise ValueError("give references or chromfilter, not both")
    dev = reader_device(context, device) if device_ingest else 0
    # indexed: the open reads the header only, the rank's share is selected below.  SAM text: the unindexed-BAM rules
    # 
    indexed = (device_ingest and bam is None and (world > 1 or references is not None or chromfilter is not None)
               and not is_bed_reads(bam_path) and not is_sam(bam_path) and find_index(bam_path) is not None)
    reader, bw = bam, None          # the caller's readers are used, not closed
    try:
        if reader is None:
            reader = open_alignments(bam_path, device_ingest, dev, references=[] if indexed else None, chrom_sizes=chrom_sizes)
        names = kept_references(reader.references, references, chromfilter)
        lengths = dict(zip(reader.references, reader.lengths))
        mask = None
        if exclude_regions is not None:
            from .region_mask import ResolvedMask, open_mask
            mask = exclude_regions      # (resolved by the caller against this file's header: taken as it is)
            if not (isinstance(mask, ResolvedMask) and mask.references == tuple(reader.references)):
                mask = getattr(mask, "mask", mask)
                mask = open_mask(mask, device_ingest, dev).resolve(reader.references, reader.lengths)
            reader.set_exclude(mask)
        if bigwig_path is not None:     # with device ingest the track is decoded on the GPU too: its intervals stay in HBM
            if track is None:           # (a genome FASTA: on this rank's GPU whenever it has one)
                gpu_track = track_on_device(bigwig_path, device_ingest, context)
                tdev = dev if (not gpu_track or device_ingest) else reader_device(context, device)
                bw = open_track(bigwig_path, gpu_track, tdev, k=read_len)
            else:
                bw = track
            # the track's chromosome sizes win where they are longer (handler/calc.py:100-115); a text track's sizes are the
            # extents of its lines: one that stops short of the chromosome is normal and says nothing
            ext = bw.chromsizes
            if getattr(bw, "chromsizes_are_extents", False):
                ext = {n: s for n, s in ext.items() if n in lengths and s > lengths[n]}
            lengths.update(reconcile_chromosome_sizes({n: lengths[n] for n in names}, ext))
        mine = [names[i] for i in sorted(lpt_assign([lengths[n] for n in names], world)[rank])]
        if indexed:
            reader.select(mine)
        kw = {}
        if context is not None:
            kw["context"] = context
        elif device is not None:
            kw["device"] = device
        if mine:
            calc = CCHipCalculator(max_shift, read_len, mine, [lengths[n] for n in mine], bwfeeder=bw,
                                   skip_ncc=skip_ncc, chrom2mappable_len=chrom2mappable_len, exclude=mask, **kw)
            try:
                after_feed = reader_hook(reader, mine) if reader_hook is not None else None
                reader.feed(calc, mapq_criteria, references=mine)
                local = {c: calc.get_result(c) for c in mine}
                if mask is not None:
                    import logging
                    logging.getLogger(__name__).info("Excluded regions: {} reads of '{}' left out.".format(reader.excluded(), bam_path))
                if after_feed is not None:
                    after_feed()
            finally:
                calc.close()
    except Exception as e:              # surfaced on every rank by the gather below
        if not on or world == 1:
            raise
        error = e
    finally:
        if bw is not None and bw is not track:
            bw.close()
        if reader is not bam:
            reader.close()
    merged = gather_chromosome_results(local, names, group, error=error)
    return aggregate_results(merged)
