#!/usr/bin/env python3
"""GPU box diagnostic: builds the library with -DEV_STAMPS and prints where a tile's cycles go in k_cc_events, and when
its workgroups start and end (their lifetimes: what the static tile ranges leave idle).

usage: tools_ev_stamps.py [both|ncc] [extra hipcc flags ...]
  EV_STAMPS_LIB=path   use a library already built with -DEV_STAMPS instead of compiling one
  EV_TRACK=fixture     the fixture track's run lengths instead of the synthetic track (bench.py --track)
  EV_DENSITY=x         read starts per strand and bit (bench.py --density; 0.005)
  EV_CLAIM_MODE=n      pmx_debug_set_claim_mode (0: claims + helping, 2: the static walk)
  EV_WG_LAYER=n        pmx_debug_set_wg_layer (0: the device's compute units, 1: tile ranges in launch order)"""
import ctypes, os, subprocess, sys, glob
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
lib = os.environ.get("EV_STAMPS_LIB")
if not lib:
    lib = "/tmp/libevstamps.so"
    extra = [a for a in sys.argv[2:]]
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-mllvm", "-amdgpu-atomic-optimizer-strategy=DPP", "-fPIC", "-shared", "-DEV_STAMPS",
                           "-o", lib] + extra + sorted(glob.glob(os.path.join(ROOT, "pymasc_amd/csrc/*.hip"))))
os.environ["PYMASC_AMD_LIB"] = lib
os.environ["PMX_AUTOCORR_FORK"] = "0"
import torch
from pymasc_amd import ffi, synth
mode = sys.argv[1] if len(sys.argv) > 1 else "both"
track = os.environ.get("EV_TRACK", "synthetic")
with_m = mode == "both"
density = float(os.environ.get("EV_DENSITY", "0.005"))
ctx = ffi.Context(0)
dev = torch.device("cuda", 0)
S, L = 1000, 36
vecs = [synth.make_chromosome(ctx, dev, n, ln, S, L, 0xC0FFEE + i, density=density, with_m=with_m, track=track) for i, (n, ln) in enumerate(synth.HG38)]
out = torch.zeros((len(vecs), ffi.PMX_NROWS, S + 1), dtype=torch.int64, device=dev)
args = ([v.F.data_ptr() for v in vecs], [v.R.data_ptr() for v in vecs], [v.M.data_ptr() for v in vecs] if with_m else None,
        [v.nbits for v in vecs], S, L, ffi.PMX_FLAG_EVENTS_HINT, [out[i].data_ptr() for i in range(len(vecs))])
Lb = ffi.load_library()
if os.environ.get("EV_CLAIM_MODE"):
    ctx.debug_set_claim_mode(int(os.environ["EV_CLAIM_MODE"]))
width = int(os.environ.get("EV_WG_LAYER", "0"))
ctx.debug_set_wg_layer(width)
ntiles = sum((v.nbits + 65535) // 65536 for v in vecs)
per_cu = int(os.environ.get("EV_PER_CU", 5 if with_m else 8))
nwg = min(256 * per_cu, ntiles)
tpw = -(-ntiles // nwg); nwg = -(-ntiles // tpw)
off = (nwg + len(vecs)) * 6 * 1024 * 4   # EV_SEG_ROWS
NS = 16   # EV_STAMP_SLOTS
NP = 10   # slots 0..9: phases of a tile, in shader cycles; slots 10, 11 of wave 0: start and end of the workgroup;
          # 12, 13: cycles and number of flushes; 14, 15: cycles and number of guarded fetches (slot 4: the interior ones)
Lb.pmx_debug_read_slab.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64]
launches = []   # three launches, the stamps of each (everything below but the placement check reads the last)
for _ in range(3):
    ctx.cc_batch_dev(*args)
    ctx.sync()
    buf = np.zeros(nwg * 4 * NS, dtype=np.uint64)
    rc = Lb.pmx_debug_read_slab(ctx._h, off, buf.ctypes.data, buf.nbytes)
    assert rc == 0
    launches.append(buf.reshape(nwg, 4, NS))
raw = launches[-1]
a = raw[:, :, :NP].astype(np.float64)
tot = (a.sum(axis=2) + raw[:, :, 12] + raw[:, :, 14]).mean()
print(f"mode={mode} track={track} density={density} nwg={nwg} tiles/wg={tpw} cycles per wave lifetime={tot:.0f}  per tile={tot / tpw:.0f}")
lab = {0: "B0 barrier wait", 1: "counts + M store + scans", 2: "Bs barrier wait", 3: "totals + emit lists", 4: "prefetch issue",
       5: "B1 barrier wait", 6: "events: forward x reverse pairs", 8: "R0 (reverse reads: M[p] M[p+c])", 7: "events: edges x reads, edge pairs",
       9: "loop tail (without the flushes)"}
for i in range(NP):
    print(f"  {lab[i]:32s} {a[:, :, i].mean() / tpw:9.0f} cyc/tile  {100 * a[:, :, i].sum() / a.sum():5.1f} %")
for w in range(4):
    print("  wave", w, " ".join(f"{a[:, w, i].mean() / tpw:7.0f}" for i in range(NP)))

# ---- the cold path of a workgroup: flushes and guarded fetches (boundary tiles), per occurrence and wave
fl_c, fl_n = raw[:, :, 12].astype(np.float64), raw[:, :, 13].astype(np.float64)
gf_c, gf_n = raw[:, :, 14].astype(np.float64), raw[:, :, 15].astype(np.float64)
tiles_w = a[:, :, 4] * 0 + tpw   # (claimed tiles move between workgroups: the static share stands in for the count)
print(f"  flushes: {fl_n.sum() / 4:.0f} in {nwg} workgroups, {fl_c.sum() / max(1.0, fl_n.sum()):9.0f} cycles per flush and wave"
      f" (longest wave mean {np.max(fl_c / np.maximum(1, fl_n)):9.0f})")
print(f"  guarded fetches: {gf_n.sum() / 4:.0f}, {gf_c.sum() / max(1.0, gf_n.sum()):9.0f} cycles per fetch and wave;"
      f" interior fetches: {a[:, :, 4].sum() / max(1.0, (tiles_w - gf_n).sum()):9.0f} cycles per fetch and wave")

# ---- workgroup lifetimes.  The constant 100 MHz clock (s_memrealtime), one reading at kernel entry and one behind the last
# flush: the shader clock (s_memtime) of one XCD says nothing about another's, and the question is who waits for whom.
TICK_US = 0.01
t0 = raw[:, 0, 10].astype(np.int64)
t1 = raw[:, 0, 11].astype(np.int64)
base = t0.min()
st = (t0 - base) * TICK_US
en = (t1 - base) * TICK_US
life = en - st
span = en.max() - st.min()
idle = 1.0 - life.sum() / (nwg * span)
print(f"workgroup lifetimes (us, from the first start): {nwg} workgroups")
print(f"  first start {st.min():8.2f}   last start {st.max():8.2f}")
print(f"  first end   {en.min():8.2f}   last end   {en.max():8.2f}")
print(f"  mean lifetime {life.mean():8.2f}   shortest {life.min():8.2f}   longest {life.max():8.2f}")
print(f"  idle share 1 - sum(lifetimes) / (workgroups x (last end - first start)) = {100 * idle:5.2f} %")
print(f"    of which before the start {100 * (st - st.min()).sum() / (nwg * span):5.2f} %, behind the end {100 * (en.max() - en).sum() / (nwg * span):5.2f} %")
# the workgroups that hold a guarded tile, or flush more than once (two jobs), against the rest
cold = (raw[:, 0, 15] > 0) | (raw[:, 0, 13] > 1)
for name, sel in (("with a guarded tile or two jobs", cold), ("the rest", ~cold)):
    if sel.any():
        print(f"  {name:32s} {int(sel.sum()):5d} workgroups  mean lifetime {life[sel].mean():8.2f}  mean end {en[sel].mean():8.2f}  last end {en[sel].max():8.2f}")
order = np.argsort(en)[::-1][:20]
print("  the last twenty to end (workgroup: end us, guarded fetches, flushes): " +
      ", ".join(f"{int(w)}: {en[w]:.2f} {int(raw[w, 0, 15])} {int(raw[w, 0, 13])}" for w in order))
hist, edges = np.histogram(en, bins=10, range=(en.min(), en.max()))
print("  end times, ten bins from the first to the last end:")
for k in range(10):
    print(f"    {edges[k]:8.2f} .. {edges[k + 1]:8.2f} us  {hist[k]:5d}  {'#' * int(round(60 * hist[k] / max(1, hist.max())))}")

# ---- dispatch layers.  Wave 1's slot 10 holds HW_ID | XCC_ID << 32 read at kernel entry: a workgroup's CU is (XCC, SE, SH, CU),
# its ARRIVAL RANK its rank by blockIdx among the workgroups of that CU.  The stamps are indexed by the physical block; the
# range a block owns (its chromosome) comes from the library's map at the width in force.
if with_m:
    num_cus = torch.cuda.get_device_properties(0).multi_processor_count
    def placement(r):
        hw = r[:, 1, 10]
        return ((hw >> np.uint64(32)) & np.uint64(0xf)) << np.uint64(8) | ((hw >> np.uint64(8)) & np.uint64(0xff))
    def ranks(cu):
        rk = np.zeros(nwg, dtype=np.int64)
        seen = {}
        for b in range(nwg):
            rk[b] = seen.get(int(cu[b]), 0)
            seen[int(cu[b])] = rk[b] + 1
        return rk
    cus = [placement(r) for r in launches]
    rks = [ranks(c) for c in cus]
    blk = np.arange(nwg)
    print(f"dispatch layers: width {width or num_cus} (EV_WG_LAYER={width}), {num_cus} compute units, claim mode {os.environ.get('EV_CLAIM_MODE', '0')}")
    for i, (c, rk) in enumerate(zip(cus, rks)):
        per = np.bincount(np.unique(c, return_inverse=True)[1])
        print(f"  launch {i}: {len(per)} distinct (XCC, SE, SH, CU), {per.min()}..{per.max()} workgroups each;"
              f" rank == blockIdx // {num_cus} for {int((rk == blk // num_cus).sum())} of {nwg} ({100.0 * (rk == blk // num_cus).mean():.1f} %);"
              f" same CU as launch 0 for {int((c == cus[0]).sum())}, same rank for {int((rk == rks[0]).sum())}")
    xcc = (cus[-1] >> np.uint64(8)).astype(np.int64)
    print("  XCC of blocks 0..15: " + " ".join(str(int(x)) for x in xcc[:16]) + "   CU key of blocks 0, 8, 16, .. 56: " + " ".join(f"{int(k) & 0xff:02x}" for k in cus[-1][0:64:8]))
    rk = rks[-1]
    print("  per arrival rank (workgroups, mean lifetime us, mean end us, last end us):")
    for k in range(int(rk.max()) + 1):
        sel = rk == k
        print(f"    rank {k}: {int(sel.sum()):5d}  {life[sel].mean():8.2f}  {en[sel].mean():8.2f}  {en[sel].max():8.2f}")
    print("  per XCC (workgroups, mean lifetime us, mean end us, last end us):")
    for x in np.unique(xcc):
        sel = xcc == x
        print(f"    xcc {int(x)}: {int(sel.sum()):5d}  {life[sel].mean():8.2f}  {en[sel].mean():8.2f}  {en[sel].max():8.2f}")
    order_v = ffi.wg_order(nwg, width or num_cus).astype(np.int64)   # the range of block b
    tile0 = np.cumsum([0] + [(v.nbits + 65535) // 65536 for v in vecs])
    chrom = np.searchsorted(tile0, order_v * tpw, side="right") - 1   # the chromosome of a range's first tile
    print("  per chromosome of the range's first tile (workgroups, arrival ranks present, mean lifetime us, mean end us, last end us):")
    for ci, (name, _ln) in enumerate(synth.HG38):
        sel = chrom == ci
        if sel.any():
            present = "".join(str(k) if (rk[sel] == k).any() else "." for k in range(int(rk.max()) + 1))
            print(f"    {str(name):6s} {int(sel.sum()):5d}  {present:6s} {life[sel].mean():8.2f}  {en[sel].mean():8.2f}  {en[sel].max():8.2f}")
