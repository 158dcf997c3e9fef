// The fragment pileup as runs of constant depth, and the text of its bedGraph track, on the device (pmx_dbam_coverage_*,
// include/pymasc_amd_ingest.h; DESIGN.md 7.18).  Included at the end of bam_device.hip, behind peakcount_device.inc: the kept records
// of a call come from cx_filter as in pmx_dbam_bincount_add, a read's extent is k_fp_count's (fp_extent), the scans over tiles,
// workgroups and line lengths are k_bam_scan.  The second half of the file makes the parts of a bigWig file from the runs (7.18.1).
//
// The reads are the ones the correlation sees: the caller's filter, the chosen references, less the reads an attached exclude mask
// drops.  L = extend, or the read's own length at 0; a forward read covers [pos1, pos1 + L - 1], a reverse read
// [pos1 + read_len - L, pos1 + read_len - 1]; the extent is clipped to [1, len] of its reference, and a read with nothing left adds
// nothing and is not in `reads`.  depth[r][p] = the kept reads whose clipped extent holds position p of reference r, a 32-bit count.
// Per chosen reference, in header order, the maximal intervals of constant depth > 0 are the runs (start0, end0, depth), 0-based and
// half-open; two reads that abut at equal depth form one run, depth 0 is not a run.  Totals: reads, runs, covered_bases =
// sum (end0 - start0), fragment_bases = sum depth * (end0 - start0) (64-bit, = the sum of the clipped extents' lengths), max_depth.
//
// The table is one int32 slot per base of every chosen reference plus one closing slot behind its last base (the -1 of a read that
// ends on the last base), the references end to end in header order, each beginning on a multiple of 4 slots (16-byte loads; up to
// 3 slots of padding that nothing writes).  Slot p - 1 of a reference holds depth[p] - depth[p - 1]: a run boundary is exactly a
// non-zero slot, and a +1 and a -1 that cancel leave none.  A reference's slots add up to 0, so no depth carries into the next.
//
//   k_cv_marks    one lane per kept read: atomicAdd(+1) at slot lo - 1 and atomicAdd(-1) at slot hi, neither with a return value;
//                 the reads that added are reduced by ballot, one 64-bit atomic per workgroup
//   k_cv_tiles    one workgroup per tile of CV_TILE slots (a reference's tiles begin at its first slot: no tile holds two
//                 references), four 16-byte loads per lane: the tile's sum and its number of non-zero slots
//   k_bam_scan    twice: the prefix of the tile sums (modulo 2^32: a depth is below 2^31) and of the tile counts.  The depth in
//                 front of a tile is its prefix less that of its reference's first tile: the scan starts again at every reference
//   k_cv_runs     per tile: the lanes' sums are scanned over the wave by shuffles and over the four loads and waves through LDS, on
//                 top of the tile's prefix; the non-zero slots are compacted by ballots into entries (reference, position, depth
//                 behind it) at the tile's offset, in position order
//   k_cv_keep / k_bam_scan / k_cv_close   entry k's run ends at entry k + 1's position; the last non-zero slot of a reference
//                 brings the depth to 0.  The entries of depth 0 are dropped by this second compaction (256 entries per
//                 workgroup, ballots); the totals are reduced by wave sums, one atomic per wave and total
//   k_ln_len<LnDepth>   one lane per run: name length + the three decimal widths + 4, and the workgroup's sum
//   k_bam_scan    the 64-bit exclusive prefix of the workgroups' sums
//   k_ln_text<LnDepth>  each lane writes its own line at the workgroup's prefix + a scan of the lengths within the workgroup
// Bound: fewer than 2^31 reads between begin and finish (add fails above it), so every depth and prefix is below 2^31.
// Device memory: 4 bytes per chosen base from begin to finish (12.4 GB for hg38) + 24 per tile, 12 per non-zero slot inside finish,
// then 16 per run until the next begin or close; 13 bytes per kept read inside a call of add; 4 per run + the text inside text.

#define CV_TILE PMX_COVERAGE_TILE             // slots per tile: 256 lanes x 4 loads x 4 slots
#define CV_MAX_READS (1ull << 31)

namespace {
struct CvSeg {          // a chosen reference: its first slot, its first tile, its slots (length + 1), its id
    u64 slot0;
    u32 tile0, nslots;
    int ref;
    u32 pad;
};
}  // namespace

// tab[2 * r] = the first slot of reference r (-1: the reference is not chosen), tab[2 * r + 1] = its length
__global__ void __launch_bounds__(256) k_cv_marks(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len,
                                                  const u8 *__restrict__ rev, u64 n, const long long *__restrict__ tab, u32 nref, u32 ext,
                                                  int *__restrict__ slots, unsigned long long *__restrict__ added)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    bool hit = false;
    if (i < n && ref[i] >= 0 && (u32)ref[i] < nref) {
        const long long first = tab[2u * (u32)ref[i]], top = tab[2u * (u32)ref[i] + 1u];
        long long lo, hi;
        if (first >= 0 && fp_extent(pos[i], len[i], rev[i] != 0, ext, top, lo, hi)) {      // (1 <= lo <= hi <= top: slots lo - 1 .. hi exist)
            hit = true;
            atomicAdd(&slots[first + lo - 1], 1);
            atomicAdd(&slots[first + hi], -1);
        }
    }
    const u64 m = __ballot(hit);
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) {
        const u32 c = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (c) atomicAdd(added, (unsigned long long)c);
    }
}

// the last reference of seg[0, nc) whose first tile is not behind `tile` (the same in every lane)
__device__ __forceinline__ u32 cv_seg_of(const CvSeg *__restrict__ seg, u32 nc, u32 tile)
{
    u32 a = 0, z = nc;
    while (z - a > 1u) {
        const u32 mid = (a + z) / 2u;
        if (seg[mid].tile0 <= tile) a = mid;
        else z = mid;
    }
    return a;
}

// load j of lane t holds the slots (j * 256 + t) * 4 .. + 3 of the tile; a reference's slots are padded with zeros to a multiple of 4
__device__ __forceinline__ void cv_load(const int *__restrict__ slots, u64 base, u32 n, u32 t, int4 v[4])
{
#pragma unroll
    for (u32 j = 0; j < 4u; j++) {
        const u32 e = (j * 256u + t) * 4u;
        v[j] = e < n ? *reinterpret_cast<const int4 *>(slots + base + e) : make_int4(0, 0, 0, 0);
    }
}

__global__ void __launch_bounds__(256) k_cv_tiles(const int *__restrict__ slots, const CvSeg *__restrict__ seg, u32 nc,
                                                  u32 *__restrict__ tsum, u32 *__restrict__ tcnt)
{
    __shared__ u32 s_s[4], s_c[4];
    const u32 t = threadIdx.x, tile = blockIdx.x;
    const CvSeg S = seg[cv_seg_of(seg, nc, tile)];
    const u32 off = (tile - S.tile0) * CV_TILE, n = S.nslots - off < CV_TILE ? S.nslots - off : CV_TILE;
    int4 v[4];
    cv_load(slots, S.slot0 + off, n, t, v);
    u32 s = 0, c = 0;
#pragma unroll
    for (u32 j = 0; j < 4u; j++) {
        s += (u32)v[j].x + (u32)v[j].y + (u32)v[j].z + (u32)v[j].w;
        c += (v[j].x != 0) + (v[j].y != 0) + (v[j].z != 0) + (v[j].w != 0);
    }
    s = (u32)cx_wave_sum((u64)s);
    c = (u32)cx_wave_sum((u64)c);
    if ((t & 63u) == 0) {
        s_s[t >> 6] = s;
        s_c[t >> 6] = c;
    }
    __syncthreads();
    if (t == 0) {
        tsum[tile] = s_s[0] + s_s[1] + s_s[2] + s_s[3];
        tcnt[tile] = s_c[0] + s_c[1] + s_c[2] + s_c[3];
    }
}

// inclusive scan of x over the wave
__device__ __forceinline__ u32 cv_wave_scan(u32 x, u32 lane)
{
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 y = __shfl_up(x, o, 64);
        if (lane >= (u32)o) x += y;
    }
    return x;
}

__global__ void __launch_bounds__(256) k_cv_runs(const int *__restrict__ slots, const CvSeg *__restrict__ seg, u32 nc,
                                                 const u64 *__restrict__ psum, const u64 *__restrict__ pcnt, int *__restrict__ eref,
                                                 u32 *__restrict__ epos, u32 *__restrict__ edep)
{
    __shared__ u32 s_s[4][4], s_c[4][4];          // [load][wave]
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6, tile = blockIdx.x;
    const CvSeg S = seg[cv_seg_of(seg, nc, tile)];
    const u32 off = (tile - S.tile0) * CV_TILE, n = S.nslots - off < CV_TILE ? S.nslots - off : CV_TILE;
    const u32 carry = (u32)psum[tile] - (u32)psum[S.tile0];      // the depth in front of the tile: the scan starts again with the reference
    int4 v[4];
    cv_load(slots, S.slot0 + off, n, t, v);
    const u64 below = (1ull << lane) - 1ull;
    u32 own[4], incl[4], before[4];
#pragma unroll
    for (u32 j = 0; j < 4u; j++) {
        own[j] = (u32)v[j].x + (u32)v[j].y + (u32)v[j].z + (u32)v[j].w;
        incl[j] = cv_wave_scan(own[j], lane);
        const u64 m0 = __ballot(v[j].x != 0), m1 = __ballot(v[j].y != 0), m2 = __ballot(v[j].z != 0), m3 = __ballot(v[j].w != 0);
        before[j] = (u32)(__popcll(m0 & below) + __popcll(m1 & below) + __popcll(m2 & below) + __popcll(m3 & below));
        if (lane == 63u) s_s[j][w] = incl[j];
        if (lane == 0) s_c[j][w] = (u32)(__popcll(m0) + __popcll(m1) + __popcll(m2) + __popcll(m3));
    }
    __syncthreads();
    const u64 out0 = pcnt[tile];
#pragma unroll
    for (u32 j = 0; j < 4u; j++) {
        u32 bs = carry, bc = 0;
        for (u32 k = 0; k < j * 4u + w; k++) {       // the loads and waves in front of this one
            bs += s_s[k >> 2][k & 3u];
            bc += s_c[k >> 2][k & 3u];
        }
        u32 run = bs + incl[j] - own[j];
        u64 o = out0 + bc + before[j];
        const u32 p0 = off + (j * 256u + t) * 4u;
        const int x[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
        for (u32 e = 0; e < 4u; e++) {
            run += (u32)x[e];
            if (x[e] != 0) {
                eref[o] = S.ref;
                epos[o] = p0 + e;
                edep[o] = run;
                o++;
            }
        }
    }
}

// entry k begins a run: its depth is above 0 and the next entry, of the same reference, ends it
__device__ __forceinline__ bool cv_keeps(const int *__restrict__ eref, const u32 *__restrict__ edep, u64 k, u64 n)
{
    return k + 1u < n && (int)edep[k] > 0 && eref[k + 1u] == eref[k];
}

// kcnt[workgroup] = its kept elements (s_w: four words of LDS)
__device__ __forceinline__ void cv_count(bool keep, u32 *__restrict__ kcnt, u32 *s_w)
{
    const u32 t = threadIdx.x;
    const u64 m = __ballot(keep);
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) kcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// where a kept element of a workgroup goes: kbase (k_bam_scan over cv_count's counts) of the workgroup + the kept ones in front of it
// (only the kept lanes do the arithmetic: done by every lane it costs k_bt_close two more VGPRs)
__device__ __forceinline__ u64 cv_slot(bool keep, const u64 *__restrict__ kbase, u32 *s_w)
{
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 m = __ballot(keep);
    if (lane == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (!keep) return 0;
    u64 o = kbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 x = 0; x < (t >> 6); x++) o += s_w[x];
    return o;
}

__global__ void __launch_bounds__(256) k_cv_keep(const int *__restrict__ eref, const u32 *__restrict__ edep, u64 n, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    cv_count(cv_keeps(eref, edep, (u64)blockIdx.x * 256u + threadIdx.x, n), kcnt, s_w);
}

// tot[0] += covered bases, tot[1] += fragment bases, tot[2] = max(tot[2], depth)
__global__ void __launch_bounds__(256) k_cv_close(const int *__restrict__ eref, const u32 *__restrict__ epos, const u32 *__restrict__ edep, u64 n,
                                                  const u64 *__restrict__ kbase, int *__restrict__ rref, u32 *__restrict__ rstart,
                                                  u32 *__restrict__ rend, u32 *__restrict__ rdepth, unsigned long long *__restrict__ tot)
{
    __shared__ u32 s_w[4];
    const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool keep = cv_keeps(eref, edep, k, n);
    const u64 o = cv_slot(keep, kbase, s_w);
    u64 width = 0, area = 0;
    u32 depth = 0;
    if (keep) {
        depth = edep[k];
        const u32 a = epos[k], z = epos[k + 1u];
        rref[o] = eref[k];
        rstart[o] = a;
        rend[o] = z;
        rdepth[o] = depth;
        width = (u64)(z - a);
        area = width * depth;
    }
    width = cx_wave_sum(width);
    area = cx_wave_sum(area);
    for (int d = 32; d > 0; d >>= 1) {
        const u32 y = __shfl_xor(depth, d, 64);
        depth = y > depth ? y : depth;
    }
    if ((threadIdx.x & 63u) == 0 && width) {       // (a run is a base wide at least)
        atomicAdd(&tot[0], (unsigned long long)width);
        atomicAdd(&tot[1], (unsigned long long)area);
        atomicMax(&tot[2], (unsigned long long)depth);
    }
}

template <class T> __device__ __forceinline__ u32 ln_width(T v)      // the decimal digits of v (a u32 divides in 32 bits)
{
    u32 w = 1;
    for (; v >= 10u; v /= 10u) w++;
    return w;
}

// the digits of v in front of `end`; returns where they begin
__device__ __forceinline__ u8 *cv_digits(u8 *end, u32 v)
{
    do {
        *--end = (u8)('0' + v % 10u);
        v /= 10u;
    } while (v);
    return end;
}

// The text of m lines, one lane per line, once for every kind of line (LnDepth below, LnSignal in signal_device.inc, LnPeak in
// call_device.inc).  A line is its reference's name and the columns behind it; a kind is a small struct L that the two kernels take by
// value, its column pointers already at the first line of the pull:
//   ref(i)       the reference of line i
//   len(i)       the bytes behind the name, from the TAB that follows it to the LF
//   put(i, q)    writes those bytes backwards from q, the line's end
template <class L> __global__ void __launch_bounds__(256) k_ln_len(L P, u64 n, const u32 *__restrict__ noff, u32 *__restrict__ len,
                                                                   u32 *__restrict__ wsum)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    u32 l = 0;
    if (i < n) {
        const u32 r = P.ref(i);
        l = noff[r + 1u] - noff[r] + P.len(i);
        len[i] = l;
    }
    l = (u32)cx_wave_sum((u64)l);
    if ((t & 63u) == 0) s_w[t >> 6] = l;
    __syncthreads();
    if (t == 0) wsum[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

template <class L> __global__ void __launch_bounds__(256) k_ln_text(L P, u64 n, const u32 *__restrict__ noff, const u8 *__restrict__ names,
                                                                    const u32 *__restrict__ len, const u64 *__restrict__ wbase,
                                                                    u8 *__restrict__ out)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 i = (u64)blockIdx.x * 256u + t;
    const u32 l = i < n ? len[i] : 0u;
    const u32 incl = cv_wave_scan(l, lane);
    if (lane == 63u) s_w[t >> 6] = incl;
    __syncthreads();
    if (i >= n) return;
    u64 o = wbase[blockIdx.x] + incl - l;
    for (u32 x = 0; x < (t >> 6); x++) o += s_w[x];
    const u32 r = P.ref(i);
    u8 *p = out + o;
    for (u32 c = noff[r]; c < noff[r + 1u]; c++) *p++ = names[c];
    P.put(i, out + o + l);              // (it ends at p: the lengths are k_ln_len's)
}

namespace {
struct LnDepth {        // a depth run: name TAB start TAB end TAB depth LF
    const int *rref;
    const u32 *start, *end, *depth;
    __device__ __forceinline__ u32 ref(u64 i) const { return (u32)rref[i]; }
    __device__ __forceinline__ u32 len(u64 i) const { return ln_width(start[i]) + ln_width(end[i]) + ln_width(depth[i]) + 4u; }
    __device__ __forceinline__ void put(u64 i, u8 *q) const
    {
        const u32 s = start[i], e = end[i], d = depth[i];
        *--q = '\n';
        q = cv_digits(q, d);
        *--q = '\t';
        q = cv_digits(q, e);
        *--q = '\t';
        q = cv_digits(q, s);
        *--q = '\t';
    }
};
}  // namespace

namespace {

// the arrays of the runs in their one block: reference, start, end, depth (4 bytes per run each)
struct CvRuns {
    int *ref;
    u32 *start, *end, *depth;
    CvRuns(u8 *p, u64 n) : ref((int *)p), start((u32 *)(p + 4 * n)), end((u32 *)(p + 8 * n)), depth((u32 *)(p + 12 * n)) {}
};

int coverage_begin_impl(pmx_dbam *b, u32 extend, const uint8_t *use_ref)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    b->cv = Coverage{};
    const u64 nref = b->ref_names.size();
    std::vector<long long> tab(2 * std::max<u64>(nref, 1), -1);
    std::vector<CvSeg> seg;
    std::vector<u32> noff(nref + 1, 0);
    std::string names;
    u64 slots = 0, tiles = 0;
    for (u64 r = 0; r < nref; r++) {
        noff[r] = (u32)names.size();
        names += b->ref_names[r];
        if (use_ref && use_ref[r] == 0) continue;
        const u64 len = (u64)std::max<int64_t>(b->ref_lens[r], 0);
        if (len >= 0xffffffffull) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_begin: a reference of 2^32 - 1 bases or more");
        tab[2 * r] = (long long)slots;
        tab[2 * r + 1] = (long long)len;
        seg.push_back(CvSeg{slots, (u32)tiles, (u32)(len + 1), (int)r, 0u});
        slots += (len + 1 + 3) / 4 * 4;
        tiles += (len + 1 + CV_TILE - 1) / CV_TILE;
        if (tiles >= (1ull << 31)) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_begin: 2^31 tiles or more");
    }
    noff[nref] = (u32)names.size();
    if (seg.empty()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_begin: no chosen reference");
    const u32 nc = (u32)seg.size();
    seg.push_back(CvSeg{slots, (u32)tiles, 0u, -1, 0u});        // (the end of the last reference's tiles)
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    HIPOK(hipMalloc(&c.tab.p, 8 * tab.size()));
    HIPOK(hipMalloc(&c.seg.p, sizeof(CvSeg) * seg.size()));
    HIPOK(hipMalloc(&c.names.p, 4 * noff.size() + std::max<u64>(names.size(), 1)));
    if (hipMalloc(&c.table.p, 4 * slots) != hipSuccess) {
        (void)hipGetLastError();
        c = Coverage{};
        return fail(PMX_DBAM_ERR_OPEN, "pmx_dbam_coverage_begin: out of device memory for the table: " + std::to_string(4 * slots) +
                                           " bytes asked for (4 per base of the chosen references)");
    }
    HIPOK(hipMemcpyAsync(c.tab.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(c.seg.p, seg.data(), sizeof(CvSeg) * seg.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(c.names.p, noff.data(), 4 * noff.size(), hipMemcpyHostToDevice, st));
    if (!names.empty()) HIPOK(hipMemcpyAsync(c.names.as<u8>() + 4 * noff.size(), names.data(), names.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemsetAsync(c.table.p, 0, 4 * slots, st));
    HIPOK(hipStreamSynchronize(st));       // (tab, seg, noff and names are locals)
    c.state = CV_TABLE;
    c.slots = slots;
    c.tiles = tiles;
    c.nc = nc;
    c.ext = extend;
    for (u32 k = 0; k < nc; k++) c.chosen.push_back(seg[k].ref);
    c.bytes = 4 * slots;
    if (b->st) stream_note(*b);
    return 0;
}

int coverage_add_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, uint64_t *reads_added)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!reads_added) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_add: null output");
    *reads_added = 0;
    if (!b->cv.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_add: no table: call pmx_dbam_coverage_begin first");
    Coverage &c = b->cv;
    unsigned long long added = 0;
    const int rc = side_add(
        b, mapq_min, flag_exclude, 1, &added,
        [&](const CxRecs &R, hipStream_t st, unsigned long long *d_added) {
            hipLaunchKernelGGL(k_cv_marks, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(),
                               R.rev.as<u8>(), R.n, c.tab.as<long long>(), (u32)b->ref_names.size(), c.ext, c.table.as<int>(), d_added);
        },
        [&](const CxRecs &R) {                  // (before a mark is made: the table stays as it is)
            return c.reads + R.n >= CV_MAX_READS
                       ? fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_add: 2^31 reads or more: the depth is a 32-bit count")
                       : 0;
        });
    if (rc) return rc;
    c.reads += added;
    *reads_added = added;
    return 0;
}

// device bytes a call holds for its own duration, counted into the handle's while it runs
struct CvHold {
    pmx_dbam *b;
    u64 n = 0;
    explicit CvHold(pmx_dbam *h) : b(h) {}
    void add(u64 bytes)
    {
        n += bytes;
        b->cv.bytes += bytes;
        if (b->st) stream_note(*b);
    }
    ~CvHold() { b->cv.bytes -= std::min(n, b->cv.bytes); }       // (a pileup freed meanwhile holds nothing)
};

// the work of finish on a handle that holds a table; a failure leaves the handle for the caller to clear
int coverage_finish_run(pmx_dbam *b, uint64_t *totals)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    const u64 nt = c.tiles;
    u64 tot[2] = {0, 0}, ne = 0, nruns = 0;
    unsigned long long sums[3] = {0, 0, 0};
    {
        DevAlloc d_t, d_p, d_tot, d_e;      // tile sums and counts; their prefixes; totals; the entries
        HIPOK(hipMalloc(&d_t.p, 8 * nt));
        HIPOK(hipMalloc(&d_p.p, 16 * nt));
        HIPOK(hipMalloc(&d_tot.p, 64));
        HIPOK(hipMemsetAsync(d_tot.p, 0, 64, st));
        u32 *tsum = d_t.as<u32>(), *tcnt = tsum + nt;
        u64 *psum = d_p.as<u64>(), *pcnt = psum + nt, *dt = d_tot.as<u64>();
        c.bytes += 24 * nt;
        if (b->st) stream_note(*b);
        hipLaunchKernelGGL(k_cv_tiles, dim3((unsigned)nt), dim3(256), 0, st, c.table.as<int>(), c.seg.as<CvSeg>(), c.nc, tsum, tcnt);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, tsum, tcnt, nt, psum, dt);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, tcnt, tcnt, nt, pcnt, dt + 2);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(tot, dt, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        ne = tot[1];
        if ((u32)tot[0] != 0) {             // (every read adds +1 and -1 to its reference)
            c = Coverage{};
            return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_finish: the table does not add up to 0");
        }
        if (ne) {
            if (hipMalloc(&d_e.p, 12 * ne) != hipSuccess) {
                (void)hipGetLastError();
                c = Coverage{};
                return fail(PMX_DBAM_ERR_OPEN, "pmx_dbam_coverage_finish: out of device memory for " + std::to_string(ne) + " run boundaries");
            }
            c.bytes += 12 * ne;
            if (b->st) stream_note(*b);
            int *eref = d_e.as<int>();
            u32 *epos = (u32 *)(eref + ne), *edep = epos + ne;
            hipLaunchKernelGGL(k_cv_runs, dim3((unsigned)nt), dim3(256), 0, st, c.table.as<int>(), c.seg.as<CvSeg>(), c.nc, psum, pcnt, eref, epos, edep);
            HIPOK(hipGetLastError());
            HIPOK(hipStreamSynchronize(st));
        }
        c.table = DevAlloc{};               // the table has become entries
        c.bytes -= 4 * c.slots + 24 * nt;
        if (ne) {
            const u64 nwg = (ne + 255) / 256;
            DevAlloc d_k, d_kb;
            HIPOK(hipMalloc(&d_k.p, 4 * nwg));
            HIPOK(hipMalloc(&d_kb.p, 8 * nwg));
            const int *eref = d_e.as<int>();
            const u32 *epos = (const u32 *)(eref + ne), *edep = epos + ne;
            hipLaunchKernelGGL(k_cv_keep, dim3((unsigned)nwg), dim3(256), 0, st, eref, edep, ne, d_k.as<u32>());
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), nwg, d_kb.as<u64>(), dt + 4);
            HIPOK(hipGetLastError());
            HIPOK(hipMemcpyAsync(&nruns, dt + 4, 8, hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            if (nruns) {
                if (hipMalloc(&c.runs.p, 16 * nruns) != hipSuccess) {
                    (void)hipGetLastError();
                    c = Coverage{};
                    return fail(PMX_DBAM_ERR_OPEN, "pmx_dbam_coverage_finish: out of device memory for " + std::to_string(nruns) + " runs");
                }
                c.bytes += 16 * nruns;
                if (b->st) stream_note(*b);
                const CvRuns V(c.runs.as<u8>(), nruns);
                HIPOK(hipMemsetAsync(dt, 0, 24, st));
                hipLaunchKernelGGL(k_cv_close, dim3((unsigned)nwg), dim3(256), 0, st, eref, epos, edep, ne, d_kb.as<u64>(), V.ref, V.start, V.end,
                                   V.depth, d_tot.as<unsigned long long>());
                HIPOK(hipGetLastError());
                HIPOK(hipMemcpyAsync(sums, dt, 24, hipMemcpyDeviceToHost, st));
                HIPOK(hipStreamSynchronize(st));
            }
            c.bytes -= 12 * ne;
        }
    }
    c.state = CV_RUNS;
    c.slots = 0;
    c.nruns = nruns;
    c.tot[0] = c.reads;
    c.tot[1] = nruns;
    c.tot[2] = sums[0];
    c.tot[3] = sums[1];
    c.tot[4] = sums[2];
    for (int k = 0; k < 5; k++) totals[k] = c.tot[k];
    return 0;
}

// A failure past the state check clears the pileup: the table may be freed or half read by then, and no later add, finish, runs or
// text may work on what is left of it.
int coverage_finish_impl(pmx_dbam *b, uint64_t *totals)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_finish: null output");
    for (int k = 0; k < 5; k++) totals[k] = 0;
    if (!b->cv.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_coverage_finish: no table: call pmx_dbam_coverage_begin first");
    struct Clear {      // (on a return code and on an exception)
        pmx_dbam *b;
        int rc;
        ~Clear()
        {
            if (rc) b->cv = Coverage{};
        }
    } run{b, PMX_DBAM_ERR_OPEN};
    return run.rc = coverage_finish_run(b, totals);
}

// The runs an entry point works on, and everything that reads their fourth column: the depth runs finish left (CV_DEPTH, defined
// behind its kernels below) or the signal runs pmx_dbam_coverage_signal made of them (SG_KIND, signal_device.inc), whose fourth
// column is a float32.  The host code below is the same for both.
struct CvKind {
    bool sg;
    const char *stem;                       // what the entry points' names begin with
    // coverage_lines<L>: the text of the runs [first, first + m) through the kind's line policy
    int64_t (*text)(pmx_dbam *b, const std::string &fn, const CvRuns &V, int64_t first, u64 m, uint8_t *buf, int64_t cap);
    void (*sections)(const u32 *, const u32 *, const u32 *, u64, u32, u32, u32 *, u32 *);       // k_tr_sections<V>
    void (*sums)(const u32 *, const u32 *, const u32 *, u64, u32, double *);      // (signal only) per section: sum and sum of squares
    // level 0; h_idof / d_idof: the id of every reference on the host and on the device, d_off: the first bin of every id, d_lens
    int (*fill)(pmx_dbam *b, const u32 *h_idof, const u32 *d_idof, const u64 *d_off, const u32 *d_lens, u32 z0, u64 nb0, u8 *bins,
                unsigned long long *d_tot);
    void (*fold)(u8 *, u64, u8 *, u64, const u64 *, const u64 *, u32);             // k_cv_zoom_fold, k_sg_zoom_fold
    void (*emit)(u8 *, u64, const u64 *, const u32 *, u32, u32, u32, const u64 *, const u64 *, u32 *, u32 *);      // k_tr_zoom_emit<V>
    std::string fn(const char *what) const { return std::string(stem) + what; }
    u8 *runs(Coverage &c) const { return sg ? c.sruns.as<u8>() : c.runs.as<u8>(); }
    u64 count(const Coverage &c) const { return sg ? c.snruns : c.nruns; }
    std::vector<u64> &ranges(Coverage &c) const { return sg ? c.sranges : c.ranges; }
};
extern const CvKind CV_DEPTH;

int coverage_range(pmx_dbam *b, const CvKind &K, const std::string &fn, int64_t first, int64_t n)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (b->cv.state != CV_RUNS) return fail(PMX_DBAM_ERR_INVALID, fn + ": no runs: call pmx_dbam_coverage_finish first");
    if (K.sg && !b->cv.shave) return fail(PMX_DBAM_ERR_INVALID, fn + ": no signal: call pmx_dbam_coverage_signal first");
    const u64 nruns = K.count(b->cv);
    if (first < 0 || n < 0 || (u64)first > nruns || (u64)n > nruns - (u64)first) return fail(PMX_DBAM_ERR_INVALID, fn + ": range outside the runs");
    return 0;
}

// depth: the fourth column as it is kept, a u32 depth or the bits of a float32 value
int coverage_runs_impl(pmx_dbam *b, const CvKind &K, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *depth)
{
    const std::string fn = K.fn("runs");
    if (int rc = coverage_range(b, K, fn, first, n)) return rc;
    if (!ref || !start || !end || !depth) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    if (n == 0) return 0;
    const CvRuns V(K.runs(b->cv), K.count(b->cv));
    HIPOK(hipMemcpy(ref, V.ref + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(start, V.start + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(end, V.end + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(depth, V.depth + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    return 0;
}

// The text of m >= 1 lines, one lane per line (`fn`: the entry point, its range checked; `lines`: their policy, k_ln_len).
// buf NULL: the size.
template <class L> int64_t coverage_text_pull(pmx_dbam *b, const std::string &fn, u64 m, uint8_t *buf, int64_t cap, L lines)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    const u64 nwg = (m + 255) / 256, nref = b->ref_names.size();
    const u32 *noff = b->cv.names.as<u32>();
    const u8 *names = b->cv.names.as<u8>() + 4 * (nref + 1);
    DevAlloc d_len, d_w, d_wb, d_tot, d_text;
    CvHold held(b);
    held.add(4 * m + 12 * nwg + 16);
    HIPOK(hipMalloc(&d_len.p, 4 * m));
    HIPOK(hipMalloc(&d_w.p, 4 * nwg));
    HIPOK(hipMalloc(&d_wb.p, 8 * nwg));
    HIPOK(hipMalloc(&d_tot.p, 16));
    hipLaunchKernelGGL(k_ln_len<L>, dim3((unsigned)nwg), dim3(256), 0, st, lines, m, noff, d_len.as<u32>(), d_w.as<u32>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_w.as<u32>(), d_w.as<u32>(), nwg, d_wb.as<u64>(), d_tot.as<u64>());
    HIPOK(hipGetLastError());
    u64 bytes = 0;
    HIPOK(hipMemcpyAsync(&bytes, d_tot.p, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (!buf) return (int64_t)bytes;
    if ((u64)cap < bytes) return fail(PMX_DBAM_ERR_INVALID, fn + ": the buffer is too small: " + std::to_string(bytes) + " bytes are needed");
    if (hipMalloc(&d_text.p, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(bytes) + " bytes of text");
    }
    held.add(bytes);
    hipLaunchKernelGGL(k_ln_text<L>, dim3((unsigned)nwg), dim3(256), 0, st, lines, m, noff, names, d_len.as<u32>(), d_wb.as<u64>(), d_text.as<u8>());
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(buf, d_text.p, bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return (int64_t)bytes;
}

// CvKind::text: the line policy L (LnDepth, LnSignal) over the four columns of the runs from `first`
template <class L> int64_t coverage_lines(pmx_dbam *b, const std::string &fn, const CvRuns &V, int64_t first, u64 m, uint8_t *buf, int64_t cap)
{
    return coverage_text_pull(b, fn, m, buf, cap, L{V.ref + first, V.start + first, V.end + first, V.depth + first});
}

int64_t coverage_text_impl(pmx_dbam *b, const CvKind &K, int64_t first, int64_t n, uint8_t *buf, int64_t cap)
{
    const std::string fn = K.fn("text");
    if (int rc = coverage_range(b, K, fn, first, n)) return rc;
    if (buf && cap < 0) return fail(PMX_DBAM_ERR_INVALID, fn + ": a negative capacity");
    if (n == 0) return 0;
    return K.text(b, fn, CvRuns(K.runs(b->cv), K.count(b->cv)), first, (u64)n, buf, cap);
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_begin(pmx_dbam *b, uint32_t extend, const uint8_t *use_ref)
{
    return guarded("pmx_dbam_coverage_begin", [&] { return coverage_begin_impl(b, extend, use_ref); });
}

int pmx_dbam_coverage_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t *reads_added)
{
    return guarded("pmx_dbam_coverage_add", [&] { return coverage_add_impl(b, mapq_min, flag_exclude, reads_added); });
}

int pmx_dbam_coverage_finish(pmx_dbam *b, uint64_t totals[5])
{
    return guarded("pmx_dbam_coverage_finish", [&] { return coverage_finish_impl(b, totals); });
}

int pmx_dbam_coverage_runs(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *depth)
{
    return guarded("pmx_dbam_coverage_runs", [&] { return coverage_runs_impl(b, CV_DEPTH, first, n, ref, start, end, depth); });
}

int64_t pmx_dbam_coverage_text(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap)
{
    return guarded("pmx_dbam_coverage_text", [&] { return coverage_text_impl(b, CV_DEPTH, first, n, buf, cap); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------------
// The pileup as the parts of a bigWig file (DESIGN.md 7.18.1): pmx_dbam_coverage_ranges / _sections / _zoom_begin / _zoom_records,
// all of them on the runs finish left.  The host puts the file together (pymasc_amd/coverage.py: assemble_bigwig); what it takes
// from here are bytes it never parses and a table per pull that says where each section begins and ends.
//
//   k_cv_ranges      one lane per run: the first run of a reference writes its index (the host closes the references without one)
//   k_tr_sections<V> one lane per run of a range of ONE reference: its 12-byte item (start0, end0, float32 depth) behind the 24-byte
//                    header of its section; a section's first lane writes the header and the table row.  V (TrDepth here, TrSignal in
//                    signal_device.inc) says what the kept fourth column and a zoom slot hold: it is all the two kinds differ in
//   k_cv_zoom_fill   one lane per run: the bins of level 0 its run overlaps take its bases, depth, bases * depth and
//                    bases * depth^2 by return-less integer atomics (add, min, max, 64-bit add); the sum of squares and the smallest
//                    depth of the whole pileup are reduced over the wave, one atomic each per wave
//   k_cv_zoom_fold   one lane per bin of level k + 1: its up to four bins of level k, no atomics
//   k_cv_zoom_keep / k_bam_scan / k_tr_zoom_emit<V>   the bins with a covered base, compacted by ballots into 32-byte records in
//                    (id, start) order; integers become float32 by round-to-nearest-even; the table row of a section is written by
//                    its first and its last record
// Every accumulator is an integer, so the records do not depend on the order the atomics arrive in.  Bound: a u64 sum of squares is
// exact while max_depth * fragment_bases < 2^64; zoom_begin refuses beyond it.  Device memory: 28 bytes per bin of level 0 and about a
// third of that again for the higher levels, from zoom_begin until the last level is pulled; 12 bytes per run + 44 per section inside
// sections; 12 per 256 bins + 32 per record + 20 per section inside zoom_records.

namespace {

struct ZmBins {         // the arrays of one level in its block
    u64 *sum, *sq;
    u32 *cnt, *mn, *mx;
    __host__ __device__ ZmBins(u8 *p, u64 n)
        : sum((u64 *)p), sq((u64 *)(p + 8 * n)), cnt((u32 *)(p + 16 * n)), mn((u32 *)(p + 20 * n)), mx((u32 *)(p + 24 * n))
    {
    }
};

struct TrDepth {        // the depth runs: a u32 depth, and a slot of integers that become float32 by round-to-nearest-even
    static __device__ __forceinline__ u32 item(u32 depth) { return __float_as_uint(__uint2float_rn(depth)); }
    static __device__ __forceinline__ void stats(const ZmBins &B, u64 b, u32 *p)      // min, max, sum, sum of squares
    {
        p[0] = __float_as_uint(__uint2float_rn(B.mn[b]));
        p[1] = __float_as_uint(__uint2float_rn(B.mx[b]));
        p[2] = __float_as_uint(__ull2float_rn((unsigned long long)B.sum[b]));
        p[3] = __float_as_uint(__ull2float_rn((unsigned long long)B.sq[b]));
    }
};

}  // namespace

__global__ void __launch_bounds__(256) k_cv_ranges(const int *__restrict__ rref, u64 n, unsigned long long *__restrict__ first)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const int r = rref[i];
    if (i == 0 || rref[i - 1u] != r) first[r] = i;
}

// out: u32 words; run i of the range lies behind the headers of sections 0 .. i / ips: word 6 * (i / ips + 1) + 3 * i
template <class V>
__global__ void __launch_bounds__(256) k_tr_sections(const u32 *__restrict__ rstart, const u32 *__restrict__ rend, const u32 *__restrict__ rval,
                                                     u64 n, u32 ips, u32 id, u32 *__restrict__ out, u32 *__restrict__ table)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 sec = i / ips;
    u32 *p = out + 6u * (sec + 1u) + 3u * i;
    const u32 a = rstart[i];
    p[0] = a;
    p[1] = rend[i];
    p[2] = V::item(rval[i]);
    if (i == sec * ips) {
        const u64 last = i + ips - 1u < n - 1u ? i + ips - 1u : n - 1u;
        const u32 cnt = (u32)(last - i) + 1u, z = rend[last];
        u32 *h = p - 6;
        h[0] = id;
        h[1] = a;
        h[2] = z;
        h[3] = 0;                           // itemStep
        h[4] = 0;                           // itemSpan
        h[5] = 1u | (cnt << 16);            // type 1 (bedGraph), a reserved byte, itemCount
        u32 *T = table + 5u * sec;
        T[0] = id;
        T[1] = a;
        T[2] = id;
        T[3] = z;
        T[4] = 24u + 12u * cnt;
    }
}

// tot[0] += sum (end0 - start0) * depth^2, tot[1] = min(tot[1], depth); bins == nullptr: no level, the two totals alone
__global__ void __launch_bounds__(256) k_cv_zoom_fill(const int *__restrict__ rref, const u32 *__restrict__ rstart, const u32 *__restrict__ rend,
                                                      const u32 *__restrict__ rdepth, u64 n, const u32 *__restrict__ idof,
                                                      const u64 *__restrict__ off0, u32 z, u64 nb, u8 *__restrict__ bins,
                                                      unsigned long long *__restrict__ tot)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    u64 q = 0;
    u32 dmin = 0xffffffffu;
    if (i < n) {
        const u32 s = rstart[i], e = rend[i], d = rdepth[i];
        q = (u64)(e - s) * d * d;
        dmin = d;
        if (bins) {
            const ZmBins B(bins, nb);
            const u64 b0 = off0[idof[rref[i]]];
            const u32 j1 = (e - 1u) / z;                      // (e > s >= 0 and e <= the reference's length: bin j1 exists)
            for (u32 j = s / z; j <= j1; j++) {
                const u64 lo = (u64)j * z, hi = lo + z;
                const u64 w = (e < hi ? (u64)e : hi) - (s > lo ? (u64)s : lo);
                const u64 b = b0 + j;
                atomicAdd(&B.cnt[b], (u32)w);
                atomicMin(&B.mn[b], d);
                atomicMax(&B.mx[b], d);
                atomicAdd((unsigned long long *)&B.sum[b], (unsigned long long)(w * d));
                atomicAdd((unsigned long long *)&B.sq[b], (unsigned long long)(w * d * d));
            }
        }
    }
    q = cx_wave_sum(q);
    for (int o = 32; o > 0; o >>= 1) {
        const u32 y = __shfl_xor(dmin, o, 64);
        dmin = y < dmin ? y : dmin;
    }
    if (lane == 0 && dmin != 0xffffffffu) {
        atomicAdd(&tot[0], (unsigned long long)q);
        atomicMin(&tot[1], (unsigned long long)dmin);
    }
}

// the last id of off[0, nc] whose first bin is not behind `b` (b < off[nc]; an id without bins is never the answer)
__device__ __forceinline__ u32 cv_zoom_id(const u64 *__restrict__ off, u32 nc, u64 b)
{
    u32 a = 0, z = nc;
    while (z - a > 1u) {
        const u32 mid = (a + z) / 2u;
        if (off[mid] <= b) a = mid;
        else z = mid;
    }
    return a;
}

__global__ void __launch_bounds__(256) k_cv_zoom_fold(u8 *__restrict__ src, u64 nsrc, u8 *__restrict__ dst, u64 ndst,
                                                      const u64 *__restrict__ offs, const u64 *__restrict__ offd, u32 nc)
{
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    if (b >= ndst) return;
    const ZmBins S(src, nsrc), D(dst, ndst);
    const u32 id = cv_zoom_id(offd, nc, b);
    const u64 j = b - offd[id], ns = offs[id + 1u] - offs[id];
    const u64 c0 = offs[id] + 4u * j, c1 = offs[id] + (4u * j + 4u < ns ? 4u * j + 4u : ns);     // (the last group may be short)
    u64 sum = 0, sq = 0;
    u32 cnt = 0, mn = 0xffffffffu, mx = 0;
    for (u64 c = c0; c < c1; c++) {
        sum += S.sum[c];
        sq += S.sq[c];
        cnt += S.cnt[c];
        mn = S.mn[c] < mn ? S.mn[c] : mn;
        mx = S.mx[c] > mx ? S.mx[c] : mx;
    }
    D.sum[b] = sum;
    D.sq[b] = sq;
    D.cnt[b] = cnt;
    D.mn[b] = mn;
    D.mx[b] = mx;
}

__global__ void __launch_bounds__(256) k_cv_zoom_keep(const u32 *__restrict__ cnt, u64 n, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    cv_count(b < n && cnt[b] != 0, kcnt, s_w);
}

// out: 8 u32 words per record; total[0]: the records of the level (k_bam_scan's total)
template <class V>
__global__ void __launch_bounds__(256) k_tr_zoom_emit(u8 *__restrict__ bins, u64 n, const u64 *__restrict__ off, const u32 *__restrict__ lens,
                                                      u32 nc, u32 z, u32 ips, const u64 *__restrict__ kbase, const u64 *__restrict__ total,
                                                      u32 *__restrict__ out, u32 *__restrict__ table)
{
    __shared__ u32 s_w[4];
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    const ZmBins B(bins, n);
    const bool keep = b < n && B.cnt[b] != 0;
    const u64 o = cv_slot(keep, kbase, s_w);
    if (!keep) return;
    const u32 id = cv_zoom_id(off, nc, b);
    const u64 a = (b - off[id]) * z;
    const u32 start = (u32)a, end = a + z < (u64)lens[id] ? (u32)(a + z) : lens[id];
    u32 *p = out + 8u * o;
    p[0] = id;
    p[1] = start;
    p[2] = end;
    p[3] = B.cnt[b];
    V::stats(B, b, p + 4);
    const u64 sec = o / ips;
    const u32 k = (u32)(o - sec * ips);
    u32 *T = table + 5u * sec;
    if (k == 0) {
        T[0] = id;
        T[1] = start;
    }
    if (k == ips - 1u || o + 1u == total[0]) {
        T[2] = id;
        T[3] = end;
        T[4] = 32u * (k + 1u);
    }
}

namespace {

// deflate_device.inc: the upper bound of nsec sections (`full` raw bytes each, the last one `last`) as zlib streams, and the streams
u64 df_sections_bound(u64 nsec, u64 full, u64 last);
int64_t df_sections_out(pmx_dbam *b, CvHold &held, const std::string &fn, const u8 *d_raw, u64 nsec, u64 full, u64 last, uint8_t *buf,
                        int64_t cap, uint32_t *zsizes);

void zoom_drop(Coverage &c)
{
    c.zbins = DevAlloc{};
    c.ztab = DevAlloc{};
    c.bytes -= std::min(c.zbytes, c.bytes);
    c.zbytes = 0;
    c.zlevels = c.z0 = 0;
    c.znb.clear();
    c.zoff.clear();
}

// the first run of every chosen reference in header order, one more entry closing them; computed once per pileup
int coverage_ranges_make(pmx_dbam *b, const CvKind &K)
{
    Coverage &c = b->cv;
    std::vector<u64> &ranges = K.ranges(c);
    const u64 nruns = K.count(c);
    if (!ranges.empty()) return 0;
    const u64 nref = b->ref_names.size(), nc = c.chosen.size();
    std::vector<u64> first(std::max<u64>(nref, 1), ~0ull);
    HIPOK(hipSetDevice(b->device));
    if (nruns) {
        DevAlloc d_first;
        CvHold held(b);
        held.add(8 * first.size());
        HIPOK(hipMalloc(&d_first.p, 8 * first.size()));
        HIPOK(hipMemsetAsync(d_first.p, 0xff, 8 * first.size(), b->stream));
        hipLaunchKernelGGL(k_cv_ranges, dim3((unsigned)((nruns + 255) / 256)), dim3(256), 0, b->stream, CvRuns(K.runs(c), nruns).ref, nruns,
                           d_first.as<unsigned long long>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(first.data(), d_first.p, 8 * first.size(), hipMemcpyDeviceToHost, b->stream));
        HIPOK(hipStreamSynchronize(b->stream));
    }
    std::vector<u64> r(nc + 1, nruns);
    for (u64 k = nc; k-- > 0;) r[k] = first[(u64)c.chosen[k]] != ~0ull ? first[(u64)c.chosen[k]] : r[k + 1];
    for (u64 k = 0; k < nc; k++)
        if (r[k] > r[k + 1]) return fail(PMX_DBAM_ERR_INVALID, K.fn("ranges") + ": the runs are not in header order");
    ranges = std::move(r);
    return 0;
}

int64_t coverage_ranges_impl(pmx_dbam *b, const CvKind &K, int64_t *first, int64_t cap)
{
    const std::string fn = K.fn("ranges");
    if (int rc = coverage_range(b, K, fn, 0, 0)) return rc;
    const int64_t n = (int64_t)b->cv.chosen.size() + 1;
    if (!first) return n;
    if (cap < n) return fail(PMX_DBAM_ERR_INVALID, fn + ": the buffer is too small: " + std::to_string(n) + " entries are needed");
    if (int rc = coverage_ranges_make(b, K)) return rc;
    for (int64_t k = 0; k < n; k++) first[k] = (int64_t)K.ranges(b->cv)[(u64)k];
    return n;
}

// z: every section as a zlib stream (pmx_dbam_coverage_sections_z), the streams' lengths in zsizes; sums (a kind that has them):
// sums[section][2], the section's sum and sum of squares
int64_t coverage_sections_impl(pmx_dbam *b, const CvKind &K, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items,
                               uint8_t *buf, int64_t cap, uint32_t *table, int64_t table_cap, bool z = false, uint32_t *zsizes = nullptr,
                               double *sums = nullptr)
{
    const std::string fn = K.fn(z ? "sections_z" : "sections");
    if (int rc = coverage_range(b, K, fn, first, n)) return rc;
    if (items < 1 || items > 65535) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": 1 to 65535 items per section");
    if (z && 24ull + 12ull * items > PMX_DEFLATE_MAX_CHUNK)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": at most 5459 items per section (a chunk of the encoder holds 65536 bytes)");
    if (buf && (cap < 0 || table_cap < 0)) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": a negative capacity");
    if (n == 0) return 0;
    if (int rc = coverage_ranges_make(b, K)) return rc;
    Coverage &c = b->cv;
    const std::vector<u64> &ranges = K.ranges(c);
    const auto it = std::upper_bound(ranges.begin(), ranges.end(), (u64)first);       // (the first reference that begins behind `first`)
    if (it == ranges.end() || (u64)first + (u64)n > *it) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": the range holds two references");
    const u64 m = (u64)n, nsec = (m + items - 1) / items, bytes = 24 * nsec + 12 * m;
    const u64 full = 24 + 12ull * items, last = bytes - (nsec - 1) * full;
    if (!buf) return (int64_t)(z ? df_sections_bound(nsec, full, last) : bytes);
    if (!z && (u64)cap < bytes)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": the buffer is too small: " + std::to_string(bytes) + " bytes are needed");
    if (!table || (u64)table_cap < nsec)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": the table is too small: " + std::to_string(nsec) + " rows are needed");
    if ((z && !zsizes) || (K.sums && !sums)) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": null output");
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    DevAlloc d_out, d_sums;
    CvHold held(b);
    if (hipMalloc(&d_out.p, bytes + 20 * nsec) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PMX_DBAM_ERR_OPEN, std::string(fn) + ": out of device memory for " + std::to_string(bytes + 20 * nsec) + " bytes of sections");
    }
    held.add(bytes + 20 * nsec);
    const CvRuns V(K.runs(c), K.count(c));
    u32 *d_table = (u32 *)(d_out.as<u8>() + bytes);
    if (K.sums) {
        HIPOK(hipMalloc(&d_sums.p, 16 * nsec));
        held.add(16 * nsec);
        hipLaunchKernelGGL(K.sums, dim3((unsigned)((nsec + 255) / 256)), dim3(256), 0, st, V.start + first, V.end + first, V.depth + first, m, items,
                           d_sums.as<double>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(sums, d_sums.p, 16 * nsec, hipMemcpyDeviceToHost, st));
    }
    hipLaunchKernelGGL(K.sections, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, V.start + first, V.end + first, V.depth + first, m, items,
                       chrom_id, d_out.as<u32>(), d_table);
    HIPOK(hipGetLastError());
    if (!z) HIPOK(hipMemcpyAsync(buf, d_out.p, bytes, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(table, d_table, 20 * nsec, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return z ? df_sections_out(b, held, fn, d_out.as<u8>(), nsec, full, last, buf, cap, zsizes) : (int64_t)bytes;
}

// level 0 of the depth runs: k_cv_zoom_fill, which also reduces the two totals
int cv_zoom_fill(pmx_dbam *b, const u32 *, const u32 *d_idof, const u64 *d_off, const u32 *, u32 z0, u64 nb0, u8 *bins, unsigned long long *d_tot)
{
    const Coverage &c = b->cv;
    if (!c.nruns) return 0;
    const CvRuns V(c.runs.as<u8>(), c.nruns);
    hipLaunchKernelGGL(k_cv_zoom_fill, dim3((unsigned)((c.nruns + 255) / 256)), dim3(256), 0, b->stream, V.ref, V.start, V.end, V.depth, c.nruns, d_idof,
                       d_off, z0, nb0, bins, d_tot);
    HIPOK(hipGetLastError());
    return 0;
}
const CvKind CV_DEPTH = {false, "pmx_dbam_coverage_", coverage_lines<LnDepth>, k_tr_sections<TrDepth>, nullptr, cv_zoom_fill,
                         k_cv_zoom_fold, k_tr_zoom_emit<TrDepth>};

// out: the depth's two totals (the signal has none: its summary comes from signal's totals and the sections' sums; 0, 0)
int coverage_zoom_begin_impl(pmx_dbam *b, const CvKind &K, uint32_t z0, uint32_t levels, const uint32_t *chrom_id, uint64_t *out)
{
    const std::string fn = K.fn("zoom_begin");
    if (int rc = coverage_range(b, K, fn, 0, 0)) return rc;
    if (!out || !chrom_id) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": null " + (out ? "chromosome ids" : "output"));
    out[0] = out[1] = 0;
    Coverage &c = b->cv;
    if (levels > PMX_COVERAGE_ZOOM_LEVELS || (levels && z0 < 1)) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": at most 10 levels, and a reduction of at least 1");
    if (!K.sg && (unsigned __int128)c.tot[4] * c.tot[3] >> 64)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": max_depth * fragment_bases is 2^64 or more: the sums of squares would not be exact");
    const u64 nref = b->ref_names.size(), nc = c.chosen.size();
    std::vector<u32> idof(std::max<u64>(nref, 1), 0), lens(nc, 0);
    std::vector<u8> seen(nc, 0);
    for (u64 k = 0; k < nc; k++) {
        const u32 id = chrom_id[c.chosen[k]];
        if (id >= nc || seen[id]) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": the chosen references' ids are not 0 .. n - 1, each once");
        seen[id] = 1;
        idof[(u64)c.chosen[k]] = id;
        lens[id] = (u32)std::max<int64_t>(b->ref_lens[(u64)c.chosen[k]], 0);
    }
    zoom_drop(c);
    std::vector<u64> off((u64)levels * (nc + 1), 0), znb(levels, 0), zoff(levels, 0);
    u64 z = z0, bin_bytes = 0;
    for (u32 k = 0; k < levels; k++, z *= 4) {
        if (z > 0xffffffffull) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": a reduction of 2^32 or more");
        u64 *o = off.data() + (u64)k * (nc + 1);
        for (u64 id = 0; id < nc; id++) o[id + 1] = o[id] + ((u64)lens[id] + z - 1) / z;
        znb[k] = o[nc];
        zoff[k] = bin_bytes;
        bin_bytes += (28 * znb[k] + 7) / 8 * 8;
    }
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    const u64 tab_bytes = 8 * off.size() + 4 * idof.size() + 4 * std::max<u64>(nc, 1);
    HIPOK(hipMalloc(&c.ztab.p, tab_bytes));
    if (bin_bytes && hipMalloc(&c.zbins.p, bin_bytes) != hipSuccess) {
        (void)hipGetLastError();
        c.ztab = DevAlloc{};
        return fail(PMX_DBAM_ERR_OPEN, std::string(fn) + ": out of device memory for the zoom bins: " + std::to_string(bin_bytes) +
                                           " bytes asked for (28 per bin of " + std::to_string(z0) + " bases, and a third again)");
    }
    c.zbytes = tab_bytes + bin_bytes;
    c.bytes += c.zbytes;
    if (b->st) stream_note(*b);
    c.zlevels = levels;
    c.zsg = K.sg;
    c.z0 = z0;
    c.znb = znb;
    c.zoff = zoff;
    struct Drop {       // a failure from here on leaves no bins
        Coverage &c;
        bool ok = false;
        ~Drop()
        {
            if (!ok) zoom_drop(c);
        }
    } drop{c};
    u64 *d_off = c.ztab.as<u64>();
    u32 *d_idof = (u32 *)(d_off + off.size()), *d_lens = d_idof + idof.size();
    if (!off.empty()) HIPOK(hipMemcpyAsync(d_off, off.data(), 8 * off.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_idof, idof.data(), 4 * idof.size(), hipMemcpyHostToDevice, st));
    if (nc) HIPOK(hipMemcpyAsync(d_lens, lens.data(), 4 * nc, hipMemcpyHostToDevice, st));
    unsigned long long tot[2] = {0, ~0ull};
    DevAlloc d_tot;
    HIPOK(hipMalloc(&d_tot.p, 16));
    HIPOK(hipMemcpyAsync(d_tot.p, tot, 16, hipMemcpyHostToDevice, st));
    if (levels && znb[0]) {
        const ZmBins B(c.zbins.as<u8>(), znb[0]);
        HIPOK(hipMemsetAsync(c.zbins.p, 0, 28 * znb[0], st));
        HIPOK(hipMemsetAsync(B.mn, 0xff, 4 * znb[0], st));
    }
    if (int rc = K.fill(b, idof.data(), d_idof, d_off, d_lens, z0, levels ? znb[0] : 0, levels && znb[0] ? c.zbins.as<u8>() : (u8 *)nullptr, d_tot.as<unsigned long long>()))
        return rc;
    for (u32 k = 0; k + 1 < levels; k++) {
        if (!znb[k + 1]) continue;
        hipLaunchKernelGGL(K.fold, dim3((unsigned)((znb[k + 1] + 255) / 256)), dim3(256), 0, st, c.zbins.as<u8>() + zoff[k], znb[k],
                           c.zbins.as<u8>() + zoff[k + 1], znb[k + 1], d_off + (u64)k * (nc + 1), d_off + (u64)(k + 1) * (nc + 1), (u32)nc);
        HIPOK(hipGetLastError());
    }
    HIPOK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));       // (off, idof and lens are locals)
    out[0] = K.sg ? 0 : tot[0];
    out[1] = !K.sg && c.nruns ? tot[1] : 0;
    drop.ok = true;
    if (!levels) zoom_drop(c);              // (nothing to pull)
    return 0;
}

int64_t coverage_zoom_records_impl(pmx_dbam *b, const CvKind &K, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap,
                                   uint32_t *table, int64_t table_cap, bool zs = false, uint32_t *zsizes = nullptr)
{
    const std::string fn = K.fn(zs ? "zoom_records_z" : "zoom_records");
    if (int rc = coverage_range(b, K, fn, 0, 0)) return rc;
    Coverage &c = b->cv;
    if (level >= c.zlevels || c.zsg != K.sg) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": no bins of that level: call " + K.fn("zoom_begin") + " first");
    if (items < 1) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": at least 1 item per section");
    if (zs && 32ull * items > PMX_DEFLATE_MAX_CHUNK)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": at most 2048 items per section (a chunk of the encoder holds 65536 bytes)");
    if (buf && (cap < 0 || table_cap < 0)) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": a negative capacity");
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    const u64 nb = c.znb[level], nwg = (nb + 255) / 256, nc = c.chosen.size();
    u8 *bins = c.zbins.as<u8>() + c.zoff[level];
    u64 total = 0;
    DevAlloc d_k, d_kb, d_tot, d_out;
    CvHold held(b);
    if (nwg) {
        held.add(12 * nwg + 16);
        HIPOK(hipMalloc(&d_k.p, 4 * nwg));
        HIPOK(hipMalloc(&d_kb.p, 8 * nwg));
        HIPOK(hipMalloc(&d_tot.p, 16));
        hipLaunchKernelGGL(k_cv_zoom_keep, dim3((unsigned)nwg), dim3(256), 0, st, ZmBins(bins, nb).cnt, nb, d_k.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), nwg, d_kb.as<u64>(), d_tot.as<u64>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&total, d_tot.p, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
    }
    const u64 bytes = 32 * total, nsec = (total + items - 1) / items, full = 32ull * items, last = nsec ? bytes - (nsec - 1) * full : 0;
    if (!buf) return (int64_t)(zs ? df_sections_bound(nsec, full, last) : bytes);
    if (!zs && (u64)cap < bytes)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": the buffer is too small: " + std::to_string(bytes) + " bytes are needed");
    if (!table || (u64)table_cap < nsec)
        return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": the table is too small: " + std::to_string(nsec) + " rows are needed");
    if (zs && !zsizes) return fail(PMX_DBAM_ERR_INVALID, std::string(fn) + ": null output");
    int64_t written = (int64_t)bytes;
    if (total) {
        if (hipMalloc(&d_out.p, bytes + 20 * nsec) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PMX_DBAM_ERR_OPEN, std::string(fn) + ": out of device memory for " + std::to_string(bytes + 20 * nsec) + " bytes of records");
        }
        held.add(bytes + 20 * nsec);
        const u64 *d_off = c.ztab.as<u64>() + (u64)level * (nc + 1);
        const u32 *d_lens = (const u32 *)(c.ztab.as<u64>() + (u64)c.zlevels * (nc + 1)) + std::max<u64>(b->ref_names.size(), 1);
        u64 z = c.z0;
        for (u32 k = 0; k < level; k++) z *= 4;
        u32 *d_table = (u32 *)(d_out.as<u8>() + bytes);
        hipLaunchKernelGGL(K.emit, dim3((unsigned)nwg), dim3(256), 0, st, bins, nb, d_off, d_lens, (u32)nc, (u32)z, items, d_kb.as<u64>(),
                           d_tot.as<u64>(), d_out.as<u32>(), d_table);
        HIPOK(hipGetLastError());
        if (!zs) HIPOK(hipMemcpyAsync(buf, d_out.p, bytes, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(table, d_table, 20 * nsec, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (zs && (written = df_sections_out(b, held, fn, d_out.as<u8>(), nsec, full, last, buf, cap, zsizes)) < 0) return written;
    }
    if (level + 1 == c.zlevels) zoom_drop(c);       // the last level is out: the bins are freed
    return written;
}

}  // namespace

extern "C" {

int64_t pmx_dbam_coverage_ranges(pmx_dbam *b, int64_t *first, int64_t cap)
{
    return guarded("pmx_dbam_coverage_ranges", [&] { return coverage_ranges_impl(b, CV_DEPTH, first, cap); });
}

int64_t pmx_dbam_coverage_sections(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                   uint32_t *table, int64_t table_cap)
{
    return guarded("pmx_dbam_coverage_sections", [&] { return coverage_sections_impl(b, CV_DEPTH, first, n, chrom_id, items, buf, cap, table, table_cap); });
}

int pmx_dbam_coverage_zoom_begin(pmx_dbam *b, uint32_t z0, uint32_t levels, const uint32_t *chrom_id, uint64_t out[2])
{
    return guarded("pmx_dbam_coverage_zoom_begin", [&] { return coverage_zoom_begin_impl(b, CV_DEPTH, z0, levels, chrom_id, out); });
}

int64_t pmx_dbam_coverage_zoom_records(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                       int64_t table_cap)
{
    return guarded("pmx_dbam_coverage_zoom_records", [&] { return coverage_zoom_records_impl(b, CV_DEPTH, level, items, buf, cap, table, table_cap); });
}

}  // extern "C"
