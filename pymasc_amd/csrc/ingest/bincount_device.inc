// Read counts per genome bin on the device (pmx_dbam_bincount_*, include/pymasc_amd_ingest.h; DESIGN.md 7.16).  Included at the end
// of bam_device.hip, behind complexity_device.inc: the kept records of a call come from cx_filter, the walk + filter with arrays of
// its own that pmx_dbam_complexity makes (BAM chain, SAM / BED parse table, the region-mask pass), so the arrays, counters and
// runs of the last pmx_dbam_decode stay untouched.
//
//   k_fp_count    one lane per kept read: its extent (its own length, or `extend` bases from its 5' end), clipped to the bins of
//                 its reference, then one 32-bit atomicAdd without a return value per overlapped bin
//   k_fp_hist     one lane per bin, workgroups striding over the table: the counts 0 .. 3 by wave ballots (nearly every bin), the
//                 others below PMX_BINCOUNT_HIST by atomics on a histogram in LDS (16 KB), flushed with one 64-bit global atomic
//                 per non-zero entry; a bin at or above PMX_BINCOUNT_HIST is compacted into `tail` (a ballot, one slot-reserving
//                 atomic per wave); the number of bins and the sum of the counts are reduced per wave, then per workgroup
// Device memory: 4 bytes per bin + 16 bytes per reference with the handle from begin to the next begin or close; 13 bytes per kept
// read inside a call of add.

#define FP_HIST PMX_BINCOUNT_HIST
#define FP_BALLOT 4u                          // the counts 0 .. FP_BALLOT - 1 are tallied by ballot
#define FP_HIST_GRID 2048u                    // workgroups of k_fp_hist at the most

// The extent [lo, hi] of a read (1-based, inclusive; also k_pk_count's, peakcount_device.inc): L = ext, or the read's own length
// when ext is 0; a forward read covers [pos1, pos1 + L - 1], a reverse read [pos1 + read_len - L, pos1 + read_len - 1] (its 5' end
// stays put); both clipped to [1, top].  False: nothing is left of it.
__device__ __forceinline__ bool fp_extent(long long p, long long rl, bool rev, u32 ext, long long top, long long &lo, long long &hi)
{
    const long long L = ext ? (long long)ext : rl;
    lo = rev ? p + rl - L : p;
    hi = rev ? p + rl - 1 : p + L - 1;
    if (lo < 1) lo = 1;
    if (hi > top) hi = top;
    return lo <= hi;
}

// tab[2 * r] = the first bin of reference r in the table (-1: the reference is not chosen), tab[2 * r + 1] = its bins
__global__ void __launch_bounds__(256) k_fp_count(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len,
                                                  const u8 *__restrict__ rev, u64 n, const long long *__restrict__ tab, u32 nref,
                                                  u32 bin, u32 ext, u32 *__restrict__ counts, unsigned long long *__restrict__ added)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    bool hit = false;
    if (i < n && ref[i] >= 0 && (u32)ref[i] < nref) {
        const long long first = tab[2u * (u32)ref[i]], nb = tab[2u * (u32)ref[i] + 1u];
        if (first >= 0 && nb > 0) {
            const long long cover = nb * (long long)bin;     // (<= the reference's length: the clip to it and the binless tail in one)
            long long lo, hi;
            if (fp_extent(pos[i], len[i], rev[i] != 0, ext, cover, lo, hi)) {
                hit = true;
                const long long j1 = (hi - 1) / bin;
                for (long long j = (lo - 1) / bin; j <= j1; j++) atomicAdd(&counts[first + j], 1u);
            }
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

// hist[k] += bins that hold k reads (k < FP_HIST); sums[0] += bins, sums[1] += reads over the bins, sums[2] += bins at or above
// FP_HIST, whose values go to tail[0 .. cap) in any order (the ones past cap are counted only)
__global__ void __launch_bounds__(256) k_fp_hist(const u32 *__restrict__ counts, u64 nbins, unsigned long long *__restrict__ hist,
                                                 unsigned long long *__restrict__ sums, u32 *__restrict__ tail, u64 cap)
{
    __shared__ u32 s_h[FP_HIST];
    __shared__ unsigned long long s_b[FP_BALLOT], s_n, s_t;
    const u32 t = threadIdx.x, lane = t & 63u;
    for (u32 k = t; k < FP_HIST; k += 256u) s_h[k] = 0;
    if (t < FP_BALLOT) s_b[t] = 0;
    if (t == 0) s_n = s_t = 0;
    __syncthreads();
    u64 small[FP_BALLOT], seen = 0, sum = 0;      // (small and seen: the same in every lane of the wave)
    for (u32 k = 0; k < FP_BALLOT; k++) small[k] = 0;
    for (u64 base = (u64)blockIdx.x * 256u; base < nbins; base += (u64)gridDim.x * 256u) {
        const u64 i = base + t;
        const bool on = i < nbins;
        const u32 c = on ? counts[i] : 0u;
        seen += (u64)__popcll(__ballot(on));
        for (u32 k = 0; k < FP_BALLOT; k++) small[k] += (u64)__popcll(__ballot(on && c == k));
        sum += c;
        if (on && c >= FP_BALLOT && c < FP_HIST) atomicAdd(&s_h[c], 1u);
        const bool big = on && c >= FP_HIST;
        const u64 m = __ballot(big);
        if (m) {
            unsigned long long slot = 0;
            if (lane == 0) slot = atomicAdd(&sums[2], (unsigned long long)__popcll(m));
            slot = __shfl(slot, 0, 64) + (u64)__popcll(m & ((1ull << lane) - 1ull));
            if (big && slot < cap) tail[slot] = c;
        }
    }
    sum = cx_wave_sum(sum);
    if (lane == 0) {
        for (u32 k = 0; k < FP_BALLOT; k++)
            if (small[k]) atomicAdd(&s_b[k], (unsigned long long)small[k]);
        atomicAdd(&s_n, (unsigned long long)seen);
        atomicAdd(&s_t, (unsigned long long)sum);
    }
    __syncthreads();
    for (u32 k = t; k < FP_HIST; k += 256u) {
        const unsigned long long v = k < FP_BALLOT ? s_b[k] : (unsigned long long)s_h[k];
        if (v) atomicAdd(&hist[k], v);
    }
    if (t == 0) {
        if (s_n) atomicAdd(&sums[0], s_n);
        if (s_t) atomicAdd(&sums[1], s_t);
    }
}

namespace {

int bincount_begin_impl(pmx_dbam *b, u32 bin_size, u32 extend, const uint8_t *use_ref)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    b->bc = Bincount{};
    if (bin_size == 0) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_begin: the bin size is 0");
    const u64 nref = b->ref_names.size();
    std::vector<long long> tab(2 * std::max<u64>(nref, 1), 0);
    u64 bins = 0;
    for (u64 r = 0; r < nref; r++) {
        const bool use = !use_ref || use_ref[r] != 0;
        const u64 nb = use && b->ref_lens[r] > 0 ? (u64)b->ref_lens[r] / bin_size : 0;
        tab[2 * r] = use ? (long long)bins : -1;
        tab[2 * r + 1] = (long long)nb;
        bins += nb;
    }
    if (bins == 0) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_begin: no chosen reference is as long as one bin");
    if (bins >= (1ull << 31)) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_begin: 2^31 bins or more: choose a larger bin size");
    Bincount &c = b->bc;
    HIPOK(hipMalloc(&c.tab.p, 8 * tab.size()));
    if (hipMalloc(&c.counts.p, 4 * bins) != hipSuccess) {
        c = Bincount{};
        return fail(PMX_DBAM_ERR_OPEN, "pmx_dbam_bincount_begin: out of device memory for the bins");
    }
    HIPOK(hipMemcpyAsync(c.tab.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, b->stream));
    HIPOK(hipMemsetAsync(c.counts.p, 0, 4 * bins, b->stream));
    HIPOK(hipStreamSynchronize(b->stream));       // (tab is a local)
    c.bins = bins;
    c.bin = bin_size;
    c.ext = extend;
    if (b->st) stream_note(*b);
    return 0;
}

int bincount_add_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, uint64_t *reads_added)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!reads_added) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_add: null output");
    *reads_added = 0;
    if (!b->bc.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_add: no table: call pmx_dbam_bincount_begin first");
    Bincount &c = b->bc;
    unsigned long long added = 0;
    const int rc = side_add(b, mapq_min, flag_exclude, 1, &added, [&](const CxRecs &R, hipStream_t st, unsigned long long *d_added) {
        hipLaunchKernelGGL(k_fp_count, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(),
                           R.rev.as<u8>(), R.n, c.tab.as<long long>(), (u32)b->ref_names.size(), c.bin, c.ext, c.counts.as<u32>(), d_added);
    });
    if (rc) return rc;
    c.reads += added;
    *reads_added = added;
    return 0;
}

int64_t bincount_hist_impl(pmx_dbam *b, uint64_t *hist, uint64_t *totals, int64_t cap, uint32_t *tail)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!hist || !totals || cap < 0) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_hist: null output");
    if (!b->bc.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_hist: no table: call pmx_dbam_bincount_begin first");
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    const u64 room = tail ? (u64)cap : 0, nres = FP_HIST + 3u;
    DevAlloc d_res, d_tail;
    HIPOK(hipMalloc(&d_res.p, 8 * nres));
    HIPOK(hipMemsetAsync(d_res.p, 0, 8 * nres, st));
    if (room) HIPOK(hipMalloc(&d_tail.p, 4 * room));
    const u64 nwg = std::min<u64>((b->bc.bins + 255) / 256, FP_HIST_GRID);
    hipLaunchKernelGGL(k_fp_hist, dim3((unsigned)nwg), dim3(256), 0, st, b->bc.counts.as<u32>(), b->bc.bins, d_res.as<unsigned long long>(),
                       d_res.as<unsigned long long>() + FP_HIST, d_tail.as<u32>(), room);
    HIPOK(hipGetLastError());
    std::vector<unsigned long long> res(nres);
    HIPOK(hipMemcpyAsync(res.data(), d_res.p, 8 * nres, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const u64 above = res[FP_HIST + 2], got = std::min<u64>(above, room);
    if (got) HIPOK(hipMemcpy(tail, d_tail.p, 4 * got, hipMemcpyDeviceToHost));
    for (u32 k = 0; k < FP_HIST; k++) hist[k] = res[k];
    totals[0] = res[FP_HIST];
    totals[1] = res[FP_HIST + 1];
    totals[2] = b->bc.reads;
    return (int64_t)(tail ? got : above);
}

int bincount_copy_impl(pmx_dbam *b, int64_t first, int64_t n, uint32_t *counts)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!counts) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_copy: null output");
    if (!b->bc.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_copy: no table: call pmx_dbam_bincount_begin first");
    if (first < 0 || n < 0 || (u64)first > b->bc.bins || (u64)n > b->bc.bins - (u64)first)
        return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_bincount_copy: range outside the table");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    if (n) HIPOK(hipMemcpy(counts, b->bc.counts.as<u32>() + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_bincount_begin(pmx_dbam *b, uint32_t bin_size, uint32_t extend, const uint8_t *use_ref)
{
    return guarded("pmx_dbam_bincount_begin", [&] { return bincount_begin_impl(b, bin_size, extend, use_ref); });
}

int pmx_dbam_bincount_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t *reads_added)
{
    return guarded("pmx_dbam_bincount_add", [&] { return bincount_add_impl(b, mapq_min, flag_exclude, reads_added); });
}

int64_t pmx_dbam_bincount_hist(pmx_dbam *b, uint64_t hist[PMX_BINCOUNT_HIST], uint64_t totals[3], int64_t cap, uint32_t *tail)
{
    return guarded("pmx_dbam_bincount_hist", [&] { return bincount_hist_impl(b, hist, totals, cap, tail); });
}

int pmx_dbam_bincount_copy(pmx_dbam *b, int64_t first, int64_t n, uint32_t *counts)
{
    return guarded("pmx_dbam_bincount_copy", [&] { return bincount_copy_impl(b, first, n, counts); });
}

}  // extern "C"
