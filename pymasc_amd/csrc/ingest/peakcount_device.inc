// Reads per peak line and reads in peaks on the device (pmx_dbam_peakcount_*, include/pymasc_amd_ingest.h; DESIGN.md 7.17).
// Included at the end of bam_device.hip, behind bincount_device.inc and region_mask_device.inc: the lines are clipped, sorted and
// scanned by the mask's kernels (rm_build: k_rm_keys, the radix sort, k_rm_merge), the kept records of a call come from cx_filter
// as in pmx_dbam_bincount_add, and a read's extent is k_fp_count's (fp_extent).
//
// A line (b, e) is 0-based and half-open: it covers the 1-based positions b + 1 .. e, clipped to its reference's length.  A read
// with the clipped extent [lo, hi] is IN the line when b + 1 <= hi and lo <= e.  count[line] = the reads in it (a read in three
// overlapping lines adds 1 to each); n_in = the reads in at least one line, once per read; N = every kept read on a chosen
// reference, in a line or not.
//
//   k_pk_keep     one lane per line: what the mask throws away is kept in sorted order -- the key ref_id << 32 | begin, the
//                 clipped end, pmax = ref_id << 32 | the running maximum of the ends within the reference, and the input line of
//                 every sorted place
//   k_pk_count    one lane per kept read: the last line j of its reference with b + 1 <= hi (binary search over the keys), then
//                 downwards while the line is of the same reference and pmax[j] >= lo -- an earlier line may still reach the read;
//                 a line passed with end >= lo gets one 32-bit atomicAdd without a return value at its input place.  N, n_in and
//                 the pair of the workgroup's first reference are reduced by ballot: one 64-bit atomic per workgroup and counter;
//                 a read of another reference (behind a chromosome boundary) adds to its own pair
// The walk is as long as the lines in front of j whose running maximum reaches the read: one or two for lines that rarely
// overlap, every line of the reference in front of j when one line nests all the others.
// Device memory: 28 bytes per line + 8 per reference with the handle from begin to the next begin or close; 13 bytes per kept
// read inside a call of add.

__global__ void __launch_bounds__(256) k_pk_keep(const u64 *__restrict__ skey, const u32 *__restrict__ perm, const u32 *__restrict__ endc,
                                                 const u64 *__restrict__ pmax, u64 n, u64 *__restrict__ okey, u64 *__restrict__ opmax,
                                                 u32 *__restrict__ oend, u32 *__restrict__ operm)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 j = perm ? perm[i] : (u32)i;
    okey[i] = skey[i];
    opmax[i] = pmax[i];
    oend[i] = endc[j];
    operm[i] = j;
}

// tab[r] = the length of reference r, -1 when it is not chosen; tot[0] += N, tot[1] += n_in, tot[2 + 2 * r + {0, 1}] += the same
// two of reference r
__global__ void __launch_bounds__(256) k_pk_count(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len,
                                                  const u8 *__restrict__ rev, u64 n, const long long *__restrict__ tab, u32 nref, u32 ext,
                                                  const u64 *__restrict__ key, const u32 *__restrict__ end, const u64 *__restrict__ pmax,
                                                  const u32 *__restrict__ perm, u64 nl, u32 *__restrict__ counts,
                                                  unsigned long long *__restrict__ tot)
{
    __shared__ u32 s_w[4][4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    const u64 i0 = (u64)blockIdx.x * 256u;      // (< n: the grid has no workgroup without a record)
    const u32 ref0 = ref[i0] >= 0 ? (u32)ref[i0] : ~0u;
    // `counted` is a compare, not a flag set inside the branches below, and no branch on the wave-uniform `nl` sits inside them
    // (no lines: the search ends at 0 and the walk does not begin).  With the flag set under `if (top >= 0) { ... if (nl && ...)`
    // the compiler (uniform regions are not structurized in this build) gave it to EVERY valid lane of a wave in which one lane
    // entered the branch: a read of a reference that is not chosen was counted in N when its wave also held chosen ones.
    const bool valid = i < n && ref[i] >= 0 && (u32)ref[i] < nref;
    const u32 r = valid ? (u32)ref[i] : 0u;
    const long long top = valid ? tab[r] : -1;
    const bool counted = top >= 0;
    bool in = false;
    long long lo = 1, hi = 0;
    if (counted && fp_extent(pos[i], len[i], rev[i] != 0, ext, top, lo, hi)) {
        const u64 target = ((u64)r << 32) | (u64)(hi - 1 < 0xffffffffll ? hi - 1 : 0xffffffffll);      // b + 1 <= hi
        u64 a = 0, z = nl;                                      // the number of keys <= target
        while (a < z) {
            const u64 mid = (a + z) / 2u;
            if (key[mid] <= target) a = mid + 1u;
            else z = mid;
        }
        for (u64 j = a; j-- > 0;) {
            const u64 pm = pmax[j];
            if ((key[j] >> 32) != (u64)r || (long long)(u32)pm < lo) break;
            if ((long long)end[j] >= lo) {
                atomicAdd(&counts[perm[j]], 1u);
                in = true;
            }
        }
    }
    const bool c0 = counted && r == ref0;
    const u64 m[4] = {__ballot(counted), __ballot(in), __ballot(c0), __ballot(in && c0)};
    if ((t & 63u) == 0)
        for (u32 k = 0; k < 4u; k++) s_w[k][t >> 6] = (u32)__popcll(m[k]);
    if (counted && !c0) {
        atomicAdd(&tot[2u + 2u * r], 1ull);
        if (in) atomicAdd(&tot[3u + 2u * r], 1ull);
    }
    __syncthreads();
    if (t < 4u) {
        const u32 c = s_w[t][0] + s_w[t][1] + s_w[t][2] + s_w[t][3];
        if (c) atomicAdd(t < 2u ? &tot[t] : &tot[2u * ref0 + t], (unsigned long long)c);
    }
}

namespace {

// the arrays of the table in its one block: keys, pmax (8 bytes per line each), ends, places, counts (4 each)
struct PkView {
    u64 *key, *pmax;
    u32 *end, *perm, *cnt;
    PkView(u8 *p, u64 n) : key((u64 *)p), pmax((u64 *)(p + 8 * n)), end((u32 *)(p + 16 * n)), perm((u32 *)(p + 20 * n)), cnt((u32 *)(p + 24 * n)) {}
};

int peakcount_begin_impl(pmx_dbam *b, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end, u32 extend,
                         const uint8_t *use_ref)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    b->pk = Peakcount{};
    RmBuilt B;
    if (int rc = rm_build(b, "pmx_dbam_peakcount_begin", nref, offsets, begin, end, B)) return rc;
    hipStream_t st = b->stream;
    const u64 n = B.n, nr = b->ref_names.size();
    std::vector<long long> tab(std::max<u64>(nr, 1), -1);
    for (u64 r = 0; r < nr; r++)
        if (!use_ref || use_ref[r] != 0) tab[r] = (long long)std::max<int64_t>(b->ref_lens[r], 0);
    // the total length of the merged lines on chosen references
    u64 uni = 0;
    if (B.merged) {
        std::vector<u64> mk(B.merged);
        std::vector<u32> me(B.merged);
        HIPOK(hipMemcpyAsync(mk.data(), B.okey.p, 8 * B.merged, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(me.data(), B.oend.p, 4 * B.merged, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        for (u64 i = 0; i < B.merged; i++)
            if (tab[mk[i] >> 32] >= 0) uni += (u64)me[i] - (u64)(u32)mk[i];
    }
    Peakcount &c = b->pk;
    HIPOK(hipMalloc(&c.tab.p, 8 * tab.size()));
    if (n && hipMalloc(&c.lines.p, 28 * n) != hipSuccess) {
        c = Peakcount{};
        return fail(PMX_DBAM_ERR_OPEN, "pmx_dbam_peakcount_begin: out of device memory for the lines");
    }
    HIPOK(hipMemcpyAsync(c.tab.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, st));
    if (n) {
        const PkView V(c.lines.as<u8>(), n);
        hipLaunchKernelGGL(k_pk_keep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, B.skey, B.perm, B.endc.as<u32>(), B.pmax.as<u64>(), n,
                           V.key, V.pmax, V.end, V.perm);
        HIPOK(hipGetLastError());
        HIPOK(hipMemsetAsync(V.cnt, 0, 4 * n, st));
    }
    HIPOK(hipStreamSynchronize(st));       // (tab and B are locals)
    c.begun = true;
    c.n = n;
    c.uni = uni;
    c.ext = extend;
    c.tot.assign(2 + 2 * std::max<u64>(nr, 1), 0);
    if (b->st) stream_note(*b);
    return 0;
}

int peakcount_add_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, uint64_t *out)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!out) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_add: null output");
    out[0] = out[1] = 0;
    if (!b->pk.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_add: no table: call pmx_dbam_peakcount_begin first");
    Peakcount &c = b->pk;
    const u64 nt = c.tot.size();
    std::vector<unsigned long long> tot(nt, 0);
    const int rc = side_add(b, mapq_min, flag_exclude, nt, tot.data(), [&](const CxRecs &R, hipStream_t st, unsigned long long *d_tot) {
        const PkView V(c.lines.as<u8>(), c.n);
        hipLaunchKernelGGL(k_pk_count, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(),
                           R.rev.as<u8>(), R.n, c.tab.as<long long>(), (u32)b->ref_names.size(), c.ext, V.key, V.end, V.pmax, V.perm, c.n, V.cnt,
                           d_tot);
    });
    if (rc) return rc;
    for (u64 k = 0; k < nt; k++) c.tot[k] += tot[k];
    out[0] = tot[0];
    out[1] = tot[1];
    return 0;
}

int peakcount_copy_impl(pmx_dbam *b, int64_t first, int64_t n, uint32_t *counts)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!counts) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_copy: null output");
    if (!b->pk.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_copy: no table: call pmx_dbam_peakcount_begin first");
    if (first < 0 || n < 0 || (u64)first > b->pk.n || (u64)n > b->pk.n - (u64)first)
        return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_copy: range outside the table");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    if (n) HIPOK(hipMemcpy(counts, PkView(b->pk.lines.as<u8>(), b->pk.n).cnt + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    return 0;
}

int peakcount_totals_impl(pmx_dbam *b, uint64_t *totals, uint64_t *per_ref)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals || !per_ref) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_totals: null output");
    if (!b->pk.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_peakcount_totals: no table: call pmx_dbam_peakcount_begin first");
    totals[0] = b->pk.tot[0];
    totals[1] = b->pk.tot[1];
    totals[2] = b->pk.uni;
    totals[3] = b->pk.n;
    for (u64 k = 0; k < 2 * b->ref_names.size(); k++) per_ref[k] = b->pk.tot[2 + k];
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_peakcount_begin(pmx_dbam *b, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end,
                             uint32_t extend, const uint8_t *use_ref)
{
    return guarded("pmx_dbam_peakcount_begin", [&] { return peakcount_begin_impl(b, nref, offsets, begin, end, extend, use_ref); });
}

int pmx_dbam_peakcount_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t out[2])
{
    return guarded("pmx_dbam_peakcount_add", [&] { return peakcount_add_impl(b, mapq_min, flag_exclude, out); });
}

int pmx_dbam_peakcount_copy(pmx_dbam *b, int64_t first, int64_t n, uint32_t *counts)
{
    return guarded("pmx_dbam_peakcount_copy", [&] { return peakcount_copy_impl(b, first, n, counts); });
}

int pmx_dbam_peakcount_totals(pmx_dbam *b, uint64_t totals[4], uint64_t *per_ref)
{
    return guarded("pmx_dbam_peakcount_totals", [&] { return peakcount_totals_impl(b, totals, per_ref); });
}

}  // extern "C"
