// The strand-aware read profile around anchor sites on the device (pmx_dbam_tss_*, include/pymasc_amd_ingest.h; DESIGN.md 7.22).
// Included at the end of bam_device.hip, behind fragments_device.inc: the kept records of a call come from cx_filter through
// side_add as in pmx_dbam_peakcount_add, a read's extent is k_fp_count's (fp_extent), and the anchors are sorted by cx_sort.
//
// An anchor is (reference, a, s): a 1-based position a and a strand s (+ or -).  Anchors may repeat; each counts separately; those
// on references that are not chosen are dropped.  The reads are the ones the correlation sees, N their number.  A read's extent
// [lo, hi] is fp_extent's with `extend` (0: the read's own length; 1: its 5' base only), clipped to [1, len].  With the flank F
// (1 .. 4095) and W = 2F + 1, a read on an anchor's reference covers, for that anchor, the offsets o = s * (p - a) for p in
// [lo, hi] with |o| <= F; for every such o, same[o + F] += 1 when the read's strand equals the anchor's, opposite[o + F] += 1
// otherwise.  pairs = the (read, anchor) pairs with at least one such offset; n_near = the reads in at least one pair, once each.
//
// The offsets of one pair are one range [o_lo, o_hi] (mirrored for a - anchor), so the table is kept as its differences: +1 at
// o_lo + F, -1 at o_hi + F + 1, in two rows of W + 1 entries (the last one closes the row); pmx_dbam_tss_copy takes the prefix sums.
//
//   k_tss_profile   a workgroup of 256 lanes takes a contiguous run of at most TS_READS kept reads, lane t the reads t, t + 256,
//                   ...  Per read one binary search over the sorted keys ref << 32 | a for the first anchor with a >= lo - F on
//                   its reference; an anchor there with a <= hi + F raises the workgroup's flag in LDS.  Reads are in (reference,
//                   position) order and anchors are few and clustered, so nearly every workgroup ends here: no flag, no table,
//                   no flush, only N.  A flagged workgroup zeroes its private difference table (2 * (W + 1) 32-bit entries of
//                   dynamic LDS, 64 KB at F = 4095), walks each read's anchors upwards while a <= hi + F -- two LDS atomics per
//                   pair, no loop over bases, no global atomic per pair -- and adds the non-zero entries to the global 64-bit
//                   table with one atomic each.  N and n_near are reduced by ballot and popcount, pairs by a wave sum: one 64-bit
//                   atomic per workgroup and counter.
// Device memory: 12 bytes per kept anchor + 16 * (W + 1) for the table + 8 per reference with the handle from begin to the next
// begin or close; 13 bytes per kept read inside a call of add.

#define TS_READS 1024u                        // reads of one workgroup at the most
#define TS_PER_LANE (TS_READS / 256u)

// tab[r] = the length of reference r, -1 when it is not chosen; key / strand: the na anchors in (reference, a) order, strand 1 = '-';
// table[2][2F + 2] += the differences; tot[0] += N, tot[1] += n_near, tot[2] += pairs
__global__ void __launch_bounds__(256) k_tss_profile(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len,
                                                     const u8 *__restrict__ rev, u64 n, const long long *__restrict__ tab, u32 nref, u32 ext,
                                                     u32 flank, const u64 *__restrict__ key, const u32 *__restrict__ strand, u64 na,
                                                     unsigned long long *__restrict__ table, unsigned long long *__restrict__ tot)
{
    // An entry receives at most one +1 or -1 per (read, anchor) pair of the workgroup: TS_READS * PMX_TSS_MAX_ANCHORS = 2^30 < 2^31.
    extern __shared__ int s_diff[];
    __shared__ u32 s_any;
    __shared__ u32 s_w[3][4];
    const u32 t = threadIdx.x;
    const u32 row = 2u * flank + 2u;            // W + 1
    const long long F = (long long)flank;
    const u64 i0 = (u64)blockIdx.x * TS_READS;
    if (t == 0) s_any = 0;
    __syncthreads();
    // the predicates below are compares outside the branches, not flags set inside them (see `counted` in k_pk_count)
    u32 first[TS_PER_LANE], r_of[TS_PER_LANE], np[TS_PER_LANE];
    int lo_of[TS_PER_LANE], hi_of[TS_PER_LANE];
    bool rev_of[TS_PER_LANE], reach_of[TS_PER_LANE];
    u32 c_n = 0;
#pragma unroll
    for (u32 k = 0; k < TS_PER_LANE; k++) {
        const u64 i = i0 + (u64)k * 256u + t;
        const bool valid = i < n && ref[i] >= 0 && (u32)ref[i] < nref;
        const u32 r = valid ? (u32)ref[i] : 0u;
        const long long top = valid ? tab[r] : -1;
        const bool counted = top >= 0;
        const bool rv = counted && rev[i] != 0;
        long long lo = 1, hi = 0;
        const bool has = counted && fp_extent(pos[i], len[i], rv, ext, top, lo, hi);
        const u64 target = ((u64)r << 32) | (u64)(lo - F > 0 ? lo - F : 0);       // the first anchor with a >= lo - F
        const u64 limit = ((u64)r << 32) | (u64)(hi + F);                         // ... and the last with a <= hi + F
        u64 a = 0, z = has ? na : 0;            // the number of keys < target
        while (a < z) {
            const u64 mid = (a + z) / 2u;
            if (key[mid] < target) a = mid + 1u;
            else z = mid;
        }
        const bool reach = has && a < na && key[a] <= limit;
        if (reach) s_any = 1u;
        first[k] = (u32)a;
        r_of[k] = r;
        lo_of[k] = (int)lo;
        hi_of[k] = (int)hi;
        rev_of[k] = rv;
        reach_of[k] = reach;
        c_n += (u32)__popcll(__ballot(counted));
    }
    __syncthreads();
    const bool any = s_any != 0;                // (the same in every lane of the workgroup)
    if (any)
        for (u32 x = t; x < 2u * row; x += 256u) s_diff[x] = 0;
    __syncthreads();
    // the walks stand outside the branch on `any`: a read without an anchor in reach walks nothing
#pragma unroll
    for (u32 k = 0; k < TS_PER_LANE; k++) {
        const long long lo = lo_of[k], hi = hi_of[k];
        const u64 limit = ((u64)r_of[k] << 32) | (u64)(hi + F);
        u32 pairs = 0;
        for (u64 j = reach_of[k] ? (u64)first[k] : na; j < na; j++) {
            const u64 kj = key[j];
            if (kj > limit) break;              // another reference, or a > hi + F
            const long long a = (long long)(u32)kj;
            const bool minus = strand[j] != 0;
            long long o_lo = minus ? a - hi : lo - a, o_hi = minus ? a - lo : hi - a;
            if (o_lo < -F) o_lo = -F;
            if (o_hi > F) o_hi = F;
            int *d = s_diff + (rev_of[k] != minus ? row : 0u);
            atomicAdd(&d[o_lo + F], 1);
            atomicAdd(&d[o_hi + F + 1], -1);
            pairs++;
        }
        np[k] = pairs;
    }
    __syncthreads();
    if (any)
        for (u32 x = t; x < 2u * row; x += 256u) {
            const int v = s_diff[x];
            if (v) atomicAdd(&table[x], (unsigned long long)(long long)v);
        }
    u32 c_near = 0;
    u64 c_pairs = 0;
#pragma unroll
    for (u32 k = 0; k < TS_PER_LANE; k++) {
        c_near += (u32)__popcll(__ballot(np[k] > 0u));
        c_pairs += np[k];
    }
    c_pairs = cx_wave_sum(c_pairs);
    if ((t & 63u) == 0) {
        s_w[0][t >> 6] = c_n;
        s_w[1][t >> 6] = c_near;
        s_w[2][t >> 6] = (u32)c_pairs;
    }
    __syncthreads();
    if (t < 3u) {
        const u32 c = s_w[t][0] + s_w[t][1] + s_w[t][2] + s_w[t][3];
        if (c) atomicAdd(&tot[t], (unsigned long long)c);
    }
}

namespace {

int tss_begin_impl(pmx_dbam *b, int64_t n, const int32_t *ref, const uint32_t *pos1, const uint8_t *reverse, u32 flank, u32 extend,
                   const uint8_t *use_ref)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    b->ts = TssProfile{};
    if (flank < 1u || flank > PMX_TSS_MAX_FLANK)
        return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_begin: the flank is " + std::to_string(flank) + ": it must lie in [1, 4095]");
    if (n < 0 || (n > 0 && (!ref || !pos1 || !reverse))) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_begin: null anchor arrays");
    if (n > (int64_t)PMX_TSS_MAX_ANCHORS) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_begin: more than 2^20 anchors");
    const u64 nr = b->ref_names.size();
    std::vector<long long> tab(std::max<u64>(nr, 1), -1);
    for (u64 r = 0; r < nr; r++)
        if (!use_ref || use_ref[r] != 0) tab[r] = (long long)std::max<int64_t>(b->ref_lens[r], 0);
    std::vector<u64> keys;
    std::vector<u32> strands;
    u64 k_or = 0, k_and = ~0ull;
    for (int64_t i = 0; i < n; i++) {
        if (ref[i] < 0 || (u64)ref[i] >= nr)
            return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_begin: anchor " + std::to_string(i) + ": no such reference");
        if (pos1[i] < 1u || (int64_t)pos1[i] > b->ref_lens[ref[i]])
            return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_begin: anchor " + std::to_string(i) + ": position " + std::to_string(pos1[i]) +
                                                  " is outside " + b->ref_names[ref[i]] + " (1 .. " + std::to_string(b->ref_lens[ref[i]]) + ")");
        if (tab[ref[i]] < 0) continue;          // (its reference is not chosen)
        const u64 key = ((u64)(u32)ref[i] << 32) | (u64)pos1[i];
        keys.push_back(key);
        strands.push_back(reverse[i] != 0 ? 1u : 0u);
        k_or |= key;
        k_and &= key;
    }
    const u64 na = keys.size(), cells = 2ull * (2ull * flank + 2ull);
    hipStream_t st = b->stream;
    TssProfile c;
    HIPOK(hipMalloc(&c.tab.p, 8 * tab.size()));
    HIPOK(hipMalloc(&c.table.p, 8 * cells));
    HIPOK(hipMemcpyAsync(c.tab.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemsetAsync(c.table.p, 0, 8 * cells, st));
    if (na) {       // sorted by (reference, a) with the strand as payload: the digits in which two keys differ
        const u32 ntiles = (u32)((na + BED_RS_TILE - 1) / BED_RS_TILE);
        const u64 ncnt = 256ull * ntiles;
        DevAlloc ka, kb, va, vb, d_cnt, d_base, d_tot;
        HIPOK(hipMalloc(&ka.p, 8 * na));
        HIPOK(hipMalloc(&kb.p, 8 * na));
        HIPOK(hipMalloc(&va.p, 4 * na));
        HIPOK(hipMalloc(&vb.p, 4 * na));
        HIPOK(hipMalloc(&d_cnt.p, 4 * ncnt));
        HIPOK(hipMalloc(&d_base.p, 8 * ncnt));
        HIPOK(hipMalloc(&d_tot.p, 16));
        HIPOK(hipMemcpyAsync(ka.p, keys.data(), 8 * na, hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(va.p, strands.data(), 4 * na, hipMemcpyHostToDevice, st));
        const u64 *kin = ka.as<u64>();
        const u32 *vin = va.as<u32>();
        if (int rc = cx_sort(st, na, k_or ^ k_and, kin, vin, ka.as<u64>(), kb.as<u64>(), va.as<u32>(), vb.as<u32>(), d_cnt.as<u32>(),
                             d_base.as<u64>(), d_tot.as<u64>()))
            return rc;
        HIPOK(hipStreamSynchronize(st));      // (keys and strands are locals, and so is the scratch of the sort)
        c.key = std::move(kin == ka.as<u64>() ? ka : kb);
        c.strand = std::move(vin == va.as<u32>() ? va : vb);
    }
    HIPOK(hipStreamSynchronize(st));          // (tab is a local)
    c.begun = true;
    c.na = na;
    c.flank = flank;
    c.ext = extend;
    b->ts = std::move(c);
    if (b->st) stream_note(*b);
    return 0;
}

int tss_add_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, uint64_t *out)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!out) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_add: null output");
    out[0] = out[1] = 0;
    if (!b->ts.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_add: no table: call pmx_dbam_tss_begin first");
    TssProfile &c = b->ts;
    unsigned long long tot[3] = {0, 0, 0};
    const int rc = side_add(b, mapq_min, flag_exclude, 3, tot, [&](const CxRecs &R, hipStream_t st, unsigned long long *d_tot) {
        const u32 lds = 4u * 2u * (2u * c.flank + 2u);
        hipLaunchKernelGGL(k_tss_profile, dim3((unsigned)((R.n + TS_READS - 1) / TS_READS)), dim3(256), lds, st, R.ref.as<int>(),
                           R.pos.as<int>(), R.len.as<int>(), R.rev.as<u8>(), R.n, c.tab.as<long long>(), (u32)b->ref_names.size(), c.ext,
                           c.flank, c.key.as<u64>(), c.strand.as<u32>(), c.na, c.table.as<unsigned long long>(), d_tot);
    });
    if (rc) return rc;
    c.tot[0] += tot[0];
    c.tot[1] += tot[1];
    c.tot[2] += tot[2];
    out[0] = tot[0];
    out[1] = tot[1];
    return 0;
}

int tss_copy_impl(pmx_dbam *b, uint64_t *profile)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!profile) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_copy: null output");
    if (!b->ts.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_copy: no table: call pmx_dbam_tss_begin first");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    const u64 row = 2ull * b->ts.flank + 2ull, w = row - 1;
    std::vector<long long> diff(2 * row);
    HIPOK(hipMemcpy(diff.data(), b->ts.table.p, 8 * 2 * row, hipMemcpyDeviceToHost));
    for (u64 s = 0; s < 2; s++) {               // the prefix sums, checked before anything is written
        long long sum = 0;
        for (u64 k = 0; k < row; k++) {
            sum += diff[s * row + k];
            if (sum < 0 || (k == w && sum != 0))
                return fail(PMX_DBAM_ERR_DEVICE, "pmx_dbam_tss_copy: the difference table does not close (row " + std::to_string(s) +
                                                     ", entry " + std::to_string(k) + ")");
            diff[s * row + k] = sum;
        }
    }
    for (u64 s = 0; s < 2; s++)
        for (u64 k = 0; k < w; k++) profile[s * w + k] = (uint64_t)diff[s * row + k];
    return 0;
}

int tss_totals_impl(pmx_dbam *b, uint64_t *totals)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_totals: null output");
    if (!b->ts.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_tss_totals: no table: call pmx_dbam_tss_begin first");
    totals[0] = b->ts.tot[0];
    totals[1] = b->ts.tot[1];
    totals[2] = b->ts.na;
    totals[3] = b->ts.tot[2];
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_tss_begin(pmx_dbam *b, int64_t n, const int32_t *ref, const uint32_t *pos1, const uint8_t *reverse, uint32_t flank,
                       uint32_t extend, const uint8_t *use_ref)
{
    return guarded("pmx_dbam_tss_begin", [&] { return tss_begin_impl(b, n, ref, pos1, reverse, flank, extend, use_ref); });
}

int pmx_dbam_tss_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t out[2])
{
    return guarded("pmx_dbam_tss_add", [&] { return tss_add_impl(b, mapq_min, flag_exclude, out); });
}

int pmx_dbam_tss_copy(pmx_dbam *b, uint64_t *profile)
{
    return guarded("pmx_dbam_tss_copy", [&] { return tss_copy_impl(b, profile); });
}

int pmx_dbam_tss_totals(pmx_dbam *b, uint64_t totals[4])
{
    return guarded("pmx_dbam_tss_totals", [&] { return tss_totals_impl(b, totals); });
}

}  // extern "C"
