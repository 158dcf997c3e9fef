// Excluded regions on the device (pmx_dbam_set_exclude, include/pymasc_amd_ingest.h; DESIGN.md 7.15).  Included at the end of
// bam_device.hip.  A handle carries the MERGED intervals of a BED mask in HBM, in (reference, begin) order, as two arrays:
// key = ref_id << 32 | begin (0-based) and end (exclusive); merged intervals of one reference are disjoint, do not abut and have
// ascending ends, so that the last interval whose begin lies below a read's last base is the only one that can overlap it.
//
//   k_rm_keys     one lane per line of the mask: its reference from the offsets (binary search), the end clipped to the
//                 reference's length, the key; a line that is empty after clipping gets the key nref << 32 and sorts to the tail
//   radix sort    the stable LSD sort of the BED reader over the digits of the key, the line index as payload (cx_sort)
//   k_rm_merge    one workgroup: v = ref_id << 32 | end in sorted order; an inclusive running maximum of v (per-thread chunks,
//                 a scan of the 1024 chunk maxima in LDS) is the running maximum of the ends WITHIN a reference, because a
//                 later reference's v is above every earlier one's; a line is a head when it begins above the running maximum
//                 in front of it (a line that abuts its predecessor is merged into it); the heads are counted, scanned and
//                 compacted, each with the running maximum at the last line of its group as its end
//   k_rm_keep     one lane per kept record of a decode: the last merged interval with begin + 1 <= pos1 + read_len - 1 (binary
//                 search over the keys), dropped when it is of the read's reference and pos1 <= end; the keep flags and their
//                 count per workgroup feed k_bam_scan and k_rm_compact (ranks by ballot, in record order)
// rm_build runs the first three for pmx_dbam_set_exclude, which keeps the merged intervals, and for pmx_dbam_peakcount_begin
// (peakcount_device.inc), which keeps the sorted lines, their ends, the running maximum and the sort's permutation as well.
// The filter runs behind every decode (pmx_dbam_decode) and inside pmx_dbam_complexity; the runs (k_ref_runs) are taken
// from the compacted arrays afterwards.

__global__ void __launch_bounds__(256) k_rm_keys(const u32 *__restrict__ begin, const u32 *__restrict__ end, const long long *__restrict__ off,
                                                 const long long *__restrict__ ref_len, u32 nref, u64 n, u64 *__restrict__ key,
                                                 u32 *__restrict__ endc)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    u32 lo = 0, hi = nref;      // the last reference whose offset is <= i
    while (lo + 1u < hi) {
        const u32 mid = (lo + hi) / 2u;
        if ((u64)off[mid] <= i) lo = mid;
        else hi = mid;
    }
    const u32 b = begin[i];
    u32 e = end[i];
    const long long len = ref_len[lo];
    if (len >= 0 && (long long)e > len) e = (u32)len;      // an interval past the chromosome's end is clipped
    endc[i] = e;
    key[i] = b < e ? ((u64)lo << 32) | b : (u64)nref << 32;
}

__device__ __forceinline__ bool rm_head(const u64 *__restrict__ key, const u64 *__restrict__ pmax, u64 i, u64 none)
{
    const u64 k = key[i];
    if (k >= none) return false;
    if (i == 0) return true;
    const u64 p = pmax[i - 1];
    return (k >> 32) != (p >> 32) || (u32)k > (u32)p;
}

__global__ void __launch_bounds__(1024) k_rm_merge(const u64 *__restrict__ key, const u32 *__restrict__ idx, const u32 *__restrict__ endc,
                                                   u64 n, u32 nref, u64 *__restrict__ pmax, u64 *__restrict__ okey, u32 *__restrict__ oend,
                                                   u64 *__restrict__ ocount)
{
    __shared__ u64 s[1024];
    const u32 t = threadIdx.x;
    const u64 none = (u64)nref << 32;
    const u64 per = (n + 1023u) / 1024u, lo = (u64)t * per < n ? (u64)t * per : n, hi = lo + per < n ? lo + per : n;
    // the running maximum of ref_id << 32 | end
    u64 a = 0;
    for (u64 i = lo; i < hi; i++) {
        const u64 v = (key[i] & ~0xffffffffull) | endc[idx ? idx[i] : (u32)i];
        a = v > a ? v : a;
    }
    s[t] = a;
    __syncthreads();
    for (u32 o = 1; o < 1024u; o <<= 1) {
        const u64 x = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] = x > s[t] ? x : s[t];
        __syncthreads();
    }
    u64 run = t ? s[t - 1] : 0;
    for (u64 i = lo; i < hi; i++) {
        const u64 v = (key[i] & ~0xffffffffull) | endc[idx ? idx[i] : (u32)i];
        run = v > run ? v : run;
        pmax[i] = run;
    }
    __threadfence();
    __syncthreads();
    // heads: counted, scanned, written
    u64 c = 0;
    for (u64 i = lo; i < hi; i++) c += rm_head(key, pmax, i, none) ? 1u : 0u;
    s[t] = c;
    __syncthreads();
    for (u32 o = 1; o < 1024u; o <<= 1) {
        const u64 x = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += x;
        __syncthreads();
    }
    u64 cnt = s[t] - c;
    for (u64 i = lo; i < hi; i++) {
        if (key[i] >= none) break;                       // (the empty lines are the tail of the sorted keys)
        if (rm_head(key, pmax, i, none)) okey[cnt++] = key[i];
        if (i + 1 == n || key[i + 1] >= none || rm_head(key, pmax, i + 1, none)) oend[cnt - 1] = (u32)pmax[i];
    }
    if (t == 1023u) *ocount = s[t];
}

// keep[i] = 1 unless record i overlaps a merged interval of its reference; bcnt[workgroup] = kept records of its 256
__global__ void __launch_bounds__(256) k_rm_keep(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len, u64 n,
                                                 const u64 *__restrict__ xkey, const u32 *__restrict__ xend, u64 xn, u8 *__restrict__ keep,
                                                 u32 *__restrict__ bcnt)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    bool k = false;
    if (i < n) {
        k = true;
        const long long p = pos[i], l = len[i] > 0 ? len[i] : 1, last = p + l - 1;   // the extent [pos1, pos1 + read_len - 1]
        if (last >= 1 && ref[i] >= 0) {
            const long long b_max = last - 1 < 0xffffffffll ? last - 1 : 0xffffffffll;   // b + 1 <= last
            const u64 target = ((u64)(u32)ref[i] << 32) | (u64)b_max;
            u64 lo = 0, hi = xn;                       // the number of keys <= target
            while (lo < hi) {
                const u64 mid = (lo + hi) / 2u;
                if (xkey[mid] <= target) lo = mid + 1u;
                else hi = mid;
            }
            if (lo > 0 && (xkey[lo - 1] >> 32) == (u64)(u32)ref[i] && (long long)xend[lo - 1] >= p) k = false;   // pos1 <= e
        }
        keep[i] = k ? 1 : 0;
    }
    const u64 m = __ballot(k);
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) bcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) k_rm_compact(const u8 *__restrict__ keep, const u64 *__restrict__ bbase, u64 n, const int *__restrict__ ref,
                                                    const int *__restrict__ pos, const int *__restrict__ len, const u8 *__restrict__ rev,
                                                    int *__restrict__ o_ref, int *__restrict__ o_pos, int *__restrict__ o_len,
                                                    u8 *__restrict__ o_rev)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 i = (u64)blockIdx.x * 256u + t;
    const bool k = i < n && keep[i] != 0;
    const u64 m = __ballot(k);
    if (lane == 0) s_w[wave] = (u32)__popcll(m);
    __syncthreads();
    if (!k) return;
    u64 o = bbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; w++) o += s_w[w];
    o_ref[o] = ref[i];
    o_pos[o] = pos[i];
    o_len[o] = len[i];
    o_rev[o] = rev[i];
}

// a device copy of n elements of `src`, which lies in host or in device memory
template <class T>
static int rm_to_device(hipStream_t st, const T *src, u64 n, DevAlloc &dst)
{
    HIPOK(hipMalloc(&dst.p, sizeof(T) * std::max<u64>(n, 1)));
    if (n) HIPOK(hipMemcpyAsync(dst.p, src, sizeof(T) * n, hipMemcpyDefault, st));
    return 0;
}

// What clipping, sorting and merging the lines of a region file leaves on the device (rm_build): the caller keeps what it needs
// (pmx_dbam_set_exclude the merged intervals; pmx_dbam_peakcount_begin, peakcount_device.inc, the sorted lines as well) and the
// rest is freed with the struct.
struct RmBuilt {
    DevAlloc key, endc, ka, kb, va, vb, pmax, okey, oend;
    const u64 *skey = nullptr;      // the keys in (reference, begin) order, the empty lines (key nref << 32) at the tail
    const u32 *perm = nullptr;      // sorted place -> input line; null: no pass moved a key, the order is the input's
    u64 n = 0, merged = 0;          // lines; merged intervals (okey / oend)
};

extern "C" {

static int rm_filter(pmx_dbam *b, int *ref, int *pos, int *len, u8 *rev, u64 n, u64 *n_out)
{
    *n_out = n;
    if (!b->x_n || n == 0) return 0;
    hipStream_t st = b->stream;
    const u64 nb = (n + 255) / 256;
    // one scratch block kept with the handle and grown when a decode holds more records than any before it: the compacted
    // fields (13 bytes per record), the block bases and counts, the totals, the keep flags
    const u64 n4 = (n + 3) & ~3ull;
    const u64 o_pos = 4 * n4, o_len = 8 * n4, o_base = 12 * n4, o_tot = o_base + 8 * nb, o_cnt = o_tot + 16, o_rev = o_cnt + 4 * nb,
              o_keep = o_rev + n4, need = o_keep + n4;
    if (need > b->xs_cap) {
        if (b->d_xs) (void)hipFree(b->d_xs);
        b->d_xs = nullptr;
        b->xs_cap = 0;
        HIPOK(hipMalloc((void **)&b->d_xs, need));
        b->xs_cap = need;
    }
    u8 *S = b->d_xs;
    int *t_ref = (int *)S, *t_pos = (int *)(S + o_pos), *t_len = (int *)(S + o_len);
    u64 *d_base = (u64 *)(S + o_base), *d_tot = (u64 *)(S + o_tot);
    u32 *d_cnt = (u32 *)(S + o_cnt);
    u8 *t_rev = S + o_rev, *d_keep = S + o_keep;
    hipLaunchKernelGGL(k_rm_keep, dim3((unsigned)nb), dim3(256), 0, st, ref, pos, len, n, b->d_xkey, b->d_xend, b->x_n, d_keep, d_cnt);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cnt, d_cnt, nb, d_base, d_tot);
    HIPOK(hipGetLastError());
    u64 totals[2] = {0, 0};
    HIPOK(hipMemcpyAsync(totals, d_tot, 16, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const u64 m = totals[0];
    if (m == n) return 0;
    if (m > 0) {     // compacted beside the arrays, then copied over their front (a workgroup may not write where another still reads)
        hipLaunchKernelGGL(k_rm_compact, dim3((unsigned)nb), dim3(256), 0, st, d_keep, d_base, n, ref, pos, len, rev, t_ref, t_pos, t_len,
                           t_rev);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(ref, t_ref, 4 * m, hipMemcpyDeviceToDevice, st));
        HIPOK(hipMemcpyAsync(pos, t_pos, 4 * m, hipMemcpyDeviceToDevice, st));
        HIPOK(hipMemcpyAsync(len, t_len, 4 * m, hipMemcpyDeviceToDevice, st));
        HIPOK(hipMemcpyAsync(rev, t_rev, m, hipMemcpyDeviceToDevice, st));
        HIPOK(hipStreamSynchronize(st));     // (the callers read the arrays and the next decode reuses the scratch block)
    }
    *n_out = m;
    return 0;
}

static void rm_detach(pmx_dbam *b)
{
    if (b->d_xkey) (void)hipFree(b->d_xkey);
    if (b->d_xend) (void)hipFree(b->d_xend);
    if (b->d_xs) (void)hipFree(b->d_xs);
    b->d_xkey = nullptr;
    b->d_xend = nullptr;
    b->d_xs = nullptr;
    b->x_n = b->xs_cap = 0;
}

// The lines of reference r are [offsets[r], offsets[r + 1]) of begin / end (host or device memory): k_rm_keys, the radix sort with
// the line index as payload, k_rm_merge.  B.n = 0: there is no line.  `who` names the caller in the messages.
static int rm_build(pmx_dbam *b, const char *who, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end,
                    RmBuilt &B)
{
    const std::string w = std::string(who) + ": ";
    if (!offsets || nref != (int32_t)b->ref_names.size())
        return fail(PMX_DBAM_ERR_INVALID, w + "nref offsets + 1 are needed, nref = the references of the header");
    if (nref == 0) return 0;
    for (int32_t r = 0; r < nref; r++)
        if (offsets[r] < 0 || offsets[r + 1] < offsets[r]) return fail(PMX_DBAM_ERR_INVALID, w + "offsets must ascend from 0");
    if (offsets[0] != 0) return fail(PMX_DBAM_ERR_INVALID, w + "offsets must ascend from 0");
    const u64 n = (u64)offsets[nref];
    if (n == 0) return 0;
    if (!begin || !end) return fail(PMX_DBAM_ERR_INVALID, w + "null interval arrays");
    if (n >= 0xffffffffull) return fail(PMX_DBAM_ERR_INVALID, w + "too many intervals");
    hipStream_t st = b->stream;
    DevAlloc d_b, d_e, d_off, d_len;
    if (int rc = rm_to_device(st, begin, n, d_b)) return rc;
    if (int rc = rm_to_device(st, end, n, d_e)) return rc;
    if (int rc = rm_to_device(st, (const long long *)offsets, (u64)nref + 1, d_off)) return rc;
    if (int rc = rm_to_device(st, (const long long *)b->ref_lens.data(), (u64)nref, d_len)) return rc;
    HIPOK(hipMalloc(&B.key.p, 8 * n));
    HIPOK(hipMalloc(&B.endc.p, 4 * n));
    hipLaunchKernelGGL(k_rm_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_b.as<u32>(), d_e.as<u32>(), d_off.as<long long>(),
                       d_len.as<long long>(), (u32)nref, n, B.key.as<u64>(), B.endc.as<u32>());
    HIPOK(hipGetLastError());
    // sorted by (reference, begin): every bit of the begin, and the bits a reference id (or nref, the empty lines' key) can have
    u64 hb = 1;
    while (hb <= (u64)nref) hb <<= 1;
    const u64 differ = ((hb - 1) << 32) | 0xffffffffull;
    const u32 ntiles = (u32)((n + BED_RS_TILE - 1) / BED_RS_TILE);
    const u64 ncnt = 256ull * ntiles;
    DevAlloc d_cnt, d_base, d_tot;
    HIPOK(hipMalloc(&B.ka.p, 8 * n));
    HIPOK(hipMalloc(&B.kb.p, 8 * n));
    HIPOK(hipMalloc(&B.va.p, 4 * n));
    HIPOK(hipMalloc(&B.vb.p, 4 * n));
    HIPOK(hipMalloc(&d_cnt.p, 4 * ncnt));
    HIPOK(hipMalloc(&d_base.p, 8 * ncnt));
    HIPOK(hipMalloc(&d_tot.p, 16));
    const u64 *kin = B.key.as<u64>();
    const u32 *vin = nullptr;
    if (int rc = cx_sort(st, n, differ, kin, vin, B.ka.as<u64>(), B.kb.as<u64>(), B.va.as<u32>(), B.vb.as<u32>(), d_cnt.as<u32>(),
                         d_base.as<u64>(), d_tot.as<u64>()))
        return rc;
    // merged: the heads with the running maximum of the ends of their group
    HIPOK(hipMalloc(&B.pmax.p, 8 * n));
    HIPOK(hipMalloc(&B.okey.p, 8 * n));
    HIPOK(hipMalloc(&B.oend.p, 4 * n));
    hipLaunchKernelGGL(k_rm_merge, dim3(1), dim3(1024), 0, st, kin, vin, B.endc.as<u32>(), n, (u32)nref, B.pmax.as<u64>(), B.okey.as<u64>(),
                       B.oend.as<u32>(), d_tot.as<u64>());
    HIPOK(hipGetLastError());
    u64 merged = 0;
    HIPOK(hipMemcpyAsync(&merged, d_tot.p, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));      // (the copies of the lines and the scratch of the sort are locals)
    B.skey = kin;
    B.perm = vin;
    B.n = n;
    B.merged = merged;
    return 0;
}

static int rm_set_exclude_impl(pmx_dbam *b, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    rm_detach(b);
    if (!offsets && !begin && !end) return 0;
    RmBuilt B;
    if (int rc = rm_build(b, "pmx_dbam_set_exclude", nref, offsets, begin, end, B)) return rc;
    if (B.merged == 0) return 0;
    b->d_xkey = B.okey.as<u64>();
    b->d_xend = B.oend.as<u32>();
    B.okey.p = B.oend.p = nullptr;
    b->x_n = B.merged;
    return 0;
}

int pmx_dbam_set_exclude(pmx_dbam *b, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end)
{
    try {
        return rm_set_exclude_impl(b, nref, offsets, begin, end);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dbam_set_exclude: ") + e.what());
    }
}

int64_t pmx_dbam_exclude_intervals(pmx_dbam *b, int64_t cap, int32_t *ref_id, uint32_t *begin, uint32_t *end)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!ref_id || !begin || !end) return (int64_t)b->x_n;
    const u64 m = std::min<u64>((u64)std::max<int64_t>(cap, 0), b->x_n);
    if (m == 0) return 0;
    HIPOK(hipSetDevice(b->device));
    std::vector<u64> key(m);
    HIPOK(hipMemcpyAsync(key.data(), b->d_xkey, 8 * m, hipMemcpyDeviceToHost, b->stream));
    HIPOK(hipMemcpyAsync(end, b->d_xend, 4 * m, hipMemcpyDeviceToHost, b->stream));
    HIPOK(hipStreamSynchronize(b->stream));
    for (u64 i = 0; i < m; i++) {
        ref_id[i] = (int32_t)(key[i] >> 32);
        begin[i] = (uint32_t)key[i];
    }
    return (int64_t)m;
}

int pmx_dbam_excluded(const pmx_dbam *b, uint64_t *dropped, uint64_t *intervals)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (dropped) *dropped = b->x_dropped;
    if (intervals) *intervals = b->x_n;
    return 0;
}

}  // extern "C"
