// Library complexity on the device (pmx_dbam_complexity, include/pymasc_amd_ingest.h; DESIGN.md 7.14).  Included at the end of
// bam_device.hip: one more walk + filter over what the handle holds in HBM (the verified record chain of a BAM stream, the parse
// table of a SAM / BED handle), into arrays of its own, then equal keys (ref_id, pos1, read_len, reverse) are grouped by a sort
// and the groups are tallied.  The arrays, counters and runs of the last pmx_dbam_decode are not touched.
//
//   k_bam_walk<0> / k_bam_scan / k_bam_walk<2>   (BAM) the kept records of the caller's filter, over the chain's verified piece
//                 starts, with piece tables of this call; k_sam_keep / k_bam_scan / k_sam_compact for a SAM / BED handle
//   k_cx_keys     the key of every kept record as two words: hi = ref_id << 32 | pos1, lo = read_len << 1 | reverse (97 bits
//                 of fields in 128: nothing is truncated)
//   k_bed_check   over hi and over lo: the OR and the AND of every word (a digit whose bits agree in both is the same in every
//                 key: its radix pass is skipped) and, for a stream, whether hi ever falls
//   radix sort    stable LSD over 8-bit digits with the record index as payload, k_bed_rs_hist / k_bam_scan / k_bed_rs_scatter
//                 as the BED reader uses them: first the digits of lo, then hi gathered through the index (k_cx_gather) and its
//                 digits.  A pile of 10^5 equal keys is 10^5 neighbours afterwards, nothing walks it
//   k_cx_head_count / k_bam_scan / k_cx_head_write   the index of every head (a key that differs from its predecessor), compacted
//   k_cx_tally    one lane per head: the group's length is the next head's index minus its own; ballots and wave sums, then LDS,
//                 then one 64-bit atomic per workgroup and counter (per-reference tallies for the workgroup's first reference
//                 the same way; a head of another reference, a chromosome boundary, adds to its row directly)
// Device memory: 13 bytes per kept read for the filtered fields, freed once the keys (16 bytes) exist; the sort adds two key
// buffers and two index buffers: the peak is 40 bytes per kept read (+ 12 bytes per digit and tile of 8192 keys, + 24 bytes per
// 16-KB piece of a BAM stream).  Everything is freed before the call returns, except a stream's held-back records (13 bytes
// each), which stay with the handle until the next call and count towards pmx_dbam_stream_info's peak.

#define CX_ITEMS 8u                           // keys per lane of the head kernels
#define CX_TILE (256u * CX_ITEMS)
#define CX_LAST (PMX_COMPLEXITY_BINS - 1u)    // the bin of "at least that often"

__global__ void __launch_bounds__(256) k_cx_keys(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len,
                                                 const u8 *__restrict__ rev, u64 n, u64 *__restrict__ hi, u64 *__restrict__ lo)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    hi[i] = ((u64)(u32)ref[i] << 32) | (u64)(u32)pos[i];
    lo[i] = ((u64)(u32)len[i] << 1) | (rev[i] ? 1ull : 0ull);
}

// dst[i] = src[idx[i]]
__global__ void __launch_bounds__(256) k_cx_gather(const u64 *__restrict__ src, const u32 *__restrict__ idx, u64 n, u64 *__restrict__ dst)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// out[0] += the number of words equal to `last` (a stream window in order: the records of its last (ref_id, pos1))
__global__ void __launch_bounds__(256) k_cx_tail(const u64 *__restrict__ hi, u64 n, u64 last, unsigned long long *__restrict__ out)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    const u64 m = __ballot(i < n && hi[i] == last);
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) {
        const u32 c = s_w[0] + s_w[1] + s_w[2] + s_w[3];
        if (c) atomicAdd(out, (unsigned long long)c);
    }
}

__device__ __forceinline__ bool cx_head(const u64 *__restrict__ hi, const u64 *__restrict__ lo, u64 i)
{
    return i == 0 || hi[i] != hi[i - 1] || lo[i] != lo[i - 1];
}

// bcnt[tile] = heads among the tile's CX_TILE sorted keys
__global__ void __launch_bounds__(256) k_cx_head_count(const u64 *__restrict__ hi, const u64 *__restrict__ lo, u64 n, u32 *__restrict__ bcnt)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 base = (u64)blockIdx.x * CX_TILE;
    u32 c = 0;
    for (u32 it = 0; it < CX_ITEMS; it++) {
        const u64 i = base + (u64)it * 256u + t;
        c += (u32)__popcll(__ballot(i < n && cx_head(hi, lo, i)));   // (the same sum in every lane of the wave)
    }
    if ((t & 63u) == 0) s_w[t >> 6] = c;
    __syncthreads();
    if (t == 0) bcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// headpos[bbase[tile] + rank] = index of the head, ranks in (item, wave, lane) order, which is the keys' order
__global__ void __launch_bounds__(256) k_cx_head_write(const u64 *__restrict__ hi, const u64 *__restrict__ lo, u64 n,
                                                       const u64 *__restrict__ bbase, u32 *__restrict__ headpos)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 base = (u64)blockIdx.x * CX_TILE;
    u64 run = bbase[blockIdx.x];
    for (u32 it = 0; it < CX_ITEMS; it++) {
        const u64 i = base + (u64)it * 256u + t;
        const bool h = i < n && cx_head(hi, lo, i);
        const u64 m = __ballot(h);
        if (lane == 0) s_w[wave] = (u32)__popcll(m);
        __syncthreads();
        u64 o = run + (u64)__popcll(m & ((1ull << lane) - 1ull));
        for (u32 w = 0; w < wave; w++) o += s_w[w];
        if (h) headpos[o] = (u32)i;
        run += s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

__device__ __forceinline__ u64 cx_wave_sum(u64 x)
{
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ u64 cx_wave_max(u64 x)
{
    for (int d = 32; d > 0; d >>= 1) {
        const u64 y = __shfl_xor(x, d, 64);
        x = y > x ? y : x;
    }
    return x;
}

// One lane per head of the sorted keys.  per_ref[4 * ref + {0, 1, 2, 3}] += {reads, keys, keys seen once, keys seen twice};
// hist[k] += keys seen k times (the last bin: at least that often), hist[0] = max multiplicity; use_ref (null: every reference)
// leaves a reference out of all of them.
__global__ void __launch_bounds__(256) k_cx_tally(const u64 *__restrict__ hi, const u32 *__restrict__ headpos, u64 nheads, u64 n,
                                                  const u8 *__restrict__ use_ref, unsigned long long *__restrict__ per_ref,
                                                  unsigned long long *__restrict__ hist)
{
    __shared__ u32 s_h[PMX_COMPLEXITY_BINS];
    __shared__ unsigned long long s_r[4], s_max;
    __shared__ u32 s_ref0;
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 j = (u64)blockIdx.x * 256u + t;
    if (t < PMX_COMPLEXITY_BINS) s_h[t] = 0;
    if (t < 4u) s_r[t] = 0;
    if (t == 0) {
        s_max = 0;
        s_ref0 = (u32)(hi[headpos[(u64)blockIdx.x * 256u]] >> 32);   // (the grid has no workgroup without a head)
    }
    __syncthreads();
    const u32 ref0 = s_ref0;
    bool on = j < nheads;
    u64 m = 0;
    u32 ref = 0;
    if (on) {
        const u64 i = headpos[j];
        m = (j + 1u < nheads ? (u64)headpos[j + 1u] : n) - i;
        ref = (u32)(hi[i] >> 32);
        on = !use_ref || use_ref[ref] != 0;
    }
    // the histogram: multiplicities 1 and 2 by ballot (nearly every key), the rest by LDS atomics
    const u32 c1 = (u32)__popcll(__ballot(on && m == 1u)), c2 = (u32)__popcll(__ballot(on && m == 2u));
    if (on && m > 2u) atomicAdd(&s_h[m < CX_LAST ? (u32)m : CX_LAST], 1u);
    const u64 wmax = cx_wave_max(on ? m : 0ull);
    // the workgroup's first reference: summed over the wave; any other reference (sorted keys: behind a chromosome boundary)
    // goes to its own row
    const bool in0 = on && ref == ref0;
    const u32 d0 = (u32)__popcll(__ballot(in0));
    const u32 a1 = (u32)__popcll(__ballot(in0 && m == 1u)), a2 = (u32)__popcll(__ballot(in0 && m == 2u));
    const u64 n0 = cx_wave_sum(in0 ? m : 0ull);
    if (lane == 0) {
        if (c1) atomicAdd(&s_h[1], c1);
        if (c2) atomicAdd(&s_h[2], c2);
        if (wmax) atomicMax(&s_max, (unsigned long long)wmax);
        if (d0) {
            atomicAdd(&s_r[0], (unsigned long long)n0);
            atomicAdd(&s_r[1], (unsigned long long)d0);
            if (a1) atomicAdd(&s_r[2], (unsigned long long)a1);
            if (a2) atomicAdd(&s_r[3], (unsigned long long)a2);
        }
    }
    if (on && !in0) {
        unsigned long long *row = per_ref + 4ull * ref;
        atomicAdd(&row[0], (unsigned long long)m);
        atomicAdd(&row[1], 1ull);
        if (m == 1u) atomicAdd(&row[2], 1ull);
        if (m == 2u) atomicAdd(&row[3], 1ull);
    }
    __syncthreads();
    if (t >= 1u && t < PMX_COMPLEXITY_BINS && s_h[t]) atomicAdd(&hist[t], (unsigned long long)s_h[t]);
    if (t == 0 && s_max) atomicMax(&hist[0], s_max);
    if (t < 4u && s_r[t]) atomicAdd(&per_ref[4ull * ref0 + t], s_r[t]);
}

namespace {

struct CxRecs {     // the kept records of one call: held-back ones of the last window in front, then the current stream's
    DevAlloc ref, pos, len, rev;
    u64 n = 0;
    int alloc(u64 cap)
    {
        cap = std::max<u64>(cap, 1);
        HIPOK(hipMalloc(&ref.p, 4 * cap));
        HIPOK(hipMalloc(&pos.p, 4 * cap));
        HIPOK(hipMalloc(&len.p, 4 * cap));
        HIPOK(hipMalloc(&rev.p, cap));
        return 0;
    }
};

void cx_free(DevAlloc &a)
{
    if (a.p) (void)hipFree(a.p);
    a.p = nullptr;
}

void cx_drop_held(StreamState *s)
{
    for (void *p : {(void *)s->cx_ref, (void *)s->cx_pos, (void *)s->cx_len, (void *)s->cx_rev})
        if (p) (void)hipFree(p);
    s->cx_ref = s->cx_pos = s->cx_len = nullptr;
    s->cx_rev = nullptr;
    s->cx_n = 0;
}

// The records of the current stream that pass the filter, behind `front` held-back ones, into R (arrays of this call).
// Also the front half of pmx_dbam_bincount_add (bincount_device.inc), with front = 0.
int cx_filter(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, u64 front, bool current, CxRecs &R)
{
    hipStream_t st = b->stream;
    const StreamState *s = b->st;
    auto put_front = [&]() -> int {
        if (!front) return 0;
        HIPOK(hipMemcpyAsync(R.ref.p, s->cx_ref, 4 * front, hipMemcpyDeviceToDevice, st));
        HIPOK(hipMemcpyAsync(R.pos.p, s->cx_pos, 4 * front, hipMemcpyDeviceToDevice, st));
        HIPOK(hipMemcpyAsync(R.len.p, s->cx_len, 4 * front, hipMemcpyDeviceToDevice, st));
        HIPOK(hipMemcpyAsync(R.rev.p, s->cx_rev, front, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    R.n = front;
    u64 totals[2] = {0, 0};
    DevAlloc d_kept, d_base, d_tot;
    HIPOK(hipMalloc(&d_tot.p, 16));
    if (current && b->sam && b->sam_lines > 0) {
        const u64 n = b->sam_lines, nb = (n + 255) / 256;
        HIPOK(hipMalloc(&d_kept.p, 4 * nb));
        HIPOK(hipMalloc(&d_base.p, 8 * nb));
        hipLaunchKernelGGL(k_sam_keep, dim3((unsigned)nb), dim3(256), 0, st, b->d_sref, b->d_sqlen, b->d_sfm, n, mapq_min, flag_exclude, -1,
                           d_kept.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_kept.as<u32>(), d_kept.as<u32>(), nb, d_base.as<u64>(), d_tot.as<u64>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(totals, d_tot.p, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (int rc = R.alloc(front + totals[0])) return rc;
        if (int rc = put_front()) return rc;
        hipLaunchKernelGGL(k_sam_compact, dim3((unsigned)nb), dim3(256), 0, st, b->d_sref, b->d_spos, b->d_sqlen, b->d_sfm, n, mapq_min,
                           flag_exclude, -1, d_base.as<u64>(), R.ref.as<int>() + front, R.pos.as<int>() + front, R.len.as<int>() + front,
                           R.rev.as<u8>() + front);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(st));
        u64 m = totals[0];      // (an attached region mask: counted are the reads the run is fed)
        if (int rc = rm_filter(b, R.ref.as<int>() + front, R.pos.as<int>() + front, R.len.as<int>() + front, R.rev.as<u8>() + front, m, &m))
            return rc;
        R.n = front + m;
        return 0;
    }
    if (current && !b->sam && b->npieces > 0) {
        const u64 np = b->npieces;
        WalkArgs A;
        A.D = b->d_out + b->data_beg;
        A.N = b->N - b->data_beg;
        A.nref = (int)b->ref_names.size();
        A.want_ref = -1;
        A.o_ref = A.o_pos = A.o_len = nullptr;
        A.o_rev = nullptr;
        if (!b->chain_ready) {   // (its counts are decode's scratch: the next decode walks with its own filter again)
            A.mapq_min = 0;
            A.flag_exclude = 0;
            if (int rc = walk_chain(b, A)) return rc;
        }
        DevAlloc d_end, d_cnt, d_err;
        HIPOK(hipMalloc(&d_end.p, 8 * np));
        HIPOK(hipMalloc(&d_cnt.p, 4 * np));
        HIPOK(hipMalloc(&d_kept.p, 4 * np));
        HIPOK(hipMalloc(&d_base.p, 8 * np));
        HIPOK(hipMalloc(&d_err.p, 8));
        A.mapq_min = mapq_min;
        A.flag_exclude = flag_exclude;
        A.npieces = np;
        A.spec = b->d_spec;          // (read only: the walks below start from the verified piece starts)
        A.end = d_end.as<u64>();
        A.cnt = d_cnt.as<u32>();
        A.kept = d_kept.as<u32>();
        A.kept_base = d_base.as<u64>();
        A.first_error = d_err.as<unsigned long long>();
        A.nmis = nullptr;
        const dim3 wg((unsigned)((np + 63) / 64));
        hipLaunchKernelGGL(k_bam_walk<0>, wg, dim3(64), 0, st, A);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_kept.as<u32>(), d_cnt.as<u32>(), np, d_base.as<u64>(), d_tot.as<u64>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(totals, d_tot.p, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (int rc = R.alloc(front + totals[0])) return rc;
        if (int rc = put_front()) return rc;
        A.o_ref = R.ref.as<int>() + front;
        A.o_pos = R.pos.as<int>() + front;
        A.o_len = R.len.as<int>() + front;
        A.o_rev = R.rev.as<u8>() + front;
        HIPOK(hipMemsetAsync(d_err.p, 0xff, 8, st));
        hipLaunchKernelGGL(k_bam_walk<2>, wg, dim3(64), 0, st, A);
        HIPOK(hipGetLastError());
        unsigned long long fe = 0;
        HIPOK(hipMemcpyAsync(&fe, d_err.p, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (fe != ~0ull) return record_error(fe);
        u64 m = totals[0];
        if (int rc = rm_filter(b, R.ref.as<int>() + front, R.pos.as<int>() + front, R.len.as<int>() + front, R.rev.as<u8>() + front, m, &m))
            return rc;
        R.n = front + m;
        return 0;
    }
    if (front) {
        if (int rc = R.alloc(front)) return rc;
        if (int rc = put_front()) return rc;
        HIPOK(hipStreamSynchronize(st));
    }
    return 0;
}

inline int side_add_any(const CxRecs &) { return 0; }

// What the add of bincount, peakcount, coverage, gcbias and tss share behind their own entry checks: the kept records of what the handle
// holds now (none: nothing is counted), `check` on them before anything is allocated or marked, n zeroed 64-bit counters on the
// device, `launch` (the family's kernel over the records, on the stream, adding to the counters), the counters into counters[n].
template <class Launch, class Check = int (*)(const CxRecs &)>
int side_add(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, u64 n, unsigned long long *counters, Launch &&launch, Check &&check = side_add_any)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    CxRecs R;
    if (int rc = cx_filter(b, mapq_min, flag_exclude, 0, true, R)) return rc;
    if (R.n == 0) return 0;
    if (int rc = check(R)) return rc;
    DevAlloc d;
    HIPOK(hipMalloc(&d.p, 8 * n));
    HIPOK(hipMemsetAsync(d.p, 0, 8 * n, st));
    launch(R, st, d.as<unsigned long long>());
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(counters, d.p, 8 * n, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return 0;
}

// stable LSD radix passes over the digits of `differ`, from key_first (left as it is) through the buffers ka / kb, the payload
// from vin (null: the key's index) through va / vb; afterwards kin / vin are the sorted keys and their payload
int cx_sort(hipStream_t st, u64 n, u64 differ, const u64 *&kin, const u32 *&vin, u64 *ka, u64 *kb, u32 *va, u32 *vb, u32 *d_cnt,
            u64 *d_base, u64 *d_tot)
{
    const u32 ntiles = (u32)((n + BED_RS_TILE - 1) / BED_RS_TILE);
    const u64 ncnt = 256ull * ntiles;
    for (u32 dig = 0; dig < 8u; dig++) {
        const u32 shift = 8u * dig;
        if (((differ >> shift) & 255u) == 0) continue;      // the same digit in every key: the pass would move nothing
        u64 *kout = kin == ka ? kb : ka;
        u32 *vout = vin == va ? vb : va;
        hipLaunchKernelGGL(k_bed_rs_hist, dim3(ntiles), dim3(256), 0, st, kin, n, shift, ntiles, d_cnt);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cnt, d_cnt, ncnt, d_base, d_tot);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bed_rs_scatter, dim3(ntiles), dim3(256), 0, st, kin, vin, n, shift, ntiles, d_base, kout, vout);
        HIPOK(hipGetLastError());
        kin = kout;
        vin = vout;
    }
    return 0;
}

int dbam_complexity_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, const uint8_t *use_ref, uint64_t *per_ref, uint64_t *hist)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!per_ref || !hist) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_complexity: null output");
    const u64 nref = b->ref_names.size();
    for (u64 i = 0; i < 4 * nref; i++) per_ref[i] = 0;
    for (u32 k = 0; k < PMX_COMPLEXITY_BINS; k++) hist[k] = 0;
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    StreamState *s = b->st;
    // a stream: this window is counted once; behind the end of the stream only what is still held back
    bool current = true;
    if (s) {
        current = s->cx_window != s->windows;
        s->cx_window = s->windows;
        if (!current && !(s->cx_end && s->cx_n)) return 0;
    }
    const u64 front = s ? s->cx_n : 0;
    CxRecs R;
    if (int rc = cx_filter(b, mapq_min, flag_exclude, front, current, R)) return rc;
    if (s) cx_drop_held(s);
    u64 n = R.n;
    if (n == 0) return 0;
    if (n >= 0xffffffffull) return fail(PMX_DBAM_ERR_OPEN, "pmx_dbam_complexity: more than 2^32 - 2 reads");
    const u64 nb = (n + 255) / 256;
    DevAlloc d_hi, d_lo, d_chk;
    HIPOK(hipMalloc(&d_hi.p, 8 * n));
    HIPOK(hipMalloc(&d_lo.p, 8 * n));
    HIPOK(hipMalloc(&d_chk.p, 64 + 8));
    hipLaunchKernelGGL(k_cx_keys, dim3((unsigned)nb), dim3(256), 0, st, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(), R.rev.as<u8>(), n,
                       d_hi.as<u64>(), d_lo.as<u64>());
    HIPOK(hipGetLastError());
    unsigned long long chk[9] = {0, 0, ~0ull, 0, 0, 0, ~0ull, 0, 0};   // k_bed_check's four words for hi, for lo; the tail count
    auto check = [&](u64 count) -> int {
        HIPOK(hipMemcpyAsync(d_chk.p, chk, 72, hipMemcpyHostToDevice, st));
        const dim3 g((unsigned)((count + 255) / 256));
        hipLaunchKernelGGL(k_bed_check, g, dim3(256), 0, st, d_hi.as<u64>(), count, ~0ull, d_chk.as<unsigned long long>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bed_check, g, dim3(256), 0, st, d_lo.as<u64>(), count, ~0ull, d_chk.as<unsigned long long>() + 4);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(chk, d_chk.p, 72, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        return 0;
    };
    if (int rc = check(n)) return rc;
    if (s) {
        if (chk[0]) return fail(PMX_DBAM_ERR_INVALID, "stream is not sorted by position");
        if (!s->cx_end) {     // the records of the last (ref_id, pos1) wait for the next window
            u64 last = 0;
            HIPOK(hipMemcpyAsync(&last, d_hi.as<u64>() + (n - 1), 8, hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            hipLaunchKernelGGL(k_cx_tail, dim3((unsigned)nb), dim3(256), 0, st, d_hi.as<u64>(), n, last, d_chk.as<unsigned long long>() + 8);
            HIPOK(hipGetLastError());
            unsigned long long held = 0;
            HIPOK(hipMemcpyAsync(&held, d_chk.as<unsigned long long>() + 8, 8, hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            const u64 keep = n - held;
            HIPOK(hipMalloc((void **)&s->cx_ref, 4 * held));
            HIPOK(hipMalloc((void **)&s->cx_pos, 4 * held));
            HIPOK(hipMalloc((void **)&s->cx_len, 4 * held));
            HIPOK(hipMalloc((void **)&s->cx_rev, held));
            HIPOK(hipMemcpyAsync(s->cx_ref, R.ref.as<int>() + keep, 4 * held, hipMemcpyDeviceToDevice, st));
            HIPOK(hipMemcpyAsync(s->cx_pos, R.pos.as<int>() + keep, 4 * held, hipMemcpyDeviceToDevice, st));
            HIPOK(hipMemcpyAsync(s->cx_len, R.len.as<int>() + keep, 4 * held, hipMemcpyDeviceToDevice, st));
            HIPOK(hipMemcpyAsync(s->cx_rev, R.rev.as<u8>() + keep, held, hipMemcpyDeviceToDevice, st));
            HIPOK(hipStreamSynchronize(st));
            s->cx_n = held;
            stream_note(*b);
            n = keep;
            if (n == 0) return 0;
            chk[0] = chk[1] = chk[3] = chk[4] = chk[5] = chk[7] = chk[8] = 0;
            chk[2] = chk[6] = ~0ull;
            if (int rc = check(n)) return rc;     // (the digits that differ among the keys that are sorted now)
        }
    }
    cx_free(R.ref);
    cx_free(R.pos);
    cx_free(R.len);
    cx_free(R.rev);
    // the sort: the digits of lo first, then those of hi
    const u32 ntiles = (u32)((n + BED_RS_TILE - 1) / BED_RS_TILE);
    const u64 ncnt = 256ull * ntiles;
    DevAlloc d_ka, d_kb, d_va, d_vb, d_cnt, d_base, d_tot;
    HIPOK(hipMalloc(&d_ka.p, 8 * n));
    HIPOK(hipMalloc(&d_kb.p, 8 * n));
    HIPOK(hipMalloc(&d_va.p, 4 * n));
    HIPOK(hipMalloc(&d_vb.p, 4 * n));
    HIPOK(hipMalloc(&d_cnt.p, 4 * ncnt));
    HIPOK(hipMalloc(&d_base.p, 8 * std::max<u64>(ncnt, (n + CX_TILE - 1) / CX_TILE)));
    HIPOK(hipMalloc(&d_tot.p, 16));
    const u64 *kin = d_lo.as<u64>();
    const u32 *vin = nullptr;
    if (int rc = cx_sort(st, n, chk[5] ^ chk[6], kin, vin, d_ka.as<u64>(), d_kb.as<u64>(), d_va.as<u32>(), d_vb.as<u32>(), d_cnt.as<u32>(),
                         d_base.as<u64>(), d_tot.as<u64>()))
        return rc;
    if (vin) {               // hi in the order of lo (the sorted words of lo themselves are not needed again)
        hipLaunchKernelGGL(k_cx_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_hi.as<u64>(), vin, n, d_ka.as<u64>());
        HIPOK(hipGetLastError());
        kin = d_ka.as<u64>();
    } else {
        kin = d_hi.as<u64>();
    }
    if (int rc = cx_sort(st, n, chk[1] ^ chk[2], kin, vin, d_ka.as<u64>(), d_kb.as<u64>(), d_va.as<u32>(), d_vb.as<u32>(), d_cnt.as<u32>(),
                         d_base.as<u64>(), d_tot.as<u64>()))
        return rc;
    const u64 *hi_s = kin, *lo_s = d_lo.as<u64>();
    if (vin) {               // lo in the final order, into the key buffer the sorted hi is not in
        u64 *dst = kin == d_ka.as<u64>() ? d_kb.as<u64>() : d_ka.as<u64>();
        hipLaunchKernelGGL(k_cx_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_lo.as<u64>(), vin, n, dst);
        HIPOK(hipGetLastError());
        lo_s = dst;
    }
    // heads, group lengths, tallies
    u32 *headpos = vin == d_va.as<u32>() ? d_vb.as<u32>() : d_va.as<u32>();   // (the index buffer the payload is not in)
    const u32 nt = (u32)((n + CX_TILE - 1) / CX_TILE);
    hipLaunchKernelGGL(k_cx_head_count, dim3(nt), dim3(256), 0, st, hi_s, lo_s, n, d_cnt.as<u32>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cnt.as<u32>(), d_cnt.as<u32>(), (u64)nt, d_base.as<u64>(), d_tot.as<u64>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_cx_head_write, dim3(nt), dim3(256), 0, st, hi_s, lo_s, n, d_base.as<u64>(), headpos);
    HIPOK(hipGetLastError());
    u64 totals[2] = {0, 0};
    HIPOK(hipMemcpyAsync(totals, d_tot.p, 16, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const u64 nheads = totals[0];
    const u64 nres = 4 * nref + PMX_COMPLEXITY_BINS;
    DevAlloc d_res, d_use;
    HIPOK(hipMalloc(&d_res.p, 8 * nres));
    HIPOK(hipMemsetAsync(d_res.p, 0, 8 * nres, st));
    if (use_ref) {
        HIPOK(hipMalloc(&d_use.p, std::max<u64>(nref, 1)));
        HIPOK(hipMemcpyAsync(d_use.p, use_ref, nref, hipMemcpyHostToDevice, st));
    }
    hipLaunchKernelGGL(k_cx_tally, dim3((unsigned)((nheads + 255) / 256)), dim3(256), 0, st, hi_s, headpos, nheads, n, d_use.as<u8>(),
                       d_res.as<unsigned long long>(), d_res.as<unsigned long long>() + 4 * nref);
    HIPOK(hipGetLastError());
    std::vector<unsigned long long> res(nres);
    HIPOK(hipMemcpyAsync(res.data(), d_res.p, 8 * nres, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    for (u64 i = 0; i < 4 * nref; i++) per_ref[i] = res[i];
    for (u32 k = 0; k < PMX_COMPLEXITY_BINS; k++) hist[k] = res[4 * nref + k];
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_complexity(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, const uint8_t *use_ref, uint64_t *per_ref,
                        uint64_t hist[PMX_COMPLEXITY_BINS])
{
    return guarded("pmx_dbam_complexity", [&] { return dbam_complexity_impl(b, mapq_min, flag_exclude, use_ref, per_ref, hist); });
}

}  // extern "C"
