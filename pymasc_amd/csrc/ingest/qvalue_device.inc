// Benjamini-Hochberg q-scores for a p-score track (pmx_dbam_coverage_qvalue*, include/pymasc_amd_ingest.h; DESIGN.md 7.18.7).  Included
// in bam_device.hip behind poisson_device.inc and before call_device.inc: the input is the signal slot of a handle that holds a p-score
// track, the table is kept beside it, and call_device.inc writes column 9 of a narrowPeak line from it.  The definitions are this
// project's own: nothing here was compared with MACS2.
//
// The definitions.  Everything is integer arithmetic or float64, each float64 operation rounded to nearest even on its own (no fused
// multiply-add).
//   input      the runs (ref, start0, end0, v) of a p-score track, v float32: +0.0 or the float32 of a positive number (ps_value), so
//              v >= 0 and never a NaN; a track whose smallest value is negative is refused
//   tests      N = the sum of the lengths of the chosen references, u64 (bintrack_run's L, the L of k_ps_lambda): every base of the
//              chosen genome is one test; a base in no run has p = 1 and counts in N only
//   distinct   u_1 > u_2 > ... > u_m: the distinct values of the runs, compared as floats; W_i = the sum of end0 - start0 over the
//              runs with the value u_i, u64
//   rank       r_1 = 1, r_i = 1 + W_1 + ... + W_(i-1), u64; r_i <= N always
//   raw score  x_i = f64(u_i) + (lg2(f64(r_i)) - lg2(f64(N))) * 0.3010299956639812, lg2 = cp_lg2 of compare_device.inc (r_i and N are
//              below 2^53: the conversions are exact)
//   monotone   Q_i = max(0.0, min(x_1 .. x_i)), q_i = f32(Q_i).  min and max are associative and exact and the sums are integers:
//              no result depends on scheduling or on the order of the sort.  q is non-increasing in i
//   table      m rows (u_i, W_i, q_i), descending in u
//   cutoff     pcut(X), X a finite float64: f64(u_i) of the largest i with f64(q_i) >= X, the smallest p-score whose q-score reaches
//              X; 2^40 when no row reaches X (v < 2^40: call then finds nothing); X <= 0 gives f64(u_m)
//   lookup     the q-score of a peak is q_i of the row with u_i == its value (a peak's value is the value of one of its runs, so the
//              row exists: a miss is an internal error, not a -1)
//
//   k_qv_keys        one lane per run: key = the complement of the bits of v as u64 (v >= +0.0: descending v is ascending key), the
//                    weight end0 - start0 as u64, and the OR and the AND of the keys (the digits that differ), as k_bed_check takes them
//   cx_sort          complexity_device.inc's stable LSD radix sort over the 8-bit digits that differ, the run index as payload
//   k_cx_gather      the weights in sorted order; k_ps_sums / k_ps_scan / k_ps_apply (poisson_device.inc): their inclusive u64 prefix P
//   k_qv_count / k_bam_scan / k_qv_heads   a position is a head where its key differs from the one before; compacted by ballots into
//                    u_i, r_i = 1 + P in front of the head, x_i.  W_i = r_(i+1) - r_i, the last against 1 + P[n - 1] (k_qv_apply)
//   k_qv_mins / k_qv_minscan / k_qv_apply  the prefix min of x over the m rows in the three-kernel form of k_ps_*: minima per 256 rows,
//                    one workgroup over those minima, every workgroup behind its base; then the clamp, the float32, W and the totals
//   k_qv_cutoff      one lane: a binary search of q (non-increasing) for pcut
// Device memory: 40 bytes per run + 3072 per tile of 8192 runs + 64 inside qvalue, then 16 per distinct value more (counted in the
// handle's bytes while it runs, freed before it returns), and 16 per distinct value for the table until the next signal, compare,
// poisson, begin or close.

#define QV_NONE 0x1p40          // pcut when no row reaches X

__device__ __forceinline__ double qv_raw(u32 ubits, u64 r, u64 N)
{
#pragma clang fp contract(off)
    const double a = cp_lg2((double)r), b = cp_lg2((double)N);
    const double d = a - b;
    const double t = d * 0.3010299956639812;
    return (double)__uint_as_float(ubits) + t;
}

// chk[0] |= every key, chk[1] &= every key
__global__ void __launch_bounds__(256) k_qv_keys(const u32 *__restrict__ rstart, const u32 *__restrict__ rend, const u32 *__restrict__ rval, u64 n,
                                                 u64 *__restrict__ key, u64 *__restrict__ wt, unsigned long long *__restrict__ chk)
{
    __shared__ unsigned long long s[4][2];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 i = (u64)blockIdx.x * 256u + t;
    u64 o = 0, a = ~0ull;
    if (i < n) {
        const u64 k = (u64)(~rval[i]);
        key[i] = k;
        wt[i] = (u64)(rend[i] - rstart[i]);
        o = a = k;
    }
    for (int d = 32; d > 0; d >>= 1) {
        o |= __shfl_xor(o, d, 64);
        a &= __shfl_xor(a, d, 64);
    }
    if (lane == 0) {
        s[wave][0] = o;
        s[wave][1] = a;
    }
    __syncthreads();
    if (t == 0) {
        for (u32 w = 1; w < 4u; w++) {
            o |= s[w][0];
            a &= s[w][1];
        }
        atomicOr(&chk[0], (unsigned long long)o);
        atomicAnd(&chk[1], (unsigned long long)a);
    }
}

__device__ __forceinline__ bool qv_head(const u64 *__restrict__ key, u64 i, u64 n) { return i < n && (i == 0 || key[i] != key[i - 1u]); }

__global__ void __launch_bounds__(256) k_qv_count(const u64 *__restrict__ key, u64 n, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    cv_count(qv_head(key, (u64)blockIdx.x * 256u + threadIdx.x, n), kcnt, s_w);
}

// key: the sorted keys; P: the inclusive prefix of the weights in that order; N: the tests
__global__ void __launch_bounds__(256) k_qv_heads(const u64 *__restrict__ key, const unsigned long long *__restrict__ P, u64 n, u64 N,
                                                  const u64 *__restrict__ kbase, u32 *__restrict__ ou, u64 *__restrict__ orank,
                                                  unsigned long long *__restrict__ ox)
{
    __shared__ u32 s_w[4];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool keep = qv_head(key, i, n);
    const u64 o = cv_slot(keep, kbase, s_w);
    if (!keep) return;
    const u32 bits = ~(u32)key[i];
    const u64 r = 1u + (i ? (u64)P[i - 1u] : 0ull);
    ou[o] = bits;
    orank[o] = r;
    ox[o] = (unsigned long long)__double_as_longlong(qv_raw(bits, r, N));
}

__device__ __forceinline__ double qv_min(double a, double b) { return b < a ? b : a; }      // (no x is a NaN)

// mins[w] = the smallest x of workgroup w's 256 rows
__global__ void __launch_bounds__(256) k_qv_mins(const unsigned long long *__restrict__ x, u64 m, unsigned long long *__restrict__ mins)
{
    __shared__ double s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    double v = i < m ? __longlong_as_double((long long)x[i]) : __builtin_inf();
    for (int d = 32; d > 0; d >>= 1) v = qv_min(v, __shfl_xor(v, d, 64));
    if ((t & 63u) == 0) s_w[t >> 6] = v;
    __syncthreads();
    if (t == 0) mins[blockIdx.x] = (unsigned long long)__double_as_longlong(qv_min(qv_min(s_w[0], s_w[1]), qv_min(s_w[2], s_w[3])));
}

// in place, one workgroup: x[i] becomes the smallest of the elements in front of it (+inf in front of the first)
__global__ void __launch_bounds__(1024) k_qv_minscan(unsigned long long *__restrict__ x, u64 n)
{
    __shared__ double s[1024];
    const u32 t = threadIdx.x;
    const u64 per = (n + 1023u) / 1024u, lo = (u64)t * per < n ? (u64)t * per : n, hi = lo + per < n ? lo + per : n;
    double a = __builtin_inf();
    for (u64 i = lo; i < hi; i++) a = qv_min(a, __longlong_as_double((long long)x[i]));
    s[t] = a;
    __syncthreads();
    for (u32 o = 1; o < 1024u; o <<= 1) {
        const double y = t >= o ? s[t - o] : __builtin_inf();
        __syncthreads();
        s[t] = qv_min(s[t], y);
        __syncthreads();
    }
    double run = t ? s[t - 1u] : __builtin_inf();
    for (u64 i = lo; i < hi; i++) {
        const double v = __longlong_as_double((long long)x[i]);
        x[i] = (unsigned long long)__double_as_longlong(run);
        run = qv_min(run, v);
    }
}

// base[w]: the smallest x in front of workgroup w; cov: the covered bases (the last prefix).  tot[0] += the bases with q > 0
__global__ void __launch_bounds__(256) k_qv_apply(const unsigned long long *__restrict__ x, const u64 *__restrict__ rank, u64 m,
                                                  const unsigned long long *__restrict__ base, u64 cov, u64 *__restrict__ oW, u32 *__restrict__ oq,
                                                  unsigned long long *__restrict__ tot)
{
    __shared__ double s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 i = (u64)blockIdx.x * 256u + t;
    double v = i < m ? __longlong_as_double((long long)x[i]) : __builtin_inf();
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double y = __shfl_up(v, o, 64);
        if (lane >= (u32)o) v = qv_min(v, y);
    }
    if (lane == 63u) s_w[t >> 6] = v;
    __syncthreads();
    double b = __longlong_as_double((long long)base[blockIdx.x]);
    for (u32 w = 0; w < (t >> 6); w++) b = qv_min(b, s_w[w]);
    u64 pos = 0;
    if (i < m) {
        const double mn = qv_min(b, v);
        const double Q = mn > 0.0 ? mn : 0.0;
        const u32 q = __float_as_uint(__double2float_rn(Q));
        const u64 W = (i + 1u < m ? rank[i + 1u] : cov + 1u) - rank[i];
        oW[i] = W;
        oq[i] = q;
        pos = q ? W : 0ull;             // (q >= +0.0: its bits are 0 or it is positive)
    }
    pos = cx_wave_sum(pos);
    if (lane == 0 && pos) atomicAdd(&tot[0], (unsigned long long)pos);
}

// out[0] = pcut(X) of the table; q is non-increasing: the rows that reach X are the first `lo`
__global__ void __launch_bounds__(64) k_qv_cutoff(const u32 *__restrict__ u, const u32 *__restrict__ q, u64 m, double X, double *__restrict__ out)
{
    if (threadIdx.x) return;
    u64 lo = 0, hi = m;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2u;
        if ((double)__uint_as_float(q[mid]) >= X) lo = mid + 1u;
        else hi = mid;
    }
    out[0] = lo ? (double)__uint_as_float(u[lo - 1u]) : QV_NONE;
}

// the q-score's bits of the value with these bits: a binary search of u (descending: every u is >= +0.0, so its bits descend too);
// a miss sets miss[0] and gives 0
__device__ __forceinline__ u32 qv_lookup(const u32 *__restrict__ u, const u32 *__restrict__ q, u64 m, u32 bits, u32 *__restrict__ miss)
{
    u64 lo = 0, hi = m;
    while (lo < hi) {
        const u64 mid = lo + (hi - lo) / 2u;
        if (u[mid] > bits) lo = mid + 1u;
        else hi = mid;
    }
    if (lo < m && u[lo] == bits) return q[lo];
    atomicOr(miss, 1u);
    return 0u;
}

namespace {

// the work of qvalue behind its checks; a failure leaves no table.  The signal runs are only read.
int coverage_qvalue_run(pmx_dbam *b, const std::string &fn)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    const u64 n = c.snruns;
    u64 N = 0, m = 0, cov = 0;
    unsigned long long pos = 0;
    for (int r : c.chosen) N += (u64)(u32)std::max<int64_t>(b->ref_lens[(u64)r], 0);
    if (n) {
        const CvRuns V(c.sruns.as<u8>(), n);
        const u64 nwg = (n + 255) / 256;
        const u32 ntiles = (u32)((n + BED_RS_TILE - 1) / BED_RS_TILE);
        const u64 ncnt = 256ull * ntiles;               // (ncnt >= nwg: the counts and the bases of the sort serve the scans behind it)
        DevAlloc d_key, d_wt, d_ka, d_kb, d_va, d_vb, d_cnt, d_base, d_tot, d_x, d_r;
        CvHold held(b);
        auto work = [&](DevAlloc &d, u64 bytes) {
            if (hipMalloc(&d.p, bytes) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory: " + std::to_string(bytes) + " bytes asked for (" + std::to_string(n) + " runs)");
            }
            held.add(bytes);
            return 0;
        };
        for (DevAlloc *d : {&d_key, &d_wt, &d_ka, &d_kb})
            if (int rc = work(*d, 8 * n)) return rc;
        for (DevAlloc *d : {&d_va, &d_vb})
            if (int rc = work(*d, 4 * n)) return rc;
        if (int rc = work(d_cnt, 4 * ncnt)) return rc;
        if (int rc = work(d_base, 8 * ncnt)) return rc;
        if (int rc = work(d_tot, 64)) return rc;
        unsigned long long tot[8] = {0, ~0ull, 0, 0, 0, 0, 0, 0};      // the OR and the AND of the keys; k_bam_scan's two totals; the bases with q > 0
        unsigned long long *dt = d_tot.as<unsigned long long>();
        HIPOK(hipMemcpyAsync(dt, tot, 64, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_qv_keys, dim3((unsigned)nwg), dim3(256), 0, st, V.start, V.end, V.depth, n, d_key.as<u64>(), d_wt.as<u64>(), dt);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(tot, dt, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        const u64 *kin = d_key.as<u64>();
        const u32 *vin = nullptr;
        if (int rc = cx_sort(st, n, tot[0] ^ tot[1], kin, vin, d_ka.as<u64>(), d_kb.as<u64>(), d_va.as<u32>(), d_vb.as<u32>(), d_cnt.as<u32>(),
                             d_base.as<u64>(), (u64 *)(dt + 2)))
            return rc;
        unsigned long long *P = d_wt.as<unsigned long long>();         // (no pass ran: every key is the same and the order is the runs')
        if (vin) {
            P = (unsigned long long *)(kin == d_ka.as<u64>() ? d_kb.as<u64>() : d_ka.as<u64>());
            hipLaunchKernelGGL(k_cx_gather, dim3((unsigned)nwg), dim3(256), 0, st, d_wt.as<u64>(), vin, n, (u64 *)P);
            HIPOK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_ps_sums, dim3((unsigned)nwg), dim3(256), 0, st, P, n, d_base.as<u64>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_ps_scan, dim3(1), dim3(1024), 0, st, d_base.as<u64>(), nwg);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_ps_apply, dim3((unsigned)nwg), dim3(256), 0, st, P, n, d_base.as<u64>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_qv_count, dim3((unsigned)nwg), dim3(256), 0, st, kin, n, d_cnt.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cnt.as<u32>(), d_cnt.as<u32>(), nwg, d_base.as<u64>(), (u64 *)(dt + 2));
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&m, dt + 2, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(&cov, P + (n - 1), 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (hipMalloc(&c.qtab.p, 16 * m) != hipSuccess) {               // (m >= 1: the first key is a head)
            (void)hipGetLastError();
            return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for the table: " + std::to_string(16 * m) + " bytes asked for (16 per distinct value)");
        }
        c.qrows = m;                    // (counted from here on: qvalue_drop takes them off again)
        c.bytes += 16 * m;
        if (b->st) stream_note(*b);
        if (int rc = work(d_x, 8 * m)) return rc;
        if (int rc = work(d_r, 8 * m)) return rc;
        const QvTable T(c.qtab.as<u8>(), m);
        const u64 mwg = (m + 255) / 256;                                // (mwg <= nwg: d_base is used again)
        hipLaunchKernelGGL(k_qv_heads, dim3((unsigned)nwg), dim3(256), 0, st, kin, P, n, N, d_base.as<u64>(), T.u, d_r.as<u64>(),
                           d_x.as<unsigned long long>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_qv_mins, dim3((unsigned)mwg), dim3(256), 0, st, d_x.as<unsigned long long>(), m, d_base.as<unsigned long long>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_qv_minscan, dim3(1), dim3(1024), 0, st, d_base.as<unsigned long long>(), mwg);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_qv_apply, dim3((unsigned)mwg), dim3(256), 0, st, d_x.as<unsigned long long>(), d_r.as<u64>(), m,
                           d_base.as<unsigned long long>(), cov, T.W, T.q, dt + 4);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&pos, dt + 4, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));            // (the keys, the sort's buffers and the scans are freed behind it)
    }
    c.qhave = true;
    c.qtot[0] = m;
    c.qtot[1] = N;
    c.qtot[2] = cov;
    c.qtot[3] = pos;
    return 0;
}

int coverage_qvalue_impl(pmx_dbam *b, uint64_t *totals)
{
    const std::string fn = "pmx_dbam_coverage_qvalue";
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    for (int k = 0; k < 4; k++) totals[k] = 0;
    Coverage &c = b->cv;
    if (c.state != CV_RUNS || !c.shave) return fail(PMX_DBAM_ERR_INVALID, fn + ": no signal: call pmx_dbam_coverage_poisson first");
    if (!c.spscore) return fail(PMX_DBAM_ERR_INVALID, fn + ": the signal is not a p-score track: call pmx_dbam_coverage_poisson first");
    if (c.snruns >= (1ull << 32)) return fail(PMX_DBAM_ERR_INVALID, fn + ": 2^32 signal runs or more");
    if (c.snruns && c.stot[2] < 0.0) return fail(PMX_DBAM_ERR_INVALID, fn + ": the smallest value of the track is negative: not a p-score");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    call_drop(c);                       // (the peaks of a call before: their lines would change; call again)
    qvalue_drop(c);
    struct Drop {       // a failure from here on leaves no table
        Coverage &c;
        bool ok = false;
        ~Drop()
        {
            if (!ok) qvalue_drop(c);
        }
    } drop{c};
    if (int rc = coverage_qvalue_run(b, fn)) return rc;
    drop.ok = true;
    for (int k = 0; k < 4; k++) totals[k] = c.qtot[k];
    return 0;
}

int coverage_qvalue_have(pmx_dbam *b, const std::string &fn)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (b->cv.state != CV_RUNS || !b->cv.qhave) return fail(PMX_DBAM_ERR_INVALID, fn + ": no table: call pmx_dbam_coverage_qvalue first");
    return 0;
}

int coverage_qvalue_rows_impl(pmx_dbam *b, int64_t first, int64_t n, float *p, uint64_t *bases, float *q)
{
    const std::string fn = "pmx_dbam_coverage_qvalue_rows";
    if (int rc = coverage_qvalue_have(b, fn)) return rc;
    const u64 m = b->cv.qrows;
    if (first < 0 || n < 0 || (u64)first > m || (u64)n > m - (u64)first) return fail(PMX_DBAM_ERR_INVALID, fn + ": range outside the rows");
    if (!p || !bases || !q) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    if (n == 0) return 0;
    const QvTable T(b->cv.qtab.as<u8>(), m);
    HIPOK(hipMemcpy(p, T.u + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(bases, T.W + first, 8 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(q, T.q + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    return 0;
}

int coverage_qvalue_cutoff_impl(pmx_dbam *b, double X, double *pcut)
{
    const std::string fn = "pmx_dbam_coverage_qvalue_cutoff";
    if (int rc = coverage_qvalue_have(b, fn)) return rc;
    if (!pcut) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    *pcut = 0.0;
    if (!std::isfinite(X)) return fail(PMX_DBAM_ERR_INVALID, fn + ": X is a finite number");
    const u64 m = b->cv.qrows;
    if (m == 0) {
        *pcut = QV_NONE;
        return 0;
    }
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    DevAlloc d_out;
    CvHold held(b);
    held.add(8);
    HIPOK(hipMalloc(&d_out.p, 8));
    const QvTable T(b->cv.qtab.as<u8>(), m);
    hipLaunchKernelGGL(k_qv_cutoff, dim3(1), dim3(64), 0, st, T.u, T.q, m, X, d_out.as<double>());
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(pcut, d_out.p, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_qvalue(pmx_dbam *b, uint64_t totals[4])
{
    return guarded("pmx_dbam_coverage_qvalue", [&] { return coverage_qvalue_impl(b, totals); });
}

int pmx_dbam_coverage_qvalue_rows(pmx_dbam *b, int64_t first, int64_t n, float *p, uint64_t *bases, float *q)
{
    return guarded("pmx_dbam_coverage_qvalue_rows", [&] { return coverage_qvalue_rows_impl(b, first, n, p, bases, q); });
}

int pmx_dbam_coverage_qvalue_cutoff(pmx_dbam *b, double X, double *pcut)
{
    return guarded("pmx_dbam_coverage_qvalue_cutoff", [&] { return coverage_qvalue_cutoff_impl(b, X, pcut); });
}

}  // extern "C"
