// Peaks called from the signal track (pmx_dbam_coverage_call*, include/pymasc_amd_ingest.h; DESIGN.md 7.18.5).  Included in
// bam_device.hip behind compare_device.inc: the input is the signal slot of the handle, whichever of signal and compare filled it.
//
// The definitions.  The signal runs (ref, start0, end0, v) are in header order; within a reference they ascend and do not overlap, and
// the bases in no run are uncovered.  cutoff is a finite float64 (negative is legal), max_gap 0 .. 2^31 - 1, min_length 1 .. 2^31 - 1.
// Values compare as floats: f64(v) against cutoff and f64(v) against f64(v'); -0.0 equals 0.0.
//   passing    a run passes when f64(v) >= cutoff (equality passes)
//   chains     two consecutive passing runs a, b of one reference are linked when b.start0 - a.end0 <= max_gap, whatever lies between
//              (failing runs or uncovered bases); runs of different references are never linked.  A candidate is a maximal chain:
//              start = its first run's start0, end = its last run's end0
//   peaks      a candidate with end - start >= min_length, in header order, then ascending
//   per peak   value: the largest v of its passing runs, float32; summit = s + (e - s) / 2 (integer division, 0-based) of the FIRST
//              passing run (s, e) with that value; runs: the number of its passing runs
//   totals     passing runs, candidates, peaks, peak bases (end - start summed over the peaks), passing bases (the widths of the
//              passing runs inside peaks), u64
// Only integers, a maximum and a first-argmax appear, so every reduction is associative and nothing depends on scheduling; a mean or
// an area over a peak would be a float sum in some order and is left out on purpose.
// The narrowPeak line of peak number n (1-based in file order: first + i + 1 of a pull):
//   chrom TAB start TAB end TAB peak_<n> TAB score TAB . TAB value TAB -1 TAB -1 TAB (summit - start) LF
// score = trunc(min(max(f64(value) * 10.0, 0.0), 1000.0)), the product exact in float64; value by ValueText of
// signal_device.inc.  No header line.  When the signal slot holds a p-score track (pmx_dbam_coverage_poisson, poisson_device.inc; DESIGN.md
// 7.18.6) the first -1 (column 8) is the value's text as well; on every other track each byte is as above.  When the handle also holds a
// q-score table (pmx_dbam_coverage_qvalue, qvalue_device.inc; DESIGN.md 7.18.7) the second -1 (column 9) is the text of the peak's
// q-score, found by a binary search of the table by the value's bits; without a table each byte is as above.
//
//   k_cl_count<0> / k_bam_scan / k_cl_list<0>   the passing runs, compacted by ballots (256 per workgroup) into the list P of run indices
//   k_cl_count<1> / k_bam_scan / k_cl_list<1>   over P: an element begins a candidate when it is the first, when its reference differs
//                    from the one before, or when start[P_k] - end[P_(k-1)] > max_gap; the begins compacted into C.  Candidate c is
//                    P[C_c .. C_(c+1)): its start and end are two loads
//   k_cl_count<2> / k_bam_scan / k_cl_close     the candidates of at least min_length: reference, start, end, runs and the slice's
//                    first element; the peak bases reduced over the wave, one atomic per wave
//   k_cl_summit      one lane per peak.  A peak of fewer than CL_LONG runs is walked by its lane; the longer ones of a wave are taken
//                    one after the other by all 64 lanes, which reduce (key, index) by shuffles: the larger key wins, on a tie the
//                    smaller index.  key = sg_key of v with zero made canonical, so that the u32 order is the float order
//   k_ln_len<LnPeak> / k_ln_text<LnPeak>        coverage_device.inc's line writer over the peak table
// Device memory: 12 bytes per 256 runs + 4 per passing run + 4 per candidate + 4 per peak inside call (counted in the handle's bytes
// while it runs, freed before it returns), then 24 per peak until the next call, signal, compare, begin or close.

#define CL_LONG 64u
#define CL_MAX_INT 0x7fffffffu

namespace {
struct ClIn {           // what the three compactions read
    const int *ref;     // the signal runs
    const u32 *start, *end, *val;
    const u32 *P, *C;   // the passing runs; the first element in P of every candidate
    u64 n, np, nc;      // signal runs, passing runs, candidates
    double cutoff;
    u32 max_gap, min_length;
};
}  // namespace

// the first and the last element in P of candidate c
__device__ __forceinline__ void cl_slice(const ClIn &A, u64 c, u32 &first, u32 &last)
{
    first = A.C[c];
    last = (c + 1u < A.nc ? A.C[c + 1u] : (u32)A.np) - 1u;
}

// whether element k of step S is kept: 0 a signal run that passes, 1 an element of P that begins a candidate, 2 a candidate that is a peak
template <int S> __device__ __forceinline__ bool cl_keeps(const ClIn &A, u64 k)
{
#pragma clang fp contract(off)
    if (S == 0) return k < A.n && (double)__uint_as_float(A.val[k]) >= A.cutoff;
    if (S == 1) {
        if (k >= A.np) return false;
        if (k == 0) return true;
        const u32 a = A.P[k - 1u], b = A.P[k];
        return A.ref[a] != A.ref[b] || A.start[b] - A.end[a] > A.max_gap;          // (b.start0 >= a.end0 within a reference)
    }
    if (k >= A.nc) return false;
    u32 first, last;
    cl_slice(A, k, first, last);
    return A.end[A.P[last]] - A.start[A.P[first]] >= A.min_length;
}

template <int S> __global__ void __launch_bounds__(256) k_cl_count(ClIn A, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    cv_count(cl_keeps<S>(A, (u64)blockIdx.x * 256u + threadIdx.x), kcnt, s_w);
}

template <int S> __global__ void __launch_bounds__(256) k_cl_list(ClIn A, const u64 *__restrict__ kbase, u32 *__restrict__ out)
{
    __shared__ u32 s_w[4];
    const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool keep = cl_keeps<S>(A, k);
    const u64 o = cv_slot(keep, kbase, s_w);
    if (keep) out[o] = (u32)k;                  // (below 2^32 runs)
}

// tot[0] += peak bases
__global__ void __launch_bounds__(256) k_cl_close(ClIn A, const u64 *__restrict__ kbase, int *__restrict__ oref, u32 *__restrict__ ostart,
                                                  u32 *__restrict__ oend, u32 *__restrict__ oruns, u32 *__restrict__ ofirst,
                                                  unsigned long long *__restrict__ tot)
{
    __shared__ u32 s_w[4];
    const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool keep = cl_keeps<2>(A, k);
    const u64 o = cv_slot(keep, kbase, s_w);
    u64 width = 0;
    if (keep) {
        u32 first, last;
        cl_slice(A, k, first, last);
        const u32 a = A.P[first], s = A.start[a], e = A.end[A.P[last]];
        oref[o] = A.ref[a];
        ostart[o] = s;
        oend[o] = e;
        oruns[o] = last - first + 1u;
        ofirst[o] = first;
        width = (u64)(e - s);
    }
    width = cx_wave_sum(width);
    if ((threadIdx.x & 63u) == 0 && width) atomicAdd(&tot[0], (unsigned long long)width);
}

// element k of P into a lane's best (key << 32 | ~k: the larger key, then the smaller k, is the larger word) and its width
__device__ __forceinline__ void cl_take(const ClIn &A, u32 k, u64 &best, u64 &width)
{
    const u32 r = A.P[k], bits = A.val[r];
    const u32 key = sg_key((bits & 0x7fffffffu) ? bits : 0u);                               // -0.0 is 0.0
    const u64 x = ((u64)key << 32) | (u64)(~k);
    best = x > best ? x : best;
    width += (u64)(A.end[r] - A.start[r]);
}

// tot[1] += passing bases
__global__ void __launch_bounds__(256) k_cl_summit(ClIn A, const u32 *__restrict__ pfirst, const u32 *__restrict__ pruns, u64 npk,
                                                   u32 *__restrict__ osummit, u32 *__restrict__ ovalue, unsigned long long *__restrict__ tot)
{
    const u32 lane = threadIdx.x & 63u;
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool have = i < npk;
    const u32 first = have ? pfirst[i] : 0u, cnt = have ? pruns[i] : 0u;
    u64 best = 0, width = 0;                    // (a key is above 0: no value is a NaN)
    if (cnt < CL_LONG)
        for (u32 j = 0; j < cnt; j++) cl_take(A, first + j, best, width);
    u64 longs = __ballot(cnt >= CL_LONG);       // the same word in every lane: the wave walks the loop together
    while (longs) {
        const int src = __ffsll((unsigned long long)longs) - 1;
        longs &= longs - 1ull;
        const u32 f = __shfl(first, src, 64), c = __shfl(cnt, src, 64);
        u64 x = 0;
        for (u32 j = lane; j < c; j += 64u) cl_take(A, f + j, x, width);
        for (int d = 32; d > 0; d >>= 1) {
            const u64 y = __shfl_xor(x, d, 64);
            x = y > x ? y : x;
        }
        if (lane == (u32)src) best = x;
    }
    if (have) {
        const u32 r = A.P[~(u32)best], s = A.start[r];
        osummit[i] = s + (A.end[r] - s) / 2u;
        ovalue[i] = A.val[r];
    }
    width = cx_wave_sum(width);
    if (lane == 0 && width) atomicAdd(&tot[1], (unsigned long long)width);
}

// trunc(min(max(f64(v) * 10.0, 0.0), 1000.0)) of the float32 with these bits
__device__ __forceinline__ u32 cl_score(u32 bits)
{
#pragma clang fp contract(off)
    double x = (double)__uint_as_float(bits) * 10.0;
    x = x > 0.0 ? x : 0.0;
    x = x < 1000.0 ? x : 1000.0;
    return (u32)x;
}

namespace {
struct ClQ {            // the q-score table of the handle for column 9 (m = 0 and null pointers: there is none); miss: set on a value without a row
    const u32 *u, *q;
    u64 m;
    u32 *miss;
};

// A peak's line (k_ln_len, coverage_device.inc).  no0: the number of the first peak of the pull; ps: the signal is a p-score track
// (poisson_device.inc): column 8 holds the value too; Q: the q-score table, when there is one: column 9 holds the peak's q-score
struct LnPeak {
    const int *pref;
    const u32 *start, *end, *summit, *val;
    u64 no0;
    int ps;
    ClQ Q;
    __device__ __forceinline__ u32 ref(u64 i) const { return (u32)pref[i]; }
    __device__ __forceinline__ u32 len(u64 i) const
    {
        const u32 vl = ValueText(val[i]).len();
        return ln_width(start[i]) + ln_width(end[i]) + 5u + ln_width(no0 + i) + ln_width(cl_score(val[i])) + 1u + vl +
               (ps ? vl + (Q.u ? ValueText(qv_lookup(Q.u, Q.q, Q.m, val[i], Q.miss)).len() : 2u) : 4u) + ln_width(summit[i] - start[i]) + 10u;
    }
    __device__ __forceinline__ void put(u64 i, u8 *q) const
    {
        const u32 s = start[i], e = end[i], bits = val[i];
        const ValueText v(bits);
        *--q = '\n';                    // from the line's end: LF, summit - start, TAB -1 TAB -1 TAB, the value, TAB . TAB, ...
        q = cv_digits(q, summit[i] - s);
        *--q = '\t';
        if (Q.u) {                      // (a q-score table: column 9 is the text of the peak's q-score)
            q = ValueText(qv_lookup(Q.u, Q.q, Q.m, bits, Q.miss)).put(q);
        } else {
            *--q = '1';
            *--q = '-';
        }
        *--q = '\t';
        if (ps) {                       // (a p-score track: column 8 is the value's text as well)
            q = v.put(q);
        } else {
            *--q = '1';
            *--q = '-';
        }
        *--q = '\t';
        q = v.put(q);
        *--q = '\t';
        *--q = '.';
        *--q = '\t';
        q = cv_digits(q, cl_score(bits));
        *--q = '\t';
        u64 no = no0 + i;               // ... the score, TAB, peak_<n>, TAB, end, TAB, start, TAB
        do {
            *--q = (u8)('0' + (u32)(no % 10u));
            no /= 10u;
        } while (no);
        *--q = '_';
        *--q = 'k';
        *--q = 'a';
        *--q = 'e';
        *--q = 'p';
        *--q = '\t';
        q = cv_digits(q, e);
        *--q = '\t';
        q = cv_digits(q, s);
        *--q = '\t';
    }
};
}  // namespace

namespace {

// the arrays of the peak table in its one block: reference, start, end, summit, value, runs (4 bytes per peak each)
struct ClPeaks {
    int *ref;
    u32 *start, *end, *summit, *value, *runs;
    ClPeaks(u8 *p, u64 n)
        : ref((int *)p), start((u32 *)(p + 4 * n)), end((u32 *)(p + 8 * n)), summit((u32 *)(p + 12 * n)), value((u32 *)(p + 16 * n)),
          runs((u32 *)(p + 20 * n))
    {
    }
};

// the work of call behind its checks; a failure leaves no peak table.  The signal runs are only read.
int coverage_call_run(pmx_dbam *b, const std::string &fn, double cutoff, u32 max_gap, u32 min_length)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    const u64 n = c.snruns;
    if (n >= (1ull << 32)) return fail(PMX_DBAM_ERR_INVALID, fn + ": 2^32 signal runs or more");
    unsigned long long tot[2] = {0, 0};
    u64 np = 0, nc = 0, npk = 0;
    if (n) {
        const CvRuns V(c.sruns.as<u8>(), n);
        const u64 nwg = (n + 255) / 256;
        DevAlloc d_tot, d_k, d_kb, d_P, d_C, d_first;
        CvHold held(b);
        held.add(64 + 12 * nwg);
        HIPOK(hipMalloc(&d_tot.p, 64));
        HIPOK(hipMalloc(&d_k.p, 4 * nwg));
        HIPOK(hipMalloc(&d_kb.p, 8 * nwg));
        HIPOK(hipMemsetAsync(d_tot.p, 0, 64, st));
        u64 *dt = d_tot.as<u64>();                  // [0] peak bases, [1] passing bases, [2], [4], [6] the three scans' totals
        u32 *dk = d_k.as<u32>();
        ClIn A{V.ref, V.start, V.end, V.depth, nullptr, nullptr, n, 0, 0, cutoff, max_gap, min_length};
        auto work = [&](DevAlloc &d, u64 m, const char *what) {        // a list of m u32
            if (hipMalloc(&d.p, 4 * m) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(m) + " " + what);
            }
            held.add(4 * m);
            return 0;
        };
        hipLaunchKernelGGL(k_cl_count<0>, dim3((unsigned)nwg), dim3(256), 0, st, A, dk);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, dk, dk, nwg, d_kb.as<u64>(), dt + 2);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&np, dt + 2, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (np) {
            if (int rc = work(d_P, np, "passing runs")) return rc;
            hipLaunchKernelGGL(k_cl_list<0>, dim3((unsigned)nwg), dim3(256), 0, st, A, d_kb.as<u64>(), d_P.as<u32>());
            HIPOK(hipGetLastError());
            A.P = d_P.as<u32>();
            A.np = np;
            const u64 pwg = (np + 255) / 256;       // (pwg <= nwg: d_k and d_kb are used again, and once more below)
            hipLaunchKernelGGL(k_cl_count<1>, dim3((unsigned)pwg), dim3(256), 0, st, A, dk);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, dk, dk, pwg, d_kb.as<u64>(), dt + 4);
            HIPOK(hipGetLastError());
            HIPOK(hipMemcpyAsync(&nc, dt + 4, 8, hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            if (int rc = work(d_C, nc, "candidates")) return rc;           // (nc >= 1: the first element of P begins one)
            hipLaunchKernelGGL(k_cl_list<1>, dim3((unsigned)pwg), dim3(256), 0, st, A, d_kb.as<u64>(), d_C.as<u32>());
            HIPOK(hipGetLastError());
            A.C = d_C.as<u32>();
            A.nc = nc;
            const u64 cwg = (nc + 255) / 256;
            hipLaunchKernelGGL(k_cl_count<2>, dim3((unsigned)cwg), dim3(256), 0, st, A, dk);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, dk, dk, cwg, d_kb.as<u64>(), dt + 6);
            HIPOK(hipGetLastError());
            HIPOK(hipMemcpyAsync(&npk, dt + 6, 8, hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            if (npk) {
                if (int rc = work(d_first, npk, "peaks")) return rc;
                if (hipMalloc(&c.peaks.p, 24 * npk) != hipSuccess) {
                    (void)hipGetLastError();
                    return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(npk) + " peaks");
                }
                c.npeaks = npk;         // (counted from here on: call_drop takes them off again)
                c.bytes += 24 * npk;
                if (b->st) stream_note(*b);
                const ClPeaks K(c.peaks.as<u8>(), npk);
                hipLaunchKernelGGL(k_cl_close, dim3((unsigned)cwg), dim3(256), 0, st, A, d_kb.as<u64>(), K.ref, K.start, K.end, K.runs, d_first.as<u32>(),
                                   d_tot.as<unsigned long long>());
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_cl_summit, dim3((unsigned)((npk + 255) / 256)), dim3(256), 0, st, A, d_first.as<u32>(), K.runs, npk, K.summit, K.value,
                                   d_tot.as<unsigned long long>());
                HIPOK(hipGetLastError());
            }
        }
        HIPOK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));            // (the lists and the scans are freed behind it)
    }
    c.phave = true;
    c.ptot[0] = np;
    c.ptot[1] = nc;
    c.ptot[2] = npk;
    c.ptot[3] = tot[0];
    c.ptot[4] = tot[1];
    return 0;
}

int coverage_call_impl(pmx_dbam *b, double cutoff, uint32_t max_gap, uint32_t min_length, uint64_t *totals)
{
    const std::string fn = "pmx_dbam_coverage_call";
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    for (int k = 0; k < 5; k++) totals[k] = 0;
    Coverage &c = b->cv;
    if (c.state != CV_RUNS || !c.shave)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": no signal: call pmx_dbam_coverage_signal or pmx_dbam_coverage_compare first");
    if (!std::isfinite(cutoff)) return fail(PMX_DBAM_ERR_INVALID, fn + ": the cutoff is a finite number");
    if (max_gap > CL_MAX_INT) return fail(PMX_DBAM_ERR_INVALID, fn + ": max_gap is 0 to 2^31 - 1");
    if (min_length < 1 || min_length > CL_MAX_INT) return fail(PMX_DBAM_ERR_INVALID, fn + ": min_length is 1 to 2^31 - 1");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    call_drop(c);
    struct Drop {       // a failure from here on leaves no peak table
        Coverage &c;
        bool ok = false;
        ~Drop()
        {
            if (!ok) call_drop(c);
        }
    } drop{c};
    if (int rc = coverage_call_run(b, fn, cutoff, max_gap, min_length)) return rc;
    drop.ok = true;
    for (int k = 0; k < 5; k++) totals[k] = c.ptot[k];
    return 0;
}

int coverage_call_range(pmx_dbam *b, const std::string &fn, int64_t first, int64_t n)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (b->cv.state != CV_RUNS || !b->cv.phave) return fail(PMX_DBAM_ERR_INVALID, fn + ": no peaks: call pmx_dbam_coverage_call first");
    const u64 np = b->cv.npeaks;
    if (first < 0 || n < 0 || (u64)first > np || (u64)n > np - (u64)first) return fail(PMX_DBAM_ERR_INVALID, fn + ": range outside the peaks");
    return 0;
}

int coverage_call_rows_impl(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *summit, float *value,
                            uint32_t *runs)
{
    const std::string fn = "pmx_dbam_coverage_call_rows";
    if (int rc = coverage_call_range(b, fn, first, n)) return rc;
    if (!ref || !start || !end || !summit || !value || !runs) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    if (n == 0) return 0;
    const ClPeaks K(b->cv.peaks.as<u8>(), b->cv.npeaks);
    HIPOK(hipMemcpy(ref, K.ref + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(start, K.start + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(end, K.end + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(summit, K.summit + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(value, K.value + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(runs, K.runs + first, 4 * (u64)n, hipMemcpyDeviceToHost));
    return 0;
}

int64_t coverage_call_text_impl(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap)
{
    const std::string fn = "pmx_dbam_coverage_call_text";
    if (int rc = coverage_call_range(b, fn, first, n)) return rc;
    if (buf && cap < 0) return fail(PMX_DBAM_ERR_INVALID, fn + ": a negative capacity");
    if (n == 0) return 0;
    hipStream_t st = b->stream;
    const u64 no0 = (u64)first + 1u;
    const int ps = (int)b->cv.spscore;
    const ClPeaks K(b->cv.peaks.as<u8>(), b->cv.npeaks);
    ClQ Q{nullptr, nullptr, 0, nullptr};
    DevAlloc d_miss;
    CvHold held(b);
    if (b->cv.qhave && ps) {            // (a table of 0 rows goes with 0 runs and 0 peaks: n == 0 has returned)
        const QvTable T(b->cv.qtab.as<u8>(), b->cv.qrows);
        held.add(4);
        HIPOK(hipSetDevice(b->device));
        HIPOK(hipMalloc(&d_miss.p, 4));
        HIPOK(hipMemsetAsync(d_miss.p, 0, 4, st));
        Q = ClQ{T.u, T.q, b->cv.qrows, d_miss.as<u32>()};
    }
    const int64_t got = coverage_text_pull(
        b, fn, (u64)n, buf, cap, LnPeak{K.ref + first, K.start + first, K.end + first, K.summit + first, K.value + first, no0, ps, Q});
    if (got >= 0 && Q.u) {
        u32 miss = 0;
        HIPOK(hipMemcpy(&miss, d_miss.p, 4, hipMemcpyDeviceToHost));
        if (miss) return fail(PMX_DBAM_ERR_DEVICE, fn + ": a peak's value has no row in the q-score table");
    }
    return got;
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_call(pmx_dbam *b, double cutoff, uint32_t max_gap, uint32_t min_length, uint64_t totals[5])
{
    return guarded("pmx_dbam_coverage_call", [&] { return coverage_call_impl(b, cutoff, max_gap, min_length, totals); });
}

int pmx_dbam_coverage_call_rows(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *summit, float *value,
                                uint32_t *runs)
{
    return guarded("pmx_dbam_coverage_call_rows", [&] { return coverage_call_rows_impl(b, first, n, ref, start, end, summit, value, runs); });
}

int64_t pmx_dbam_coverage_call_text(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap)
{
    return guarded("pmx_dbam_coverage_call_text", [&] { return coverage_call_text_impl(b, first, n, buf, cap); });
}

}  // extern "C"
