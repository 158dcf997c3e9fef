// Two pileups as one signal track: treatment against control (pmx_dbam_coverage_compare, include/pymasc_amd_ingest.h; DESIGN.md
// 7.18.4).  Included in bam_device.hip behind signal_device.inc: the runs are kept in the treatment handle's signal slot, and every
// pmx_dbam_coverage_signal_* consumer serves them.
//
// The definitions.  Two pileups in the runs state over the same chosen references (the same names and lengths in the same order).
// S_t[j] and S_c[j] are the integer depth sums per bin of B bases, with the bins, the widths w_j and the bound on S of
// signal_device.inc; B is 1 .. 65536.  a_t, a_c and the pseudocount p are float64.  Per bin, in float64, each operation rounded to
// nearest even on its own (no fused multiply-add):
//   t = (f64(S_t) * a_t) / f64(w)        c = (f64(S_c) * a_c) / f64(w)
//   subtract: v = f32(t - c)     ratio: v = f32((t + p) / (c + p))     log2: v = f32(lg2((t + p) / (c + p)))
// lg2(x) of a positive normal float64, a stated algorithm:
//   1. (m, e) = frexp(x), m in [0.5, 1): the exponent field, taken with integer operations
//   2. if m < C = 0.7071067811865476 (the float64 of sqrt(1/2)): m = 2 m, e = e - 1
//   3. f = m - 1.0; s = f / (2.0 + f); z = s * s
//   4. P = c_10; for k = 9 .. 0: P = P * z + c_k, c_k = 1.0 / (2 k + 1) as a float64 division (c_0 = 1.0)
//   5. ln = (2.0 * s) * P; lg2 = f64(e) + ln * 1.4426950408889634
// Consecutive bins of one reference are one run when they have the same S_t, the same S_c and the same width -- the rule is on the
// sums, not on v --; bins with S_t = 0 and S_c = 0 are in no run; a bin only the control covers is in one.  A run is (ref, start0,
// end0, v), in header order.  Totals: runs, covered bases, the smallest and the largest v as signed floats.
// Refused: a factor, or for log2 / ratio p, below 2^-64 or not finite; a * max_depth >= 2^40 of either track; p >= 2^40; for ratio
// (a_t * max_depth_t + p) / p >= 2^40 (|v| < 2^40: the text stays integer arithmetic).  subtract ignores p.
//
//   k_cv_bin_fill    once per handle into its own dense u64 table, for B = 1 as for any other bin (two run lists do not line up)
//   k_cp_mark / k_bam_scan / k_cp_entries   sg_begins extended to both sums; compacted into (reference, bin, S_t, S_c)
//   k_cp_keep / k_bam_scan / k_cp_close     the (0, 0) entries dropped, v by op, the totals through sg_totals
// Device memory: 16 bytes per bin + 24 per entry inside compare (counted in the handle's bytes while it runs, freed before it
// returns), then 16 per run in the signal slot.

#define CP_LOG2 0
#define CP_RATIO 1
#define CP_SUBTRACT 2

__device__ __forceinline__ double cp_lg2(double x)
{
#pragma clang fp contract(off)
    const u64 bits = (u64)__double_as_longlong(x);
    int e = (int)((bits >> 52) & 2047u) - 1022;                                             // (x is normal and positive)
    double m = __longlong_as_double((long long)((bits & 0x000fffffffffffffull) | (1022ull << 52)));
    if (m < 0.7071067811865476) {
        m = 2.0 * m;
        e = e - 1;
    }
    const double f = m - 1.0;
    const double d = 2.0 + f;
    const double s = f / d;
    const double z = s * s;
    const double ck[10] = {1.0, 1.0 / 3.0, 1.0 / 5.0, 1.0 / 7.0, 1.0 / 9.0, 1.0 / 11.0, 1.0 / 13.0, 1.0 / 15.0, 1.0 / 17.0, 1.0 / 19.0};
    double P = 1.0 / 21.0;
#pragma unroll
    for (int k = 9; k >= 0; k--) {
        const double q = P * z;
        P = q + ck[k];
    }
    const double s2 = 2.0 * s;
    const double ln = s2 * P;
    const double l2 = ln * 1.4426950408889634;
    return (double)e + l2;
}

// the bits of v of a bin with the sums St, Sc and the width w
__device__ __forceinline__ u32 cp_value(u64 St, u64 Sc, u32 w, int op, double at, double ac, double p)
{
#pragma clang fp contract(off)
    const double xt = (double)St * at, xc = (double)Sc * ac;
    const double t = xt / (double)w, c = xc / (double)w;
    double v;
    if (op == CP_SUBTRACT) {
        v = t - c;
    } else {
        const double tp = t + p, cp = c + p;
        const double x = tp / cp;
        v = op == CP_RATIO ? x : cp_lg2(x);
    }
    return __float_as_uint(__double2float_rn(v));
}

// sg_begins over both tables
__device__ __forceinline__ bool cp_begins(const unsigned long long *__restrict__ tt, const unsigned long long *__restrict__ tc, u64 b,
                                          const SgGeo &G, u32 &k, u32 &j)
{
    k = cv_zoom_id(G.boff, G.nc, b);
    j = (u32)(b - G.boff[k]);
    if (j == 0) return true;
    return ((u64)j + 1u) * G.B > (u64)G.lens[k] || tt[b - 1u] != tt[b] || tc[b - 1u] != tc[b];
}

__global__ void __launch_bounds__(256) k_cp_mark(const unsigned long long *__restrict__ tt, const unsigned long long *__restrict__ tc, u64 nb,
                                                 SgGeo G, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 b = (u64)blockIdx.x * 256u + t;
    u32 k, j;
    const u64 m = __ballot(b < nb && cp_begins(tt, tc, b, G, k, j));
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) kcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) k_cp_entries(const unsigned long long *__restrict__ tt, const unsigned long long *__restrict__ tc, u64 nb,
                                                    SgGeo G, const u64 *__restrict__ kbase, u32 *__restrict__ eid, u32 *__restrict__ ej,
                                                    unsigned long long *__restrict__ eSt, unsigned long long *__restrict__ eSc)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 b = (u64)blockIdx.x * 256u + t;
    u32 k = 0, j = 0;
    const bool keep = b < nb && cp_begins(tt, tc, b, G, k, j);
    const u64 m = __ballot(keep);
    if (lane == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (!keep) return;
    u64 o = kbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 x = 0; x < (t >> 6); x++) o += s_w[x];
    eid[o] = k;
    ej[o] = j;
    eSt[o] = tt[b];
    eSc[o] = tc[b];
}

__global__ void __launch_bounds__(256) k_cp_keep(const unsigned long long *__restrict__ eSt, const unsigned long long *__restrict__ eSc, u64 n,
                                                 u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 k = (u64)blockIdx.x * 256u + t;
    const u64 m = __ballot(k < n && (eSt[k] | eSc[k]) != 0);
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) kcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) k_cp_close(const u32 *__restrict__ eid, const u32 *__restrict__ ej, const unsigned long long *__restrict__ eSt,
                                                  const unsigned long long *__restrict__ eSc, u64 n, const u64 *__restrict__ kbase, SgGeo G,
                                                  int op, double at, double ac, double p, int *__restrict__ oref, u32 *__restrict__ ostart,
                                                  u32 *__restrict__ oend, u32 *__restrict__ oval, unsigned long long *__restrict__ tot)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 k = (u64)blockIdx.x * 256u + t;
    const bool keep = k < n && (eSt[k] | eSc[k]) != 0;
    const u64 m = __ballot(keep);
    if (lane == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    u64 width = 0;
    u32 bits = 0;
    if (keep) {
        u64 o = kbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
        for (u32 x = 0; x < (t >> 6); x++) o += s_w[x];
        const u32 id = eid[k], len = G.lens[id];
        const u32 a = ej[k] * G.B;                                                         // (below len < 2^32)
        const u32 z = k + 1u < n && eid[k + 1u] == id ? ej[k + 1u] * G.B : len;
        const u32 w = len - a < G.B ? len - a : G.B;                                       // the width of the run's bins
        bits = cp_value((u64)eSt[k], (u64)eSc[k], w, op, at, ac, p);
        oref[o] = G.cref[id];
        ostart[o] = a;
        oend[o] = z;
        oval[o] = bits;
        width = (u64)(z - a);
    }
    sg_totals(lane, keep, width, bits, tot);
}

namespace {

// the work of compare behind its checks; a failure leaves no signal.  The control's stream has been waited for.
int coverage_compare_run(pmx_dbam *b, pmx_dbam *ctl, const std::string &fn, u32 bin, int op, double at, double ac, double p)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    const Coverage &cc = ctl->cv;
    unsigned long long tot[3] = {0, ~0ull, 0};
    u64 nout = 0;
    if (c.nruns || cc.nruns) {
        const u64 nc = c.chosen.size();
        std::vector<u64> boff(nc + 1, 0), boft(std::max<u64>(b->ref_names.size(), 1), 0), bofc(std::max<u64>(ctl->ref_names.size(), 1), 0);
        std::vector<u32> lens(nc, 0);
        std::vector<int> cref(nc, 0);
        for (u64 k = 0; k < nc; k++) {
            lens[k] = (u32)std::max<int64_t>(b->ref_lens[(u64)c.chosen[k]], 0);
            cref[k] = c.chosen[k];
            boft[(u64)c.chosen[k]] = boff[k];
            bofc[(u64)cc.chosen[k]] = boff[k];
            boff[k + 1] = boff[k] + ((u64)lens[k] + bin - 1) / bin;
        }
        const u64 nb = boff[nc], nwg = (nb + 255) / 256;
        if (nwg >= (1ull << 31)) return fail(PMX_DBAM_ERR_INVALID, fn + ": 2^39 bins or more");
        DevAlloc d_tot, d_geo, d_tab, d_k, d_kb, d_e;
        CvHold held(b);
        HIPOK(hipMalloc(&d_tot.p, 64));
        HIPOK(hipMemcpyAsync(d_tot.p, tot, 24, hipMemcpyHostToDevice, st));
        u64 *dt = d_tot.as<u64>();
        const u64 geo_bytes = 8 * boff.size() + 8 * boft.size() + 8 * bofc.size() + 8 * std::max<u64>(nc, 1);
        HIPOK(hipMalloc(&d_geo.p, geo_bytes));
        if (hipMalloc(&d_tab.p, 16 * std::max<u64>(nb, 1)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for the bin tables: " + std::to_string(16 * nb) +
                                               " bytes asked for (16 per bin of " + std::to_string(bin) + " bases)");
        }
        held.add(geo_bytes + 16 * nb + 12 * nwg);
        HIPOK(hipMalloc(&d_k.p, 4 * std::max<u64>(nwg, 1)));
        HIPOK(hipMalloc(&d_kb.p, 8 * std::max<u64>(nwg, 1)));
        u64 *d_boff = d_geo.as<u64>(), *d_boft = d_boff + boff.size(), *d_bofc = d_boft + boft.size();
        u32 *d_lens = (u32 *)(d_bofc + bofc.size());
        int *d_cref = (int *)(d_lens + std::max<u64>(nc, 1));
        HIPOK(hipMemcpyAsync(d_boff, boff.data(), 8 * boff.size(), hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_boft, boft.data(), 8 * boft.size(), hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_bofc, bofc.data(), 8 * bofc.size(), hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_lens, lens.data(), 4 * nc, hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_cref, cref.data(), 4 * nc, hipMemcpyHostToDevice, st));
        HIPOK(hipMemsetAsync(d_tab.p, 0, 16 * nb, st));
        const SgGeo G{d_boff, d_lens, d_cref, (u32)nc, bin};
        unsigned long long *tt = d_tab.as<unsigned long long>(), *tc = tt + nb;
        if (c.nruns) {
            const CvRuns V(c.runs.as<u8>(), c.nruns);
            hipLaunchKernelGGL(k_cv_bin_fill, dim3((unsigned)((c.nruns + 255) / 256)), dim3(256), 0, st, V.ref, V.start, V.end, V.depth, c.nruns, d_boft,
                               bin, tt);
            HIPOK(hipGetLastError());
        }
        if (cc.nruns) {
            const CvRuns V((u8 *)cc.runs.p, cc.nruns);
            hipLaunchKernelGGL(k_cv_bin_fill, dim3((unsigned)((cc.nruns + 255) / 256)), dim3(256), 0, st, V.ref, V.start, V.end, V.depth, cc.nruns,
                               d_bofc, bin, tc);
            HIPOK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_cp_mark, dim3((unsigned)nwg), dim3(256), 0, st, tt, tc, nb, G, d_k.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), nwg, d_kb.as<u64>(), dt + 4);
        HIPOK(hipGetLastError());
        u64 ne = 0;
        HIPOK(hipMemcpyAsync(&ne, dt + 4, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));       // (boff, boft, bofc, lens and cref are locals)
        if (hipMalloc(&d_e.p, 24 * ne) != hipSuccess) {      // (ne >= 1: a run lies in a bin, so a reference has one)
            (void)hipGetLastError();
            return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(ne) + " bin boundaries");
        }
        held.add(24 * ne);
        unsigned long long *eSt = d_e.as<unsigned long long>(), *eSc = eSt + ne;
        u32 *eid = (u32 *)(eSc + ne), *ej = eid + ne;
        hipLaunchKernelGGL(k_cp_entries, dim3((unsigned)nwg), dim3(256), 0, st, tt, tc, nb, G, d_kb.as<u64>(), eid, ej, eSt, eSc);
        HIPOK(hipGetLastError());
        const u64 ewg = (ne + 255) / 256;          // (ewg <= nwg: d_k and d_kb are used again)
        hipLaunchKernelGGL(k_cp_keep, dim3((unsigned)ewg), dim3(256), 0, st, eSt, eSc, ne, d_k.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), ewg, d_kb.as<u64>(), dt + 6);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&nout, dt + 6, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (nout) {
            if (hipMalloc(&c.sruns.p, 16 * nout) != hipSuccess) {
                (void)hipGetLastError();
                return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(nout) + " runs");
            }
            c.snruns = nout;        // (counted from here on: signal_drop takes them off again)
            c.bytes += 16 * nout;
            if (b->st) stream_note(*b);
            const CvRuns O(c.sruns.as<u8>(), nout);
            hipLaunchKernelGGL(k_cp_close, dim3((unsigned)ewg), dim3(256), 0, st, eid, ej, eSt, eSc, ne, d_kb.as<u64>(), G, op, at, ac, p, O.ref, O.start,
                               O.end, O.depth, d_tot.as<unsigned long long>());
            HIPOK(hipGetLastError());
        }
        HIPOK(hipMemcpyAsync(tot, d_tot.p, 24, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));            // (the tables, the entries and the scans are freed behind it)
    }
    float lo = 0.0f, hi = 0.0f;
    if (nout) {
        const u32 l = sg_unkey((u32)tot[1]), h = sg_unkey((u32)tot[2]);
        memcpy(&lo, &l, 4);
        memcpy(&hi, &h, 4);
    }
    c.shave = true;
    c.sbin = bin;
    c.stot[0] = (double)nout;
    c.stot[1] = (double)(nout ? tot[0] : 0);
    c.stot[2] = (double)lo;
    c.stot[3] = (double)hi;
    return 0;
}

int coverage_compare_impl(pmx_dbam *b, pmx_dbam *ctl, uint32_t bin, int op, double at, double ac, double p, double *totals)
{
    const std::string fn = "pmx_dbam_coverage_compare";
    if (!b || !ctl) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    for (int k = 0; k < 4; k++) totals[k] = 0;
    Coverage &c = b->cv;
    const Coverage &cc = ctl->cv;
    if (c.state != CV_RUNS) return fail(PMX_DBAM_ERR_INVALID, fn + ": no runs: call pmx_dbam_coverage_finish first");
    if (cc.state != CV_RUNS) return fail(PMX_DBAM_ERR_INVALID, fn + ": the control has no runs: call pmx_dbam_coverage_finish on it first");
    if (b->device != ctl->device) return fail(PMX_DBAM_ERR_INVALID, fn + ": the control is on another device");
    bool same = c.chosen.size() == cc.chosen.size();
    for (u64 k = 0; same && k < c.chosen.size(); k++) {
        const u64 x = (u64)c.chosen[k], y = (u64)cc.chosen[k];
        same = b->ref_names[x] == ctl->ref_names[y] && std::max<int64_t>(b->ref_lens[x], 0) == std::max<int64_t>(ctl->ref_lens[y], 0);
    }
    if (!same) return fail(PMX_DBAM_ERR_INVALID, fn + ": the chosen references of the control differ in name, length or order");
    if (bin < 1 || bin > SG_MAX_BIN) return fail(PMX_DBAM_ERR_INVALID, fn + ": a bin of 1 to 65536 bases");
    if (op != CP_LOG2 && op != CP_RATIO && op != CP_SUBTRACT)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": the operation is 0 (log2), 1 (ratio) or 2 (subtract)");
    if (!std::isfinite(at) || at < 0x1p-64 || !std::isfinite(ac) || ac < 0x1p-64)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": a factor is a finite number of at least 2^-64");
    if (at * (double)c.tot[4] >= 0x1p40 || ac * (double)cc.tot[4] >= 0x1p40)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": factor * max_depth is 2^40 or more (a value's text is made in 64-bit integers)");
    if (op != CP_SUBTRACT) {
        if (!std::isfinite(p) || p < 0x1p-64) return fail(PMX_DBAM_ERR_INVALID, fn + ": the pseudocount is a finite number of at least 2^-64");
        if (p >= 0x1p40) return fail(PMX_DBAM_ERR_INVALID, fn + ": the pseudocount is 2^40 or more");
        if (op == CP_RATIO && (at * (double)c.tot[4] + p) / p >= 0x1p40)
            return fail(PMX_DBAM_ERR_INVALID, fn + ": (factor * max_depth + pseudocount) / pseudocount is 2^40 or more (a value's text is "
                                                   "made in 64-bit integers)");
    } else {
        p = 0.0;
    }
    HIPOK(hipSetDevice(b->device));
    if (ctl != b) HIPOK(hipStreamSynchronize(ctl->stream));
    HIPOK(hipStreamSynchronize(b->stream));
    signal_drop(c);
    struct Drop {       // a failure from here on leaves no signal
        Coverage &c;
        bool ok = false;
        ~Drop()
        {
            if (!ok) signal_drop(c);
        }
    } drop{c};
    if (int rc = coverage_compare_run(b, ctl, fn, bin, op, at, ac, p)) return rc;
    drop.ok = true;
    for (int k = 0; k < 4; k++) totals[k] = c.stot[k];
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_compare(pmx_dbam *b, pmx_dbam *c, uint32_t bin, int op, double a_t, double a_c, double pseudo, double totals[4])
{
    return guarded("pmx_dbam_coverage_compare", [&] { return coverage_compare_impl(b, c, bin, op, a_t, a_c, pseudo, totals); });
}

}  // extern "C"
