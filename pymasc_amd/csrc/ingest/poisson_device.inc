// The treatment scored against the control: -log10 of a Poisson upper tail per bin (pmx_dbam_coverage_poisson,
// include/pymasc_amd_ingest.h; DESIGN.md 7.18.6).  Included in bam_device.hip behind compare_device.inc and before call_device.inc:
// the tables are compare's, the runs are kept in the treatment handle's signal slot, and every pmx_dbam_coverage_signal_* consumer and
// pmx_dbam_coverage_call serve them.  The definitions are this project's own: nothing here was compared with MACS2.
//
// The definitions.  Everything is integer arithmetic or float64, each float64 operation rounded to nearest even on its own (no fused
// multiply-add).  Two pileups in the runs state over the same chosen references (compare's check).  S_t[j] and S_c[j] are the integer
// depth sums per bin of B bases (1 .. 65536) with the bins and the widths w_j of signal_device.inc; reference r has the bins
// 0 .. n_r - 1 and the length len_r.  a_c is a float64 factor (the range of signal's scale, against the control's max_depth); the
// treatment is not scaled: the score counts reads.  W_s and W_l are two window sizes in bases, each 0 (off) .. 2^31 - 1.
//   k          k[j] = S_t[j] / w_j, an integer division
//   window     for W > 0: h = (W / B) / 2 bins; lo = max(0, j - h), hi = min(n_r - 1, j + h), inside j's own reference (a window
//              never crosses into another reference); N = sum S_c[lo .. hi] as u64; D = min(len_r, (hi + 1) * B) - lo * B;
//              c_W = (f64(N) * a_c) / f64(D).  h = 0 gives the bin's own value; a window that is off contributes nothing
//   lambda     c_0 = (f64(S_c[j]) * a_c) / f64(w_j); l_bg = (f64(sum of every S_c) * a_c) / f64(sum of the chosen lengths);
//              l[j] = max(l_bg, c_0, c_Ws, c_Wl).  A control without a covered base is refused: l > 0 and normal everywhere
//   ln, F      ln(x) = lg2(x) * 0.6931471805599453 with cp_lg2 of compare_device.inc; F[0] = F[1] = 0.0, F[i] = F[i - 1] + ln(f64(i)),
//              a sequential sum, made by the caller for max_depth_t + 1 entries (max_depth_t <= 2^20) and handed in as an array
//   score      f64(k) <= l: v = 0.0 (not enriched; equality counts as not enriched).  Otherwise S = 1.0, T = 1.0 and for
//              i = 1, 2, ...: r = l / f64(k + i); T = T * r; S' = S + T; stop when S' == S, else S = S' (r is below 1 and falling:
//              the loop ends).  A = f64(k) * ln(l); C = (l - A) + F[k];
//              v = f32(C * 0.4342944819032518 - lg2(S) * 0.3010299956639812): -log10 of P(X >= k | l), 0 <= v < 2^40
//   runs       a bin with S_t = 0 is in no run.  A kept bin begins a run when it is the first bin of its reference, when the bin
//              before it is not kept, or when k or the bits of l differ from the bin before: the rule is on (k, l), not on v and not
//              on the width.  A run is (ref, start0, end0, v), in header order.  Totals: signal's four
//
//   k_cv_bin_fill                          once per handle, as in compare
//   k_ps_sums / k_ps_scan / k_ps_apply     the inclusive u64 prefix sum of the control's table over the whole concatenated table, in
//                    place: sums of 256 bins per workgroup, one workgroup scans those sums, every workgroup scans its 256 bins behind
//                    its base.  The last element is the sum of every S_c; S_c[j] is a difference of neighbours
//   k_ps_lambda      one lane per bin: the window sums as differences of the prefix at lo - 1 and hi, clipped to the reference through
//                    SgGeo's offsets; l as float64
//                    (the four are the stage poisson puts between the fills and the marks of signal_device.inc's bintrack_run)
//   k_bt_count<PsTrack, false> / k_bam_scan / k_bt_entries<PsTrack>   a bin begins an entry where it is kept and the bin before is
//                    not (or the other way round), where k or l differs between two kept bins, or where its reference begins;
//                    compacted into (reference, bin, k, l), k = PS_OFF for an entry of bins that are not kept
//   k_bt_count<PsTrack, true> / k_bam_scan / k_bt_close<PsTrack>      the PS_OFF entries dropped; per run (not per bin) the series
//                    -- a data-dependent loop per lane, tens of steps for ordinary bins, thousands for a deep bin with k near l: the
//                    lanes of a wave leave it at different times --, F[k], two lg2; the totals through sg_totals
// Device memory: 24 bytes per bin + 12 per 256 bins + 8 per entry of F + 20 per entry inside poisson (counted in the handle's bytes
// while it runs, freed before it returns), then 16 per run in the signal slot.

#define PS_MAX_WINDOW 0x7fffffffu
#define PS_MAX_DEPTH (1u << 20)
#define PS_OFF 0xffffffffu

__device__ __forceinline__ double ps_ln(double x)
{
#pragma clang fp contract(off)
    const double l = cp_lg2(x);
    return l * 0.6931471805599453;
}

// the bits of v of a run with k and l; F[k] is the caller's table
__device__ __forceinline__ u32 ps_value(u32 k, double lam, const double *__restrict__ F)
{
#pragma clang fp contract(off)
    const double kd = (double)k;
    if (kd <= lam) return 0u;
    double S = 1.0, T = 1.0;
    for (u32 i = 1;; i++) {
        const double r = lam / (double)(k + i);            // (k <= 2^20 and the series ends long before 2^31 steps: no wrap)
        T = T * r;
        const double S2 = S + T;
        if (!(S2 > S)) break;           // (T >= 0, so S2 >= S: this is S2 == S, and it also ends on a value that is no number)
        S = S2;
    }
    const double A = kd * ps_ln(lam);
    const double d = lam - A;
    const double C = d + F[k];
    const double x = C * 0.4342944819032518;
    const double y = cp_lg2(S) * 0.3010299956639812;
    return __float_as_uint(__double2float_rn(x - y));
}

__global__ void __launch_bounds__(256) k_ps_sums(const unsigned long long *__restrict__ x, u64 n, u64 *__restrict__ sums)
{
    __shared__ u64 s_w[4];
    const u32 t = threadIdx.x;
    const u64 i = (u64)blockIdx.x * 256u + t;
    const u64 v = cx_wave_sum(i < n ? (u64)x[i] : 0ull);
    if ((t & 63u) == 0) s_w[t >> 6] = v;
    __syncthreads();
    if (t == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// in place, one workgroup: x[i] becomes the sum of the elements in front of it
__global__ void __launch_bounds__(1024) k_ps_scan(u64 *__restrict__ x, u64 n)
{
    __shared__ u64 s[1024];
    const u32 t = threadIdx.x;
    const u64 per = (n + 1023u) / 1024u, lo = (u64)t * per < n ? (u64)t * per : n, hi = lo + per < n ? lo + per : n;
    u64 a = 0;
    for (u64 i = lo; i < hi; i++) a += x[i];
    s[t] = a;
    __syncthreads();
    for (u32 o = 1; o < 1024u; o <<= 1) {
        const u64 y = t >= o ? s[t - o] : 0;
        __syncthreads();
        s[t] += y;
        __syncthreads();
    }
    u64 run = s[t] - a;
    for (u64 i = lo; i < hi; i++) {
        const u64 v = x[i];
        x[i] = run;
        run += v;
    }
}

// in place: x[i] becomes the sum of x[0 .. i]; base[w]: the sum in front of workgroup w
__global__ void __launch_bounds__(256) k_ps_apply(unsigned long long *__restrict__ x, u64 n, const u64 *__restrict__ base)
{
    __shared__ u64 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 i = (u64)blockIdx.x * 256u + t;
    u64 v = i < n ? (u64)x[i] : 0ull;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 y = __shfl_up(v, o, 64);
        if (lane >= (u32)o) v += y;
    }
    if (lane == 63u) s_w[t >> 6] = v;
    __syncthreads();
    u64 o = base[blockIdx.x];
    for (u32 w = 0; w < (t >> 6); w++) o += s_w[w];
    if (i < n) x[i] = (unsigned long long)(o + v);
}

// P: the inclusive prefix of the control's table; hs, hl: the half windows in bins (ons, onl: whether the window is on); L: the sum
// of the chosen lengths
__global__ void __launch_bounds__(256) k_ps_lambda(const unsigned long long *__restrict__ P, u64 nb, SgGeo G, double ac, u32 hs, u32 hl, int ons,
                                                   int onl, u64 L, unsigned long long *__restrict__ lam)
{
#pragma clang fp contract(off)
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    const u32 id = cv_zoom_id(G.boff, G.nc, b);
    const u64 b0 = G.boff[id], n = G.boff[id + 1u] - b0, j = b - b0, len = G.lens[id], B = G.B;
    const u64 w = len - j * B < B ? len - j * B : B;
    const u64 Sc = (u64)P[b] - (b ? (u64)P[b - 1u] : 0ull);
    const double all = (double)(u64)P[nb - 1u] * ac;
    double l = all / (double)L;
    const double x0 = (double)Sc * ac;
    const double c0 = x0 / (double)w;
    l = c0 > l ? c0 : l;
    for (int s = 0; s < 2; s++) {
        if (!(s ? onl : ons)) continue;
        const u64 h = s ? hl : hs;
        const u64 lo = j > h ? j - h : 0ull, hi = j + h < n - 1u ? j + h : n - 1u;
        const u64 N = (u64)P[b0 + hi] - (b0 + lo ? (u64)P[b0 + lo - 1u] : 0ull);
        const u64 D = ((hi + 1u) * B < len ? (hi + 1u) * B : len) - lo * B;
        const double xw = (double)N * ac;
        const double cw = xw / (double)D;
        l = cw > l ? cw : l;
    }
    lam[b] = (unsigned long long)__double_as_longlong(l);
}

namespace {

struct PsTrack {        // poisson: an entry is (reference, bin, k, l), k = PS_OFF for an entry of bins that are not kept
    static constexpr u64 TABLES = 3, ENTRY = 20;
    const double *F;
    const unsigned long long *tt, *lam;
    unsigned long long *elam;
    u32 *eid, *ej, *ek;
    void tables(const unsigned long long *t, u64 nb)
    {
        tt = t;
        lam = t + 2 * nb;
    }
    void entries(u8 *q, u64 ne)
    {
        elam = (unsigned long long *)q;
        eid = (u32 *)(elam + ne);
        ej = eid + ne;
        ek = ej + ne;
    }
    // k: the bin's k, or PS_OFF when it is not kept
    __device__ __forceinline__ bool begins(u64 b, const SgGeo &G, u32 id, u32 j, u32 &k) const
    {
        const u64 St = tt[b], len = G.lens[id], a = (u64)j * G.B;
        const u64 w = len - a < G.B ? len - a : G.B;
        k = St ? (u32)(St / w) : PS_OFF;                        // (k <= max_depth_t <= 2^20)
        if (j == 0) return true;
        const u64 Sp = tt[b - 1u];                              // (the bin before is of the same reference and B wide)
        if ((St != 0) != (Sp != 0)) return true;
        return St != 0 && (k != (u32)(Sp / G.B) || lam[b] != lam[b - 1u]);
    }
    __device__ __forceinline__ void put(u64 o, u64 b, u32 k) const
    {
        ek[o] = k;
        elam[o] = lam[b];
    }
    __device__ __forceinline__ bool kept(u64 e) const { return ek[e] != PS_OFF; }
    // per run, not per bin: the series is a data-dependent loop per lane, and the lanes of a wave leave it at different times
    __device__ __forceinline__ u32 value(u64 e, u32) const { return ps_value(ek[e], __longlong_as_double((long long)elam[e]), F); }
};

int coverage_poisson_impl(pmx_dbam *b, pmx_dbam *ctl, uint32_t bin, double ac, uint32_t small, uint32_t large, const double *lnfact,
                          uint64_t n_lnfact, double *totals)
{
    const std::string fn = "pmx_dbam_coverage_poisson";
    if (int rc = track_checks(b, ctl, true, fn, bin, totals)) return rc;
    Coverage &c = b->cv;
    const Coverage &cc = ctl->cv;
    if (small > PS_MAX_WINDOW || large > PS_MAX_WINDOW) return fail(PMX_DBAM_ERR_INVALID, fn + ": a window is 0 (off) to 2^31 - 1 bases");
    if (c.tot[4] > PS_MAX_DEPTH) return fail(PMX_DBAM_ERR_INVALID, fn + ": the treatment's max_depth is above 2^20");
    if (!lnfact || n_lnfact <= c.tot[4])
        return fail(PMX_DBAM_ERR_INVALID, fn + ": the table of ln(i!) has " + std::to_string(lnfact ? n_lnfact : 0) + " entries, the treatment's max_depth + 1 = " +
                                              std::to_string(c.tot[4] + 1) + " are needed");
    if (!std::isfinite(ac) || ac < 0x1p-64) return fail(PMX_DBAM_ERR_INVALID, fn + ": the factor is a finite number of at least 2^-64");
    if (ac * (double)cc.tot[4] >= 0x1p40)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": factor * max_depth is 2^40 or more (a value's text is made in 64-bit integers)");
    if (cc.tot[3] == 0) return fail(PMX_DBAM_ERR_INVALID, fn + ": the control has no covered base: there is no background to score against");
    DevAlloc d_f;
    // between the fills and the marks: F to the device, the control's table made its prefix sum, l per bin (the control has a run)
    auto lambda = [&](PsTrack &T, const BtStage &R) {
        const u64 nF = c.tot[4] + 1;
        unsigned long long *tc = R.tab + R.nb, *lam = tc + R.nb;
        R.held.add(8 * nF);
        HIPOK(hipMalloc(&d_f.p, 8 * nF));
        HIPOK(hipMemcpyAsync(d_f.p, lnfact, 8 * nF, hipMemcpyHostToDevice, R.st));
        T.F = d_f.as<double>();
        hipLaunchKernelGGL(k_ps_sums, dim3((unsigned)R.nwg), dim3(256), 0, R.st, tc, R.nb, R.kb);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_ps_scan, dim3(1), dim3(1024), 0, R.st, R.kb, R.nwg);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_ps_apply, dim3((unsigned)R.nwg), dim3(256), 0, R.st, tc, R.nb, R.kb);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_ps_lambda, dim3((unsigned)R.nwg), dim3(256), 0, R.st, tc, R.nb, R.G, ac, (small / bin) / 2u, (large / bin) / 2u,
                           (int)(small != 0), (int)(large != 0), R.L, lam);
        HIPOK(hipGetLastError());
        return 0;
    };
    return track_make(b, ctl, totals, [&] {
        if (int rc = bintrack_run(b, ctl, fn, bin, PsTrack{}, lambda)) return rc;
        c.spscore = true;
        return 0;
    });
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_poisson(pmx_dbam *b, pmx_dbam *c, uint32_t bin, double a_c, uint32_t small, uint32_t large, const double *lnfact,
                              uint64_t n_lnfact, double totals[4])
{
    return guarded("pmx_dbam_coverage_poisson", [&] { return coverage_poisson_impl(b, c, bin, a_c, small, large, lnfact, n_lnfact, totals); });
}

}  // extern "C"
