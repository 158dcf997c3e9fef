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
//   k_ps_mark / k_bam_scan / k_ps_entries  a bin begins an entry where it is kept and the bin before is not (or the other way round),
//                    where k or l differs between two kept bins, or where its reference begins; compacted into (reference, bin, k, l),
//                    k = PS_OFF for an entry of bins that are not kept
//   k_ps_keep / k_bam_scan / k_ps_close    the PS_OFF entries dropped; per run (not per bin) the series -- a data-dependent loop per
//                    lane, tens of steps for ordinary bins, thousands for a deep bin with k near l: the lanes of a wave leave it at
//                    different times --, F[k], two lg2; the totals through sg_totals
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

// whether bin b begins an entry; id: its reference, j: its bin there, k: its k, or PS_OFF when it is not kept
__device__ __forceinline__ bool ps_begins(const unsigned long long *__restrict__ tt, const unsigned long long *__restrict__ lam, u64 b,
                                          const SgGeo &G, u32 &id, u32 &j, u32 &k)
{
    id = cv_zoom_id(G.boff, G.nc, b);
    j = (u32)(b - G.boff[id]);
    const u64 St = tt[b], len = G.lens[id], a = (u64)j * G.B;
    const u64 w = len - a < G.B ? len - a : G.B;
    k = St ? (u32)(St / w) : PS_OFF;                        // (k <= max_depth_t <= 2^20)
    if (j == 0) return true;
    const u64 Sp = tt[b - 1u];                              // (the bin before is of the same reference and B wide)
    if ((St != 0) != (Sp != 0)) return true;
    return St != 0 && (k != (u32)(Sp / G.B) || lam[b] != lam[b - 1u]);
}

__global__ void __launch_bounds__(256) k_ps_mark(const unsigned long long *__restrict__ tt, const unsigned long long *__restrict__ lam, u64 nb,
                                                 SgGeo G, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 b = (u64)blockIdx.x * 256u + t;
    u32 id, j, k;
    const u64 m = __ballot(b < nb && ps_begins(tt, lam, b, G, id, j, k));
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) kcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) k_ps_entries(const unsigned long long *__restrict__ tt, const unsigned long long *__restrict__ lam, u64 nb,
                                                    SgGeo G, const u64 *__restrict__ kbase, u32 *__restrict__ eid, u32 *__restrict__ ej,
                                                    u32 *__restrict__ ek, unsigned long long *__restrict__ elam)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 b = (u64)blockIdx.x * 256u + t;
    u32 id = 0, j = 0, k = 0;
    const bool keep = b < nb && ps_begins(tt, lam, b, G, id, j, k);
    const u64 m = __ballot(keep);
    if (lane == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (!keep) return;
    u64 o = kbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 x = 0; x < (t >> 6); x++) o += s_w[x];
    eid[o] = id;
    ej[o] = j;
    ek[o] = k;
    elam[o] = lam[b];
}

__global__ void __launch_bounds__(256) k_ps_keep(const u32 *__restrict__ ek, u64 n, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x;
    const u64 e = (u64)blockIdx.x * 256u + t;
    const u64 m = __ballot(e < n && ek[e] != PS_OFF);
    if ((t & 63u) == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    if (t == 0) kcnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__global__ void __launch_bounds__(256) k_ps_close(const u32 *__restrict__ eid, const u32 *__restrict__ ej, const u32 *__restrict__ ek,
                                                  const unsigned long long *__restrict__ elam, u64 n, const u64 *__restrict__ kbase, SgGeo G,
                                                  const double *__restrict__ F, int *__restrict__ oref, u32 *__restrict__ ostart,
                                                  u32 *__restrict__ oend, u32 *__restrict__ oval, unsigned long long *__restrict__ tot)
{
    __shared__ u32 s_w[4];
    const u32 t = threadIdx.x, lane = t & 63u;
    const u64 e = (u64)blockIdx.x * 256u + t;
    const bool keep = e < n && ek[e] != PS_OFF;
    const u64 m = __ballot(keep);
    if (lane == 0) s_w[t >> 6] = (u32)__popcll(m);
    __syncthreads();
    u64 width = 0;
    u32 bits = 0;
    if (keep) {
        u64 o = kbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
        for (u32 x = 0; x < (t >> 6); x++) o += s_w[x];
        const u32 id = eid[e], len = G.lens[id];
        const u32 a = ej[e] * G.B;                                                         // (below len < 2^32)
        const u32 z = e + 1u < n && eid[e + 1u] == id ? ej[e + 1u] * G.B : len;
        bits = ps_value(ek[e], __longlong_as_double((long long)elam[e]), F);
        oref[o] = G.cref[id];
        ostart[o] = a;
        oend[o] = z;
        oval[o] = bits;
        width = (u64)(z - a);
    }
    sg_totals(lane, keep, width, bits, tot);
}

namespace {

// the work of poisson behind its checks; a failure leaves no signal.  The control's stream has been waited for; its pileup has a run.
int coverage_poisson_run(pmx_dbam *b, pmx_dbam *ctl, const std::string &fn, u32 bin, double ac, u32 small, u32 large, const double *lnfact)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    const Coverage &cc = ctl->cv;
    unsigned long long tot[3] = {0, ~0ull, 0};
    u64 nout = 0;
    const u64 nc = c.chosen.size(), nF = c.tot[4] + 1;
    std::vector<u64> boff(nc + 1, 0), boft(std::max<u64>(b->ref_names.size(), 1), 0), bofc(std::max<u64>(ctl->ref_names.size(), 1), 0);
    std::vector<u32> lens(nc, 0);
    std::vector<int> cref(nc, 0);
    u64 L = 0;
    for (u64 k = 0; k < nc; k++) {
        lens[k] = (u32)std::max<int64_t>(b->ref_lens[(u64)c.chosen[k]], 0);
        cref[k] = c.chosen[k];
        boft[(u64)c.chosen[k]] = boff[k];
        bofc[(u64)cc.chosen[k]] = boff[k];
        boff[k + 1] = boff[k] + ((u64)lens[k] + bin - 1) / bin;
        L += lens[k];
    }
    const u64 nb = boff[nc], nwg = (nb + 255) / 256;        // (nb >= 1: the control has a run, and a run lies in a bin)
    if (nwg >= (1ull << 31)) return fail(PMX_DBAM_ERR_INVALID, fn + ": 2^39 bins or more");
    DevAlloc d_tot, d_geo, d_tab, d_k, d_kb, d_f, d_e;
    CvHold held(b);
    HIPOK(hipMalloc(&d_tot.p, 64));
    HIPOK(hipMemcpyAsync(d_tot.p, tot, 24, hipMemcpyHostToDevice, st));
    u64 *dt = d_tot.as<u64>();
    const u64 geo_bytes = 8 * boff.size() + 8 * boft.size() + 8 * bofc.size() + 8 * std::max<u64>(nc, 1);
    HIPOK(hipMalloc(&d_geo.p, geo_bytes));
    if (hipMalloc(&d_tab.p, 24 * nb) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for the bin tables: " + std::to_string(24 * nb) +
                                           " bytes asked for (24 per bin of " + std::to_string(bin) + " bases)");
    }
    held.add(geo_bytes + 24 * nb + 12 * nwg + 8 * nF);
    HIPOK(hipMalloc(&d_k.p, 4 * nwg));
    HIPOK(hipMalloc(&d_kb.p, 8 * nwg));
    HIPOK(hipMalloc(&d_f.p, 8 * nF));
    u64 *d_boff = d_geo.as<u64>(), *d_boft = d_boff + boff.size(), *d_bofc = d_boft + boft.size();
    u32 *d_lens = (u32 *)(d_bofc + bofc.size());
    int *d_cref = (int *)(d_lens + std::max<u64>(nc, 1));
    HIPOK(hipMemcpyAsync(d_boff, boff.data(), 8 * boff.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_boft, boft.data(), 8 * boft.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_bofc, bofc.data(), 8 * bofc.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_lens, lens.data(), 4 * nc, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_cref, cref.data(), 4 * nc, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_f.p, lnfact, 8 * nF, hipMemcpyHostToDevice, st));
    HIPOK(hipMemsetAsync(d_tab.p, 0, 16 * nb, st));
    const SgGeo G{d_boff, d_lens, d_cref, (u32)nc, bin};
    unsigned long long *tt = d_tab.as<unsigned long long>(), *tc = tt + nb, *lam = tc + nb;
    if (c.nruns) {
        const CvRuns V(c.runs.as<u8>(), c.nruns);
        hipLaunchKernelGGL(k_cv_bin_fill, dim3((unsigned)((c.nruns + 255) / 256)), dim3(256), 0, st, V.ref, V.start, V.end, V.depth, c.nruns, d_boft, bin,
                           tt);
        HIPOK(hipGetLastError());
    }
    {
        const CvRuns V((u8 *)cc.runs.p, cc.nruns);
        hipLaunchKernelGGL(k_cv_bin_fill, dim3((unsigned)((cc.nruns + 255) / 256)), dim3(256), 0, st, V.ref, V.start, V.end, V.depth, cc.nruns, d_bofc,
                           bin, tc);
        HIPOK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_ps_sums, dim3((unsigned)nwg), dim3(256), 0, st, tc, nb, d_kb.as<u64>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_ps_scan, dim3(1), dim3(1024), 0, st, d_kb.as<u64>(), nwg);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_ps_apply, dim3((unsigned)nwg), dim3(256), 0, st, tc, nb, d_kb.as<u64>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_ps_lambda, dim3((unsigned)nwg), dim3(256), 0, st, tc, nb, G, ac, (small / bin) / 2u, (large / bin) / 2u, (int)(small != 0),
                       (int)(large != 0), L, lam);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_ps_mark, dim3((unsigned)nwg), dim3(256), 0, st, tt, lam, nb, G, d_k.as<u32>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), nwg, d_kb.as<u64>(), dt + 4);
    HIPOK(hipGetLastError());
    u64 ne = 0;
    HIPOK(hipMemcpyAsync(&ne, dt + 4, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));       // (boff, boft, bofc, lens, cref and the caller's lnfact have been read)
    if (hipMalloc(&d_e.p, 20 * ne) != hipSuccess) {         // (ne >= 1: the first bin begins an entry)
        (void)hipGetLastError();
        return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(ne) + " bin boundaries");
    }
    held.add(20 * ne);
    unsigned long long *elam = d_e.as<unsigned long long>();
    u32 *eid = (u32 *)(elam + ne), *ej = eid + ne, *ek = ej + ne;
    hipLaunchKernelGGL(k_ps_entries, dim3((unsigned)nwg), dim3(256), 0, st, tt, lam, nb, G, d_kb.as<u64>(), eid, ej, ek, elam);
    HIPOK(hipGetLastError());
    const u64 ewg = (ne + 255) / 256;          // (ewg <= nwg: d_k and d_kb are used again)
    hipLaunchKernelGGL(k_ps_keep, dim3((unsigned)ewg), dim3(256), 0, st, ek, ne, d_k.as<u32>());
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
        hipLaunchKernelGGL(k_ps_close, dim3((unsigned)ewg), dim3(256), 0, st, eid, ej, ek, elam, ne, d_kb.as<u64>(), G, d_f.as<double>(), O.ref, O.start,
                           O.end, O.depth, d_tot.as<unsigned long long>());
        HIPOK(hipGetLastError());
    }
    HIPOK(hipMemcpyAsync(tot, d_tot.p, 24, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));            // (the tables, the entries and the scans are freed behind it)
    float lo = 0.0f, hi = 0.0f;
    if (nout) {
        const u32 l = sg_unkey((u32)tot[1]), h = sg_unkey((u32)tot[2]);
        memcpy(&lo, &l, 4);
        memcpy(&hi, &h, 4);
    }
    c.shave = true;
    c.spscore = true;
    c.sbin = bin;
    c.stot[0] = (double)nout;
    c.stot[1] = (double)(nout ? tot[0] : 0);
    c.stot[2] = (double)lo;
    c.stot[3] = (double)hi;
    return 0;
}

int coverage_poisson_impl(pmx_dbam *b, pmx_dbam *ctl, uint32_t bin, double ac, uint32_t small, uint32_t large, const double *lnfact,
                          uint64_t n_lnfact, double *totals)
{
    const std::string fn = "pmx_dbam_coverage_poisson";
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
    if (small > PS_MAX_WINDOW || large > PS_MAX_WINDOW) return fail(PMX_DBAM_ERR_INVALID, fn + ": a window is 0 (off) to 2^31 - 1 bases");
    if (c.tot[4] > PS_MAX_DEPTH) return fail(PMX_DBAM_ERR_INVALID, fn + ": the treatment's max_depth is above 2^20");
    if (!lnfact || n_lnfact <= c.tot[4])
        return fail(PMX_DBAM_ERR_INVALID, fn + ": the table of ln(i!) has " + std::to_string(lnfact ? n_lnfact : 0) + " entries, the treatment's max_depth + 1 = " +
                                              std::to_string(c.tot[4] + 1) + " are needed");
    if (!std::isfinite(ac) || ac < 0x1p-64) return fail(PMX_DBAM_ERR_INVALID, fn + ": the factor is a finite number of at least 2^-64");
    if (ac * (double)cc.tot[4] >= 0x1p40)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": factor * max_depth is 2^40 or more (a value's text is made in 64-bit integers)");
    if (cc.tot[3] == 0) return fail(PMX_DBAM_ERR_INVALID, fn + ": the control has no covered base: there is no background to score against");
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
    if (int rc = coverage_poisson_run(b, ctl, fn, bin, ac, small, large, lnfact)) return rc;
    drop.ok = true;
    for (int k = 0; k < 4; k++) totals[k] = c.stot[k];
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_poisson(pmx_dbam *b, pmx_dbam *c, uint32_t bin, double a_c, uint32_t small, uint32_t large, const double *lnfact,
                              uint64_t n_lnfact, double totals[4])
{
    return guarded("pmx_dbam_coverage_poisson", [&] { return coverage_poisson_impl(b, c, bin, a_c, small, large, lnfact, n_lnfact, totals); });
}

}  // extern "C"
