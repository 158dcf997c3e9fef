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
// signal_device.inc's pipeline (bintrack_run) with the kind CpTrack:
//   k_cv_bin_fill    once per handle into its own dense u64 table, for B = 1 as for any other bin (two run lists do not line up)
//   k_bt_count<CpTrack, false> / k_bam_scan / k_bt_entries<CpTrack>   SgTrack's rule extended to both sums; compacted into
//                    (reference, bin, S_t, S_c)
//   k_bt_count<CpTrack, true> / k_bam_scan / k_bt_close<CpTrack>      the (0, 0) entries dropped, v by op, the totals through sg_totals
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

namespace {

struct CpTrack {        // compare: an entry is (reference, bin, S_t, S_c); SgTrack's rule over both tables
    static constexpr u64 TABLES = 2, ENTRY = 24;
    int op;
    double at, ac, p;
    const unsigned long long *tt, *tc;
    unsigned long long *eSt, *eSc;
    u32 *eid, *ej;
    void tables(const unsigned long long *t, u64 nb)
    {
        tt = t;
        tc = t + nb;
    }
    void entries(u8 *q, u64 ne)
    {
        eSt = (unsigned long long *)q;
        eSc = eSt + ne;
        eid = (u32 *)(eSc + ne);
        ej = eid + ne;
    }
    __device__ __forceinline__ bool begins(u64 b, const SgGeo &G, u32 id, u32 j, u32 &) const
    {
        if (j == 0) return true;
        return ((u64)j + 1u) * G.B > (u64)G.lens[id] || tt[b - 1u] != tt[b] || tc[b - 1u] != tc[b];
    }
    __device__ __forceinline__ void put(u64 o, u64 b, u32) const
    {
        eSt[o] = tt[b];
        eSc[o] = tc[b];
    }
    __device__ __forceinline__ bool kept(u64 e) const { return (eSt[e] | eSc[e]) != 0; }
    __device__ __forceinline__ u32 value(u64 e, u32 w) const { return cp_value((u64)eSt[e], (u64)eSc[e], w, op, at, ac, p); }
};

int coverage_compare_impl(pmx_dbam *b, pmx_dbam *ctl, uint32_t bin, int op, double at, double ac, double p, double *totals)
{
    const std::string fn = "pmx_dbam_coverage_compare";
    if (int rc = track_checks(b, ctl, true, fn, bin, totals)) return rc;
    const Coverage &c = b->cv, &cc = ctl->cv;
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
    return track_make(b, ctl, totals, [&] { return bintrack_run(b, ctl, fn, bin, CpTrack{op, at, ac, p}, bt_no_stage); });
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_compare(pmx_dbam *b, pmx_dbam *c, uint32_t bin, int op, double a_t, double a_c, double pseudo, double totals[4])
{
    return guarded("pmx_dbam_coverage_compare", [&] { return coverage_compare_impl(b, c, bin, op, a_t, a_c, pseudo, totals); });
}

}  // extern "C"
