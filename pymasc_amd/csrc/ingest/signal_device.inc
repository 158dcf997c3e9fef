// The pileup as a signal track: the mean depth per bin times a scale factor, float32 (pmx_dbam_coverage_signal*,
// include/pymasc_amd_ingest.h; DESIGN.md 7.18.3).  Included in bam_device.hip behind coverage_device.inc and deflate_device.inc: the
// host code of every consumer is coverage_device.inc's, run with SG_KIND in place of CV_DEPTH.
//
// The definitions.  Reference r of length len has the bins j = 0 .. ceil(len / B) - 1; bin j covers [j * B, min((j + 1) * B, len)) and
// has the width w_j (only the last bin can be short); S_j is the integer sum of the depth over its bases (below 2^47: exact as u64 and
// as float64); B is 1 .. 65536.  v_j = f32((f64(S_j) * scale) / f64(w_j)): one float64 multiply, one float64 divide, one conversion
// to float32, each rounded to nearest even.  scale is a finite float64 of at least 2^-64 (no value is a float32 denormal) with
// scale * max_depth < 2^40 (v * 10^6 < 2^63: the text is integer arithmetic).  Consecutive bins of one reference are one run when
// they have the same S and the same width -- the rule is on S, not on v --, bins with S = 0 are in no run; a run is (ref, start0, end0,
// v), in header order.  With B = 1 the signal runs are the depth runs with v = f32(f64(depth) * scale).  Totals: runs, covered bases
// (the runs' widths summed), the smallest and the largest v.
// The text of a value is the decimal expansion of the exact value of v rounded to six decimals, ties to even, without trailing
// zeros and without a trailing '.': a float32 is m * 2^e with m < 2^24, so m * 10^6 fits 64 bits and the rounding is a shift, a
// remainder and a comparison with half.
// A zoom bin of level 0 takes the signal runs that overlap it in ascending start order, each by ov bases: validCount = sum ov, min
// and max over v, sum: acc += f64(ov) * f64(v), sumSquares: acc += f64(ov) * (f64(v) * f64(v)), both from 0.0, every multiply and
// add rounded on its own (no fused multiply-add); a bin of level k + 1 adds its up to four bins of level k in index order the same
// way.  The two sums of a data section: its runs in order with the same two products, from 0.0.
//
//   k_sg_convert     B = 1: one lane per depth run
//   k_cv_bin_fill    B > 1: one lane per depth run; the bins it overlaps take overlap * depth by a return-less 64-bit atomic add into a
//                    dense u64 table, one slot per bin of every chosen reference, the references end to end (integers: no order)
//   k_bt_count<K, false> / k_bam_scan / k_bt_entries<K>   the bins-to-runs pipeline every kind of track K shares (SgTrack here,
//                    CpTrack, PsTrack; bintrack_run).  SgTrack: a bin begins an entry where S differs from the bin before, where
//                    its width does (the short last bin) or where its reference begins; compacted by ballots (256 bins per
//                    workgroup; cv_count, cv_slot) into (reference, bin, S)
//   k_bt_count<K, true> / k_bam_scan / k_bt_close<K>      entry k ends where entry k + 1 of its reference begins, the last at the
//                    reference's end; the entries with S = 0 are dropped by this second compaction; the totals are reduced over the
//                    wave, one atomic each per wave, min and max of the float32 through the order-preserving map of their bits to u32
//   k_ln_len<LnSignal> / k_ln_text<LnSignal>   coverage_device.inc's line writer with the value formatted as above (ValueText)
//   k_tr_sections<TrSignal> / k_sg_secsums  one lane per run: its item; one lane per section: its two sums over its runs in order
//   k_sg_zoom_fill   one lane per bin of level 0: a binary search for the first run of its reference that ends behind the bin's
//                    beginning, then forward in order; no atomics
//   k_sg_zoom_fold / k_tr_zoom_emit<TrSignal>   over (u32 valid, f32 min, f32 max, f64 sum, f64 sq), in ZmBins' 28 bytes
// Device memory: 8 bytes per bin + 16 per entry inside signal (counted in the handle's bytes while it runs), then 16 per signal run
// until the next signal, begin or close.

#define SG_MAX_BIN 65536u

namespace {
struct SgGeo {          // the bins of the chosen references k = 0 .. nc - 1 in header order
    const u64 *boff;    // [nc + 1]: the first bin of k
    const u32 *lens;    // [nc]
    const int *cref;    // [nc]: the reference id of k
    u32 nc, B;
};
}  // namespace

__device__ __forceinline__ u32 sg_value(u64 S, double scale, u32 w)
{
#pragma clang fp contract(off)
    const double x = (double)S * scale;
    const double q = x / (double)w;
    return __float_as_uint(__double2float_rn(q));
}

// the order-preserving map of a float32's bits to u32 (all bits of a negative flipped, the top bit of a non-negative set), and back
__host__ __device__ __forceinline__ u32 sg_key(u32 bits) { return bits & 0x80000000u ? ~bits : bits | 0x80000000u; }
__host__ __device__ __forceinline__ u32 sg_unkey(u32 key) { return key & 0x80000000u ? key & 0x7fffffffu : ~key; }

// covered bases, and the keys (sg_key) of the smallest and largest value, of the lanes that `have` a run: tot[0] +=, tot[1] = min,
// tot[2] = max (no value is a NaN: the keys 0 and 0xffffffff stand for no lane)
__device__ __forceinline__ void sg_totals(u32 lane, bool have, u64 width, u32 bits, unsigned long long *__restrict__ tot)
{
    u32 lo = have ? sg_key(bits) : 0xffffffffu, hi = have ? sg_key(bits) : 0u;
    width = cx_wave_sum(have ? width : 0ull);
    for (int d = 32; d > 0; d >>= 1) {
        const u32 x = __shfl_xor(lo, d, 64), y = __shfl_xor(hi, d, 64);
        lo = x < lo ? x : lo;
        hi = y > hi ? y : hi;
    }
    if (lane == 0 && lo != 0xffffffffu) {
        atomicAdd(&tot[0], (unsigned long long)width);
        atomicMin(&tot[1], (unsigned long long)lo);
        atomicMax(&tot[2], (unsigned long long)hi);
    }
}

__global__ void __launch_bounds__(256) k_sg_convert(const int *__restrict__ rref, const u32 *__restrict__ rstart, const u32 *__restrict__ rend,
                                                    const u32 *__restrict__ rdepth, u64 n, double scale, int *__restrict__ oref,
                                                    u32 *__restrict__ ostart, u32 *__restrict__ oend, u32 *__restrict__ oval,
                                                    unsigned long long *__restrict__ tot)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 bits = 0;
    u64 width = 0;
    if (i < n) {
        const u32 s = rstart[i], e = rend[i];
        bits = sg_value((u64)rdepth[i], scale, 1u);
        oref[i] = rref[i];
        ostart[i] = s;
        oend[i] = e;
        oval[i] = bits;
        width = (u64)(e - s);
    }
    sg_totals(threadIdx.x & 63u, i < n, width, bits, tot);
}

// bof[r]: the first bin of reference r (every run lies on a chosen reference)
__global__ void __launch_bounds__(256) k_cv_bin_fill(const int *__restrict__ rref, const u32 *__restrict__ rstart, const u32 *__restrict__ rend,
                                                     const u32 *__restrict__ rdepth, u64 n, const u64 *__restrict__ bof, u32 B,
                                                     unsigned long long *__restrict__ tab)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 s = rstart[i], e = rend[i], d = rdepth[i];
    const u64 b0 = bof[rref[i]];
    const u32 j1 = (e - 1u) / B;                          // (e > s and e <= the reference's length: bin j1 exists)
    for (u32 j = s / B; j <= j1; j++) {
        const u64 lo = (u64)j * B, hi = lo + B;
        const u64 w = (e < hi ? (u64)e : hi) - (s > lo ? (u64)s : lo);
        atomicAdd(&tab[b0 + j], (unsigned long long)(w * d));
    }
}

// From the bin tables to runs, once for every kind of track (signal below, compare_device.inc, poisson_device.inc).  A kind is a small
// struct K that the kernels take by value:
//   TABLES, ENTRY     its u64 tables per bin (the depth sums of k_cv_bin_fill in front) and its bytes per entry: what the call holds
//   tables, entries   where they lie in the call's two blocks (host)
//   eid, ej           the reference and the bin of every entry, written here; the rest of an entry is the kind's
//   begins(b, G, id, j, x)    whether bin b = bin j of reference id begins an entry; x: a word of the kind's own for put
//   put(o, b, x)      the kind's part of entry o, which begins at bin b
//   kept(e)           whether entry e becomes a run
//   value(e, w)       the bits of v of entry e, whose bins are w bases wide
template <class K> __device__ __forceinline__ bool bt_begins(const K &T, u64 b, const SgGeo &G, u32 &id, u32 &j, u32 &x)
{
    id = cv_zoom_id(G.boff, G.nc, b);
    j = (u32)(b - G.boff[id]);
    return T.begins(b, G, id, j, x);
}

// the bins that begin an entry, or with ENTRIES the entries that are kept, per workgroup of 256
template <class K, bool ENTRIES> __global__ void __launch_bounds__(256) k_bt_count(K T, u64 n, SgGeo G, u32 *__restrict__ kcnt)
{
    __shared__ u32 s_w[4];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 id, j, x;
    cv_count(i < n && (ENTRIES ? T.kept(i) : bt_begins(T, i, G, id, j, x)), kcnt, s_w);
}

template <class K> __global__ void __launch_bounds__(256) k_bt_entries(K T, u64 nb, SgGeo G, const u64 *__restrict__ kbase)
{
    __shared__ u32 s_w[4];
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 id = 0, j = 0, x = 0;
    const bool keep = b < nb && bt_begins(T, b, G, id, j, x);
    const u64 o = cv_slot(keep, kbase, s_w);
    if (!keep) return;
    T.eid[o] = id;
    T.ej[o] = j;
    T.put(o, b, x);
}

// entry e ends where entry e + 1 of its reference begins, the last at the reference's end
template <class K> __global__ void __launch_bounds__(256) k_bt_close(K T, u64 n, const u64 *__restrict__ kbase, SgGeo G, int *__restrict__ oref,
                                                                     u32 *__restrict__ ostart, u32 *__restrict__ oend, u32 *__restrict__ oval,
                                                                     unsigned long long *__restrict__ tot)
{
    __shared__ u32 s_w[4];
    const u64 e = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool keep = e < n && T.kept(e);
    const u64 o = cv_slot(keep, kbase, s_w);
    u64 width = 0;
    u32 bits = 0;
    if (keep) {
        const u32 id = T.eid[e], len = G.lens[id];
        const u32 a = T.ej[e] * G.B;                                                       // (below len < 2^32)
        const u32 z = e + 1u < n && T.eid[e + 1u] == id ? T.ej[e + 1u] * G.B : len;
        bits = T.value(e, len - a < G.B ? len - a : G.B);                                  // the width of the run's bins
        oref[o] = G.cref[id];
        ostart[o] = a;
        oend[o] = z;
        oval[o] = bits;
        width = (u64)(z - a);
    }
    sg_totals(threadIdx.x & 63u, keep, width, bits, tot);
}

namespace {
struct SgTrack {        // signal: an entry is (reference, bin, S)
    static constexpr u64 TABLES = 1, ENTRY = 16;
    double scale;
    const unsigned long long *tab;
    unsigned long long *eS;
    u32 *eid, *ej;
    void tables(const unsigned long long *t, u64) { tab = t; }
    void entries(u8 *p, u64 ne)
    {
        eS = (unsigned long long *)p;
        eid = (u32 *)(eS + ne);
        ej = eid + ne;
    }
    __device__ __forceinline__ bool begins(u64 b, const SgGeo &G, u32 id, u32 j, u32 &) const
    {
        if (j == 0) return true;
        return ((u64)j + 1u) * G.B > (u64)G.lens[id] || tab[b - 1u] != tab[b];         // the short last bin; another S
    }
    __device__ __forceinline__ void put(u64 o, u64 b, u32) const { eS[o] = tab[b]; }
    __device__ __forceinline__ bool kept(u64 e) const { return eS[e] != 0; }
    __device__ __forceinline__ u32 value(u64 e, u32 w) const { return sg_value((u64)eS[e], scale, w); }
};
}  // namespace

// round(|v| * 10^6), ties to even, of the float32 with these bits (|v| < 2^40), in integers; the sign is the caller's (sg_minus)
__device__ __forceinline__ u64 sg_micro(u32 bits)
{
    bits &= 0x7fffffffu;
    const u32 ex = (bits >> 23) & 255u;
    const u64 P = (u64)((bits & 0x7fffffu) | (ex ? 0x800000u : 0u)) * 1000000ull;          // m * 10^6 < 2^44; v = m * 2^e
    const int e = (int)(ex ? ex : 1u) - 150;
    if (e >= 0) return P << (e < 19 ? e : 19);                                             // (v < 2^40: e <= 16)
    const u32 sh = (u32)-e;
    if (sh >= 46u) return 0;                                                               // P is below half of 2^sh
    const u64 q = P >> sh, r = P & ((1ull << sh) - 1ull), half = 1ull << (sh - 1u);
    return q + (u64)(r > half || (r == half && (q & 1ull)));
}

// whether the text of the value begins with '-': a negative whose micro-count N is not 0 ("0", never "-0")
__device__ __forceinline__ u32 sg_minus(u32 bits, u64 N) { return (bits >> 31) & (u32)(N != 0); }

// N = round(v * 10^6) as whole part and fraction: the fraction's digits without trailing zeros (nd of them, 0 .. 6)
__device__ __forceinline__ void sg_split(u64 N, u64 &whole, u32 &frac, u32 &nd)
{
    whole = N / 1000000ull;
    frac = (u32)(N - whole * 1000000ull);
    nd = frac ? 6u : 0u;
    while (nd && frac % 10u == 0) {
        frac /= 10u;
        nd--;
    }
}

namespace {
struct ValueText {      // the text of the float32 with these bits: '-', whole part, '.', fraction
    u32 bits, frac, nd;
    u64 N, whole;
    __device__ __forceinline__ explicit ValueText(u32 b) : bits(b), N(sg_micro(b)) { sg_split(N, whole, frac, nd); }
    __device__ __forceinline__ u32 len() const { return sg_minus(bits, N) + ln_width(whole) + (nd ? nd + 1u : 0u); }
    __device__ __forceinline__ u8 *put(u8 *q) const     // in front of q; returns where it begins
    {
        u64 wh = whole;
        u32 fr = frac;
        if (nd) {
            for (u32 c = 0; c < nd; c++) {  // (nd digits, leading zeros among them)
                *--q = (u8)('0' + fr % 10u);
                fr /= 10u;
            }
            *--q = '.';
        }
        do {
            *--q = (u8)('0' + (u32)(wh % 10u));
            wh /= 10u;
        } while (wh);
        if (sg_minus(bits, N)) *--q = '-';
        return q;
    }
};

struct LnSignal {       // a signal run (k_ln_len): name TAB start TAB end TAB value LF
    const int *rref;
    const u32 *start, *end, *val;
    __device__ __forceinline__ u32 ref(u64 i) const { return (u32)rref[i]; }
    __device__ __forceinline__ u32 len(u64 i) const { return ln_width(start[i]) + ln_width(end[i]) + ValueText(val[i]).len() + 4u; }
    __device__ __forceinline__ void put(u64 i, u8 *q) const
    {
        const u32 s = start[i], e = end[i];
        const ValueText v(val[i]);
        *--q = '\n';
        q = v.put(q);
        *--q = '\t';
        q = cv_digits(q, e);
        *--q = '\t';
        q = cv_digits(q, s);
        *--q = '\t';
    }
};

struct TrSignal {       // the signal runs (k_tr_sections): the bits of a float32, and a slot of float32 min / max and float64 sums
    static __device__ __forceinline__ u32 item(u32 bits) { return bits; }
    static __device__ __forceinline__ void stats(const ZmBins &B, u64 b, u32 *p)
    {
        p[0] = B.mn[b];
        p[1] = B.mx[b];
        p[2] = __float_as_uint(__double2float_rn(__longlong_as_double((long long)B.sum[b])));
        p[3] = __float_as_uint(__double2float_rn(__longlong_as_double((long long)B.sq[b])));
    }
};
}  // namespace

// sums[2 * section], [2 * section + 1]: the section's runs in order, acc += f64(ov) * f64(v) and acc += f64(ov) * (f64(v) * f64(v))
__global__ void __launch_bounds__(256) k_sg_secsums(const u32 *rstart, const u32 *rend, const u32 *rval, u64 n, u32 ips, double *sums)
{
#pragma clang fp contract(off)
    const u64 sec = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 i0 = sec * ips;
    if (i0 >= n) return;
    const u64 i1 = i0 + ips < n ? i0 + ips : n;
    double sum = 0.0, sq = 0.0;
    for (u64 i = i0; i < i1; i++) {
        const double ov = (double)(rend[i] - rstart[i]), v = (double)__uint_as_float(rval[i]);
        const double a = ov * v, vv = v * v;
        const double q = ov * vv;
        sum = sum + a;
        sq = sq + q;
    }
    sums[2u * sec] = sum;
    sums[2u * sec + 1u] = sq;
}

// rng[2 * id], rng[2 * id + 1]: the runs of the reference with that id; off0, lens: by id
__global__ void __launch_bounds__(256) k_sg_zoom_fill(const u32 *__restrict__ rstart, const u32 *__restrict__ rend, const u32 *__restrict__ rval,
                                                      const u64 *__restrict__ rng, const u64 *__restrict__ off0, const u32 *__restrict__ lens,
                                                      u32 nc, u32 z, u64 nb, u8 *__restrict__ bins)
{
#pragma clang fp contract(off)
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    if (b >= nb) return;
    const ZmBins B(bins, nb);
    const u32 id = cv_zoom_id(off0, nc, b);
    const u64 lo = (b - off0[id]) * z, hi = lo + z < (u64)lens[id] ? lo + z : (u64)lens[id];
    u64 a = rng[2u * id], top = rng[2u * id + 1u], zz = top;
    while (a < zz) {                        // the first run that ends behind lo
        const u64 mid = a + (zz - a) / 2u;
        if ((u64)rend[mid] > lo) zz = mid;
        else a = mid + 1u;
    }
    u32 cnt = 0;
    float mn = 0.0f, mx = 0.0f;
    double sum = 0.0, sq = 0.0;
    for (u64 i = a; i < top && (u64)rstart[i] < hi; i++) {
        const u64 s = rstart[i], e = rend[i];
        const u32 w = (u32)((e < hi ? e : hi) - (s > lo ? s : lo));
        const float f = __uint_as_float(rval[i]);
        const double ov = (double)w, v = (double)f;
        const double p = ov * v, vv = v * v;
        const double q = ov * vv;
        sum = sum + p;
        sq = sq + q;
        mn = cnt == 0 || f < mn ? f : mn;
        mx = cnt == 0 || f > mx ? f : mx;
        cnt += w;
    }
    B.sum[b] = (u64)__double_as_longlong(sum);
    B.sq[b] = (u64)__double_as_longlong(sq);
    B.cnt[b] = cnt;
    B.mn[b] = __float_as_uint(mn);
    B.mx[b] = __float_as_uint(mx);
}

__global__ void __launch_bounds__(256) k_sg_zoom_fold(u8 *__restrict__ src, u64 nsrc, u8 *__restrict__ dst, u64 ndst,
                                                      const u64 *__restrict__ offs, const u64 *__restrict__ offd, u32 nc)
{
#pragma clang fp contract(off)
    const u64 b = (u64)blockIdx.x * 256u + threadIdx.x;
    if (b >= ndst) return;
    const ZmBins S(src, nsrc), D(dst, ndst);
    const u32 id = cv_zoom_id(offd, nc, b);
    const u64 j = b - offd[id], ns = offs[id + 1u] - offs[id];
    const u64 c0 = offs[id] + 4u * j, c1 = offs[id] + (4u * j + 4u < ns ? 4u * j + 4u : ns);     // (the last group may be short)
    double sum = 0.0, sq = 0.0;
    u32 cnt = 0;
    float mn = 0.0f, mx = 0.0f;
    for (u64 c = c0; c < c1; c++) {                 // in index order; an empty child adds 0.0
        sum = sum + __longlong_as_double((long long)S.sum[c]);
        sq = sq + __longlong_as_double((long long)S.sq[c]);
        if (S.cnt[c]) {
            const float lo = __uint_as_float(S.mn[c]), hi = __uint_as_float(S.mx[c]);
            mn = cnt == 0 || lo < mn ? lo : mn;
            mx = cnt == 0 || hi > mx ? hi : mx;
            cnt += S.cnt[c];
        }
    }
    D.sum[b] = (u64)__double_as_longlong(sum);
    D.sq[b] = (u64)__double_as_longlong(sq);
    D.cnt[b] = cnt;
    D.mn[b] = __float_as_uint(mn);
    D.mx[b] = __float_as_uint(mx);
}

namespace {

extern const CvKind SG_KIND;

// level 0 of the signal runs: the runs of every id from the signal's ranges, then one lane per bin
int sg_zoom_fill(pmx_dbam *b, const u32 *h_idof, const u32 *, const u64 *d_off, const u32 *d_lens, u32 z0, u64 nb0, u8 *bins, unsigned long long *)
{
    Coverage &c = b->cv;
    if (!bins || !nb0) return 0;
    if (int rc = coverage_ranges_make(b, SG_KIND)) return rc;
    const u64 nc = c.chosen.size();
    std::vector<u64> rng(2 * std::max<u64>(nc, 1), 0);
    for (u64 k = 0; k < nc; k++) {
        const u32 id = h_idof[(u64)c.chosen[k]];
        rng[2 * id] = c.sranges[k];
        rng[2 * id + 1] = c.sranges[k + 1];
    }
    DevAlloc d_rng;
    CvHold held(b);
    held.add(8 * rng.size());
    HIPOK(hipMalloc(&d_rng.p, 8 * rng.size()));
    HIPOK(hipMemcpyAsync(d_rng.p, rng.data(), 8 * rng.size(), hipMemcpyHostToDevice, b->stream));
    const CvRuns V(c.sruns.as<u8>(), c.snruns);
    hipLaunchKernelGGL(k_sg_zoom_fill, dim3((unsigned)((nb0 + 255) / 256)), dim3(256), 0, b->stream, V.start, V.end, V.depth, d_rng.as<u64>(), d_off, d_lens,
                       (u32)nc, z0, nb0, bins);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(b->stream));        // (rng and d_rng are locals)
    return 0;
}
const CvKind SG_KIND = {true, "pmx_dbam_coverage_signal_", coverage_lines<LnSignal>, k_tr_sections<TrSignal>, k_sg_secsums, sg_zoom_fill,
                        k_sg_zoom_fold, k_tr_zoom_emit<TrSignal>};

// the peaks called from the signal runs (call_device.inc) go with them
void call_drop(Coverage &c)
{
    c.bytes -= std::min<u64>(24 * c.npeaks, c.bytes);
    c.peaks = DevAlloc{};
    c.phave = false;
    c.npeaks = 0;
    for (u64 &x : c.ptot) x = 0;
}

// the arrays of the q-score table (qvalue_device.inc) in its one block: covered bases (8 bytes per row), p-score, q-score (4 each)
struct QvTable {
    u64 *W;
    u32 *u, *q;
    QvTable(u8 *p, u64 m) : W((u64 *)p), u((u32 *)(p + 8 * m)), q((u32 *)(p + 12 * m)) {}
};

// the q-scores of a p-score track go with its runs
void qvalue_drop(Coverage &c)
{
    c.bytes -= std::min<u64>(16 * c.qrows, c.bytes);
    c.qtab = DevAlloc{};
    c.qhave = false;
    c.qrows = 0;
    for (u64 &x : c.qtot) x = 0;
}

void signal_drop(Coverage &c)
{
    call_drop(c);
    qvalue_drop(c);
    if (c.zsg) zoom_drop(c);
    c.zsg = false;
    c.bytes -= std::min<u64>(16 * c.snruns, c.bytes);
    c.sruns = DevAlloc{};
    c.shave = false;
    c.spscore = false;
    c.snruns = 0;
    c.sbin = 0;
    c.sranges.clear();
    for (double &x : c.stot) x = 0;
}

// the signal slot for m runs, counted from here on: signal_drop takes them off again
int signal_alloc(pmx_dbam *b, const std::string &fn, u64 m)
{
    Coverage &c = b->cv;
    if (hipMalloc(&c.sruns.p, 16 * m) != hipSuccess) {
        (void)hipGetLastError();
        return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(m) + " runs");
    }
    c.snruns = m;
    c.bytes += 16 * m;
    if (b->st) stream_note(*b);
    return 0;
}

// the totals of the nout runs in the slot; tot: sg_totals' three words
void signal_have(Coverage &c, u32 bin, u64 nout, const unsigned long long *tot)
{
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
}

struct BtStage {        // what a kind's own stage between the fills and the marks is given (poisson's lambda)
    hipStream_t st;
    CvHold &held;
    SgGeo G;
    unsigned long long *tab;        // the kind's tables, TABLES * nb words
    u64 nb, nwg, L;                 // bins, workgroups of 256 bins, the sum of the chosen lengths
    u64 *kb;                        // nwg words, free until the marks
};

// The work of a track of kind K behind its checks, from the depth runs of b (and of the control, where the kind has one, whose
// stream has been waited for) to the runs in b's signal slot and their totals; a failure leaves no signal.  stage(T, BtStage) runs
// between the fills and the marks.
template <class K, class Stage> int bintrack_run(pmx_dbam *b, pmx_dbam *ctl, const std::string &fn, u32 bin, K T, Stage stage)
{
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    Coverage &c = b->cv;
    pmx_dbam *const src[2] = {b, ctl};
    const u32 ns = ctl ? 2u : 1u;
    unsigned long long tot[3] = {0, ~0ull, 0};
    u64 nout = 0;
    if (c.nruns || (ctl && ctl->cv.nruns)) {
        const u64 nc = c.chosen.size();
        std::vector<u64> boff(nc + 1, 0), bof[2];       // bof[h][r]: the first bin of reference r of src[h] (every run lies on a chosen one)
        std::vector<u32> lens(nc, 0);
        std::vector<int> cref(nc, 0);
        u64 L = 0, geo_bytes = 8 * boff.size() + 8 * std::max<u64>(nc, 1);
        for (u32 h = 0; h < ns; h++) {
            bof[h].assign(std::max<u64>(src[h]->ref_names.size(), 1), 0);
            geo_bytes += 8 * bof[h].size();
        }
        for (u64 k = 0; k < nc; k++) {
            lens[k] = (u32)std::max<int64_t>(b->ref_lens[(u64)c.chosen[k]], 0);
            cref[k] = c.chosen[k];
            for (u32 h = 0; h < ns; h++) bof[h][(u64)src[h]->cv.chosen[k]] = boff[k];
            boff[k + 1] = boff[k] + ((u64)lens[k] + bin - 1) / bin;
            L += lens[k];
        }
        const u64 nb = boff[nc], nwg = (nb + 255) / 256, tab_bytes = 8 * K::TABLES * nb;      // (nb >= 1: a run lies in a bin)
        if (nwg >= (1ull << 31)) return fail(PMX_DBAM_ERR_INVALID, fn + ": 2^39 bins or more");
        DevAlloc d_tot, d_geo, d_tab, d_k, d_kb, d_e;
        CvHold held(b);
        HIPOK(hipMalloc(&d_tot.p, 64));
        HIPOK(hipMemcpyAsync(d_tot.p, tot, 24, hipMemcpyHostToDevice, st));
        u64 *dt = d_tot.as<u64>();
        HIPOK(hipMalloc(&d_geo.p, geo_bytes));
        if (hipMalloc(&d_tab.p, tab_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for the bin table" + (K::TABLES > 1 ? "s" : "") + ": " + std::to_string(tab_bytes) +
                                               " bytes asked for (" + std::to_string(8 * K::TABLES) + " per bin of " + std::to_string(bin) + " bases)");
        }
        held.add(geo_bytes + tab_bytes + 12 * nwg);
        HIPOK(hipMalloc(&d_k.p, 4 * nwg));
        HIPOK(hipMalloc(&d_kb.p, 8 * nwg));
        u64 *d_boff = d_geo.as<u64>(), *d_bof[2] = {d_boff + boff.size(), d_boff + boff.size() + bof[0].size()};
        u32 *d_lens = (u32 *)(d_bof[ns - 1] + bof[ns - 1].size());
        int *d_cref = (int *)(d_lens + std::max<u64>(nc, 1));
        HIPOK(hipMemcpyAsync(d_boff, boff.data(), 8 * boff.size(), hipMemcpyHostToDevice, st));
        for (u32 h = 0; h < ns; h++) HIPOK(hipMemcpyAsync(d_bof[h], bof[h].data(), 8 * bof[h].size(), hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_lens, lens.data(), 4 * nc, hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_cref, cref.data(), 4 * nc, hipMemcpyHostToDevice, st));
        HIPOK(hipMemsetAsync(d_tab.p, 0, 8 * ns * nb, st));            // (the depth sums; a kind fills its further tables itself)
        const SgGeo G{d_boff, d_lens, d_cref, (u32)nc, bin};
        unsigned long long *tab = d_tab.as<unsigned long long>();
        for (u32 h = 0; h < ns; h++) {      // once per handle into its own table, for B = 1 as for any other bin (two run lists do not line up)
            const Coverage &s = src[h]->cv;
            if (!s.nruns) continue;
            const CvRuns V((u8 *)s.runs.p, s.nruns);
            hipLaunchKernelGGL(k_cv_bin_fill, dim3((unsigned)((s.nruns + 255) / 256)), dim3(256), 0, st, V.ref, V.start, V.end, V.depth, s.nruns, d_bof[h],
                               bin, tab + h * nb);
            HIPOK(hipGetLastError());
        }
        T.tables(tab, nb);
        if (int rc = stage(T, BtStage{st, held, G, tab, nb, nwg, L, d_kb.as<u64>()})) return rc;
        hipLaunchKernelGGL((k_bt_count<K, false>), dim3((unsigned)nwg), dim3(256), 0, st, T, nb, G, d_k.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), nwg, d_kb.as<u64>(), dt + 4);
        HIPOK(hipGetLastError());
        u64 ne = 0;
        HIPOK(hipMemcpyAsync(&ne, dt + 4, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));       // (the geometry is of locals, and a stage's host arrays have been read)
        if (hipMalloc(&d_e.p, K::ENTRY * ne) != hipSuccess) {        // (ne >= 1: the first bin begins an entry)
            (void)hipGetLastError();
            return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(ne) + " bin boundaries");
        }
        held.add(K::ENTRY * ne);
        T.entries(d_e.as<u8>(), ne);
        hipLaunchKernelGGL(k_bt_entries<K>, dim3((unsigned)nwg), dim3(256), 0, st, T, nb, G, d_kb.as<u64>());
        HIPOK(hipGetLastError());
        const u64 ewg = (ne + 255) / 256;          // (ewg <= nwg: d_k and d_kb are used again)
        hipLaunchKernelGGL((k_bt_count<K, true>), dim3((unsigned)ewg), dim3(256), 0, st, T, ne, G, d_k.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_k.as<u32>(), d_k.as<u32>(), ewg, d_kb.as<u64>(), dt + 6);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&nout, dt + 6, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (nout) {
            if (int rc = signal_alloc(b, fn, nout)) return rc;
            const CvRuns O(c.sruns.as<u8>(), nout);
            hipLaunchKernelGGL(k_bt_close<K>, dim3((unsigned)ewg), dim3(256), 0, st, T, ne, d_kb.as<u64>(), G, O.ref, O.start, O.end, O.depth,
                               d_tot.as<unsigned long long>());
            HIPOK(hipGetLastError());
        }
        HIPOK(hipMemcpyAsync(tot, d_tot.p, 24, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));            // (the tables, the entries and the scans are freed behind it)
    }
    signal_have(c, bin, nout, tot);
    return 0;
}

const auto bt_no_stage = [](auto &, const BtStage &) { return 0; };

// the work of signal behind its checks; a failure leaves no signal
int coverage_signal_run(pmx_dbam *b, const std::string &fn, u32 bin, double scale)
{
    Coverage &c = b->cv;
    const u64 n = c.nruns;
    if (bin > 1 || !n) return bintrack_run(b, nullptr, fn, bin, SgTrack{scale}, bt_no_stage);
    HIPOK(hipSetDevice(b->device));         // B = 1: the signal runs are the depth runs
    hipStream_t st = b->stream;
    unsigned long long tot[3] = {0, ~0ull, 0};
    const CvRuns V(c.runs.as<u8>(), n);
    DevAlloc d_tot;
    HIPOK(hipMalloc(&d_tot.p, 64));
    HIPOK(hipMemcpyAsync(d_tot.p, tot, 24, hipMemcpyHostToDevice, st));
    if (int rc = signal_alloc(b, fn, n)) return rc;
    const CvRuns O(c.sruns.as<u8>(), n);
    hipLaunchKernelGGL(k_sg_convert, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, V.ref, V.start, V.end, V.depth, n, scale, O.ref, O.start, O.end,
                       O.depth, d_tot.as<unsigned long long>());
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(tot, d_tot.p, 24, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    signal_have(c, bin, n, tot);
    return 0;
}

// The checks every track call begins with, in the order the calls have always made them; two: the kind has a control (ctl).
int track_checks(pmx_dbam *b, pmx_dbam *ctl, bool two, const std::string &fn, uint32_t bin, double *totals)
{
    if (!b || (two && !ctl)) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals) return fail(PMX_DBAM_ERR_INVALID, fn + ": null output");
    for (int k = 0; k < 4; k++) totals[k] = 0;
    const Coverage &c = b->cv;
    if (c.state != CV_RUNS) return fail(PMX_DBAM_ERR_INVALID, fn + ": no runs: call pmx_dbam_coverage_finish first");
    if (two) {          // the same device, the same chosen references in name, length and order
        const Coverage &cc = ctl->cv;
        if (cc.state != CV_RUNS) return fail(PMX_DBAM_ERR_INVALID, fn + ": the control has no runs: call pmx_dbam_coverage_finish on it first");
        if (b->device != ctl->device) return fail(PMX_DBAM_ERR_INVALID, fn + ": the control is on another device");
        bool same = c.chosen.size() == cc.chosen.size();
        for (u64 k = 0; same && k < c.chosen.size(); k++) {
            const u64 x = (u64)c.chosen[k], y = (u64)cc.chosen[k];
            same = b->ref_names[x] == ctl->ref_names[y] && std::max<int64_t>(b->ref_lens[x], 0) == std::max<int64_t>(ctl->ref_lens[y], 0);
        }
        if (!same) return fail(PMX_DBAM_ERR_INVALID, fn + ": the chosen references of the control differ in name, length or order");
    }
    if (bin < 1 || bin > SG_MAX_BIN) return fail(PMX_DBAM_ERR_INVALID, fn + ": a bin of 1 to 65536 bases");
    return 0;
}

// run() behind the checks: both streams waited for, the signal before dropped, and none left by a failure; then the totals
template <class Run> int track_make(pmx_dbam *b, pmx_dbam *ctl, double *totals, Run run)
{
    Coverage &c = b->cv;
    HIPOK(hipSetDevice(b->device));
    if (ctl && ctl != b) HIPOK(hipStreamSynchronize(ctl->stream));
    HIPOK(hipStreamSynchronize(b->stream));
    signal_drop(c);
    struct Drop {
        Coverage &c;
        bool ok = false;
        ~Drop()
        {
            if (!ok) signal_drop(c);
        }
    } drop{c};
    if (int rc = run()) return rc;
    drop.ok = true;
    for (int k = 0; k < 4; k++) totals[k] = c.stot[k];
    return 0;
}

int coverage_signal_impl(pmx_dbam *b, uint32_t bin, double scale, double *totals)
{
    const std::string fn = "pmx_dbam_coverage_signal";
    if (int rc = track_checks(b, nullptr, false, fn, bin, totals)) return rc;
    if (!std::isfinite(scale) || scale < 0x1p-64)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": the scale is a finite number of at least 2^-64 (below it a value could be a float32 denormal)");
    if (scale * (double)b->cv.tot[4] >= 0x1p40)
        return fail(PMX_DBAM_ERR_INVALID, fn + ": scale * max_depth is 2^40 or more (a value's text is made in 64-bit integers)");
    return track_make(b, nullptr, totals, [&] { return coverage_signal_run(b, fn, bin, scale); });
}

}  // namespace

extern "C" {

int pmx_dbam_coverage_signal(pmx_dbam *b, uint32_t bin, double scale, double totals[4])
{
    return guarded("pmx_dbam_coverage_signal", [&] { return coverage_signal_impl(b, bin, scale, totals); });
}

int pmx_dbam_coverage_signal_runs(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, float *value)
{
    return guarded("pmx_dbam_coverage_signal_runs", [&] { return coverage_runs_impl(b, SG_KIND, first, n, ref, start, end, (uint32_t *)value); });
}

int64_t pmx_dbam_coverage_signal_text(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap)
{
    return guarded("pmx_dbam_coverage_signal_text", [&] { return coverage_text_impl(b, SG_KIND, first, n, buf, cap); });
}

int64_t pmx_dbam_coverage_signal_ranges(pmx_dbam *b, int64_t *first, int64_t cap)
{
    return guarded("pmx_dbam_coverage_signal_ranges", [&] { return coverage_ranges_impl(b, SG_KIND, first, cap); });
}

int64_t pmx_dbam_coverage_signal_sections(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                          uint32_t *table, int64_t table_cap, double *sums)
{
    return guarded("pmx_dbam_coverage_signal_sections", [&] {
        return coverage_sections_impl(b, SG_KIND, first, n, chrom_id, items, buf, cap, table, table_cap, false, nullptr, sums);
    });
}

int pmx_dbam_coverage_signal_zoom_begin(pmx_dbam *b, uint32_t z0, uint32_t levels, const uint32_t *chrom_id, uint64_t out[2])
{
    return guarded("pmx_dbam_coverage_signal_zoom_begin", [&] { return coverage_zoom_begin_impl(b, SG_KIND, z0, levels, chrom_id, out); });
}

int64_t pmx_dbam_coverage_signal_zoom_records(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                              int64_t table_cap)
{
    return guarded("pmx_dbam_coverage_signal_zoom_records",
                   [&] { return coverage_zoom_records_impl(b, SG_KIND, level, items, buf, cap, table, table_cap); });
}

int64_t pmx_dbam_coverage_signal_sections_z(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                            uint32_t *table, int64_t table_cap, uint32_t *zsizes, double *sums)
{
    return guarded("pmx_dbam_coverage_signal_sections_z", [&] {
        return coverage_sections_impl(b, SG_KIND, first, n, chrom_id, items, buf, cap, table, table_cap, true, zsizes, sums);
    });
}

int64_t pmx_dbam_coverage_signal_zoom_records_z(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                                int64_t table_cap, uint32_t *zsizes)
{
    return guarded("pmx_dbam_coverage_signal_zoom_records_z",
                   [&] { return coverage_zoom_records_impl(b, SG_KIND, level, items, buf, cap, table, table_cap, true, zsizes); });
}

}  // extern "C"
