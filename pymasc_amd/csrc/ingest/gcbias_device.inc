// GC bias on the device (pmx_dgc_*, pmx_dbam_gcbias_*, include/pymasc_amd_ingest.h; DESIGN.md 7.19).  Included at the end of
// bam_device.hip behind kmer_track_device.inc (km_parse: the packed genome), complexity_device.inc (cx_filter: the kept records
// of a call, with arrays of its own) and region_mask_device.inc (the merged mask intervals of the handle).
//
// The table's own coordinates: the chosen references lie end to end in header order, each followed by one separator position;
// base p (0-based) of the k-th chosen reference is at T[k] + p, T[k + 1] = T[k] + len[k] + 1.  Two bit vectors of 64-bit words
// over these positions, GC (the base is C or G) and BLOCKED (the base is not A C G T, or lies inside a merged mask interval, or
// the position is a separator or behind the last one).  A window of W positions is unblocked when its W blocked bits are 0, so
// no window test knows about record ends.  Both vectors hold GC_PAD words more than the positions need, GC 0 and BLOCKED all
// ones, and every load of the kernels stays below that.
//
//   k_gc_bits      one lane per word of 64 table positions: the reference(s) it covers (binary search over T), 64 GC and valid
//                  bits from the packed genome (an unaligned extract over three words), the mask intervals that reach into it
//   k_gc_windows   one lane per 64 consecutive window starts: g and the blocked count of the first window by popcounts over its
//                  words, then 63 slides by the bit that enters and the bit that leaves, all in registers; the lane carries
//                  (g, count) and adds to the histogram in LDS only when g changes; one 64-bit global atomic per non-zero entry
//   k_gc_reads     one lane per kept read: the placement, the bounds test, the two popcounts of its one window, then the lanes of
//                  a wave that hold the same g add once (a loop over the distinct values); off_end / blocked / placed by ballot,
//                  one atomic per workgroup each
// Device memory: 16 bytes per 64 chosen positions (0.25 bytes per base) + 16 bytes per reference + 8 (W + 4) with the handle from
// begin to the next begin or close; 13 bytes per kept read inside a call of add.

#define GC_PAD 24u                            // words behind the positions: a window of 1024 from the last start reads 17 of them
#define GC_WINDOW_MAX 1024u
#define GC_GRID 8192u                         // workgroups of k_gc_windows at the most

struct pmx_dgc {
    int device = 0;
    hipStream_t stream = nullptr;
    TtDev g;                                  // the packed genome (freed with the handle)
    KmGenome G;
    std::vector<std::string> names;
    std::vector<int64_t> sizes;
};

// 32 GC bits of one packed word: a base is C or G when the two bits of its code differ (A C G T = 0 1 2 3)
__device__ __forceinline__ u32 gc_word_bits(u64 x)
{
    x = (x ^ (x >> 1)) & 0x5555555555555555ull;
    x = (x | (x >> 1)) & 0x3333333333333333ull;
    x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
    x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
    x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
    x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
    return (u32)x;
}

// the 64 bits from bit s (< 32) of the 96 bits a | b << 32 | c << 64
__device__ __forceinline__ u64 gc_take64(u32 a, u32 b, u32 c, u32 s)
{
    const u64 lo = (u64)a | ((u64)b << 32);
    return s ? (lo >> s) | ((u64)c << (64u - s)) : lo;
}

// ones at the bits [lo, hi) of a word, lo < hi <= 64
__device__ __forceinline__ u64 gc_bit_run(u32 lo, u32 hi)
{
    const u64 m = hi - lo >= 64u ? ~0ull : ((1ull << (hi - lo)) - 1ull);
    return m << lo;
}

// the set bits of B over the positions [t, t + n)
__device__ __forceinline__ u32 gc_range_pop(const u64 *__restrict__ B, u64 t, u32 n)
{
    u32 c = 0;
    const u64 e = t + n;
    while (t < e) {
        const u32 s = (u32)(t & 63u), k = (u32)(e - t < (u64)(64u - s) ? e - t : (u64)(64u - s));
        c += (u32)__popcll(B[t >> 6] & gc_bit_run(s, s + k));
        t += k;
    }
    return c;
}

// T[0 .. nc]: first position of every chosen reference (T[nc] = npos); src: its first position in the genome; rid: its id in
// the alignment header; its length is T[k + 1] - T[k] - 1.  xkey / xend: the handle's merged mask intervals.
__global__ void __launch_bounds__(256) k_gc_bits(const u64 *__restrict__ P, const u32 *__restrict__ V, const u64 *__restrict__ T,
                                                 const u64 *__restrict__ src, const u32 *__restrict__ rid, u32 nc, u64 nwords,
                                                 const u64 *__restrict__ xkey, const u32 *__restrict__ xend, u64 xn,
                                                 u64 *__restrict__ GC, u64 *__restrict__ BL)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= nwords + GC_PAD) return;
    u64 gcw = 0, blw = ~0ull;
    const u64 t0 = 64ull * i, npos = T[nc];
    if (t0 < npos) {
        u32 lo = 0, hi = nc;                     // the last chosen reference with T[k] <= t0
        while (hi - lo > 1u) {
            const u32 mid = (lo + hi) >> 1;
            if (T[mid] <= t0) lo = mid;
            else hi = mid;
        }
        u32 k = lo;
        u64 t = t0;
        while (t < t0 + 64u && k < nc) {
            const u64 rel = t - T[k], len = T[k + 1] - T[k] - 1u;
            if (rel >= len) {                    // the separator: it stays blocked
                t++;
                k++;
                continue;
            }
            const u32 n = (u32)(t0 + 64u - t < len - rel ? t0 + 64u - t : len - rel), sh = (u32)(t - t0);
            const u64 q = src[k] + rel, w = q >> 5;
            const u32 s = (u32)(q & 31u);
            const u64 take = gc_bit_run(0, n);
            const u64 valid = gc_take64(V[w], V[w + 1], V[w + 2], s) & take;
            const u64 gc = gc_take64(gc_word_bits(P[w]), gc_word_bits(P[w + 1]), gc_word_bits(P[w + 2]), s) & valid;
            u64 x = 0;                           // the positions of [rel, rel + n) inside a mask interval
            if (xn) {
                const u64 r64 = (u64)rid[k], key0 = (r64 << 32) | rel;
                u64 a = 0, b = xn;               // the number of keys <= key0
                while (a < b) {
                    const u64 mid = (a + b) >> 1;
                    if (xkey[mid] <= key0) a = mid + 1u;
                    else b = mid;
                }
                for (u64 j = a ? a - 1u : 0ull; j < xn; j++) {
                    const u64 kx = xkey[j];
                    if ((kx >> 32) < r64) continue;
                    if ((kx >> 32) > r64) break;
                    const u64 xb = (u32)kx, xe = xend[j];
                    if (xb >= rel + n) break;
                    if (xe > rel) {
                        const u64 b0 = xb > rel ? xb - rel : 0ull, e0 = (xe < rel + n ? xe : rel + n) - rel;
                        if (e0 > b0) x |= gc_bit_run((u32)b0, (u32)e0);
                    }
                }
            }
            gcw |= gc << sh;
            blw &= ~((valid & ~x) << sh);
            t += n;
        }
    }
    GC[i] = gcw;
    BL[i] = blw;
}

// hist[g] += the unblocked windows of W positions with g GC bases, over every start in [0, 64 nwords)
__global__ void __launch_bounds__(256) k_gc_windows(const u64 *__restrict__ GC, const u64 *__restrict__ BL, u64 nwords, u32 W,
                                                    unsigned long long *__restrict__ hist)
{
    __shared__ u32 s_h[GC_WINDOW_MAX + 1u];
    const u32 t = threadIdx.x;
    for (u32 k = t; k <= W; k += 256u) s_h[k] = 0;
    __syncthreads();
    const u32 wq = W >> 6, wr = W & 63u;
    for (u64 i = (u64)blockIdx.x * 256u + t; i < nwords; i += (u64)gridDim.x * 256u) {
        // the first window [64 i, 64 i + W): whole words, then the bits below wr of the next one
        u32 g = 0, bl = 0;
        for (u32 k = 0; k < wq; k++) {
            g += (u32)__popcll(GC[i + k]);
            bl += (u32)__popcll(BL[i + k]);
        }
        const u64 g0 = GC[i + wq], b0 = BL[i + wq];
        u64 gin = g0, bin = b0;                  // bit j: the position 64 i + W + j, which enters at slide j
        if (wr) {
            const u64 low = gc_bit_run(0, wr);
            g += (u32)__popcll(g0 & low);
            bl += (u32)__popcll(b0 & low);
            gin = (g0 >> wr) | (GC[i + wq + 1u] << (64u - wr));
            bin = (b0 >> wr) | (BL[i + wq + 1u] << (64u - wr));
        }
        const u64 gout = GC[i], bout = BL[i];    // bit j: the position 64 i + j, which leaves at slide j
        u32 cur = 0, cnt = 0;
        for (u32 j = 0; j < 64u; j++) {
            if (bl == 0) {
                if (cnt && g != cur) {
                    atomicAdd(&s_h[cur], cnt);
                    cnt = 0;
                }
                cur = g;
                cnt++;
            }
            g += (u32)((gin >> j) & 1ull) - (u32)((gout >> j) & 1ull);
            bl += (u32)((bin >> j) & 1ull) - (u32)((bout >> j) & 1ull);
        }
        if (cnt) atomicAdd(&s_h[cur], cnt);
    }
    __syncthreads();
    for (u32 k = t; k <= W; k += 256u)
        if (s_h[k]) atomicAdd(&hist[k], (unsigned long long)s_h[k]);
}

// tab[2 * r] = T of reference r (-1: the reference is not chosen), tab[2 * r + 1] = its length.  F[g] += 1 per placed read;
// cnt[0 .. 2] += placed, off_end, blocked.
__global__ void __launch_bounds__(256) k_gc_reads(const int *__restrict__ ref, const int *__restrict__ pos, const int *__restrict__ len,
                                                  const u8 *__restrict__ rev, u64 n, const long long *__restrict__ tab, u32 nref, u32 W,
                                                  const u64 *__restrict__ GC, const u64 *__restrict__ BL,
                                                  unsigned long long *__restrict__ F, unsigned long long *__restrict__ cnt)
{
    __shared__ u32 s_c[3][4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 i = (u64)blockIdx.x * 256u + t;
    bool chosen = false, inside = false;
    u32 g = 0, bl = 0;
    if (i < n && ref[i] >= 0 && (u32)ref[i] < nref) {
        const long long first = tab[2u * (u32)ref[i]], rl = tab[2u * (u32)ref[i] + 1u];
        const long long s = rev[i] ? (long long)pos[i] + (long long)len[i] - (long long)W : (long long)pos[i];
        chosen = first >= 0;
        inside = chosen && s >= 1 && s + (long long)W - 1 <= rl;
        if (inside) {
            const u64 at = (u64)first + (u64)(s - 1);
            bl = gc_range_pop(BL, at, W);
            g = gc_range_pop(GC, at, W);
        }
    }
    const bool placed = inside && bl == 0, blocked = inside && bl != 0, off = chosen && !inside;
    u64 left = __ballot(placed);                 // the lanes of the wave with the same g add once
    while (left) {
        const u32 leader = (u32)(__ffsll((long long)left) - 1);
        const u32 gl = (u32)__shfl((int)g, (int)leader, 64);
        const u64 same = __ballot(placed && g == gl) & left;
        if (lane == leader) atomicAdd(&F[gl], (unsigned long long)__popcll(same));
        left &= ~same;
    }
    const u64 mp = __ballot(placed), mo = __ballot(off), mb = __ballot(blocked);
    if (lane == 0) {
        s_c[0][wave] = (u32)__popcll(mp);
        s_c[1][wave] = (u32)__popcll(mo);
        s_c[2][wave] = (u32)__popcll(mb);
    }
    __syncthreads();
    if (t < 3u) {
        const u32 c = s_c[t][0] + s_c[t][1] + s_c[t][2] + s_c[t][3];
        if (c) atomicAdd(&cnt[t], (unsigned long long)c);
    }
}

namespace {

int dgc_open_impl(const char *path, int device, int nthreads, pmx_dgc **out)
{
    if (!path || !out) return fail(PMX_DBAM_ERR_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMX_DBAM_ERR_DEVICE, "no HIP device: the device ingest needs a GPU");
    if (device < 0 || device >= ndev) return fail(PMX_DBAM_ERR_INVALID, "no such device");
    HIPOK(hipSetDevice(device));
    if (nthreads <= 0) nthreads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    pmx_dgc *g = new pmx_dgc;
    g->device = device;
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) {
        delete g;
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    u8 *d_text = nullptr;
    u64 N = 0;
    int rc = tt_upload(path, device, nthreads, &d_text, &N);
    if (!rc) rc = km_parse(g->stream, g->names, g->sizes, d_text, N, g->g, g->G);
    (void)hipStreamSynchronize(g->stream);
    if (d_text) (void)hipFree(d_text);           // (the genome is packed: the text is not needed any more)
    if (rc) {
        const std::string keep = g_err;
        pmx_dgc_close(g);
        g_err = keep.compare(0, strlen(path), path) == 0 ? keep : std::string(path) + ": " + keep;
        return rc;
    }
    *out = g;
    return 0;
}

int gcbias_begin_impl(pmx_dbam *b, const pmx_dgc *genome, u32 window, const uint8_t *use_ref)
{
    const std::string who = "pmx_dbam_gcbias_begin: ";
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    b->gc = GcBias{};
    if (!genome) return fail(PMX_DBAM_ERR_INVALID, who + "null genome");
    if (window == 0 || window > GC_WINDOW_MAX)
        return fail(PMX_DBAM_ERR_INVALID, who + "the window is " + std::to_string(window) + ": it must lie in [1, " +
                                              std::to_string(GC_WINDOW_MAX) + "]");
    if (genome->device != b->device)
        return fail(PMX_DBAM_ERR_INVALID, who + "the genome is on device " + std::to_string(genome->device) + ", the reads on device " +
                                              std::to_string(b->device));
    // the chosen references against the records: the same name and the same length
    std::unordered_map<std::string, u32> record;
    for (u32 h = 0; h < genome->names.size(); h++) record.emplace(genome->names[h], h);
    const u64 nref = b->ref_names.size();
    std::vector<long long> tab(2 * std::max<u64>(nref, 1), -1);
    std::vector<u64> T, src;
    std::vector<u32> rid;
    u64 npos = 0;
    for (u64 r = 0; r < nref; r++) {
        tab[2 * r + 1] = (long long)b->ref_lens[r];
        if (use_ref && !use_ref[r]) continue;
        const auto it = record.find(b->ref_names[r]);
        if (it == record.end()) return fail(PMX_DBAM_ERR_INVALID, who + "reference '" + b->ref_names[r] + "' has no record in the genome");
        if (genome->sizes[it->second] != b->ref_lens[r])
            return fail(PMX_DBAM_ERR_INVALID, who + "reference '" + b->ref_names[r] + "' is " + std::to_string(b->ref_lens[r]) +
                                                  " long in the alignment header and " + std::to_string(genome->sizes[it->second]) +
                                                  " in the genome");
        tab[2 * r] = (long long)npos;
        T.push_back(npos);
        src.push_back((u64)genome->G.sep[it->second] + 1u);
        rid.push_back((u32)r);
        npos += (u64)b->ref_lens[r] + 1u;
    }
    if (T.empty()) return fail(PMX_DBAM_ERR_INVALID, who + "no chosen reference");
    T.push_back(npos);
    const u32 nc = (u32)rid.size();
    const u64 nwords = (npos + 63) / 64, alloc = 8 * (nwords + GC_PAD), nf = (u64)window + 1u + 3u;
    hipStream_t st = b->stream;
    DevAlloc d_T, d_src, d_rid;
    if (int rc = rm_to_device(st, T.data(), (u64)nc + 1, d_T)) return rc;
    if (int rc = rm_to_device(st, src.data(), (u64)nc, d_src)) return rc;
    if (int rc = rm_to_device(st, rid.data(), (u64)nc, d_rid)) return rc;
    GcBias &c = b->gc;
    auto get = [&](DevAlloc &d, u64 bytes) -> int {
        if (hipMalloc(&d.p, bytes) == hipSuccess) return 0;
        c = GcBias{};
        return fail(PMX_DBAM_ERR_OPEN, who + "out of device memory for the bit vectors (" + std::to_string(2 * alloc) + " bytes)");
    };
    if (int rc = get(c.gc, alloc)) return rc;
    if (int rc = get(c.bl, alloc)) return rc;
    if (int rc = get(c.tab, 8 * tab.size())) return rc;
    if (int rc = get(c.f, 8 * nf)) return rc;
    DevAlloc d_hist;
    HIPOK(hipMalloc(&d_hist.p, 8 * ((u64)window + 1u)));
    HIPOK(hipMemsetAsync(d_hist.p, 0, 8 * ((u64)window + 1u), st));
    HIPOK(hipMemsetAsync(c.f.p, 0, 8 * nf, st));
    HIPOK(hipMemcpyAsync(c.tab.p, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_gc_bits, dim3(km_grid(nwords + GC_PAD)), dim3(256), 0, st, genome->G.P, genome->G.V, d_T.as<u64>(), d_src.as<u64>(),
                       d_rid.as<u32>(), nc, nwords, b->d_xkey, b->d_xend, b->x_n, c.gc.as<u64>(), c.bl.as<u64>());
    HIPOK(hipGetLastError());
    const u64 nwg = std::min<u64>((nwords + 255) / 256, GC_GRID);
    hipLaunchKernelGGL(k_gc_windows, dim3((unsigned)nwg), dim3(256), 0, st, c.gc.as<u64>(), c.bl.as<u64>(), nwords, window,
                       d_hist.as<unsigned long long>());
    HIPOK(hipGetLastError());
    c.n.assign((u64)window + 1u, 0);
    HIPOK(hipMemcpyAsync(c.n.data(), d_hist.p, 8 * ((u64)window + 1u), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));             // (the genome is not read after this; the tables above are locals)
    c.w = window;
    c.words = nwords + GC_PAD;
    if (b->st) stream_note(*b);
    return 0;
}

int gcbias_add_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, uint64_t *out)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!out) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_gcbias_add: null output");
    out[0] = out[1] = out[2] = 0;
    if (!b->gc.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_gcbias_add: no table: call pmx_dbam_gcbias_begin first");
    GcBias &c = b->gc;
    unsigned long long cnt[3] = {0, 0, 0};
    const int rc = side_add(b, mapq_min, flag_exclude, 3, cnt, [&](const CxRecs &R, hipStream_t st, unsigned long long *d_cnt) {
        hipLaunchKernelGGL(k_gc_reads, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(),
                           R.rev.as<u8>(), R.n, c.tab.as<long long>(), (u32)b->ref_names.size(), c.w, c.gc.as<u64>(), c.bl.as<u64>(),
                           c.f.as<unsigned long long>(), d_cnt);
    });
    if (rc) return rc;
    for (int k = 0; k < 3; k++) {
        out[k] = cnt[k];
        c.tot[k] += cnt[k];
    }
    return 0;
}

int64_t gcbias_tables_impl(pmx_dbam *b, uint64_t *windows, uint64_t *reads, int64_t cap, uint64_t *totals)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (!totals || (cap > 0 && (!windows || !reads))) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_gcbias_tables: null output");
    if (!b->gc.on()) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_gcbias_tables: no table: call pmx_dbam_gcbias_begin first");
    const u64 n = (u64)b->gc.w + 1u;
    totals[0] = 0;
    for (u64 v : b->gc.n) totals[0] += v;
    totals[1] = b->gc.tot[0];
    totals[2] = b->gc.tot[1];
    totals[3] = b->gc.tot[2];
    if (cap >= (int64_t)n) {
        HIPOK(hipSetDevice(b->device));
        HIPOK(hipMemcpyAsync(reads, b->gc.f.p, 8 * n, hipMemcpyDeviceToHost, b->stream));
        HIPOK(hipStreamSynchronize(b->stream));
        for (u64 k = 0; k < n; k++) windows[k] = b->gc.n[k];
    }
    return (int64_t)n;
}

}  // namespace

extern "C" {

int pmx_dgc_open(const char *path, int device, int nthreads, pmx_dgc **out)
{
    return guarded("pmx_dgc_open", [&] { return dgc_open_impl(path, device, nthreads, out); });
}

void pmx_dgc_close(pmx_dgc *g)
{
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->stream) {
        (void)hipStreamSynchronize(g->stream);
        (void)hipStreamDestroy(g->stream);
    }
    delete g;
}

int32_t pmx_dgc_nrec(const pmx_dgc *g) { return g ? (int32_t)g->names.size() : 0; }
const char *pmx_dgc_rec_name(const pmx_dgc *g, int32_t i) { return g && i >= 0 && (size_t)i < g->names.size() ? g->names[i].c_str() : nullptr; }
int64_t pmx_dgc_rec_len(const pmx_dgc *g, int32_t i) { return g && i >= 0 && (size_t)i < g->sizes.size() ? g->sizes[i] : -1; }

int pmx_dbam_gcbias_begin(pmx_dbam *b, const pmx_dgc *genome, uint32_t window, const uint8_t *use_ref)
{
    return guarded("pmx_dbam_gcbias_begin", [&] { return gcbias_begin_impl(b, genome, window, use_ref); });
}

int pmx_dbam_gcbias_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t out[3])
{
    return guarded("pmx_dbam_gcbias_add", [&] { return gcbias_add_impl(b, mapq_min, flag_exclude, out); });
}

int64_t pmx_dbam_gcbias_tables(pmx_dbam *b, uint64_t *windows, uint64_t *reads, int64_t cap, uint64_t totals[4])
{
    return guarded("pmx_dbam_gcbias_tables", [&] { return gcbias_tables_impl(b, windows, reads, cap, totals); });
}

}  // extern "C"
