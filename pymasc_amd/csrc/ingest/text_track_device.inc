// Text tracks on the device (pmx_dtt_open, include/pymasc_amd_ingest.h; DESIGN.md 7.10).  Included by bam_device.hip behind
// sam_device.inc: the handle is a pmx_dbw whose intervals come from text instead of BigWig blocks, so pmx_dbw_fetch /
// device_arrays / sorted / copy / close work on it unchanged but for one branch (dbw_fetch_impl -> tt_decode_all).
//
//   host          plain text: the staging buffers into HBM as it is; BGZF: the BAM open's member scan, k_bgzf_inflate and
//                 k_bgzf_crc; other gzip: zlib on the host (one DEFLATE stream cannot be split), then one copy.  The kind of track
//                 (io/text_track_parse.h: detect_kind) from the text's first lines.
//   k_sam_count / k_bam_scan / k_sam_lines   the line index, as for SAM text (the end of every line)
//   k_tt_parse    one lane per line: classify, split, parse the numbers (values by Clinger's fast path; a value outside it and
//                 every track line go to a short list the host finishes with strtod); the first error by line (atomicMin)
//   WIG           k_bam_scan of the per-workgroup declaration and data-line counts; k_tt_decls records every declaration, and
//                 k_tt_wig gives each data line its declaration (the last one before it) and its rank in the block
//   k_tt_list     the data lines in file order; k_tt_heads: where the chromosome name changes from the previous data line (names
//                 compared by hash, length and bytes) -- only these heads are named and merged into chromosomes on the host
//   k_tt_scatter  a stable counting pass: the lines of every chromosome together, in file order, and each chromosome's extent
//   per threshold k_tt_keep + k_bam_scan + k_tt_compact into the handle's arrays, k_tt_ranges: each chromosome's range in them
// Every load of the text lies below its end rounded up to 16 bytes; the buffer holds 64 more bytes.

#include "../io/text_track_parse.h"

#include <deque>
#include <unordered_map>

struct TtTab {          // one entry per line
    u32 *tag;           // type | min(fields, 255) << 8
    u32 *b, *e;         // data: begin / end (WIG "pos value": pos until k_tt_wig); declaration: start / step
    float *v;           // data: the value; declaration: the span (as bits)
    u64 *nm;            // the chromosome name: offset << 8 | length
    u32 *h;             // ... and its hash
};

struct TtSlow {         // a line the host finishes: a value outside the fast path, or a track line (len == ~0u)
    u64 off;
    u32 line, len;
};

// exclusive rank of this lane's `pred` among the workgroup's 256 lanes (every lane of the workgroup calls it)
__device__ __forceinline__ u32 tt_block_rank(bool pred, u32 *s_wave)
{
    const u32 lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const u64 m = __ballot(pred);
    if (lane == 0) s_wave[wave] = (u32)__popcll(m);
    __syncthreads();
    u32 r = (u32)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; w++) r += s_wave[w];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(256) k_tt_parse(const u8 *__restrict__ D, const u64 *__restrict__ nl, u64 n, u32 kind, TtTab T,
                                                  u32 *__restrict__ cdata, u32 *__restrict__ cdecl, unsigned long long *__restrict__ first_err,
                                                  unsigned long long *__restrict__ first_data, TtSlow *__restrict__ slow, u32 *__restrict__ nslow,
                                                  u32 slow_cap)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 type = ttrack::L_SKIP;
    if (i < n) {
        DevSrc s{D, ~0ull, make_uint4(0, 0, 0, 0)};
        ttrack::Line L;
        const u32 err = ttrack::parse_line(s, i ? nl[i - 1] + 1u : 0ull, nl[i], kind, L);
        type = L.type;
        if (err) atomicMin(first_err, (unsigned long long)((i << 8) | err));
        const bool decl = type == ttrack::L_VAR || type == ttrack::L_FIXED;
        T.tag[i] = type | ((L.nfields < 255u ? L.nfields : 255u) << 8);
        T.b[i] = L.b;
        T.e[i] = L.e;
        T.v[i] = decl ? __uint_as_float(L.span) : L.v;
        T.nm[i] = (L.name << 8) | L.nlen;
        T.h[i] = L.hash;
        if (!err && (L.slow || type == ttrack::L_TRACK)) {
            const u32 j = atomicAdd(nslow, 1u);
            if (j < slow_cap) {
                TtSlow x;
                x.off = L.voff;
                x.line = (u32)i;
                x.len = type == ttrack::L_TRACK ? ~0u : L.vlen;
                slow[j] = x;
            }
        }
    }
    const bool data = type == ttrack::L_DATA, decl = type == ttrack::L_VAR || type == ttrack::L_FIXED;
    const u64 m = __ballot(data || decl);
    if ((threadIdx.x & 63u) == 0 && m) atomicMin(first_data, (unsigned long long)(i + (u64)(__ffsll((long long)m) - 1)));
    const int nd = __syncthreads_count(data), nc = __syncthreads_count(decl);
    if (threadIdx.x == 0) {
        cdata[blockIdx.x] = (u32)nd;
        cdecl[blockIdx.x] = (u32)nc;
    }
}

__device__ __forceinline__ u32 tt_type(const TtTab &T, u64 i, u64 n) { return i < n ? (T.tag[i] & 255u) : ttrack::L_SKIP; }

// WIG: every declaration's line and the number of data lines before it
__global__ void __launch_bounds__(256) k_tt_decls(TtTab T, u64 n, const u64 *__restrict__ decl_base, const u64 *__restrict__ data_base,
                                                  u32 *__restrict__ decl_line, u64 *__restrict__ decl_d0)
{
    __shared__ u32 s_wave[4];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 t = tt_type(T, i, n);
    const bool decl = t == ttrack::L_VAR || t == ttrack::L_FIXED, data = t == ttrack::L_DATA;
    const u32 rc = tt_block_rank(decl, s_wave), rd = tt_block_rank(data, s_wave);
    if (decl) {
        const u64 d = decl_base[blockIdx.x] + rc;
        decl_line[d] = (u32)i;
        decl_d0[d] = data_base[blockIdx.x] + rd;
    }
}

// WIG: a data line's declaration (the last one before it) gives its chromosome and, with its rank k in the block, its interval
__global__ void __launch_bounds__(256) k_tt_wig(TtTab T, u64 n, const u64 *__restrict__ decl_base, const u64 *__restrict__ data_base,
                                                const u32 *__restrict__ decl_line, const u64 *__restrict__ decl_d0,
                                                unsigned long long *__restrict__ first_err)
{
    __shared__ u32 s_wave[4];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 t = tt_type(T, i, n);
    const bool decl = t == ttrack::L_VAR || t == ttrack::L_FIXED, data = t == ttrack::L_DATA;
    const u32 rc = tt_block_rank(decl, s_wave), rd = tt_block_rank(data, s_wave);
    if (!data) return;
    const u64 d = decl_base[blockIdx.x] + rc;          // declarations before this line
    if (d == 0) {
        atomicMin(first_err, (unsigned long long)((i << 8) | ttrack::TT_ERR_NODECL));
        return;
    }
    const u32 j = decl_line[d - 1];
    const u64 k = data_base[blockIdx.x] + rd - decl_d0[d - 1];
    u32 b = 0, e = 0;
    const u32 err = ttrack::wig_interval(T.tag[j] & 255u, T.tag[i] >> 8, T.b[i], T.b[j], T.e[j], __float_as_uint(T.v[j]), k, b, e);
    if (err) {
        atomicMin(first_err, (unsigned long long)((i << 8) | err));
        return;
    }
    T.b[i] = b;
    T.e[i] = e;
    T.nm[i] = T.nm[j];
    T.h[i] = T.h[j];
}

// the data lines in file order
__global__ void __launch_bounds__(256) k_tt_list(TtTab T, u64 n, const u64 *__restrict__ data_base, u32 *__restrict__ dl)
{
    __shared__ u32 s_wave[4];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool data = tt_type(T, i, n) == ttrack::L_DATA;
    const u32 rd = tt_block_rank(data, s_wave);
    if (data) dl[data_base[blockIdx.x] + rd] = (u32)i;
}

__device__ __forceinline__ bool tt_same_name(const u8 *D, const TtTab &T, u32 x, u32 y)
{
    const u64 a = T.nm[x], b = T.nm[y];
    if (a == b) return true;
    if (T.h[x] != T.h[y] || (a & 255u) != (b & 255u)) return false;
    const u64 pa = a >> 8, pb = b >> 8;
    for (u32 k = 0; k < (u32)(a & 255u); k++)
        if (D[pa + k] != D[pb + k]) return false;
    return true;
}

// chromosome block heads among the data lines: counted per workgroup (WRITE = false), then listed (rank of the data line)
template <bool WRITE>
__global__ void __launch_bounds__(256) k_tt_heads(const u8 *__restrict__ D, TtTab T, const u32 *__restrict__ dl, u64 nd,
                                                  u32 *__restrict__ hcnt, const u64 *__restrict__ hbase, u32 *__restrict__ heads)
{
    __shared__ u32 s_wave[4];
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool head = r < nd && (r == 0 || !tt_same_name(D, T, dl[r - 1], dl[r]));
    if (!WRITE) {
        const int c = __syncthreads_count(head);
        if (threadIdx.x == 0) hcnt[blockIdx.x] = (u32)c;
        return;
    }
    const u32 rk = tt_block_rank(head, s_wave);
    if (head) heads[hbase[blockIdx.x] + rk] = (u32)r;
}

// the names of the heads, 256 bytes each, and their lengths
__global__ void __launch_bounds__(256) k_tt_headnames(const u8 *__restrict__ D, TtTab T, const u32 *__restrict__ dl,
                                                      const u32 *__restrict__ heads, u32 nh, u8 *__restrict__ names, u8 *__restrict__ lens)
{
    const u32 hx = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (hx >= nh) return;
    const u64 nm = T.nm[dl[heads[hx]]];
    const u32 len = (u32)(nm & 255u);
    const u64 off = nm >> 8;
    for (u32 k = lane; k < len; k += 64u) names[(u64)hx * 256u + k] = D[off + k];
    if (lane == 0) lens[hx] = (u8)len;
}

// a stable counting pass: data rank r of head run h goes to head_dest[h] + (r - heads[h]); each chromosome's largest end
__global__ void __launch_bounds__(256) k_tt_scatter(TtTab T, const u32 *__restrict__ dl, u64 nd, const u32 *__restrict__ heads, u32 nh,
                                                    const u32 *__restrict__ head_chrom, const u64 *__restrict__ head_dest,
                                                    u32 *__restrict__ sb, u32 *__restrict__ se, float *__restrict__ sv, u32 *__restrict__ ext)
{
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= nd) return;
    u32 lo = 0, hi = nh;                    // the last head at or before r (heads[0] == 0)
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if ((u64)heads[mid] <= r) lo = mid;
        else hi = mid;
    }
    const u32 line = dl[r];
    const u64 dst = head_dest[lo] + (r - heads[lo]);
    const u32 e = T.e[line];
    sb[dst] = T.b[line];
    se[dst] = e;
    sv[dst] = T.v[line];
    atomicMax(&ext[head_chrom[lo]], e);
}

__global__ void __launch_bounds__(256) k_tt_patch(float *__restrict__ v, const u32 *__restrict__ line, const float *__restrict__ val, u32 n)
{
    const u32 j = blockIdx.x * 256u + threadIdx.x;
    if (j < n) v[line[j]] = val[j];
}

// the value tokens of the slow list, 64 bytes each (longer ones are copied one by one)
__global__ void __launch_bounds__(256) k_tt_gather(const u8 *__restrict__ D, const TtSlow *__restrict__ slow, u32 n, u8 *__restrict__ out)
{
    const u32 j = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (j >= n) return;
    const TtSlow x = slow[j];
    if (x.len < 64u && lane < x.len) out[(u64)j * 64u + lane] = D[x.off + lane];
}

__device__ __forceinline__ bool tt_keep(float v, float threshold) { return !(threshold > 0.f && !(v >= threshold)); }

__global__ void __launch_bounds__(256) k_tt_keep(const float *__restrict__ sv, u64 nd, float threshold, u32 *__restrict__ cnt)
{
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    const int c = __syncthreads_count(r < nd && tt_keep(sv[r], threshold));
    if (threadIdx.x == 0) cnt[blockIdx.x] = (u32)c;
}

__global__ void __launch_bounds__(256) k_tt_compact(const u32 *__restrict__ sb, const u32 *__restrict__ se, const float *__restrict__ sv,
                                                    u64 nd, float threshold, const u64 *__restrict__ base, u32 *__restrict__ ob,
                                                    u32 *__restrict__ oe, float *__restrict__ ov)
{
    __shared__ u32 s_wave[4];
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool k = r < nd && tt_keep(sv[r], threshold);
    const u32 rk = tt_block_rank(k, s_wave);
    if (!k) return;
    const u64 o = base[blockIdx.x] + rk;
    ob[o] = sb[r];
    oe[o] = se[r];
    ov[o] = sv[r];
}

// the kept intervals before position p of the per-chromosome order, for every chromosome start (cbase[0..nc])
__global__ void __launch_bounds__(256) k_tt_ranges(const float *__restrict__ sv, u64 nd, float threshold, const u64 *__restrict__ base,
                                                   const u64 *__restrict__ total, const u64 *__restrict__ cbase, u32 nc1, u64 *__restrict__ out)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c >= nc1) return;
    const u64 p = cbase[c];
    if (p >= nd) {
        out[c] = total[0];
        return;
    }
    u64 k = base[p >> 8];
    for (u64 r = p & ~255ull; r < p; r++) k += tt_keep(sv[r], threshold) ? 1u : 0u;
    out[c] = k;
}

namespace {

// the text of `path` into HBM (+ 64 zero-padded bytes): *d_text, *N
int tt_upload(const char *path, int device, int nthreads, u8 **d_text, u64 *N)
{
    u8 head[18] = {0};
    u64 fsize = 0;
    {
        OpenFile f;
        if (int rc = open_file(path, f)) return rc;
        fsize = f.size;
        if (fsize && !pread_all(f.fd, head, 0, std::min<u64>(fsize, sizeof head), 1))
            return fail(PMX_DBAM_ERR_OPEN, std::string("read error on ") + path);
    }
    const int comp = ttrack::detect_compression(head, std::min<u64>(fsize, sizeof head));
    auto host_gzip = [&](std::vector<u8> &text, std::string &err) -> int {   // the whole file through zlib on the host
        OpenFile f;
        if (int rc = open_file(path, f)) return rc;
        std::vector<u8> file(f.size);
        if (f.size && !pread_all(f.fd, file.data(), 0, f.size, nthreads)) return fail(PMX_DBAM_ERR_OPEN, std::string("read error on ") + path);
        return ttrack::inflate_gzip(file.data(), file.size(), text, err) ? 0 : 1;
    };
    if (comp == ttrack::COMP_GZIP) {
        std::vector<u8> text;
        std::string err;
        const int rc = host_gzip(text, err);
        if (rc < 0) return rc;
        if (rc) return fail(PMX_DBAM_ERR_FORMAT, err);
        HIPOK(hipMalloc((void **)d_text, text.size() + 64));
        HIPOK(hipMemset(*d_text + text.size(), 0, 64));
        if (!text.empty()) HIPOK(hipMemcpy(*d_text, text.data(), text.size(), hipMemcpyHostToDevice));
        *N = text.size();
        return 0;
    }
    // plain text or BGZF: the SAM open's paths, through a pmx_dbam that hands its text over
    pmx_dbam *b = new pmx_dbam;
    b->device = device;
    b->sam = true;
    b->pipelined = false;
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&b->kstream, hipStreamNonBlocking) != hipSuccess) {
        pmx_dbam_close(b);
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    int rc = comp == ttrack::COMP_BGZF ? read_and_upload(*b, path, nthreads) : sam_upload_plain(*b, path, nthreads);
    if (!rc && comp == ttrack::COMP_BGZF) rc = inflate_all(*b);
    if (!rc) {
        if (!b->d_out) rc = fail(PMX_DBAM_ERR_DEVICE, "no text buffer");
        *d_text = b->d_out;
        *N = b->N;
        b->d_out = nullptr;
    }
    const std::string keep = g_err;
    pmx_dbam_close(b);
    g_err = keep;
    if (rc == PMX_DBAM_ERR_FORMAT && comp == ttrack::COMP_BGZF) {   // the words of the host reader: where the text breaks off
        std::vector<u8> text;
        std::string err;
        if (host_gzip(text, err) == 1) return fail(PMX_DBAM_ERR_FORMAT, err);
    }
    return rc;
}

struct TtDev {              // the open's device tables, freed however it ends (a deque: its elements never move)
    std::deque<DevAlloc> a;
    template <class T>
    int get(T **out, u64 bytes)
    {
        a.emplace_back();
        HIPOK(hipMalloc(&a.back().p, std::max<u64>(bytes, 16)));
        *out = (T *)a.back().p;
        return 0;
    }
};

int tt_build(pmx_dbw &w, const char *path, u8 *D, u64 N)
{
    hipStream_t st = w.stream;
    // the kind of track from the first lines
    u32 kind = 0;
    {
        std::vector<u8> pre;
        for (u64 L = std::min<u64>(N, 1u << 16);; L = std::min<u64>(N, 4 * L)) {
            pre.resize(L);
            if (L) HIPOK(hipMemcpy(pre.data(), D, L, hipMemcpyDeviceToHost));
            if (ttrack::detect_kind(pre.data(), L, L == N, path, kind) == 0) break;
        }
    }
    if (N == 0) return 0;
    TtDev t;
    // the line index
    const u64 nch = (N + SAM_CHUNK - 1) / SAM_CHUNK;
    u32 *d_ccnt;
    u64 *d_cbase, *d_tot;
    if (int rc = t.get(&d_ccnt, 4 * nch)) return rc;
    if (int rc = t.get(&d_cbase, 8 * nch)) return rc;
    if (int rc = t.get(&d_tot, 16)) return rc;
    hipLaunchKernelGGL(k_sam_count, dim3((unsigned)nch), dim3(256), 0, st, D, 0ull, N, 0ull, d_ccnt);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_ccnt, d_ccnt, nch, d_cbase, d_tot);
    HIPOK(hipGetLastError());
    u64 tot[2] = {0, 0};
    u8 last = 0;
    HIPOK(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&last, D + N - 1, 1, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const u64 nnl = tot[0], n = nnl + (last != '\n' ? 1u : 0u);
    if (n >= 0xffffffffull) return fail(PMX_DBAM_ERR_FORMAT, "more than 2^32 - 2 lines");
    u64 *d_nl;
    if (int rc = t.get(&d_nl, 8 * n)) return rc;
    hipLaunchKernelGGL(k_sam_lines, dim3((unsigned)nch), dim3(256), 0, st, D, 0ull, N, 0ull, d_cbase, d_nl);
    HIPOK(hipGetLastError());
    if (n > nnl) HIPOK(hipMemcpyAsync(d_nl + nnl, &N, 8, hipMemcpyHostToDevice, st));
    // the line table
    const u64 nb = (n + 255) / 256;
    TtTab T;
    if (int rc = t.get(&T.tag, 4 * n)) return rc;
    if (int rc = t.get(&T.b, 4 * n)) return rc;
    if (int rc = t.get(&T.e, 4 * n)) return rc;
    if (int rc = t.get(&T.v, 4 * n)) return rc;
    if (int rc = t.get(&T.nm, 8 * n)) return rc;
    if (int rc = t.get(&T.h, 4 * n)) return rc;
    u32 *d_cdata, *d_cdecl, *d_nslow;
    u64 *d_data_base, *d_decl_base, *d_tot2;
    unsigned long long *d_err, *d_first_data;
    if (int rc = t.get(&d_cdata, 4 * nb)) return rc;
    if (int rc = t.get(&d_cdecl, 4 * nb)) return rc;
    if (int rc = t.get(&d_data_base, 8 * nb)) return rc;
    if (int rc = t.get(&d_decl_base, 8 * nb)) return rc;
    if (int rc = t.get(&d_tot2, 16)) return rc;
    if (int rc = t.get(&d_err, 8)) return rc;
    if (int rc = t.get(&d_first_data, 8)) return rc;
    if (int rc = t.get(&d_nslow, 4)) return rc;
    u32 slow_cap = (u32)std::min<u64>(n, 1u << 16), nslow = 0;
    TtSlow *d_slow = nullptr;
    unsigned long long fe = 0, fd = 0;
    for (int pass = 0; pass < 2; pass++) {      // (a second pass only when the slow list did not fit)
        if (int rc = t.get(&d_slow, sizeof(TtSlow) * slow_cap)) return rc;
        HIPOK(hipMemsetAsync(d_err, 0xff, 8, st));
        HIPOK(hipMemsetAsync(d_first_data, 0xff, 8, st));
        HIPOK(hipMemsetAsync(d_nslow, 0, 4, st));
        hipLaunchKernelGGL(k_tt_parse, dim3((unsigned)nb), dim3(256), 0, st, D, d_nl, n, kind, T, d_cdata, d_cdecl, d_err, d_first_data,
                           d_slow, d_nslow, slow_cap);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&nslow, d_nslow, 4, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (nslow <= slow_cap) break;
        slow_cap = nslow;
    }
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cdata, d_cdata, nb, d_data_base, d_tot2);
    HIPOK(hipGetLastError());
    u64 nd = 0;
    HIPOK(hipMemcpyAsync(&nd, d_tot2, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (kind == ttrack::KIND_WIG) {
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cdecl, d_cdecl, nb, d_decl_base, d_tot2);
        HIPOK(hipGetLastError());
        u64 ndecl = 0;
        HIPOK(hipMemcpyAsync(&ndecl, d_tot2, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        u32 *d_decl_line;
        u64 *d_decl_d0;
        if (int rc = t.get(&d_decl_line, 4 * ndecl)) return rc;
        if (int rc = t.get(&d_decl_d0, 8 * ndecl)) return rc;
        hipLaunchKernelGGL(k_tt_decls, dim3((unsigned)nb), dim3(256), 0, st, T, n, d_decl_base, d_data_base, d_decl_line, d_decl_d0);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_tt_wig, dim3((unsigned)nb), dim3(256), 0, st, T, n, d_decl_base, d_data_base, d_decl_line, d_decl_d0, d_err);
        HIPOK(hipGetLastError());
    }
    HIPOK(hipMemcpyAsync(&fe, d_err, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&fd, d_first_data, 8, hipMemcpyDeviceToHost, st));
    std::vector<TtSlow> slow(nslow);
    if (nslow) HIPOK(hipMemcpyAsync(slow.data(), d_slow, sizeof(TtSlow) * nslow, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    // the slow list: track lines (at most one, before the first data line) and the values strtod decides
    u64 err_line = fe == ~0ull ? ~0ull : (fe >> 8);
    u32 err_code = fe == ~0ull ? 0u : (u32)(fe & 255u);
    std::sort(slow.begin(), slow.end(), [](const TtSlow &x, const TtSlow &y) { return x.line < y.line; });
    {
        bool seen = false;
        for (const TtSlow &x : slow) {
            if (x.len != ~0u) continue;
            const u32 code = (u64)x.line > fd ? ttrack::TT_ERR_LATE_TRACK : seen ? ttrack::TT_ERR_TRACK : 0u;
            seen = true;
            if (code) {
                if ((u64)x.line < err_line) {
                    err_line = x.line;
                    err_code = code;
                }
                break;
            }
        }
    }
    if (err_code) return fail(PMX_DBAM_ERR_FORMAT, ttrack::line_error(err_line, err_code));
    std::vector<u32> pl;
    std::vector<float> pv;
    {
        std::vector<u32> idx;
        for (u32 j = 0; j < nslow; j++)
            if (slow[j].len != ~0u) idx.push_back(j);
        if (!idx.empty()) {
            TtSlow *d_s2;
            u8 *d_tok;
            if (int rc = t.get(&d_s2, sizeof(TtSlow) * idx.size())) return rc;
            if (int rc = t.get(&d_tok, 64ull * idx.size())) return rc;
            std::vector<TtSlow> s2;
            for (u32 j : idx) s2.push_back(slow[j]);
            HIPOK(hipMemcpyAsync(d_s2, s2.data(), sizeof(TtSlow) * s2.size(), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_tt_gather, dim3((unsigned)((s2.size() + 3) / 4)), dim3(256), 0, st, D, d_s2, (u32)s2.size(), d_tok);
            HIPOK(hipGetLastError());
            std::vector<u8> tok(64ull * s2.size());
            HIPOK(hipMemcpyAsync(tok.data(), d_tok, tok.size(), hipMemcpyDeviceToHost, st));
            HIPOK(hipStreamSynchronize(st));
            std::vector<char> longtok;
            for (size_t j = 0; j < s2.size(); j++) {
                const char *p = (const char *)tok.data() + 64 * j;
                if (s2[j].len >= 64u) {
                    longtok.resize(s2[j].len);
                    HIPOK(hipMemcpy(longtok.data(), D + s2[j].off, s2[j].len, hipMemcpyDeviceToHost));
                    p = longtok.data();
                }
                pl.push_back(s2[j].line);
                pv.push_back(ttrack::slow_value(p, s2[j].len));
            }
            u32 *d_pl;
            float *d_pv;
            if (int rc = t.get(&d_pl, 4 * pl.size())) return rc;
            if (int rc = t.get(&d_pv, 4 * pv.size())) return rc;
            HIPOK(hipMemcpyAsync(d_pl, pl.data(), 4 * pl.size(), hipMemcpyHostToDevice, st));
            HIPOK(hipMemcpyAsync(d_pv, pv.data(), 4 * pv.size(), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(k_tt_patch, dim3((unsigned)((pl.size() + 255) / 256)), dim3(256), 0, st, T.v, d_pl, d_pv, (u32)pl.size());
            HIPOK(hipGetLastError());
        }
    }
    w.text_slow = pl.size();
    if (nd == 0) {
        HIPOK(hipStreamSynchronize(st));
        return 0;
    }
    // the data lines in file order, and the heads of their chromosome blocks
    const u64 nbd = (nd + 255) / 256;
    u32 *d_dl, *d_hcnt;
    u64 *d_hbase;
    if (int rc = t.get(&d_dl, 4 * nd)) return rc;
    if (int rc = t.get(&d_hcnt, 4 * nbd)) return rc;
    if (int rc = t.get(&d_hbase, 8 * nbd)) return rc;
    hipLaunchKernelGGL(k_tt_list, dim3((unsigned)nb), dim3(256), 0, st, T, n, d_data_base, d_dl);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_tt_heads<false>, dim3((unsigned)nbd), dim3(256), 0, st, D, T, d_dl, nd, d_hcnt, (const u64 *)nullptr, (u32 *)nullptr);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_hcnt, d_hcnt, nbd, d_hbase, d_tot2);
    HIPOK(hipGetLastError());
    u64 nh64 = 0;
    HIPOK(hipMemcpyAsync(&nh64, d_tot2, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const u32 nh = (u32)nh64;
    u32 *d_heads;
    u8 *d_names, *d_nlen;
    if (int rc = t.get(&d_heads, 4ull * nh)) return rc;
    if (int rc = t.get(&d_names, 256ull * nh)) return rc;
    if (int rc = t.get(&d_nlen, nh)) return rc;
    hipLaunchKernelGGL(k_tt_heads<true>, dim3((unsigned)nbd), dim3(256), 0, st, D, T, d_dl, nd, d_hcnt, d_hbase, d_heads);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_tt_headnames, dim3((nh + 3) / 4), dim3(256), 0, st, D, T, d_dl, d_heads, nh, d_names, d_nlen);
    HIPOK(hipGetLastError());
    std::vector<u32> heads(nh);
    std::vector<u8> names(256ull * nh), nlen(nh);
    HIPOK(hipMemcpyAsync(heads.data(), d_heads, 4ull * nh, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(names.data(), d_names, names.size(), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(nlen.data(), d_nlen, nh, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    // the heads named and merged into chromosomes (in the order of their first line); each run's place in per-chromosome order
    std::unordered_map<std::string, u32> ids;
    std::vector<u32> head_chrom(nh);
    std::vector<u64> run_len(nh), count;
    for (u32 h = 0; h < nh; h++) {
        const u8 *p = names.data() + 256ull * h;
        std::string nm((const char *)p, nlen[h]);
        auto it = ids.find(nm);
        if (it == ids.end()) {
            it = ids.emplace(nm, (u32)w.names.size()).first;
            w.names.push_back(nm);
            count.push_back(0);
        }
        head_chrom[h] = it->second;
        run_len[h] = (h + 1 < nh ? (u64)heads[h + 1] : nd) - heads[h];
        count[it->second] += run_len[h];
    }
    const size_t nc = w.names.size();
    std::vector<u64> cbase(nc + 1, 0), at(nc), head_dest(nh);
    for (size_t c = 0; c < nc; c++) cbase[c + 1] = cbase[c] + count[c];
    for (size_t c = 0; c < nc; c++) at[c] = cbase[c];
    for (u32 h = 0; h < nh; h++) {
        head_dest[h] = at[head_chrom[h]];
        at[head_chrom[h]] += run_len[h];
    }
    u32 *d_hchrom, *d_ext;
    u64 *d_hdest;
    if (int rc = t.get(&d_hchrom, 4ull * nh)) return rc;
    if (int rc = t.get(&d_hdest, 8ull * nh)) return rc;
    if (int rc = t.get(&d_ext, 4ull * nc)) return rc;
    HIPOK(hipMemcpyAsync(d_hchrom, head_chrom.data(), 4ull * nh, hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_hdest, head_dest.data(), 8ull * nh, hipMemcpyHostToDevice, st));
    HIPOK(hipMemsetAsync(d_ext, 0, 4ull * nc, st));
    HIPOK(hipMalloc((void **)&w.t_b, 4 * nd));
    HIPOK(hipMalloc((void **)&w.t_e, 4 * nd));
    HIPOK(hipMalloc((void **)&w.t_v, 4 * nd));
    HIPOK(hipMalloc((void **)&w.t_cbase, 8 * (nc + 1)));
    HIPOK(hipMemcpyAsync(w.t_cbase, cbase.data(), 8 * (nc + 1), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_tt_scatter, dim3((unsigned)nbd), dim3(256), 0, st, T, d_dl, nd, d_heads, nh, d_hchrom, d_hdest, w.t_b, w.t_e,
                       w.t_v, d_ext);
    HIPOK(hipGetLastError());
    std::vector<u32> ext(nc);
    HIPOK(hipMemcpyAsync(ext.data(), d_ext, 4ull * nc, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    for (size_t c = 0; c < nc; c++) w.sizes.push_back((int64_t)ext[c]);
    w.t_n = nd;
    w.text_heads = nh;
    w.text_lines = n;
    return 0;
}

}  // namespace

// the dbw_fetch_impl branch of a text track: every chromosome's lines with value >= threshold, kept and compacted in one pass
static int tt_decode_all(pmx_dbw *w, float threshold)
{
    for (void *p : {(void *)w->d_begin, (void *)w->d_end, (void *)w->d_value})
        if (p) w->retired.push_back(p);
    w->d_begin = w->d_end = nullptr;
    w->d_value = nullptr;
    w->range.assign(w->names.size(), std::pair<u64, u64>(0, 0));
    w->order.assign(w->names.size(), -1);
    w->have = true;
    w->have_threshold = threshold;
    w->total = 0;
    const u64 nd = w->t_n;
    if (!nd) return 0;
    hipStream_t st = w->stream;
    const u64 nb = (nd + 255) / 256;
    const u32 nc1 = (u32)w->names.size() + 1u;
    DevAlloc d_cnt, d_base, d_tot, d_rng;
    HIPOK(hipMalloc(&d_cnt.p, 4 * nb));
    HIPOK(hipMalloc(&d_base.p, 8 * nb));
    HIPOK(hipMalloc(&d_tot.p, 16));
    HIPOK(hipMalloc(&d_rng.p, 8ull * nc1));
    hipLaunchKernelGGL(k_tt_keep, dim3((unsigned)nb), dim3(256), 0, st, w->t_v, nd, threshold, d_cnt.as<u32>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cnt.as<u32>(), d_cnt.as<u32>(), nb, d_base.as<u64>(), d_tot.as<u64>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_tt_ranges, dim3((nc1 + 255) / 256), dim3(256), 0, st, w->t_v, nd, threshold, d_base.as<u64>(), d_tot.as<u64>(),
                       w->t_cbase, nc1, d_rng.as<u64>());
    HIPOK(hipGetLastError());
    u64 tot[2] = {0, 0};
    std::vector<u64> rng(nc1);
    HIPOK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(rng.data(), d_rng.p, 8ull * nc1, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    for (u32 c = 0; c + 1 < nc1; c++) w->range[c] = std::pair<u64, u64>(rng[c], rng[c + 1]);
    if (tot[0]) {
        HIPOK(hipMalloc((void **)&w->d_begin, 4 * tot[0]));
        HIPOK(hipMalloc((void **)&w->d_end, 4 * tot[0]));
        HIPOK(hipMalloc((void **)&w->d_value, 4 * tot[0]));
        hipLaunchKernelGGL(k_tt_compact, dim3((unsigned)nb), dim3(256), 0, st, w->t_b, w->t_e, w->t_v, nd, threshold, d_base.as<u64>(),
                           w->d_begin, w->d_end, w->d_value);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(st));
    }
    w->total = tot[0];
    return 0;
}

extern "C" {

static int dtt_open_impl(const char *path, int device, int nthreads, pmx_dbw **out);
int pmx_dtt_open(const char *path, int device, int nthreads, pmx_dbw **out)
{
    try {
        return dtt_open_impl(path, device, nthreads, out);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dtt_open: ") + e.what());
    }
}
static int dtt_open_impl(const char *path, int device, int nthreads, pmx_dbw **out)
{
    if (!path || !out) return fail(PMX_DBAM_ERR_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMX_DBAM_ERR_DEVICE, "no HIP device: the device ingest needs a GPU");
    if (device < 0 || device >= ndev) return fail(PMX_DBAM_ERR_INVALID, "no such device");
    HIPOK(hipSetDevice(device));
    if (nthreads <= 0) nthreads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    pmx_dbw *w = new pmx_dbw;
    w->device = device;
    w->text = true;
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    u8 *d_text = nullptr;
    u64 N = 0;
    int rc = tt_upload(path, device, nthreads, &d_text, &N);
    if (!rc) rc = tt_build(*w, path, d_text, N);
    if (d_text) {
        (void)hipStreamSynchronize(w->stream);
        (void)hipFree(d_text);          // (the intervals are in per-chromosome order: the text is not needed any more)
    }
    if (rc) {
        const std::string keep = g_err;
        pmx_dbw_close(w);
        g_err = keep.compare(0, strlen(path), path) == 0 ? keep : std::string(path) + ": " + keep;
        return rc;
    }
    *out = w;
    return 0;
}

}  // extern "C"
