// SAM text on the device (pmx_dsam_open, include/pymasc_amd_ingest.h; DESIGN.md 7.4).  Included at the end of bam_device.hip:
// the handle is a pmx_dbam whose stream is the text, so decode / fetch / runs / readlen_hist / counters work on it unchanged
// but for two branches (dbam_decode_impl -> dsam_decode, the histogram's launch -> dsam_launch_readlen).
//
//   host          plain SAM: the file through the page-locked staging buffers into HBM as it is; BGZF SAM: the BAM open's
//                 member scan, k_bgzf_inflate and k_bgzf_crc.  The header is parsed on the host from the stream's prefix.
//   k_sam_count   the record area cut into 64-KB chunks, one workgroup each, 16-B loads per lane: '\n' per chunk
//   k_bam_scan    exclusive prefix of the chunk counts (the record chain's scan)
//   k_sam_lines   the same chunks again: each lane's 16 bytes get their rank among the chunk's newlines from a workgroup scan,
//                 and the newline offsets are written in text order = the end of every line
//   k_sam_parse   one lane per line: fields 1-6 by the rules of io/sam_parse.h (shared with the host reader, which is the
//                 checker), RNAME through an open-addressing table of the @SQ names; the first error by line (atomicMin)
//   decode        k_sam_keep (kept per workgroup) + k_bam_scan + k_sam_compact (ballot ranks): the four arrays of the BAM decode
//   k_sam_readlen the read-length histogram over the line table, with k_bam_readlen's run-length + LDS-table scheme
// Every load of the text lies below the text's end rounded up to 16 bytes; the buffer holds 64 more bytes (no load past it).
#include "../io/sam_parse.h"

#define SAM_CHUNK 65536ull            // bytes of text per workgroup of the line index
#define SAM_RL_LINES 32u              // lines per lane of the histogram (a run of one length stays in registers)

// the text through 16-byte loads, the last one kept: a lane walking its line sequentially loads each 16 bytes once
struct DevSrc {
    const u8 *D;
    u64 a;
    uint4 v;
    __device__ u8 at(u64 i)
    {
        const u64 al = i & ~15ull;
        if (al != a) {
            a = al;
            v = *reinterpret_cast<const uint4 *>(D + al);
        }
        const u32 k = (u32)(i >> 2) & 3u;
        const u32 w = k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w;
        return (u8)(w >> (8u * ((u32)i & 3u)));
    }
};

__device__ __forceinline__ u32 nl_in_word(u32 w)
{
    const u32 x = w ^ 0x0a0a0a0au;                                   // a '\n' byte -> 0
    const u32 t = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x;             // bit 7 of a byte set unless it is 0 (exact, no carries)
    return __popc(~t & 0x80808080u);
}

// '\n' in the 16 bytes at `a` (16-aligned) that lie in [beg, N); also returns them as a 16-bit mask in *mask
__device__ __forceinline__ u32 nl_in_seg(const u8 *D, u64 a, u64 beg, u64 N, u32 *mask)
{
    if (a + 16u <= beg || a >= N) {
        *mask = 0;
        return 0;
    }
    const uint4 v = *reinterpret_cast<const uint4 *>(D + a);
    const u32 w[4] = {v.x, v.y, v.z, v.w};
    u32 m = 0;
#pragma unroll
    for (int q = 0; q < 4; q++)
        if (nl_in_word(w[q]))
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (((w[q] >> (8 * j)) & 255u) == 10u) m |= 1u << (4 * q + j);
    if (a < beg) m &= ~0u << (u32)(beg - a);                         // (beg - a < 16 here)
    if (a + 16u > N) m &= (1u << (u32)(N - a)) - 1u;
    *mask = m;
    return __popc(m);
}

__global__ void __launch_bounds__(256) k_sam_count(const u8 *__restrict__ D, u64 beg, u64 N, u64 c0, u32 *__restrict__ cnt)
{
    __shared__ u32 s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const u64 base = (c0 + blockIdx.x) * SAM_CHUNK;
    u32 n = 0, m;
    for (u32 k = 0; k < SAM_CHUNK / (16u * 256u); k++) n += nl_in_seg(D, base + 16ull * (k * 256u + threadIdx.x), beg, N, &m);
    for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o, 64);
    if ((threadIdx.x & 63u) == 0 && n) atomicAdd(&s_n, n);
    __syncthreads();
    if (threadIdx.x == 0) cnt[blockIdx.x] = s_n;
}

__global__ void __launch_bounds__(256) k_sam_lines(const u8 *__restrict__ D, u64 beg, u64 N, u64 c0, const u64 *__restrict__ chunk_base,
                                                   u64 *__restrict__ nl)
{
    __shared__ u32 s_wave[4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 base = (c0 + blockIdx.x) * SAM_CHUNK;
    u64 out = chunk_base[blockIdx.x];
    for (u32 k = 0; k < SAM_CHUNK / (16u * 256u); k++) {
        const u64 a = base + 16ull * (k * 256u + t);
        u32 m;
        const u32 n = nl_in_seg(D, a, beg, N, &m);
        u32 incl = n;                                                // inclusive scan over the wave
        for (u32 o = 1; o < 64u; o <<= 1) {
            const u32 y = __shfl_up(incl, o, 64);
            if (lane >= o) incl += y;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        u32 before = 0, total = 0;
        for (u32 w = 0; w < 4u; w++) {
            if (w < wave) before += s_wave[w];
            total += s_wave[w];
        }
        u64 o = out + before + (incl - n);
        while (m) {
            const u32 j = (u32)__ffs(m) - 1u;
            nl[o++] = a + j;
            m &= m - 1u;
        }
        out += total;
        __syncthreads();                                             // (s_wave is reused by the next step)
    }
}

__global__ void __launch_bounds__(256) k_sam_parse(const u8 *__restrict__ D, u64 beg, const u64 *__restrict__ nl, u64 nrec,
                                                   const samtext::Names nm, int *__restrict__ o_ref, int *__restrict__ o_pos,
                                                   u32 *__restrict__ o_qlen, u32 *__restrict__ o_fm, unsigned long long *__restrict__ first_err)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= nrec) return;
    DevSrc s{D, ~0ull, make_uint4(0, 0, 0, 0)};
    samtext::Rec r;
    r.ref = -1;
    r.pos1 = 0;
    r.qlen = 0;
    r.flag = r.mapq = 0;
    const u32 e = samtext::parse_line(s, i ? nl[i - 1] + 1u : beg, nl[i], nm, r);
    if (e) {
        atomicMin(first_err, (unsigned long long)((i << 8) | e));
        r.ref = -1;
    }
    o_ref[i] = r.ref;
    o_pos[i] = r.pos1;
    o_qlen[i] = r.qlen;
    o_fm[i] = r.flag | (r.mapq << 16);
}

__device__ __forceinline__ bool sam_keep(const int *ref, const u32 *qlen, const u32 *fm, u64 i, u32 mapq_min, u32 flag_exclude,
                                         int want_ref)
{
    const u32 f = fm[i];
    const int r = ref[i];
    return !((f & 0xffffu) & flag_exclude) && (f >> 16) >= mapq_min && r >= 0 && (want_ref < 0 || r == want_ref) && qlen[i] != 0u;
}

__global__ void __launch_bounds__(256) k_sam_keep(const int *__restrict__ ref, const u32 *__restrict__ qlen, const u32 *__restrict__ fm,
                                                  u64 nrec, u32 mapq_min, u32 flag_exclude, int want_ref, u32 *__restrict__ bcnt)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool k = i < nrec && sam_keep(ref, qlen, fm, i, mapq_min, flag_exclude, want_ref);
    const int n = __syncthreads_count(k);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = (u32)n;
}

__global__ void __launch_bounds__(256) k_sam_compact(const int *__restrict__ ref, const int *__restrict__ pos, const u32 *__restrict__ qlen,
                                                     const u32 *__restrict__ fm, u64 nrec, u32 mapq_min, u32 flag_exclude, int want_ref,
                                                     const u64 *__restrict__ bbase, int *__restrict__ o_ref, int *__restrict__ o_pos,
                                                     int *__restrict__ o_len, u8 *__restrict__ o_rev)
{
    __shared__ u32 s_wave[4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 i = (u64)blockIdx.x * 256u + t;
    const bool k = i < nrec && sam_keep(ref, qlen, fm, i, mapq_min, flag_exclude, want_ref);
    const u64 m = __ballot(k);
    if (lane == 0) s_wave[wave] = (u32)__popcll(m);
    __syncthreads();
    if (!k) return;
    u64 o = bbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; w++) o += s_wave[w];
    o_ref[o] = ref[i];
    o_pos[o] = pos[i];
    o_len[o] = (int)qlen[i];
    o_rev[o] = (fm[i] & 0x10u) ? 1 : 0;
}

// k_bam_readlen over the line table: SAM_RL_LINES consecutive lines per lane; the first-occurrence key is the line's offset
template <int PASS>
__global__ void __launch_bounds__(256) k_sam_readlen(const RlArgs A, const int *__restrict__ ref, const u32 *__restrict__ qlen,
                                                     const u32 *__restrict__ fm, const u64 *__restrict__ nl, u64 beg, u64 nrec)
{
    readlen_lane<PASS>(A, [&](auto add) {
        const u64 lo = ((u64)blockIdx.x * 256u + threadIdx.x) * SAM_RL_LINES;
        const u64 hi = lo + SAM_RL_LINES < nrec ? lo + SAM_RL_LINES : nrec;
        for (u64 i = lo; i < hi; i++)
            if (ref[i] >= 0)
                add(fm[i] & 0xffffu, fm[i] >> 16, [&]() { return qlen[i]; }, [&]() { return A.base + (i ? nl[i - 1] + 1u : beg); });
    });
}

namespace {

// plain SAM: the file -> HBM through the page-locked staging buffers, as it is (+ 64 zero bytes behind it)
int sam_upload_plain(pmx_dbam &b, const char *path, int nthreads)
{
    OpenFile f;
    if (int rc = open_file(path, f)) return rc;
    b.fsize = f.size;
    HIPOK(hipMalloc((void **)&b.d_out, b.fsize + 64));
    b.dout_cap = b.fsize + 64;
    HIPOK(hipMemsetAsync(b.d_out + b.fsize, 0, 64, b.stream));
    std::lock_guard<std::mutex> stage_guard(g_stage_mu);
    StageReset stage_reset{b.stream};
    if (int rc = stage_setup()) return rc;
    const size_t npieces = (b.fsize + STAGE_PAYLOAD - 1) / STAGE_PAYLOAD;
    for (size_t k = 0; k < npieces; k++) {
        const int j = (int)(k % NSTAGE);
        if (g_stage.used[j]) HIPOK(hipEventSynchronize(g_stage.ev[j]));
        const u64 a = (u64)k * STAGE_PAYLOAD;
        const u64 len = std::min<u64>(STAGE_PAYLOAD, b.fsize - a);
        if (!pread_all(f.fd, g_stage.buf[j], a, len, (int)std::max<u64>(1, std::min<u64>((u64)nthreads, len >> 20))))
            return fail(PMX_DBAM_ERR_OPEN, std::string("read error on ") + path);
        HIPOK(hipMemcpyAsync(b.d_out + a, g_stage.buf[j], len, hipMemcpyHostToDevice, b.stream));
        HIPOK(hipEventRecord(g_stage.ev[j], b.stream));
        g_stage.used[j] = true;
    }
    HIPOK(hipStreamSynchronize(b.stream));
    b.N = b.fsize;
    return 0;
}

// the header from the stream's prefix (grown until the first record line is in it)
int sam_header(pmx_dbam &b, samtext::Header &h)
{
    std::vector<u8> pre;
    for (u64 L = std::min<u64>(b.N, 1u << 20);; L = std::min<u64>(b.N, 2 * L)) {
        pre.resize(L);
        if (L) HIPOK(hipMemcpy(pre.data(), b.d_out, L, hipMemcpyDeviceToHost));
        std::string err;
        const int rc = samtext::parse_header((const char *)pre.data(), L, L == b.N, h, err);
        if (rc < 0) return fail(PMX_DBAM_ERR_FORMAT, err);
        if (rc == 0) break;
    }
    b.text = h.text;
    b.ref_names = h.names;
    b.ref_lens = h.lens;
    b.data_beg = h.data_beg;
    b.sam_hdr_lines = h.lines;
    return 0;
}

// line index + parse of the record area: b.d_nl, the line table, b.sam_lines
int sam_index_parse(pmx_dbam &b, const samtext::Header &h)
{
    const u64 beg = b.data_beg, N = b.N;
    if (N <= beg) return 0;
    const u8 *D = b.d_out;
    double t0 = now_s();
    const u64 c0 = beg / SAM_CHUNK, nch = (N + SAM_CHUNK - 1) / SAM_CHUNK - c0;
    DevAlloc d_cnt, d_base, d_tot;
    HIPOK(hipMalloc(&d_cnt.p, 4 * nch));
    HIPOK(hipMalloc(&d_base.p, 8 * nch));
    HIPOK(hipMalloc(&d_tot.p, 16));
    hipLaunchKernelGGL(k_sam_count, dim3((unsigned)nch), dim3(256), 0, b.stream, D, beg, N, c0, d_cnt.as<u32>());
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, b.stream, d_cnt.as<u32>(), d_cnt.as<u32>(), nch, d_base.as<u64>(),
                       d_tot.as<u64>());
    HIPOK(hipGetLastError());
    u64 tot[2] = {0, 0};
    u8 last = 0;
    HIPOK(hipMemcpyAsync(tot, d_tot.p, 16, hipMemcpyDeviceToHost, b.stream));
    HIPOK(hipMemcpyAsync(&last, D + N - 1, 1, hipMemcpyDeviceToHost, b.stream));
    HIPOK(hipStreamSynchronize(b.stream));
    const u64 nnl = tot[0];
    const bool tail = last != '\n';                      // the last line without its '\n': its end is the end of the text
    u64 n = nnl + (tail ? 1u : 0u);
    HIPOK(hipMalloc((void **)&b.d_nl, 8 * std::max<u64>(n, 1)));
    hipLaunchKernelGGL(k_sam_lines, dim3((unsigned)nch), dim3(256), 0, b.stream, D, beg, N, c0, d_base.as<u64>(), b.d_nl);
    HIPOK(hipGetLastError());
    if (tail) HIPOK(hipMemcpyAsync(b.d_nl + nnl, &N, 8, hipMemcpyHostToDevice, b.stream));
    // one empty line at the very end is allowed: it is no record
    u64 ends[2] = {0, 0};
    HIPOK(hipMemcpyAsync(ends, b.d_nl + (n >= 2 ? n - 2 : 0), 8 * std::min<u64>(n, 2), hipMemcpyDeviceToHost, b.stream));
    HIPOK(hipStreamSynchronize(b.stream));
    const u64 ls = n >= 2 ? ends[0] + 1 : beg, le = n >= 2 ? ends[1] : ends[0];
    u64 len = le - ls;
    if (len == 1) {
        u8 c = 0;
        HIPOK(hipMemcpy(&c, D + ls, 1, hipMemcpyDeviceToHost));
        if (c == '\r') len = 0;
    }
    if (len == 0) n--;
    b.sam_lines = n;
    b.sam_line0 = h.lines;
    double t1 = now_s();
    b.t[4] = t1 - t0;
    if (n == 0) return 0;
    // the @SQ name table
    DevAlloc d_bytes, d_off, d_slot, d_err;
    HIPOK(hipMalloc(&d_bytes.p, std::max<size_t>(h.bytes.size(), 1)));
    HIPOK(hipMalloc(&d_off.p, 4 * h.off.size()));
    HIPOK(hipMalloc(&d_slot.p, 4 * h.slot.size()));
    HIPOK(hipMalloc(&d_err.p, 8));
    if (!h.bytes.empty()) HIPOK(hipMemcpyAsync(d_bytes.p, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice, b.stream));
    HIPOK(hipMemcpyAsync(d_off.p, h.off.data(), 4 * h.off.size(), hipMemcpyHostToDevice, b.stream));
    HIPOK(hipMemcpyAsync(d_slot.p, h.slot.data(), 4 * h.slot.size(), hipMemcpyHostToDevice, b.stream));
    HIPOK(hipMemsetAsync(d_err.p, 0xff, 8, b.stream));
    HIPOK(hipMalloc((void **)&b.d_sref, 4 * n));
    HIPOK(hipMalloc((void **)&b.d_spos, 4 * n));
    HIPOK(hipMalloc((void **)&b.d_sqlen, 4 * n));
    HIPOK(hipMalloc((void **)&b.d_sfm, 4 * n));
    const samtext::Names nm{d_bytes.as<u8>(), d_off.as<u32>(), d_slot.as<int32_t>(), (u32)h.slot.size() - 1u};
    hipLaunchKernelGGL(k_sam_parse, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, b.stream, D, beg, b.d_nl, n, nm, b.d_sref, b.d_spos,
                       b.d_sqlen, b.d_sfm, d_err.as<unsigned long long>());
    HIPOK(hipGetLastError());
    unsigned long long fe = 0;
    HIPOK(hipMemcpyAsync(&fe, d_err.p, 8, hipMemcpyDeviceToHost, b.stream));
    HIPOK(hipStreamSynchronize(b.stream));
    b.t[5] = b.sam_parse_t = now_s() - t1;
    if (fe != ~0ull) return fail(PMX_DBAM_ERR_FORMAT, samtext::line_error(h, fe >> 8, (u32)(fe & 255u)));
    return 0;
}

}  // namespace

static int64_t dsam_decode(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, int32_t want_ref)
{
    const u64 n = b->sam_lines;
    b->n_kept = 0;
    b->n_records = n;
    if (n == 0) return 0;
    const double t0 = now_s();
    const u64 nb = (n + 255) / 256;
    if (!b->d_kept || nb > b->sam_nb_cap) {   // (the per-workgroup counts and bases; freed with the chain's tables)
        for (void *p : {(void *)b->d_kept, (void *)b->d_kept_base, (void *)b->d_totals})
            if (p) (void)hipFree(p);
        b->d_kept = nullptr;
        b->d_kept_base = b->d_totals = nullptr;
        b->sam_nb_cap = 0;
        HIPOK(hipMalloc((void **)&b->d_kept, 4 * nb));
        HIPOK(hipMalloc((void **)&b->d_kept_base, 8 * nb));
        HIPOK(hipMalloc((void **)&b->d_totals, 16));
        b->sam_nb_cap = nb;
    }
    hipLaunchKernelGGL(k_sam_keep, dim3((unsigned)nb), dim3(256), 0, b->stream, b->d_sref, b->d_sqlen, b->d_sfm, n, mapq_min, flag_exclude,
                       want_ref, b->d_kept);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, b->stream, b->d_kept, b->d_kept, nb, b->d_kept_base, b->d_totals);
    HIPOK(hipGetLastError());
    u64 totals[2] = {0, 0};
    HIPOK(hipMemcpyAsync(totals, b->d_totals, 16, hipMemcpyDeviceToHost, b->stream));
    HIPOK(hipStreamSynchronize(b->stream));
    if (totals[0] > b->out_cap) {
        for (void *p : {(void *)b->d_ref, (void *)b->d_pos, (void *)b->d_len, (void *)b->d_rev})
            if (p) (void)hipFree(p);
        b->d_ref = b->d_pos = b->d_len = nullptr;
        b->d_rev = nullptr;
        b->out_cap = 0;
        HIPOK(hipMalloc((void **)&b->d_ref, 4 * totals[0]));
        HIPOK(hipMalloc((void **)&b->d_pos, 4 * totals[0]));
        HIPOK(hipMalloc((void **)&b->d_len, 4 * totals[0]));
        HIPOK(hipMalloc((void **)&b->d_rev, totals[0]));
        b->out_cap = totals[0];
    }
    hipLaunchKernelGGL(k_sam_compact, dim3((unsigned)nb), dim3(256), 0, b->stream, b->d_sref, b->d_spos, b->d_sqlen, b->d_sfm, n, mapq_min,
                       flag_exclude, want_ref, b->d_kept_base, b->d_ref, b->d_pos, b->d_len, b->d_rev);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(b->stream));
    b->t[5] = b->sam_parse_t + (now_s() - t0);
    b->n_kept = totals[0];
    return (int64_t)b->n_kept;
}

static hipError_t dbed_launch_readlen(const pmx_dbam *b, int pass, const RlArgs &A);   // bed_reads_device.inc
static hipError_t dsam_launch_readlen(const pmx_dbam *b, int pass, const RlArgs &A)
{
    if (b->bed) return dbed_launch_readlen(b, pass, A);
    const u64 lanes = (b->sam_lines + SAM_RL_LINES - 1) / SAM_RL_LINES;
    const dim3 wg((unsigned)((lanes + 255) / 256));
    if (pass == 0)
        hipLaunchKernelGGL(k_sam_readlen<0>, wg, dim3(256), 0, b->stream, A, b->d_sref, b->d_sqlen, b->d_sfm, b->d_nl, b->data_beg,
                           b->sam_lines);
    else
        hipLaunchKernelGGL(k_sam_readlen<1>, wg, dim3(256), 0, b->stream, A, b->d_sref, b->d_sqlen, b->d_sfm, b->d_nl, b->data_beg,
                           b->sam_lines);
    return hipGetLastError();
}

extern "C" {

static int dsam_open_impl(const char *path, int device, int nthreads, pmx_dbam **out);
int pmx_dsam_open(const char *path, int device, int nthreads, pmx_dbam **out)
{
    try {
        return dsam_open_impl(path, device, nthreads, out);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dsam_open: ") + e.what());
    }
}
static int dsam_open_impl(const char *path, int device, int nthreads, pmx_dbam **out)
{
    if (!path || !out) return fail(PMX_DBAM_ERR_INVALID, "null argument");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMX_DBAM_ERR_DEVICE, "no HIP device: the device ingest needs a GPU");
    if (device < 0 || device >= ndev) return fail(PMX_DBAM_ERR_INVALID, "no such device");
    HIPOK(hipSetDevice(device));
    if (nthreads <= 0) nthreads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    // plain text or BGZF?
    u8 magic[4] = {0, 0, 0, 0};
    {
        OpenFile f;
        if (int rc = open_file(path, f)) return rc;
        if (f.size >= 4 && !pread_all(f.fd, magic, 0, 4, 1)) return fail(PMX_DBAM_ERR_OPEN, std::string("read error on ") + path);
    }
    const bool gz = magic[0] == 0x1f && magic[1] == 0x8b;
    if (gz && (magic[2] != 8 || !(magic[3] & 4)))
        return fail(PMX_DBAM_ERR_FORMAT, std::string(path) + ": gzip-compressed SAM that is not BGZF: recompress it with bgzip");
    pmx_dbam *b = new pmx_dbam;
    b->device = device;
    b->sam = true;
    b->pipelined = false;
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&b->kstream, hipStreamNonBlocking) != hipSuccess) {
        if (b->stream) (void)hipStreamDestroy(b->stream);
        delete b;
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    double t0 = now_s();
    int rc = gz ? read_and_upload(*b, path, nthreads) : sam_upload_plain(*b, path, nthreads);
    b->t[0] = now_s() - t0;
    if (!rc && gz) rc = inflate_all(*b);
    samtext::Header h;
    if (!rc) {
        t0 = now_s();
        rc = sam_header(*b, h);
        b->t[3] = now_s() - t0;
    }
    if (!rc) rc = sam_index_parse(*b, h);
    if (rc) {
        const std::string keep = g_err;
        pmx_dbam_close(b);
        g_err = keep.compare(0, strlen(path), path) == 0 ? keep : std::string(path) + ": " + keep;
        return rc;
    }
    b->npieces = 0;                     // (no record chain: the line table stands for it)
    *out = b;
    return 0;
}

}  // extern "C"
