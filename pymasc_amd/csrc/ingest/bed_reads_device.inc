// BED read files on the device (pmx_dbed_open, include/pymasc_amd_ingest.h; DESIGN.md 7.11).  Included at the end of
// bam_device.hip behind text_track_device.inc: the handle is a SAM handle (pmx_dbam, sam = true) whose table of records is in
// (reference, start) order, so decode / fetch / runs / readlen_hist / counters work on it through the SAM branches; only the
// histogram's launch differs (dbed_launch_readlen: each record's line start comes from a table of its own).
//
//   host          tt_upload (text_track_device.inc): plain text, BGZF (k_bgzf_inflate) or other gzip (zlib on the host)
//   k_sam_count / k_bam_scan / k_sam_lines   the line index, as for SAM text
//   k_bed_parse   one lane per line by the rules of io/bed_reads_parse.h (shared with the host reader, the checker): the SAM
//                 parse table (ref, pos1, qlen, flag | mapq << 16) and the sort key ref << 31 | start (a line without a read:
//                 nref << 31, behind every read); the first error by line (atomicMin), the first read line, the track lines
//   k_bed_check   one pass over the keys: out of order or not, the OR and the AND of every key (a digit whose bits agree in
//                 both is the same in every key: its radix pass is skipped), the number of reads
//   radix sort    stable LSD over 8-bit digits of the keys with the line index as payload, per pass that is not skipped:
//                 k_bed_rs_hist (digit counts of each tile of BED_RS_TILE keys) + k_bam_scan over (digit, tile) + k_bed_rs_scatter
//                 (ranks in a tile from 64-bit ballots and LDS, in item, wave, lane order = key order)
//   k_bed_gather  the table and the line starts in sorted order (only the reads); a file in order: the line starts only
// Every load of the text lies below its end rounded up to 16 bytes; the buffer holds 64 more bytes.  The line index, the keys
// and the sort buffers are freed at the end of the open.
#include "../io/bed_reads_parse.h"

#define BED_RS_ITEMS 32u                      // keys per lane of a sort tile
#define BED_RS_TILE (256u * BED_RS_ITEMS)

__global__ void __launch_bounds__(256) k_bed_parse(const u8 *__restrict__ D, const u64 *__restrict__ nl, u64 n, const samtext::Names nm,
                                                   u32 nref, int *__restrict__ o_ref, int *__restrict__ o_pos, u32 *__restrict__ o_qlen,
                                                   u32 *__restrict__ o_fm, u64 *__restrict__ o_key, unsigned long long *__restrict__ first_err,
                                                   unsigned long long *__restrict__ first_read, u32 *__restrict__ tracks,
                                                   u32 *__restrict__ ntracks, u32 track_cap)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 type = bedreads::L_SKIP;
    if (i < n) {
        DevSrc s{D, ~0ull, make_uint4(0, 0, 0, 0)};
        samtext::Rec r;
        r.ref = -1;
        r.pos1 = 0;
        r.qlen = 0;
        r.flag = r.mapq = 0;
        const u32 e = bedreads::parse_line(s, i ? nl[i - 1] + 1u : 0ull, nl[i], nm, type, r);
        if (e) {
            atomicMin(first_err, (unsigned long long)((i << 8) | e));
            r.ref = -1;
        }
        if (type == bedreads::L_TRACK) {
            const u32 j = atomicAdd(ntracks, 1u);
            if (j < track_cap) tracks[j] = (u32)i;
        }
        o_ref[i] = r.ref;
        o_pos[i] = r.pos1;
        o_qlen[i] = r.qlen;
        o_fm[i] = r.flag | (r.mapq << 16);
        o_key[i] = bedreads::sort_key(r.ref, r.pos1, nref);
    }
    const u64 m = __ballot(type == bedreads::L_READ);
    if ((threadIdx.x & 63u) == 0 && m) atomicMin(first_read, (unsigned long long)(i + (u64)(__ffsll((long long)m) - 1)));
}

// out[0] |= 1 when a key is below its predecessor; out[1] = OR of the keys; out[2] = AND of the keys; out[3] += reads
__global__ void __launch_bounds__(256) k_bed_check(const u64 *__restrict__ key, u64 n, u64 none, unsigned long long *__restrict__ out)
{
    __shared__ unsigned long long s[4][4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 i = (u64)blockIdx.x * 256u + t;
    u64 desc = 0, o = 0, a = ~0ull, r = 0;
    if (i < n) {
        const u64 k = key[i];
        desc = (i > 0 && k < key[i - 1]) ? 1u : 0u;
        o = a = k;
        r = k < none ? 1u : 0u;
    }
    for (int d = 32; d > 0; d >>= 1) {
        desc |= __shfl_xor(desc, d, 64);
        o |= __shfl_xor(o, d, 64);
        a &= __shfl_xor(a, d, 64);
        r += __shfl_xor(r, d, 64);
    }
    if (lane == 0) {
        s[wave][0] = desc;
        s[wave][1] = o;
        s[wave][2] = a;
        s[wave][3] = r;
    }
    __syncthreads();
    if (t == 0) {
        for (u32 w = 1; w < 4u; w++) {
            desc |= s[w][0];
            o |= s[w][1];
            a &= s[w][2];
            r += s[w][3];
        }
        if (desc) atomicOr(&out[0], 1ull);
        atomicOr(&out[1], (unsigned long long)o);
        atomicAnd(&out[2], (unsigned long long)a);
        if (r) atomicAdd(&out[3], (unsigned long long)r);
    }
}

// cnt[digit * ntiles + tile] = keys of the tile whose digit at `shift` is `digit`
__global__ void __launch_bounds__(256) k_bed_rs_hist(const u64 *__restrict__ key, u64 n, u32 shift, u32 ntiles, u32 *__restrict__ cnt)
{
    __shared__ u32 s_h[256];
    const u32 t = threadIdx.x;
    s_h[t] = 0;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * BED_RS_TILE;
    for (u32 it = 0; it < BED_RS_ITEMS; it++) {
        const u64 i = base + (u64)it * 256u + t;
        if (i < n) atomicAdd(&s_h[(u32)(key[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    cnt[(u64)t * ntiles + blockIdx.x] = s_h[t];
}

// The stable scatter of one pass: key i of the tile goes to base[digit * ntiles + tile] + its rank among the tile's keys of that
// digit, ranks counted in (item, wave, lane) order, which is the keys' order.  val_in null: the payload is the key's index.
__global__ void __launch_bounds__(256) k_bed_rs_scatter(const u64 *__restrict__ key_in, const u32 *__restrict__ val_in, u64 n, u32 shift,
                                                        u32 ntiles, const u64 *__restrict__ base, u64 *__restrict__ key_out,
                                                        u32 *__restrict__ val_out)
{
    __shared__ u32 s_run[256];        // keys of each digit placed so far by this tile
    __shared__ u32 s_wc[4][256];      // this item's keys per wave and digit
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    s_run[t] = 0;
    for (u32 w = 0; w < 4u; w++) s_wc[w][t] = 0;
    const u64 tile0 = (u64)blockIdx.x * BED_RS_TILE;
    const u64 below_me = (1ull << lane) - 1ull;
    for (u32 it = 0; it < BED_RS_ITEMS; it++) {
        const u64 i = tile0 + (u64)it * 256u + t;
        const bool valid = i < n;
        const u64 k = valid ? key_in[i] : 0ull;
        const u32 v = valid ? (val_in ? val_in[i] : (u32)i) : 0u;
        const u32 d = (u32)(k >> shift) & 255u;
        u64 peers = __ballot(valid);                       // the lanes of this wave with the same digit
#pragma unroll
        for (u32 bit = 0; bit < 8u; bit++) {
            const u64 m = __ballot((d >> bit) & 1u);
            peers &= ((d >> bit) & 1u) ? m : ~m;
        }
        const u32 rank = (u32)__popcll(peers & below_me);
        __syncthreads();                                   // (the last item's s_run / s_wc updates are done)
        if (valid && rank == 0) s_wc[wave][d] = (u32)__popcll(peers);
        __syncthreads();
        if (valid) {
            u32 r = s_run[d] + rank;
            for (u32 w = 0; w < wave; w++) r += s_wc[w][d];
            const u64 dst = base[(u64)d * ntiles + blockIdx.x] + r;
            key_out[dst] = k;
            val_out[dst] = v;
        }
        __syncthreads();
        s_run[t] += s_wc[0][t] + s_wc[1][t] + s_wc[2][t] + s_wc[3][t];
        for (u32 w = 0; w < 4u; w++) s_wc[w][t] = 0;
    }
}

// Row r of the sorted table: line idx[r] (idx null: line r, the table stays as it is); its line start into ls[r]
__global__ void __launch_bounds__(256) k_bed_gather(const u32 *__restrict__ idx, u64 nrows, const u64 *__restrict__ nl,
                                                    const int *__restrict__ ref, const int *__restrict__ pos, const u32 *__restrict__ qlen,
                                                    const u32 *__restrict__ fm, int *__restrict__ o_ref, int *__restrict__ o_pos,
                                                    u32 *__restrict__ o_qlen, u32 *__restrict__ o_fm, u64 *__restrict__ ls)
{
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= nrows) return;
    const u64 j = idx ? (u64)idx[r] : r;
    ls[r] = j ? nl[j - 1] + 1u : 0ull;
    if (idx) {
        o_ref[r] = ref[j];
        o_pos[r] = pos[j];
        o_qlen[r] = qlen[j];
        o_fm[r] = fm[j];
    }
}

// k_sam_readlen over the sorted table: the first-occurrence key is the line start of the record, the smallest of a run
template <int PASS>
__global__ void __launch_bounds__(256) k_bed_readlen(const RlArgs A, const u32 *__restrict__ qlen, const u32 *__restrict__ fm,
                                                     const u64 *__restrict__ ls, u64 nrec)
{
    readlen_lane<PASS, true>(A, [&](auto add) {
        const u64 lo = ((u64)blockIdx.x * 256u + threadIdx.x) * SAM_RL_LINES;
        const u64 hi = lo + SAM_RL_LINES < nrec ? lo + SAM_RL_LINES : nrec;
        for (u64 i = lo; i < hi; i++)
            add(fm[i] & 0xffffu, fm[i] >> 16, [&]() { return qlen[i]; }, [&]() { return A.base + ls[i]; });
    });
}

static hipError_t dbed_launch_readlen(const pmx_dbam *b, int pass, const RlArgs &A)
{
    const u64 lanes = (b->sam_lines + SAM_RL_LINES - 1) / SAM_RL_LINES;
    const dim3 wg((unsigned)((lanes + 255) / 256));
    if (pass == 0)
        hipLaunchKernelGGL(k_bed_readlen<0>, wg, dim3(256), 0, b->stream, A, b->d_sqlen, b->d_sfm, b->d_ls, b->sam_lines);
    else
        hipLaunchKernelGGL(k_bed_readlen<1>, wg, dim3(256), 0, b->stream, A, b->d_sqlen, b->d_sfm, b->d_ls, b->sam_lines);
    return hipGetLastError();
}

namespace {

// The text in HBM (b.d_out, b.N) -> b's table of reads in (reference, start) order and their line starts (b.d_ls)
int bed_index_parse_sort(pmx_dbam &b)
{
    hipStream_t st = b.stream;
    const u8 *D = b.d_out;
    const u64 N = b.N;
    const u32 nref = (u32)b.ref_names.size();
    b.sam_lines = 0;
    if (N == 0) return 0;
    double t0 = now_s();
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
    double t1 = now_s();
    b.t[4] = t1 - t0;
    // the name table of the sizes
    std::vector<u8> bytes;
    std::vector<u32> off;
    std::vector<int32_t> slot;
    bedreads::name_table(b.ref_names, bytes, off, slot);
    u8 *d_bytes;
    u32 *d_off;
    int32_t *d_slot;
    if (int rc = t.get(&d_bytes, bytes.size())) return rc;
    if (int rc = t.get(&d_off, 4 * off.size())) return rc;
    if (int rc = t.get(&d_slot, 4 * slot.size())) return rc;
    if (!bytes.empty()) HIPOK(hipMemcpyAsync(d_bytes, bytes.data(), bytes.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_off, off.data(), 4 * off.size(), hipMemcpyHostToDevice, st));
    HIPOK(hipMemcpyAsync(d_slot, slot.data(), 4 * slot.size(), hipMemcpyHostToDevice, st));
    const samtext::Names nm{d_bytes, d_off, d_slot, (u32)slot.size() - 1u};
    // the parse: the table of every line and its key
    HIPOK(hipMalloc((void **)&b.d_sref, 4 * n));      // (the handle's: a file in order keeps this table)
    HIPOK(hipMalloc((void **)&b.d_spos, 4 * n));
    HIPOK(hipMalloc((void **)&b.d_sqlen, 4 * n));
    HIPOK(hipMalloc((void **)&b.d_sfm, 4 * n));
    int *d_ref = b.d_sref, *d_pos = b.d_spos;
    u32 *d_qlen = b.d_sqlen, *d_fm = b.d_sfm, *d_ntr, *d_tracks = nullptr;
    u64 *d_key;
    unsigned long long *d_err;                    // [0] first error, [1] first read line
    if (int rc = t.get(&d_key, 8 * n)) return rc;
    if (int rc = t.get(&d_err, 16)) return rc;
    if (int rc = t.get(&d_ntr, 4)) return rc;
    const u64 nb = (n + 255) / 256;
    u32 track_cap = 256, ntr = 0;
    for (int pass = 0; pass < 2; pass++) {        // (a second pass only when the track lines did not fit)
        if (int rc = t.get(&d_tracks, 4 * track_cap)) return rc;
        HIPOK(hipMemsetAsync(d_err, 0xff, 16, st));
        HIPOK(hipMemsetAsync(d_ntr, 0, 4, st));
        hipLaunchKernelGGL(k_bed_parse, dim3((unsigned)nb), dim3(256), 0, st, D, d_nl, n, nm, nref, d_ref, d_pos, d_qlen, d_fm, d_key,
                           d_err, d_err + 1, d_tracks, d_ntr, track_cap);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&ntr, d_ntr, 4, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (ntr <= track_cap) break;
        track_cap = ntr;
    }
    unsigned long long fe[2] = {0, 0};
    std::vector<u32> tr32(ntr);
    HIPOK(hipMemcpyAsync(fe, d_err, 16, hipMemcpyDeviceToHost, st));
    if (ntr) HIPOK(hipMemcpyAsync(tr32.data(), d_tracks, 4 * (u64)ntr, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    {
        std::vector<u64> tr(tr32.begin(), tr32.end());
        std::sort(tr.begin(), tr.end());
        u64 tline = 0;
        if (const u32 tc = bedreads::track_error(tr, fe[1], tline))
            if ((tline << 8 | tc) < fe[0]) fe[0] = tline << 8 | tc;
    }
    if (fe[0] != ~0ull) return fail(PMX_DBAM_ERR_FORMAT, bedreads::line_error(fe[0] >> 8, (u32)(fe[0] & 255u)));
    // in order already?  which digits differ between keys?
    const u64 none = (u64)nref << 31;
    unsigned long long chk[4] = {0, 0, ~0ull, 0};
    unsigned long long *d_chk;
    if (int rc = t.get(&d_chk, 32)) return rc;
    HIPOK(hipMemcpyAsync(d_chk, chk, 32, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_bed_check, dim3((unsigned)nb), dim3(256), 0, st, d_key, n, none, d_chk);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(chk, d_chk, 32, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    const bool sorted = chk[0] == 0;
    const u64 reads = chk[3];
    const u64 differ = chk[1] ^ chk[2];
    HIPOK(hipMalloc((void **)&b.d_ls, 8 * std::max<u64>(reads, 1)));
    const u64 gb = (std::max<u64>(reads, 1) + 255) / 256;
    if (sorted) {                                 // the table as it is: its reads come first, the other lines behind them
        hipLaunchKernelGGL(k_bed_gather, dim3((unsigned)gb), dim3(256), 0, st, (const u32 *)nullptr, reads, d_nl, d_ref, d_pos, d_qlen,
                           d_fm, (int *)nullptr, (int *)nullptr, (u32 *)nullptr, (u32 *)nullptr, b.d_ls);
        HIPOK(hipGetLastError());
    } else {
        const u32 ntiles = (u32)((n + BED_RS_TILE - 1) / BED_RS_TILE);
        const u64 ncnt = 256ull * ntiles;
        u64 *d_k2, *d_base, *d_tot2;
        u32 *d_v1, *d_v2, *d_cnt;
        if (int rc = t.get(&d_k2, 8 * n)) return rc;
        if (int rc = t.get(&d_v1, 4 * n)) return rc;
        if (int rc = t.get(&d_v2, 4 * n)) return rc;
        if (int rc = t.get(&d_cnt, 4 * ncnt)) return rc;
        if (int rc = t.get(&d_base, 8 * ncnt)) return rc;
        if (int rc = t.get(&d_tot2, 16)) return rc;
        u64 *kin = d_key, *kout = d_k2;
        u32 *vin = nullptr, *vout = d_v1;
        for (u32 dig = 0; dig < 8u; dig++) {
            const u32 shift = 8u * dig;
            if (((differ >> shift) & 255u) == 0) continue;      // the same digit in every key: the pass would move nothing
            hipLaunchKernelGGL(k_bed_rs_hist, dim3(ntiles), dim3(256), 0, st, kin, n, shift, ntiles, d_cnt);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_cnt, d_cnt, ncnt, d_base, d_tot2);
            HIPOK(hipGetLastError());
            hipLaunchKernelGGL(k_bed_rs_scatter, dim3(ntiles), dim3(256), 0, st, kin, vin, n, shift, ntiles, d_base, kout, vout);
            HIPOK(hipGetLastError());
            std::swap(kin, kout);
            vin = vout;
            vout = vout == d_v1 ? d_v2 : d_v1;
        }
        DevAlloc g_ref, g_pos, g_qlen, g_fm;      // the sorted table; the one in line order is freed with them below
        HIPOK(hipMalloc(&g_ref.p, 4 * std::max<u64>(reads, 1)));
        HIPOK(hipMalloc(&g_pos.p, 4 * std::max<u64>(reads, 1)));
        HIPOK(hipMalloc(&g_qlen.p, 4 * std::max<u64>(reads, 1)));
        HIPOK(hipMalloc(&g_fm.p, 4 * std::max<u64>(reads, 1)));
        hipLaunchKernelGGL(k_bed_gather, dim3((unsigned)gb), dim3(256), 0, st, vin, reads, d_nl, d_ref, d_pos, d_qlen, d_fm,
                           g_ref.as<int>(), g_pos.as<int>(), g_qlen.as<u32>(), g_fm.as<u32>(), b.d_ls);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(st));
        int *o_ref = b.d_sref, *o_pos = b.d_spos;
        u32 *o_qlen = b.d_sqlen, *o_fm = b.d_sfm;
        b.d_sref = g_ref.as<int>();
        b.d_spos = g_pos.as<int>();
        b.d_sqlen = g_qlen.as<u32>();
        b.d_sfm = g_fm.as<u32>();
        g_ref.p = o_ref;
        g_pos.p = o_pos;
        g_qlen.p = o_qlen;
        g_fm.p = o_fm;
    }
    HIPOK(hipStreamSynchronize(st));
    b.sam_lines = reads;
    b.t[5] = b.sam_parse_t = now_s() - t1;
    return 0;
}

}  // namespace

extern "C" {

static int dbed_open_impl(const char *path, int device, int nthreads, int32_t nref, const char *const *names, const int64_t *lengths,
                          pmx_dbam **out);
int pmx_dbed_open(const char *path, int device, int nthreads, int32_t nref, const char *const *names, const int64_t *lengths,
                  pmx_dbam **out)
{
    try {
        return dbed_open_impl(path, device, nthreads, nref, names, lengths, out);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dbed_open: ") + e.what());
    }
}
static int dbed_open_impl(const char *path, int device, int nthreads, int32_t nref, const char *const *names, const int64_t *lengths,
                          pmx_dbam **out)
{
    if (!path || !out) return fail(PMX_DBAM_ERR_INVALID, "null argument");
    *out = nullptr;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;
    const std::string why = bedreads::check_sizes(nref, names, lengths, ref_names, ref_lens);
    if (!why.empty()) return fail(PMX_DBAM_ERR_INVALID, std::string(path) + ": " + why);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMX_DBAM_ERR_DEVICE, "no HIP device: the device ingest needs a GPU");
    if (device < 0 || device >= ndev) return fail(PMX_DBAM_ERR_INVALID, "no such device");
    HIPOK(hipSetDevice(device));
    if (nthreads <= 0) nthreads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    pmx_dbam *b = new pmx_dbam;
    b->device = device;
    b->sam = true;
    b->bed = true;
    b->pipelined = false;
    b->ref_names = std::move(ref_names);
    b->ref_lens = std::move(ref_lens);
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&b->kstream, hipStreamNonBlocking) != hipSuccess) {
        pmx_dbam_close(b);
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    double t0 = now_s();
    int rc = 0;
    {
        OpenFile f;
        rc = open_file(path, f);
        if (!rc) b->fsize = f.size;
        if (!rc && f.size == 0) rc = fail(PMX_DBAM_ERR_FORMAT, "empty file");     // (the host reader's words)
    }
    if (!rc) rc = tt_upload(path, device, nthreads, &b->d_out, &b->N);
    b->t[0] = now_s() - t0;
    if (!rc) rc = bed_index_parse_sort(*b);
    if (rc) {
        const std::string keep = g_err;
        pmx_dbam_close(b);
        g_err = keep.compare(0, strlen(path), path) == 0 ? keep : std::string(path) + ": " + keep;
        return rc;
    }
    b->npieces = 0;                     // (no record chain: the sorted table stands for it)
    *out = b;
    return 0;
}

}  // extern "C"
