// A DEFLATE encoder on the device (pmx_ddeflate, pmx_dbam_coverage_sections_z / _zoom_records_z, include/pymasc_amd_ingest.h;
// DESIGN.md 7.18.2).  Included in bam_device.hip behind coverage_device.inc.  Independent chunks of at most PMX_DEFLATE_MAX_CHUNK
// bytes each become one zlib stream (RFC 1950 around RFC 1951): the sections of a bigWig file, compressed where they were made.
//
//   k_df_deflate<NB, HB, SB>   one workgroup per chunk of at most 2^NB bytes, the chunk in LDS (zeros behind its end):
//     stage     the bytes, and the two Adler-32 sums as k_bw_adler takes them (A = 1 + sum d_i, B = n + sum (n - i) d_i), reduced
//               over the wave and the four waves
//     match     256 positions at a time in position order.  A position's candidate is the nearest earlier position with the same
//               next four bytes inside its wave (ballots over the distinct values), else the nearest earlier position with the same
//               hash of them: s_head[hash] holds the largest position + 1 seen, read and then raised (atomicMax) wave by wave
//               between barriers, so what a lane reads is every earlier wave's positions and nothing of its own or a later one.
//               Every lane extends its own candidate four bytes at a time, up to 258; a match has length >= 4 and distance
//               <= 32768.  Nothing depends on the order lanes arrive in: the same bytes give the same table.
//     parse     greedy, one lane, over the table of 2^SB positions just made (match or literal, one LDS read per token); the
//               tokens go to the chunk's place in `tok` (4 bytes per token, at most one per byte)
//     count     the tokens' literal / length and distance symbols by LDS atomics
//     lengths   the used symbols ranked by (count, symbol) in parallel; one lane merges them (df_lengths: 15 bits, then 7 for
//               the code-length alphabet), makes the canonical codes and the header's sequence, and takes the exact size of the
//               dynamic, the fixed and the stored form: the smallest is written (stored on a tie, then fixed)
//     emit      256 tokens per trip: code and extra bits of a token in one 64-bit value, their lengths scanned over the wave
//               (cv_wave_scan) and the waves, the bits OR-ed into LDS words (the stream lies where the chunk lay: the tokens hold
//               the literals); the Adler-32 big-endian behind the last byte; 4-byte stores into the chunk's slot.  A stored stream
//               is written from the chunk itself, in blocks of at most 65535 bytes.
//   k_bam_scan  the exclusive prefix of the streams' sizes
//   k_df_pack   one workgroup per chunk: its stream from its slot to its place among the others
// Device memory inside a call: the raw bytes (pmx_ddeflate; the coverage calls compress what k_tr_sections / k_tr_zoom_emit wrote),
// 4 bytes per raw byte of tokens, a slot of pmx_ddeflate_bound rounded up to 16 per chunk, 36 per chunk of tables, then the packed
// streams.  LDS per workgroup: 37 / 62 / 119 KB for chunks up to 16 / 32 / 64 KB, so 4 / 2 / 1 workgroups per CU.

#include "deflate_codes.inc"

#define DF_MAX PMX_DEFLATE_MAX_CHUNK
#define DF_MATCH 0x80000000u            // a token that is a match: DF_MATCH | (distance - 1) << 8 | (length - 3); else the literal
#define DF_STORED_BLOCK 65535u

namespace {
struct DfJob {          // a chunk: its first byte in the raw bytes (and its first token in `tok`), its slot, its length
    u64 off, slot;
    u32 n, pad;
};
}  // namespace

// the four bytes at byte a of words[]
__device__ __forceinline__ u32 df_ld32(const u32 *words, u32 a)
{
    const u64 two = ((u64)words[(a >> 2) + 1u] << 32) | words[a >> 2];
    return (u32)(two >> (8u * (a & 3u)));
}

// `bits` (at most 48 of them) into the stream at bit `at`
__device__ __forceinline__ void df_put(u32 *out, u32 at, u64 bits)
{
    const u32 sh = at & 31u;
    u32 *p = out + (at >> 5);
    const u32 a = (u32)(bits << sh);
    const u64 rest = bits >> (32u - sh);
    if (a) atomicOr(p, a);
    if ((u32)rest) atomicOr(p + 1, (u32)rest);
    if (rest >> 32) atomicOr(p + 2, (u32)(rest >> 32));
}

template <u32 NB, u32 HB, u32 SB>
__global__ void __launch_bounds__(256) k_df_deflate(const u8 *__restrict__ src, const DfJob *__restrict__ jobs, const u32 *__restrict__ list,
                                                    u8 *__restrict__ slots, u32 *__restrict__ tok, u32 *__restrict__ sizes)
{
    constexpr u32 NMAX = 1u << NB, SEG = 1u << SB;
    static_assert(SEG % 256u == 0 && (4u << HB) >= 8u * DF_NODES, "the work arrays of df_lengths lie in s_head");
    __shared__ u32 s_in[NMAX / 4 + 16];             // the chunk, zeros behind its end; then the stream
    __shared__ u32 s_head[1u << HB];                // per hash: the largest position + 1 so far; then the work arrays of df_lengths
    __shared__ u32 s_mt[SEG];                       // per position of the segment: its token, should the parse stop there
    __shared__ u32 s_llf[288], s_df[32], s_llt[288], s_dt[32], s_clf[DF_CL], s_clt[DF_CL];
    __shared__ u16 s_order[288], s_dorder[32], s_seq[320];
    __shared__ u8 s_len[320], s_dlen[32], s_cll[DF_CL];
    __shared__ u64 s_red[8];
    __shared__ u32 s_scan[4], s_var[8];             // [0] Adler-32, [1] tokens, [2] / [3] used symbols, [4] mode, [5] bits, [6] bytes
    const u32 t = threadIdx.x, lane = t & 63u, w = t >> 6, chunk = list[blockIdx.x];
    const DfJob J = jobs[chunk];
    const u32 n = J.n;
    const u8 *in = src + J.off;
    u32 *mytok = tok + J.off;
    u8 *slot = slots + J.slot;
    const u8 *s_bytes = (const u8 *)s_in;

    // stage
    {
        const bool aligned = ((u64)in & 3u) == 0;
        u64 a = 0, b = 0;
        for (u32 j = t; j < (n + 3u) / 4u + 4u; j += 256u) {
            u32 x = 0;
            if (aligned && 4u * j + 4u <= n) {
                x = *reinterpret_cast<const u32 *>(in + 4u * j);
            } else {
                for (u32 k = 0; k < 4u; k++)
                    if (4u * j + k < n) x |= (u32)in[4u * j + k] << (8u * k);
            }
            s_in[j] = x;
            for (u32 k = 0; k < 4u; k++) {
                const u64 d = (x >> (8u * k)) & 255u;       // (zero behind the end)
                a += d;
                b += (u64)(n - (4u * j + k)) * d;
            }
        }
        for (u32 j = t; j < (1u << HB); j += 256u) s_head[j] = 0;
        for (u32 j = t; j < 288u; j += 256u) s_llf[j] = 0;
        if (t < 32u) s_df[t] = 0;
        if (t < 8u) s_var[t] = 0;
        a = cx_wave_sum(a);
        b = cx_wave_sum(b);
        if (lane == 0) {
            s_red[w] = a;
            s_red[4u + w] = b;
        }
        __syncthreads();
        if (t == 0) {
            const u64 A = 1u + s_red[0] + s_red[1] + s_red[2] + s_red[3], B = n + s_red[4] + s_red[5] + s_red[6] + s_red[7];
            s_var[0] = ((u32)(B % 65521u) << 16) | (u32)(A % 65521u);
        }
    }

    // match and parse, a segment at a time
    u32 ntok = 0, at = 0;                           // (thread 0) tokens so far; where the next token begins
    const u64 below = (1ull << lane) - 1ull;
    for (u32 seg = 0; seg < n; seg += SEG) {
        const u32 segend = seg + SEG < n ? seg + SEG : n;
        for (u32 base = seg; base < segend; base += 256u) {
            const u32 p = base + t;
            const bool valid = p + 4u <= n;
            const u32 v = valid ? df_ld32(s_in, p) : 0u;
            u32 near = 64u;                         // the nearest lower lane with the same four bytes
            for (u64 todo = __ballot(valid); todo;) {
                const u32 x = (u32)__shfl((int)v, __ffsll((unsigned long long)todo) - 1, 64);
                const u64 m = __ballot(valid && v == x);
                if (valid && v == x) {
                    const u64 e = m & below;
                    near = e ? 63u - (u32)__clzll((long long)e) : 64u;
                }
                todo &= ~m;
            }
            const u32 h = (v * 2654435761u) >> (32u - HB);
            u32 c0 = 0;
            for (u32 k = 0; k < 4u; k++) {
                if (w == k && valid) {
                    c0 = s_head[h];
                    atomicMax(&s_head[h], p + 1u);
                }
                __syncthreads();
            }
            u32 entry = p < n ? s_bytes[p] : 0u;
            if (valid && (near < 64u || c0)) {
                const u32 c = near < 64u ? p - (lane - near) : c0 - 1u;
                const u32 most = n - p < 258u ? n - p : 258u;
                if (p - c <= 32768u) {
                    u32 len = 0;
                    while (len < most) {
                        const u32 x = df_ld32(s_in, p + len) ^ df_ld32(s_in, c + len);
                        if (x) {
                            len += (u32)__builtin_ctz(x) >> 3;
                            break;
                        }
                        len += 4u;
                    }
                    len = len < most ? len : most;
                    if (len >= 4u) entry = DF_MATCH | (p - c - 1u) << 8 | (len - 3u);
                }
            }
            if (p < segend) s_mt[p - seg] = entry;
        }
        __syncthreads();
        if (t == 0) {
            while (at < segend) {
                const u32 e = s_mt[at - seg];
                mytok[ntok++] = e;
                at += e & DF_MATCH ? (e & 255u) + 3u : 1u;
            }
        }
        __syncthreads();
    }
    if (t == 0) s_var[1] = ntok;
    __threadfence_block();
    __syncthreads();
    ntok = s_var[1];

    // count
    for (u32 i = t; i < ntok; i += 256u) {
        const u32 e = mytok[i];
        if (e & DF_MATCH) {
            u32 sym, nb, ex;
            df_len_code((e & 255u) + 3u, sym, nb, ex);
            atomicAdd(&s_llf[sym], 1u);
            df_dist_code(((e >> 8) & 0x7fffu) + 1u, sym, nb, ex);
            atomicAdd(&s_df[sym], 1u);
        } else {
            atomicAdd(&s_llf[e], 1u);
        }
    }
    if (t == 0) atomicAdd(&s_llf[256], 1u);
    for (u32 j = t; j < 320u; j += 256u) s_len[j] = 0;
    if (t < 32u) s_dlen[t] = 0;
    __syncthreads();

    // lengths: the used symbols in (count, symbol) order, then one lane
    for (u32 s = t; s < DF_LL + DF_D; s += 256u) {
        const bool ll = s < DF_LL;
        const u32 *f = ll ? s_llf : s_df;
        const u32 me = ll ? s : s - DF_LL, cnt = ll ? DF_LL : DF_D, mine = f[me];
        if (!mine) continue;
        u32 rank = 0;
        for (u32 o = 0; o < cnt; o++) rank += f[o] && (f[o] < mine || (f[o] == mine && o < me));
        (ll ? s_order : s_dorder)[rank] = (u16)me;
        atomicAdd(&s_var[ll ? 2 : 3], 1u);
    }
    __syncthreads();
    if (t == 0) {
        u32 *node = s_head;
        u16 *up = (u16 *)(s_head + DF_NODES), *dep = up + DF_NODES;
        const u32 mll = s_var[2], md = s_var[3];
        df_lengths(s_llf, s_order, mll, 15u, s_len, node, up, dep);
        if (mll == 1u) s_len[0] = 1;                // (the end-of-block symbol alone, n == 0: a second code completes the set)
        df_lengths(s_df, s_dorder, md, 15u, s_dlen, node, up, dep);
        if (md == 0) s_dlen[0] = 1;                 // (no match at all: one distance code must still be declared)
        u32 hlit = DF_LL, hdist = DF_D;
        while (hlit > 257u && s_len[hlit - 1u] == 0) hlit--;
        while (hdist > 1u && s_dlen[hdist - 1u] == 0) hdist--;
        u32 data = 0, fixed = 0;                    // the bits of the tokens and the end-of-block symbol under the two codes
        for (u32 s = 0; s < DF_LL; s++) {
            const u32 x = s >= 257u ? df_len_extra_bits(s) : 0u;
            data += s_llf[s] * (s_len[s] + x);
            fixed += s_llf[s] * (df_fixed_len(s) + x);
        }
        for (u32 s = 0; s < DF_D; s++) {
            data += s_df[s] * (s_dlen[s] + df_dist_extra_bits(s));
            fixed += s_df[s] * (5u + df_dist_extra_bits(s));
        }
        df_codes(s_len, DF_LL, s_llt);
        df_codes(s_dlen, DF_D, s_dt);
        for (u32 s = 0; s < hdist; s++) s_len[hlit + s] = s_dlen[s];
        const u32 nseq = df_header_seq(s_len, hlit + hdist, s_seq, s_clf);
        df_cl_lengths(s_clf, s_cll, s_order, node, up, dep);
        df_codes(s_cll, DF_CL, s_clt);
        const u32 hclen = df_hclen(s_cll);
        const u32 blocks = n > DF_STORED_BLOCK ? (n + DF_STORED_BLOCK - 1u) / DF_STORED_BLOCK : 1u;
        const u32 dyn = 3u + df_header_bits(hclen, s_clf, s_cll) + data, fix = 3u + fixed, stored = 8u * (n + 5u * blocks);
        const u32 mode = stored <= dyn && stored <= fix ? 0u : fix <= dyn ? 1u : 2u;
        const u32 bits = mode == 0 ? stored : mode == 1u ? fix : dyn;
        s_var[4] = mode;
        s_var[6] = 2u + (bits + 7u) / 8u + 4u;
        s_var[2] = hlit | hdist << 10 | hclen << 16;
        s_var[3] = nseq;
    }
    __syncthreads();
    const u32 mode = s_var[4], bytes = s_var[6], adler = s_var[0];
    if (t == 0) sizes[chunk] = bytes;

    if (mode == 0) {                                // stored: 0x78 0x01, the blocks (final?, LEN, ~LEN, bytes), the Adler-32
        const u32 blocks = n > DF_STORED_BLOCK ? (n + DF_STORED_BLOCK - 1u) / DF_STORED_BLOCK : 1u;
        for (u32 i = t; i < bytes; i += 256u) {
            u32 x;
            if (i < 2u) {
                x = i ? 0x01u : 0x78u;
            } else if (i >= bytes - 4u) {
                x = adler >> (8u * (bytes - 1u - i));
            } else {
                const u32 k = (i - 2u) / (DF_STORED_BLOCK + 5u), r = (i - 2u) % (DF_STORED_BLOCK + 5u);
                const u32 len = n - k * DF_STORED_BLOCK < DF_STORED_BLOCK ? n - k * DF_STORED_BLOCK : DF_STORED_BLOCK;
                x = r == 0 ? (k + 1u == blocks) : r == 1u ? len : r == 2u ? len >> 8 : r == 3u ? ~len : r == 4u ? ~len >> 8
                                                                                                           : s_bytes[k * DF_STORED_BLOCK + r - 5u];
            }
            slot[i] = (u8)x;
        }
        return;
    }

    // emit: the stream takes the chunk's place
    const u32 words = (bytes + 3u) / 4u;
    for (u32 j = t; j < words + 2u; j += 256u) s_in[j] = 0;
    if (mode == 1u) {
        for (u32 s = t; s < 288u; s += 256u) {
            const u32 l = df_fixed_len(s), code = s < 144u ? 0x30u + s : s < 256u ? 0x190u + (s - 144u) : s < 280u ? s - 256u : 0xc0u + (s - 280u);
            s_llt[s] = l << 16 | df_reverse(code, l);
        }
        if (t < 32u) s_dt[t] = 5u << 16 | df_reverse(t, 5u);
    }
    __syncthreads();
    if (t == 0) {
        u32 o = 0;
        auto put = [&](u32 value, u32 nbits) {
            df_put(s_in, o, value);
            o += nbits;
        };
        put(0x9c78u, 16u);
        put(1u, 1u);
        put(mode, 2u);
        if (mode == 2u) df_header_write(put, s_var[2] & 1023u, (s_var[2] >> 10) & 63u, s_var[2] >> 16, s_cll, s_clt, s_seq, s_var[3]);
        s_var[5] = o;
    }
    __syncthreads();
    u32 run = s_var[5];
    for (u32 first = 0; first <= ntok; first += 256u) {     // token ntok is the end of the block
        const u32 i = first + t;
        u64 bits = 0;
        u32 nb = 0;
        if (i < ntok) {
            const u32 e = mytok[i];
            if (e & DF_MATCH) {
                u32 sym, xb, ex;
                df_len_code((e & 255u) + 3u, sym, xb, ex);
                const u32 lc = s_llt[sym];
                bits = (lc & 0xffffu) | (u64)ex << (lc >> 16);
                nb = (lc >> 16) + xb;
                df_dist_code(((e >> 8) & 0x7fffu) + 1u, sym, xb, ex);
                const u32 dc = s_dt[sym];
                bits |= (u64)(dc & 0xffffu) << nb;
                nb += dc >> 16;
                bits |= (u64)ex << nb;
                nb += xb;
            } else {
                bits = s_llt[e] & 0xffffu;
                nb = s_llt[e] >> 16;
            }
        } else if (i == ntok) {
            bits = s_llt[256] & 0xffffu;
            nb = s_llt[256] >> 16;
        }
        const u32 incl = cv_wave_scan(nb, lane);
        if (lane == 63u) s_scan[w] = incl;
        __syncthreads();
        u32 o = run + incl - nb;
        for (u32 x = 0; x < w; x++) o += s_scan[x];
        if (nb) df_put(s_in, o, bits);
        run += s_scan[0] + s_scan[1] + s_scan[2] + s_scan[3];
        __syncthreads();
    }
    if (t == 0) df_put(s_in, (run + 7u) & ~7u, (u64)__builtin_bswap32(adler));       // (big-endian; run + 7 >> 3 == bytes - 4)
    __syncthreads();
    for (u32 j = t; j < words; j += 256u) reinterpret_cast<u32 *>(slot)[j] = s_in[j];   // (a slot begins on a multiple of 16 and has room for the last word)
}

__global__ void __launch_bounds__(256) k_df_pack(const u8 *__restrict__ slots, const DfJob *__restrict__ jobs, const u32 *__restrict__ sizes,
                                                 const u64 *__restrict__ base, u8 *__restrict__ out)
{
    const u8 *p = slots + jobs[blockIdx.x].slot;
    u8 *q = out + base[blockIdx.x];
    for (u32 i = threadIdx.x, n = sizes[blockIdx.x]; i < n; i += 256u) q[i] = p[i];
}

namespace {

u64 df_bound(u64 n) { return n + 5 * std::max<u64>(1, (n + DF_STORED_BLOCK - 1) / DF_STORED_BLOCK) + 6; }

int df_alloc(DevAlloc &d, u64 bytes, const std::string &fn, const char *what)
{
    if (hipMalloc(&d.p, std::max<u64>(bytes, 16)) == hipSuccess) return 0;
    (void)hipGetLastError();
    return fail(PMX_DBAM_ERR_OPEN, fn + ": out of device memory for " + std::to_string(bytes) + " bytes of " + what);
}

// The chunks d_raw[off[i], off[i + 1]) (off[0] == 0; every chunk at most DF_MAX bytes: the callers have checked) as zlib streams, end
// to end in buf with their lengths in sizes.  Returns the bytes written; cap below them: PMX_DBAM_ERR_INVALID and nothing written.
// `held` (may be null) counts the scratch into a handle's device bytes.
int64_t df_run(const std::string &fn, hipStream_t st, const u8 *d_raw, const std::vector<u64> &off, uint8_t *buf, int64_t cap, uint32_t *sizes,
               CvHold *held)
{
    const u64 nch = off.size() - 1, raw = off[nch];
    if (nch == 0) return 0;
    if (nch >= (1ull << 31)) return fail(PMX_DBAM_ERR_INVALID, fn + ": 2^31 chunks or more");
    std::vector<DfJob> jobs(nch);
    std::vector<u32> list[3];
    u64 slots = 0;
    for (u64 i = 0; i < nch; i++) {
        const u64 n = off[i + 1] - off[i];
        jobs[i] = DfJob{off[i], slots, (u32)n, 0u};
        slots += (df_bound(n) + 15) / 16 * 16;
        list[n <= 16384 ? 0 : n <= 32768 ? 1 : 2].push_back((u32)i);
    }
    DevAlloc d_jobs, d_list, d_tok, d_slots, d_tab, d_out;
    const u64 tab = 4 * nch + 8 * nch + 16, scratch = sizeof(DfJob) * nch + 4 * nch + 4 * raw + slots + tab;
    if (held) held->add(scratch);
    if (int rc = df_alloc(d_jobs, sizeof(DfJob) * nch, fn, "chunk tables")) return rc;
    if (int rc = df_alloc(d_list, 4 * nch, fn, "chunk tables")) return rc;
    if (int rc = df_alloc(d_tok, 4 * raw, fn, "tokens")) return rc;
    if (int rc = df_alloc(d_slots, slots, fn, "stream slots")) return rc;
    if (int rc = df_alloc(d_tab, tab, fn, "chunk tables")) return rc;
    u64 *d_base = d_tab.as<u64>(), *d_tot = d_base + nch;
    u32 *d_sizes = (u32 *)(d_tot + 2);
    HIPOK(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(DfJob) * nch, hipMemcpyHostToDevice, st));
    u64 first = 0;
    for (int k = 0; k < 3; k++) {
        const u64 m = list[k].size();
        if (!m) continue;
        u32 *d_l = d_list.as<u32>() + first;
        HIPOK(hipMemcpyAsync(d_l, list[k].data(), 4 * m, hipMemcpyHostToDevice, st));
        const dim3 grid((unsigned)m), wg(256);
        if (k == 0)
            hipLaunchKernelGGL((k_df_deflate<14, 11, 11>), grid, wg, 0, st, d_raw, d_jobs.as<DfJob>(), d_l, d_slots.as<u8>(), d_tok.as<u32>(), d_sizes);
        else if (k == 1)
            hipLaunchKernelGGL((k_df_deflate<15, 12, 11>), grid, wg, 0, st, d_raw, d_jobs.as<DfJob>(), d_l, d_slots.as<u8>(), d_tok.as<u32>(), d_sizes);
        else
            hipLaunchKernelGGL((k_df_deflate<16, 13, 12>), grid, wg, 0, st, d_raw, d_jobs.as<DfJob>(), d_l, d_slots.as<u8>(), d_tok.as<u32>(), d_sizes);
        HIPOK(hipGetLastError());
        first += m;
    }
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_sizes, d_sizes, nch, d_base, d_tot);
    HIPOK(hipGetLastError());
    u64 total = 0;
    HIPOK(hipMemcpyAsync(&total, d_tot, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));       // (jobs and the lists are locals)
    if ((u64)cap < total) return fail(PMX_DBAM_ERR_INVALID, fn + ": the buffer is too small: " + std::to_string(total) + " bytes are needed");
    if (held) held->add(total);
    if (int rc = df_alloc(d_out, total, fn, "streams")) return rc;
    hipLaunchKernelGGL(k_df_pack, dim3((unsigned)nch), dim3(256), 0, st, d_slots.as<u8>(), d_jobs.as<DfJob>(), d_sizes, d_base, d_out.as<u8>());
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(buf, d_out.p, total, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(sizes, d_sizes, 4 * nch, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return (int64_t)total;
}

// nsec sections of `full` raw bytes each, the last one of `last`: from byte 0 of d_raw on
std::vector<u64> df_section_offsets(u64 nsec, u64 full, u64 last)
{
    std::vector<u64> off(nsec + 1, 0);
    for (u64 k = 0; k < nsec; k++) off[k + 1] = off[k] + (k + 1 < nsec ? full : last);
    return off;
}

u64 df_sections_bound(u64 nsec, u64 full, u64 last) { return nsec ? (nsec - 1) * df_bound(full) + df_bound(last) : 0; }

int64_t df_sections_out(pmx_dbam *b, CvHold &held, const std::string &fn, const u8 *d_raw, u64 nsec, u64 full, u64 last, uint8_t *buf,
                        int64_t cap, uint32_t *zsizes)
{
    return df_run(fn, b->stream, d_raw, df_section_offsets(nsec, full, last), buf, cap, zsizes, &held);
}

int64_t ddeflate_impl(int device, const uint8_t *src, const uint64_t *offsets, int64_t n, uint8_t *dst, int64_t cap, uint32_t *sizes)
{
    const std::string fn = "pmx_ddeflate";
    if (n < 0 || cap < 0) return fail(PMX_DBAM_ERR_INVALID, fn + ": a negative count or capacity");
    if (!offsets || !dst || !sizes || (!src && n > 0 && offsets[n] > offsets[0])) return fail(PMX_DBAM_ERR_INVALID, fn + ": null pointer");
    std::vector<u64> off((u64)n + 1, 0);
    for (int64_t i = 0; i < n; i++) {
        if (offsets[i + 1] < offsets[i]) return fail(PMX_DBAM_ERR_INVALID, fn + ": the offsets descend");
        if (offsets[i + 1] - offsets[i] > DF_MAX)
            return fail(PMX_DBAM_ERR_INVALID, fn + ": a chunk of more than " + std::to_string(DF_MAX) + " bytes");
        off[(u64)i + 1] = offsets[i + 1] - offsets[0];
    }
    if (n == 0) return 0;
    HIPOK(hipSetDevice(device));
    DevAlloc d_raw;
    if (int rc = df_alloc(d_raw, off[(u64)n], fn, "chunks")) return rc;
    if (off[(u64)n]) HIPOK(hipMemcpy(d_raw.p, src + offsets[0], off[(u64)n], hipMemcpyHostToDevice));
    return df_run(fn, nullptr, d_raw.as<u8>(), off, dst, cap, sizes, nullptr);
}

}  // namespace

extern "C" {

uint64_t pmx_ddeflate_bound(uint64_t n) { return df_bound(n); }

int64_t pmx_ddeflate(int device, const uint8_t *src, const uint64_t *offsets, int64_t n, uint8_t *dst, int64_t cap, uint32_t *sizes)
{
    return guarded("pmx_ddeflate", [&] { return ddeflate_impl(device, src, offsets, n, dst, cap, sizes); });
}

int64_t pmx_dbam_coverage_sections_z(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                     uint32_t *table, int64_t table_cap, uint32_t *zsizes)
{
    return guarded("pmx_dbam_coverage_sections_z",
                   [&] { return coverage_sections_impl(b, CV_DEPTH, first, n, chrom_id, items, buf, cap, table, table_cap, true, zsizes); });
}

int64_t pmx_dbam_coverage_zoom_records_z(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                         int64_t table_cap, uint32_t *zsizes)
{
    return guarded("pmx_dbam_coverage_zoom_records_z",
                   [&] { return coverage_zoom_records_impl(b, CV_DEPTH, level, items, buf, cap, table, table_cap, true, zsizes); });
}

}  // extern "C"
