// The k-mer uniqueness track of a genome FASTA on the device (pmx_dkm_open, include/pymasc_amd_ingest.h; DESIGN.md 7.13).
// Included at the end of bam_device.hip behind bed_reads_device.inc: the handle is a pmx_dbw (kind 2) whose intervals are
// computed here, so pmx_dbw_fetch / device_arrays / sorted / copy / close work on it unchanged but for one branch
// (dbw_fetch_impl -> km_select: every value is 1.0).  The rules are io/fasta_parse.h's, shared with pmx_kmer_open, the checker.
//
//   host          tt_upload (text_track_device.inc): plain text, BGZF (k_bgzf_inflate) or other gzip (zlib on the host)
//   k_sam_count / k_bam_scan / k_sam_lines   the line index, as for SAM text
//   k_fa_class    one lane per line: blank, header or sequence, the name's or the body's length, an empty name (atomicMin)
//   k_fa_list     the sequence lines and the headers in file order, with each sequence line's first position and each
//                 record's separator position (block ranks and a block scan of the lengths over the per-workgroup scans)
//   k_fa_names    the header names, gathered for the host (duplicates and records without bases are found there)
//   k_fa_pack     one lane per 32 positions: 2 bits and a valid bit per position, a letter check of every byte (atomicMin)
//   k_km_keys     one lane per position: the k-mer exists and is no palindrome -> h = min(H(F), H(R)) over its packed words;
//                 <false> a histogram of the top 16 kept bits (plans the passes), <true> the pass's keys and positions
//   sort          per pass k_bed_check (digits that differ) and, for each such digit, k_bed_rs_hist + the multi-workgroup
//                 scan (k_km_scan_reduce / k_km_scan_top / k_km_scan_down) + k_bed_rs_scatter
//   k_km_heads    runs of equal hashes: a singleton is unique; head indices for the segmented max-scan (the same scan)
//   k_km_verify   every element against its run's first element, either strand; a mismatch marks the run
//   k_km_badlist / k_km_canon   the elements of marked runs (64-bit collisions) and their canonical words, resolved exactly
//                 on the host by sorting, the unique ones set back by k_km_setbits
//   k_km_edges / k_km_emit / k_km_cranges / k_km_local   the runs of unique positions as per-chromosome [begin, end)
// Every load of the text lies below its end rounded up to 16 bytes (the buffer holds 64 more); the packed genome and the
// unique bits hold two words more than the positions need.  All of it but the intervals is freed at the end of the open.
#include "../io/fasta_parse.h"

#define KM_SCAN_ITEMS 16u
#define KM_SCAN_TILE (256u * KM_SCAN_ITEMS)

struct KmSum {
    template <class T> __device__ static T op(T a, T b) { return a + b; }
};
struct KmMax {
    template <class T> __device__ static T op(T a, T b) { return a > b ? a : b; }
};

// exclusive OP-scan of one value per lane over the workgroup's 256 lanes; *total = OP over all of them (every lane calls it)
template <class OP, class T>
__device__ __forceinline__ T km_block_excl(T v, T *s, T *total)
{
    const u32 t = threadIdx.x;
    s[t] = v;
    __syncthreads();
    for (u32 o = 1; o < 256u; o <<= 1) {
        const T y = t >= o ? s[t - o] : (T)0;
        __syncthreads();
        s[t] = OP::op(s[t], y);
        __syncthreads();
    }
    const T r = t ? s[t - 1] : (T)0;
    *total = s[255];
    __syncthreads();                 // (before the next call writes s)
    return r;
}

// The multi-workgroup reduce-then-scan, three launches (visibility from the kernel boundaries, no look-back):
// part[g] = OP over tile g of in[]
template <class OP, class TI, class TO>
__global__ void __launch_bounds__(256) k_km_scan_reduce(const TI *__restrict__ in, u64 n, TO *__restrict__ part)
{
    __shared__ TO s[256];
    const u64 base = (u64)blockIdx.x * KM_SCAN_TILE + (u64)threadIdx.x * KM_SCAN_ITEMS;
    TO a = 0;
    for (u32 j = 0; j < KM_SCAN_ITEMS; j++)
        if (base + j < n) a = OP::op(a, (TO)in[base + j]);
    TO tot;
    (void)km_block_excl<OP, TO>(a, s, &tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}

// one workgroup: part[0..np) -> its exclusive OP-scan, part[np] = the total
template <class OP, class TO>
__global__ void __launch_bounds__(256) k_km_scan_top(TO *__restrict__ part, u64 np)
{
    __shared__ TO s[256];
    const u64 per = (np + 255u) / 256u, lo = min((u64)threadIdx.x * per, np), hi = min(lo + per, np);
    TO a = 0;
    for (u64 i = lo; i < hi; i++) a = OP::op(a, part[i]);
    TO tot;
    TO run = km_block_excl<OP, TO>(a, s, &tot);
    for (u64 i = lo; i < hi; i++) {
        const TO x = part[i];
        part[i] = run;
        run = OP::op(run, x);
    }
    if (threadIdx.x == 0) part[np] = tot;
}

// out[i] = OP over in[0..i) (INCL: in[0..i]), from the tile's scanned part
template <class OP, bool INCL, class TI, class TO>
__global__ void __launch_bounds__(256) k_km_scan_down(const TI *in, u64 n, const TO *__restrict__ part, TO *out)
{
    __shared__ TO s[256];
    const u64 base = (u64)blockIdx.x * KM_SCAN_TILE + (u64)threadIdx.x * KM_SCAN_ITEMS;
    TO v[KM_SCAN_ITEMS];
    TO a = 0;
#pragma unroll
    for (u32 j = 0; j < KM_SCAN_ITEMS; j++) {
        v[j] = base + j < n ? (TO)in[base + j] : (TO)0;
        a = OP::op(a, v[j]);
    }
    TO tot;
    TO run = OP::op(part[blockIdx.x], km_block_excl<OP, TO>(a, s, &tot));
#pragma unroll
    for (u32 j = 0; j < KM_SCAN_ITEMS; j++) {
        if (base + j < n) {
            if (INCL) run = OP::op(run, v[j]);
            out[base + j] = run;
            if (!INCL) run = OP::op(run, v[j]);
        }
    }
}

// one lane per line: type, the body's length (sequence) or the name's (header); per workgroup: sequence lines, headers, bases
__global__ void __launch_bounds__(256) k_fa_class(const u8 *__restrict__ D, const u64 *__restrict__ nl, u64 n, u8 *__restrict__ tag,
                                                  u32 *__restrict__ len, u32 *__restrict__ cseq, u32 *__restrict__ chdr,
                                                  u64 *__restrict__ cbases, unsigned long long *__restrict__ first_err)
{
    __shared__ u64 s_b[4];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 type = fasta::L_BLANK;
    u64 bases = 0;
    if (i < n) {
        DevSrc s{D, ~0ull, make_uint4(0, 0, 0, 0)};
        const u64 b = i ? nl[i - 1] + 1u : 0ull;
        u64 body = 0, name_end = 0;
        const u32 err = fasta::classify(s, b, nl[i], type, body, name_end);
        if (err) atomicMin(first_err, (unsigned long long)((i << 8) | err));
        const u64 l = type == fasta::L_SEQ ? body - b : type == fasta::L_HEADER ? name_end - b - 1u : 0ull;
        tag[i] = (u8)type;
        const u32 l32 = l < 0xffffffffull ? (u32)l : 0xffffffffu;
        len[i] = l32;
        if (type == fasta::L_SEQ) bases = l32;
    }
    for (int o = 32; o > 0; o >>= 1) bases += __shfl_xor(bases, o, 64);
    if ((threadIdx.x & 63u) == 0) s_b[threadIdx.x >> 6] = bases;
    const int ns = __syncthreads_count(type == fasta::L_SEQ), nh = __syncthreads_count(type == fasta::L_HEADER);
    if (threadIdx.x == 0) {
        cseq[blockIdx.x] = (u32)ns;
        chdr[blockIdx.x] = (u32)nh;
        cbases[blockIdx.x] = s_b[0] + s_b[1] + s_b[2] + s_b[3];
    }
}

struct FaSeq {              // the sequence lines in file order
    u64 *start;             // text offset of the first byte
    u32 *len, *line;        // bytes; line index
    u64 *pos0;              // position of the first byte
};

__global__ void __launch_bounds__(256) k_fa_list(const u64 *__restrict__ nl, u64 n, const u8 *__restrict__ tag, const u32 *__restrict__ len,
                                                 const u64 *__restrict__ seq_base, const u64 *__restrict__ hdr_base,
                                                 const u64 *__restrict__ bases_base, FaSeq S, u32 *__restrict__ hd_line,
                                                 u64 *__restrict__ hd_sep, u32 *__restrict__ hd_nlen, unsigned long long *__restrict__ first_err)
{
    __shared__ u32 s_wave[4];
    __shared__ u64 s_scan[256];
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 type = i < n ? tag[i] : (u32)fasta::L_BLANK;
    const bool seq = type == fasta::L_SEQ, hdr = type == fasta::L_HEADER;
    const u32 rs = tt_block_rank(seq, s_wave), rh = tt_block_rank(hdr, s_wave);
    u64 tot;
    const u64 bexcl = km_block_excl<KmSum, u64>(seq ? (u64)len[i] : 0ull, s_scan, &tot);
    const u64 bases_before = bases_base[blockIdx.x] + bexcl;
    if (seq) {
        const u64 hb = hdr_base[blockIdx.x] + rh;              // headers before this line
        const u64 j = seq_base[blockIdx.x] + rs;
        S.start[j] = i ? nl[i - 1] + 1u : 0ull;
        S.len[j] = len[i];
        S.line[j] = (u32)i;
        S.pos0[j] = bases_before + hb;
        if (hb == 0) atomicMin(first_err, (unsigned long long)((i << 8) | fasta::FA_ERR_BEFORE));
    }
    if (hdr) {
        const u64 h = hdr_base[blockIdx.x] + rh;
        hd_line[h] = (u32)i;
        hd_sep[h] = bases_before + h;
        hd_nlen[h] = len[i];
    }
}

// one wavefront per header: its name's bytes to names[noff[h] ..)
__global__ void __launch_bounds__(256) k_fa_names(const u8 *__restrict__ D, const u64 *__restrict__ nl, const u32 *__restrict__ hd_line,
                                                  const u32 *__restrict__ hd_nlen, const u64 *__restrict__ noff, u32 nh, u8 *__restrict__ names)
{
    const u32 h = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (h >= nh) return;
    const u32 line = hd_line[h];
    const u64 b = (line ? nl[line - 1] + 1u : 0ull) + 1u;
    for (u32 k = lane; k < hd_nlen[h]; k += 64u) names[noff[h] + k] = D[b + k];
}

// one lane per 32 positions: the packed bases and the valid bits; a byte that is not a letter reports its line
__global__ void __launch_bounds__(256) k_fa_pack(const u8 *__restrict__ D, FaSeq S, u64 nseq, u64 npos, u64 nwords, u64 *__restrict__ P,
                                                 u32 *__restrict__ V, unsigned long long *__restrict__ first_err)
{
    const u64 w = (u64)blockIdx.x * 256u + threadIdx.x;
    if (w >= nwords) return;
    const u64 q0 = 32ull * w;
    u64 lo = 0, hi = nseq;                       // the last line with pos0 <= q0 (or line 0)
    while (hi - lo > 1u) {
        const u64 mid = (lo + hi) >> 1;
        if (S.pos0[mid] <= q0) lo = mid;
        else hi = mid;
    }
    u64 j = lo, pk = 0;
    u32 vm = 0;
    for (u32 t = 0; t < 32u; t++) {
        const u64 q = q0 + t;
        if (q >= npos) break;
        while (j < nseq && q >= S.pos0[j] + S.len[j]) j++;
        if (j >= nseq) break;
        if (q < S.pos0[j]) continue;             // a separator
        const u8 c = D[S.start[j] + (q - S.pos0[j])];
        if (!fasta::is_letter(c)) atomicMin(first_err, (unsigned long long)(((u64)S.line[j] << 8) | fasta::FA_ERR_BYTE));
        const u32 code = fasta::base_code(c);
        if (code < 4u) {
            pk |= (u64)code << (2u * t);
            vm |= 1u << t;
        }
    }
    P[w] = pk;
    V[w] = vm;
}

__device__ __forceinline__ bool km_key(const u64 *__restrict__ P, const u32 *__restrict__ V, u64 q, u32 k, u64 npos, u64 mask, u64 &key)
{
    if (!fasta::window_valid(V, q, k, npos)) return false;
    const u32 nw = (k + 31u) / 32u;
    u64 hf = fasta::mix64(k), hr = hf;
    bool pal = true;
    for (u32 i = 0; i < nw; i++) {
        const u64 f = fasta::kmer_word(P, q, k, i, false), r = fasta::kmer_word(P, q, k, i, true);
        pal = pal && f == r;
        hf = fasta::mix64(hf ^ f) + 0x9E3779B97F4A7C15ull;
        hr = fasta::mix64(hr ^ r) + 0x9E3779B97F4A7C15ull;
    }
    key = (hf < hr ? hf : hr) & mask;
    return !pal;
}

// one lane per position: EMIT false, hist[bin]++ for every k-mer that exists and is no palindrome; EMIT true, the keys of bins
// [lo, hi) with their positions, appended at *cursor (one atomic per wavefront)
template <bool EMIT>
__global__ void __launch_bounds__(256) k_km_keys(const u64 *__restrict__ P, const u32 *__restrict__ V, u64 npos, u32 k, u64 mask,
                                                 u32 bshift, u32 *__restrict__ hist, u32 lo, u32 hi, u64 *__restrict__ key,
                                                 u32 *__restrict__ val, unsigned long long *__restrict__ cursor, u64 cap)
{
    const u64 q = (u64)blockIdx.x * 256u + threadIdx.x;
    u64 h = 0;
    const bool ok = q < npos && km_key(P, V, q, k, npos, mask, h);
    const u32 bin = (u32)(h >> bshift);
    if (!EMIT) {
        if (ok) atomicAdd(&hist[bin], 1u);
        return;
    }
    const bool keep = ok && bin >= lo && bin < hi;
    const u64 m = __ballot(keep);
    if (!m) return;
    const u32 lane = threadIdx.x & 63u, leader = (u32)(__ffsll((long long)m) - 1);
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
    base = __shfl(base, (int)leader, 64);
    if (keep) {
        const u64 at = base + (u64)__popcll(m & ((1ull << lane) - 1ull));
        if (at < cap) {
            key[at] = h;
            val[at] = (u32)q;
        }
    }
}

// runs of equal keys: a singleton's position is unique; hv[i] = i at a run's head (0 elsewhere) for the segmented max-scan
__global__ void __launch_bounds__(256) k_km_heads(const u64 *__restrict__ key, const u32 *__restrict__ val, u64 n, u32 *__restrict__ hv,
                                                  u32 *__restrict__ U)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 x = key[i];
    const bool head = i == 0 || key[i - 1] != x, tail = i + 1 == n || key[i + 1] != x;
    hv[i] = head ? (u32)i : 0u;
    if (head && tail) {
        const u32 q = val[i];
        atomicOr(&U[q >> 5], 1u << (q & 31u));
    }
}

// every element of a run against the run's first element (head[i], from the max-scan); a mismatch marks the run
__global__ void __launch_bounds__(256) k_km_verify(const u64 *__restrict__ P, u32 k, const u32 *__restrict__ val, u64 n,
                                                   const u32 *__restrict__ head, u8 *__restrict__ bad)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u32 h = head[i];
    if ((u64)h == i) return;
    if (!fasta::same_kmer(P, val[i], val[h], k)) bad[h] = 1;
}

// the positions of the elements of marked runs, appended at *cursor (the first cap kept)
__global__ void __launch_bounds__(256) k_km_badlist(const u32 *__restrict__ val, u64 n, const u32 *__restrict__ head, const u8 *__restrict__ bad,
                                                    u32 *__restrict__ list, unsigned long long *__restrict__ cursor, u64 cap)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    const bool mine = i < n && bad[head[i]];
    const u64 m = __ballot(mine);
    if (!m) return;
    const u32 lane = threadIdx.x & 63u, leader = (u32)(__ffsll((long long)m) - 1);
    unsigned long long base = 0;
    if (lane == leader) base = atomicAdd(cursor, (unsigned long long)__popcll(m));
    base = __shfl(base, (int)leader, 64);
    if (mine) {
        const u64 at = base + (u64)__popcll(m & ((1ull << lane) - 1ull));
        if (at < cap) list[at] = val[i];
    }
}

// the canonical packed k-mer (the smaller of F and R, word by word) of every listed position
__global__ void __launch_bounds__(256) k_km_canon(const u64 *__restrict__ P, u32 k, const u32 *__restrict__ list, u64 n, u64 *__restrict__ out)
{
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 q = list[j], nw = (k + 31u) / 32u;
    const bool rev = fasta::strand_order(P, q, k) > 0;
    for (u32 i = 0; i < nw; i++) out[j * nw + i] = fasta::canon_word(P, q, k, i, rev);
}

__global__ void __launch_bounds__(256) k_km_setbits(const u32 *__restrict__ list, u64 n, u32 *__restrict__ U)
{
    const u64 j = (u64)blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const u32 q = list[j];
    atomicOr(&U[q >> 5], 1u << (q & 31u));
}

// the starts (END false) or ends (END true) of the runs of unique positions in word w of U
template <bool END>
__device__ __forceinline__ u32 km_edge_bits(const u32 *__restrict__ U, u64 w)
{
    const u32 u = U[w];
    if (END) return u & ~((u >> 1) | ((U[w + 1] & 1u) << 31));
    return u & ~((u << 1) | (w ? U[w - 1] >> 31 : 0u));
}

template <bool END>
__global__ void __launch_bounds__(256) k_km_edges(const u32 *__restrict__ U, u64 nwords, u32 *__restrict__ cnt)
{
    const u64 w = (u64)blockIdx.x * 256u + threadIdx.x;
    if (w < nwords) cnt[w] = (u32)__popc(km_edge_bits<END>(U, w));
}

template <bool END>
__global__ void __launch_bounds__(256) k_km_emit(const u32 *__restrict__ U, u64 nwords, const u64 *__restrict__ base, u32 *__restrict__ out)
{
    const u64 w = (u64)blockIdx.x * 256u + threadIdx.x;
    if (w >= nwords) return;
    u32 m = km_edge_bits<END>(U, w);
    u64 o = base[w];
    while (m) {
        const u32 b = (u32)(__ffs(m) - 1);
        out[o++] = (u32)(32ull * w + b + (END ? 1u : 0u));
        m &= m - 1u;
    }
}

// the first run at or after each record's separator (runs in global order); cr[nrec] = the number of runs
__global__ void __launch_bounds__(256) k_km_cranges(const u32 *__restrict__ begin, u64 nruns, const u32 *__restrict__ sep, u32 nrec,
                                                    u64 *__restrict__ cr)
{
    const u32 c = blockIdx.x * 256u + threadIdx.x;
    if (c > nrec) return;
    if (c == nrec) {
        cr[c] = nruns;
        return;
    }
    u64 lo = 0, hi = nruns;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (begin[mid] < sep[c]) lo = mid + 1;
        else hi = mid;
    }
    cr[c] = lo;
}

// every run to its record's coordinates (the record whose separator is the last before it), value 1.0
__global__ void __launch_bounds__(256) k_km_local(u32 *__restrict__ begin, u32 *__restrict__ end, float *__restrict__ value, u64 nruns,
                                                  const u32 *__restrict__ sep, u32 nrec)
{
    const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
    if (r >= nruns) return;
    const u32 b = begin[r];
    u32 lo = 0, hi = nrec;
    while (hi - lo > 1u) {
        const u32 mid = (lo + hi) >> 1;
        if (sep[mid] < b) lo = mid;
        else hi = mid;
    }
    const u32 off = sep[lo] + 1u;
    begin[r] = b - off;
    end[r] = end[r] - off;
    value[r] = 1.0f;
}

namespace {

inline unsigned km_grid(u64 n) { return (unsigned)std::max<u64>(1, (n + 255) / 256); }

// out = the OP-scan of in[0, n) (exclusive, or inclusive with INCL); part holds at least n / KM_SCAN_TILE + 2 entries, and
// part[n / KM_SCAN_TILE rounded up] = the total afterwards
template <class OP, bool INCL, class TI, class TO>
int km_scan(const TI *in, u64 n, TO *out, TO *part, hipStream_t st)
{
    if (n == 0) return 0;
    const u64 np = (n + KM_SCAN_TILE - 1) / KM_SCAN_TILE;
    hipLaunchKernelGGL((k_km_scan_reduce<OP, TI, TO>), dim3((unsigned)np), dim3(256), 0, st, in, n, part);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL((k_km_scan_top<OP, TO>), dim3(1), dim3(256), 0, st, part, np);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL((k_km_scan_down<OP, INCL, TI, TO>), dim3((unsigned)np), dim3(256), 0, st, in, n, (const TO *)part, out);
    HIPOK(hipGetLastError());
    return 0;
}

template <class T>
int km_total(const T *part, u64 n, T *out, hipStream_t st)
{
    *out = 0;
    if (n == 0) return 0;
    const u64 np = (n + KM_SCAN_TILE - 1) / KM_SCAN_TILE;
    HIPOK(hipMemcpyAsync(out, part + np, sizeof(T), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return 0;
}

struct KmGenome {
    u64 *P = nullptr;
    u32 *V = nullptr;
    u64 npos = 0, nwords = 0;
    std::vector<u32> sep;           // each record's separator position
};

inline u64 km_parts(u64 n) { return n / KM_SCAN_TILE + 2; }

// text -> records (names, lengths) and the packed genome; the first error by line (also pmx_dgc_open's, gcbias_device.inc)
int km_parse(hipStream_t st, std::vector<std::string> &rec_names, std::vector<int64_t> &rec_sizes, const u8 *D, u64 N, TtDev &g,
             KmGenome &G)
{
    TtDev t;                        // the line tables: freed when the genome is packed
    if (N == 0) return fail(PMX_DBAM_ERR_FORMAT, fasta::no_record_text());
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
    // classify, count, list
    const u64 nb = (n + 255) / 256;
    u8 *d_tag;
    u32 *d_len, *d_cseq, *d_chdr;
    u64 *d_cbases, *d_seqb, *d_hdrb, *d_basb, *d_part;
    unsigned long long *d_err;
    if (int rc = t.get(&d_tag, n)) return rc;
    if (int rc = t.get(&d_len, 4 * n)) return rc;
    if (int rc = t.get(&d_cseq, 4 * nb)) return rc;
    if (int rc = t.get(&d_chdr, 4 * nb)) return rc;
    if (int rc = t.get(&d_cbases, 8 * nb)) return rc;
    if (int rc = t.get(&d_seqb, 8 * nb)) return rc;
    if (int rc = t.get(&d_hdrb, 8 * nb)) return rc;
    if (int rc = t.get(&d_basb, 8 * nb)) return rc;
    if (int rc = t.get(&d_part, 8 * 3 * km_parts(nb))) return rc;
    if (int rc = t.get(&d_err, 8)) return rc;
    HIPOK(hipMemsetAsync(d_err, 0xff, 8, st));
    hipLaunchKernelGGL(k_fa_class, dim3((unsigned)nb), dim3(256), 0, st, D, d_nl, n, d_tag, d_len, d_cseq, d_chdr, d_cbases, d_err);
    HIPOK(hipGetLastError());
    u64 *p1 = d_part, *p2 = d_part + km_parts(nb), *p3 = d_part + 2 * km_parts(nb);
    if (int rc = km_scan<KmSum, false>(d_cseq, nb, d_seqb, p1, st)) return rc;
    if (int rc = km_scan<KmSum, false>(d_chdr, nb, d_hdrb, p2, st)) return rc;
    if (int rc = km_scan<KmSum, false>(d_cbases, nb, d_basb, p3, st)) return rc;
    u64 nseq = 0, nhdr = 0, bases = 0;
    if (int rc = km_total(p1, nb, &nseq, st)) return rc;
    if (int rc = km_total(p2, nb, &nhdr, st)) return rc;
    if (int rc = km_total(p3, nb, &bases, st)) return rc;
    FaSeq S;
    u32 *d_hline, *d_hnlen;
    u64 *d_hsep;
    if (int rc = t.get(&S.start, 8 * nseq)) return rc;
    if (int rc = t.get(&S.len, 4 * nseq)) return rc;
    if (int rc = t.get(&S.line, 4 * nseq)) return rc;
    if (int rc = t.get(&S.pos0, 8 * nseq)) return rc;
    if (int rc = t.get(&d_hline, 4 * nhdr)) return rc;
    if (int rc = t.get(&d_hnlen, 4 * nhdr)) return rc;
    if (int rc = t.get(&d_hsep, 8 * nhdr)) return rc;
    hipLaunchKernelGGL(k_fa_list, dim3((unsigned)nb), dim3(256), 0, st, d_nl, n, d_tag, d_len, d_seqb, d_hdrb, d_basb, S, d_hline,
                       d_hsep, d_hnlen, d_err);
    HIPOK(hipGetLastError());
    std::vector<u32> hline(nhdr), hnlen(nhdr);
    std::vector<u64> hsep(nhdr);
    unsigned long long fe = ~0ull;
    if (nhdr) {
        HIPOK(hipMemcpyAsync(hline.data(), d_hline, 4 * nhdr, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(hnlen.data(), d_hnlen, 4 * nhdr, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(hsep.data(), d_hsep, 8 * nhdr, hipMemcpyDeviceToHost, st));
    }
    HIPOK(hipMemcpyAsync(&fe, d_err, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    // the names (duplicates) and the records' lengths (no bases) on the host
    std::vector<u64> noff(nhdr + 1, 0);
    for (u64 h = 0; h < nhdr; h++) noff[h + 1] = noff[h] + hnlen[h];
    std::string names(noff[nhdr], '\0');
    if (nhdr) {
        u64 *d_noff;
        u8 *d_names;
        if (int rc = t.get(&d_noff, 8 * (nhdr + 1))) return rc;
        if (int rc = t.get(&d_names, noff[nhdr])) return rc;
        HIPOK(hipMemcpyAsync(d_noff, noff.data(), 8 * (nhdr + 1), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_fa_names, dim3((unsigned)((nhdr + 3) / 4)), dim3(256), 0, st, D, d_nl, d_hline, d_hnlen, d_noff, (u32)nhdr,
                           d_names);
        HIPOK(hipGetLastError());
        if (noff[nhdr]) HIPOK(hipMemcpyAsync(&names[0], d_names, noff[nhdr], hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
    }
    std::unordered_map<std::string, u32> seen;
    const u64 total_pos = bases + nhdr;              // (the closing separator's position)
    for (u64 h = 0; h < nhdr; h++) {
        std::string nm = names.substr(noff[h], hnlen[h]);
        const u64 len = (h + 1 < nhdr ? hsep[h + 1] : total_pos) - hsep[h] - 1u;
        if (len == 0) fe = std::min<unsigned long long>(fe, ((u64)hline[h] << 8) | fasta::FA_ERR_EMPTY);
        if (hnlen[h] && !seen.emplace(nm, (u32)h).second) fe = std::min<unsigned long long>(fe, ((u64)hline[h] << 8) | fasta::FA_ERR_DUP);
        rec_names.push_back(nm);
        rec_sizes.push_back((int64_t)len);
    }
    const bool big = fasta::too_large(bases, nhdr);
    if (big || !nhdr) {
        if (fe != ~0ull) return fail(PMX_DBAM_ERR_FORMAT, fasta::line_error(fe >> 8, (u32)(fe & 255u)));
        return fail(PMX_DBAM_ERR_FORMAT, nhdr ? fasta::too_large_text() : fasta::no_record_text());
    }
    // the packed genome (the letters are checked here: an earlier bad byte may win over the errors above)
    G.npos = total_pos + 1u;
    G.nwords = (G.npos + 31) / 32;
    if (int rc = g.get(&G.P, 8 * (G.nwords + 2))) return rc;
    if (int rc = g.get(&G.V, 4 * (G.nwords + 2))) return rc;
    HIPOK(hipMemsetAsync(G.P + G.nwords, 0, 16, st));
    HIPOK(hipMemsetAsync(G.V + G.nwords, 0, 8, st));
    HIPOK(hipMemcpyAsync(d_err, &fe, 8, hipMemcpyHostToDevice, st));
    if (nseq)
        hipLaunchKernelGGL(k_fa_pack, dim3(km_grid(G.nwords)), dim3(256), 0, st, D, S, nseq, G.npos, G.nwords, G.P, G.V, d_err);
    else
        HIPOK(hipMemsetAsync(G.V, 0, 4 * G.nwords, st));
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(&fe, d_err, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (fe != ~0ull) return fail(PMX_DBAM_ERR_FORMAT, fasta::line_error(fe >> 8, (u32)(fe & 255u)));
    for (u64 h = 0; h < nhdr; h++) G.sep.push_back((u32)hsep[h]);
    return 0;
}

// the exact resolution of the runs whose hashes collide: their positions' canonical k-mers sorted on the host
int km_resolve(hipStream_t st, const KmGenome &G, u32 k, const u32 *d_list, u64 nlist, u32 *U, u64 &resolved)
{
    const u32 nw = (k + 31u) / 32u;
    DevAlloc d_words, d_uniq;
    HIPOK(hipMalloc(&d_words.p, 8 * nw * nlist));
    hipLaunchKernelGGL(k_km_canon, dim3(km_grid(nlist)), dim3(256), 0, st, G.P, k, d_list, nlist, d_words.as<u64>());
    HIPOK(hipGetLastError());
    std::vector<u64> words(nw * nlist);
    std::vector<u32> list(nlist);
    HIPOK(hipMemcpyAsync(words.data(), d_words.p, 8 * nw * nlist, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(list.data(), d_list, 4 * nlist, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    std::vector<u32> idx(nlist);
    for (u64 j = 0; j < nlist; j++) idx[j] = (u32)j;
    auto cmp = [&](u32 a, u32 b) -> int {
        for (u32 i = 0; i < nw; i++) {
            const u64 x = words[(u64)a * nw + i], y = words[(u64)b * nw + i];
            if (x != y) return x < y ? -1 : 1;
        }
        return 0;
    };
    std::sort(idx.begin(), idx.end(), [&](u32 a, u32 b) { return cmp(a, b) < 0; });
    std::vector<u32> uniq;
    for (u64 i = 0; i < nlist;) {
        u64 j = i + 1;
        while (j < nlist && cmp(idx[i], idx[j]) == 0) j++;
        if (j == i + 1) uniq.push_back(list[idx[i]]);
        i = j;
    }
    resolved += nlist;
    if (uniq.empty()) return 0;
    HIPOK(hipMalloc(&d_uniq.p, 4 * uniq.size()));
    HIPOK(hipMemcpyAsync(d_uniq.p, uniq.data(), 4 * uniq.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_km_setbits, dim3(km_grid(uniq.size())), dim3(256), 0, st, d_uniq.as<u32>(), (u64)uniq.size(), U);
    HIPOK(hipGetLastError());
    HIPOK(hipStreamSynchronize(st));
    return 0;
}

int km_build(pmx_dbw &w, u32 k, u64 budget, u32 hash_bits, const KmGenome &G)
{
    hipStream_t st = w.stream;
    TtDev t;
    const u64 mask = hash_bits >= 64u ? ~0ull : ((1ull << hash_bits) - 1ull);
    const u32 bbits = hash_bits < 16u ? hash_bits : 16u, bshift = hash_bits - bbits;
    const u64 nbins = 1ull << bbits;
    u32 *U, *d_hist;
    if (int rc = t.get(&U, 4 * (G.nwords + 2))) return rc;
    if (int rc = t.get(&d_hist, 4 * nbins)) return rc;
    HIPOK(hipMemsetAsync(U, 0, 4 * (G.nwords + 2), st));
    HIPOK(hipMemsetAsync(d_hist, 0, 4 * nbins, st));
    hipLaunchKernelGGL(k_km_keys<false>, dim3(km_grid(G.npos)), dim3(256), 0, st, G.P, G.V, G.npos, k, mask, bshift, d_hist, 0u, 0u,
                       (u64 *)nullptr, (u32 *)nullptr, (unsigned long long *)nullptr, 0ull);
    HIPOK(hipGetLastError());
    std::vector<u32> hist(nbins);
    HIPOK(hipMemcpyAsync(hist.data(), d_hist, 4 * nbins, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    // the passes: consecutive bin ranges of at most `cap` k-mers (24 bytes each: two buffers of key + payload)
    const u64 cap = std::max<u64>(budget / 24u, 1);
    std::vector<std::pair<u32, u32>> passes;
    std::vector<u64> pass_n;
    u64 biggest = 0, acc = 0;
    u32 first = 0;
    for (u64 b = 0; b < nbins; b++) {
        if (hist[b] > cap)
            return fail(PMX_DBAM_ERR_OPEN, "a hash bin of " + std::to_string(hist[b]) + " k-mers does not fit the sort budget of " +
                                               std::to_string(budget) + " bytes");
        if (acc + hist[b] > cap) {
            passes.emplace_back(first, (u32)b);
            pass_n.push_back(acc);
            biggest = std::max(biggest, acc);
            first = (u32)b;
            acc = 0;
        }
        acc += hist[b];
    }
    passes.emplace_back(first, (u32)nbins);
    pass_n.push_back(acc);
    biggest = std::max(biggest, acc);
    w.km_passes = (u32)passes.size();
    w.km_kmers = 0;
    for (u64 x : pass_n) w.km_kmers += x;
    // the sort buffers, sized for the largest pass
    const u64 nmax = std::max<u64>(biggest, 1);
    const u32 ntiles_max = (u32)((nmax + BED_RS_TILE - 1) / BED_RS_TILE);
    const u64 ncnt_max = 256ull * ntiles_max;
    u64 *K1, *K2, *d_base, *d_part;
    u32 *V1, *V2, *d_cnt;
    unsigned long long *d_cur, *d_chk;
    if (int rc = t.get(&K1, 8 * nmax)) return rc;
    if (int rc = t.get(&K2, 8 * nmax)) return rc;
    if (int rc = t.get(&V1, 4 * nmax)) return rc;
    if (int rc = t.get(&V2, 4 * nmax)) return rc;
    if (int rc = t.get(&d_cnt, 4 * ncnt_max)) return rc;
    if (int rc = t.get(&d_base, 8 * ncnt_max)) return rc;
    if (int rc = t.get(&d_part, 8 * km_parts(std::max<u64>(ncnt_max, nmax)))) return rc;
    if (int rc = t.get(&d_cur, 8)) return rc;
    if (int rc = t.get(&d_chk, 32)) return rc;
    for (size_t ps = 0; ps < passes.size(); ps++) {
        const u64 n = pass_n[ps];
        if (n == 0) continue;
        HIPOK(hipMemsetAsync(d_cur, 0, 8, st));
        hipLaunchKernelGGL(k_km_keys<true>, dim3(km_grid(G.npos)), dim3(256), 0, st, G.P, G.V, G.npos, k, mask, bshift, (u32 *)nullptr,
                           passes[ps].first, passes[ps].second, K1, V1, d_cur, n);
        HIPOK(hipGetLastError());
        unsigned long long chk[4] = {0, 0, ~0ull, 0}, got = 0;
        HIPOK(hipMemcpyAsync(d_chk, chk, 32, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_bed_check, dim3(km_grid(n)), dim3(256), 0, st, K1, n, 0ull, d_chk);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(chk, d_chk, 32, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(&got, d_cur, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (got != n) return fail(PMX_DBAM_ERR_DEVICE, "k-mer pass: " + std::to_string(got) + " keys where the histogram counted " + std::to_string(n));
        const u64 differ = chk[1] ^ chk[2];
        const u32 ntiles = (u32)((n + BED_RS_TILE - 1) / BED_RS_TILE);
        const u64 ncnt = 256ull * ntiles;
        u64 *kin = K1, *kout = K2;
        u32 *vin = V1, *vout = V2;
        for (u32 dig = 0; dig < 8u; dig++) {
            const u32 shift = 8u * dig;
            if (((differ >> shift) & 255u) == 0) continue;     // the same digit in every key of the pass
            hipLaunchKernelGGL(k_bed_rs_hist, dim3(ntiles), dim3(256), 0, st, kin, n, shift, ntiles, d_cnt);
            HIPOK(hipGetLastError());
            if (int rc = km_scan<KmSum, false>(d_cnt, ncnt, d_base, d_part, st)) return rc;
            hipLaunchKernelGGL(k_bed_rs_scatter, dim3(ntiles), dim3(256), 0, st, kin, vin, n, shift, ntiles, d_base, kout, vout);
            HIPOK(hipGetLastError());
            std::swap(kin, kout);
            std::swap(vin, vout);
        }
        // group: the free pair holds the head indices (vout) and the run marks (kout)
        u32 *head = vout;
        u8 *bad = (u8 *)kout;
        hipLaunchKernelGGL(k_km_heads, dim3(km_grid(n)), dim3(256), 0, st, kin, vin, n, head, U);
        HIPOK(hipGetLastError());
        if (int rc = km_scan<KmMax, true>(head, n, head, (u32 *)d_part, st)) return rc;
        HIPOK(hipMemsetAsync(bad, 0, n, st));
        hipLaunchKernelGGL(k_km_verify, dim3(km_grid(n)), dim3(256), 0, st, G.P, k, vin, n, head, bad);
        HIPOK(hipGetLastError());
        // the runs with a mismatch: their elements to the host, resolved exactly (the list goes where the keys were)
        u32 *list = (u32 *)kin;
        HIPOK(hipMemsetAsync(d_cur, 0, 8, st));
        hipLaunchKernelGGL(k_km_badlist, dim3(km_grid(n)), dim3(256), 0, st, vin, n, head, bad, list, d_cur, 2 * n);
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(&got, d_cur, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (got) {
            if (int rc = km_resolve(st, G, k, list, got, U, w.km_resolved)) return rc;
        }
    }
    // the runs of unique positions
    u32 *d_sc, *d_ec;
    u64 *d_sb, *d_eb, *d_p2;
    if (int rc = t.get(&d_sc, 4 * G.nwords)) return rc;
    if (int rc = t.get(&d_ec, 4 * G.nwords)) return rc;
    if (int rc = t.get(&d_sb, 8 * G.nwords)) return rc;
    if (int rc = t.get(&d_eb, 8 * G.nwords)) return rc;
    if (int rc = t.get(&d_p2, 8 * km_parts(G.nwords))) return rc;
    hipLaunchKernelGGL(k_km_edges<false>, dim3(km_grid(G.nwords)), dim3(256), 0, st, U, G.nwords, d_sc);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_km_edges<true>, dim3(km_grid(G.nwords)), dim3(256), 0, st, U, G.nwords, d_ec);
    HIPOK(hipGetLastError());
    if (int rc = km_scan<KmSum, false>(d_sc, G.nwords, d_sb, d_part, st)) return rc;
    if (int rc = km_scan<KmSum, false>(d_ec, G.nwords, d_eb, d_p2, st)) return rc;
    u64 nruns = 0, nends = 0;
    if (int rc = km_total(d_part, G.nwords, &nruns, st)) return rc;
    if (int rc = km_total(d_p2, G.nwords, &nends, st)) return rc;
    if (nruns != nends) return fail(PMX_DBAM_ERR_DEVICE, "unique runs: starts and ends differ");
    const u32 nrec = (u32)G.sep.size();
    u32 *d_sep;
    u64 *d_cr;
    if (int rc = t.get(&d_sep, 4ull * nrec)) return rc;
    if (int rc = t.get(&d_cr, 8ull * (nrec + 1))) return rc;
    HIPOK(hipMemcpyAsync(d_sep, G.sep.data(), 4ull * nrec, hipMemcpyHostToDevice, st));
    HIPOK(hipMalloc((void **)&w.d_begin, 4 * std::max<u64>(nruns, 1)));
    HIPOK(hipMalloc((void **)&w.d_end, 4 * std::max<u64>(nruns, 1)));
    HIPOK(hipMalloc((void **)&w.d_value, 4 * std::max<u64>(nruns, 1)));
    hipLaunchKernelGGL(k_km_emit<false>, dim3(km_grid(G.nwords)), dim3(256), 0, st, U, G.nwords, d_sb, w.d_begin);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_km_emit<true>, dim3(km_grid(G.nwords)), dim3(256), 0, st, U, G.nwords, d_eb, w.d_end);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_km_cranges, dim3(km_grid(nrec + 1)), dim3(256), 0, st, w.d_begin, nruns, d_sep, nrec, d_cr);
    HIPOK(hipGetLastError());
    hipLaunchKernelGGL(k_km_local, dim3(km_grid(nruns)), dim3(256), 0, st, w.d_begin, w.d_end, w.d_value, nruns, d_sep, nrec);
    HIPOK(hipGetLastError());
    std::vector<u64> cr(nrec + 1);
    HIPOK(hipMemcpyAsync(cr.data(), d_cr, 8ull * (nrec + 1), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    w.km_range.resize(nrec);
    for (u32 c = 0; c < nrec; c++) w.km_range[c] = std::pair<u64, u64>(cr[c], cr[c + 1]);
    w.total = nruns;
    return 0;
}

}  // namespace

// the dbw_fetch_impl branch of a k-mer track: every value is 1.0, so a threshold above 1 keeps nothing and any other keeps all
static int km_select(pmx_dbw *w, float threshold)
{
    const bool all = !(threshold > 1.0f);
    w->range.assign(w->names.size(), std::pair<u64, u64>(0, 0));
    if (all) w->range = w->km_range;
    w->order.assign(w->names.size(), 1);        // (runs: ascending and disjoint)
    w->have = true;
    w->have_threshold = threshold;
    return 0;
}

extern "C" {

static int dkm_open_impl(const char *path, int32_t k, int device, int nthreads, int64_t budget_bytes, int32_t hash_bits, pmx_dbw **out);
int pmx_dkm_open(const char *path, int32_t k, int device, int nthreads, int64_t budget_bytes, int32_t hash_bits, pmx_dbw **out)
{
    try {
        return dkm_open_impl(path, k, device, nthreads, budget_bytes, hash_bits, out);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dkm_open: ") + e.what());
    }
}
static int dkm_open_impl(const char *path, int32_t k, int device, int nthreads, int64_t budget_bytes, int32_t hash_bits, pmx_dbw **out)
{
    if (!path || !out) return fail(PMX_DBAM_ERR_INVALID, "null argument");
    *out = nullptr;
    if (k < (int32_t)fasta::K_MIN || k > (int32_t)fasta::K_MAX) return fail(PMX_DBAM_ERR_INVALID, fasta::bad_k_text(k));
    if (hash_bits < 1 || hash_bits > 64) return fail(PMX_DBAM_ERR_INVALID, "hash_bits must lie in [1, 64]");
    if (budget_bytes < 0) return fail(PMX_DBAM_ERR_INVALID, "budget_bytes < 0");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMX_DBAM_ERR_DEVICE, "no HIP device: the device ingest needs a GPU");
    if (device < 0 || device >= ndev) return fail(PMX_DBAM_ERR_INVALID, "no such device");
    HIPOK(hipSetDevice(device));
    if (nthreads <= 0) nthreads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency()));
    pmx_dbw *w = new pmx_dbw;
    w->device = device;
    w->kmer = true;
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    u64 budget = (u64)budget_bytes;
    if (budget == 0) {              // half of the free memory less the ingest margin (DEVICE_INGEST_MARGIN, inputs.py)
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess) fr = 0;
        budget = fr / 2 > (4ull << 30) + (1ull << 30) ? fr / 2 - (4ull << 30) : fr / 4;
    }
    int rc = 0;
    {
        TtDev g;                    // the packed genome
        KmGenome G;
        u8 *d_text = nullptr;
        u64 N = 0;
        rc = tt_upload(path, device, nthreads, &d_text, &N);
        if (!rc) rc = km_parse(w->stream, w->names, w->sizes, d_text, N, g, G);
        if (d_text) {
            (void)hipStreamSynchronize(w->stream);
            (void)hipFree(d_text);  // (the genome is packed: the text is not needed any more)
        }
        if (!rc) rc = km_build(*w, (u32)k, budget, (u32)hash_bits, G);
        (void)hipStreamSynchronize(w->stream);
    }
    if (!rc) rc = km_select(w, 0.f);
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
