// Paired-end fragment sizes and the pair pileup (pmx_dbam_fragments_*, pmx_dbam_coverage_add_fragments; include/pymasc_amd_ingest.h;
// DESIGN.md 7.21).  Included at the end of bam_device.hip behind complexity_device.inc (CxRecs), region_mask_device.inc (rm_filter)
// and coverage_device.inc (k_cv_marks).  A pair is counted at its read1 record from that record's own fields: nothing is matched
// and nothing is held back between a stream's windows.
//
//   fr_classify   the pair rule on (flag, same reference, pos1, mate_pos1, tlen): which counter the record counts in, or its row
//   k_fr_walk<0> / k_bam_scan / k_fr_walk<1>   (BAM) k_bam_walk's record step over the verified chain with the 12 mate bytes read:
//                 the rows per piece and the counters (reduced over the wave, pass 0 only), then the rows written
//   k_sam_mates   (SAM) one lane per line of d_nl: mate_pos1, tlen and the same-reference bit by samtext::parse_mates, once per
//                 table, kept with the handle; k_fr_sam_keep / k_bam_scan / k_fr_sam_compact in the shape of k_sam_keep / k_sam_compact
//   rm_filter     an attached mask on the rows as they are: a row is (ref_id, start1, size, orientation) in a CxRecs
//   k_fr_hist     one lane per row: H[o][s - 1] += 1, through a per-workgroup LDS table for the sizes up to FR_LDS
// Memory: 8 * 3 * max_size bytes from begin to the next begin or close (1.5 MB at 65536), one byte per reference; 9 bytes per SAM
// line once a pair call has run; 13 bytes per row inside a call.

#define FR_LDS 4096u                          // sizes 1 .. FR_LDS of every orientation are counted in LDS
#define FR_GRID 256u                          // workgroups of k_fr_hist at most (unless 2^31 rows per workgroup would be passed)

enum { FR_NOT_PAIRED = 0, FR_MATE_UNMAPPED = 1, FR_MATE_ELSEWHERE = 2, FR_NO_SIZE = 3, FR_OVER = 4, FR_ROW = 7 };
enum { FRC_READS = 0, FRC_PAIRED = 1, FRC_OVER = 5, FRC_ROWS = 8, FRC_MASKED = 9 };

// The pair rule (the first that holds wins): FR_NOT_PAIRED, FR_MATE_UNMAPPED, FR_MATE_ELSEWHERE, FR_NO_SIZE, FR_OVER + orientation,
// or FR_ROW with start1 / size / orient set.  Orientation: 0 FR, 1 RF, 2 TANDEM.
__device__ __forceinline__ u32 fr_classify(u32 flag, bool same_ref, int pos1, int mate_pos1, int tlen, u32 max_size, int &start1, u32 &size,
                                           u32 &orient)
{
    if (!(flag & 0x1u)) return FR_NOT_PAIRED;
    if (flag & 0x8u) return FR_MATE_UNMAPPED;
    if (!same_ref) return FR_MATE_ELSEWHERE;
    if (tlen == 0 || tlen == (int)0x80000000u || mate_pos1 <= 0) return FR_NO_SIZE;
    size = tlen < 0 ? 0u - (u32)tlen : (u32)tlen;
    const bool rev = (flag & 0x10u) != 0, mate_rev = (flag & 0x20u) != 0;
    orient = rev == mate_rev ? 2u : ((!rev && tlen > 0) || (rev && tlen < 0)) ? 0u : 1u;
    if (size > max_size) return FR_OVER + orient;
    start1 = pos1 < mate_pos1 ? pos1 : mate_pos1;
    return FR_ROW;
}

struct FrArgs {
    u32 max_size;
    u32 fr_only;                     // rows of orientation FR only (the pair pileup); the counters are not taken then
    const u8 *use;                   // per reference: chosen (null: every reference)
    unsigned long long *counters;    // (pass 0) FRC_ROWS + 1 sums
};

// a lane's counters into the global ones: summed over the wave first, one atomic per counter and wave
__device__ __forceinline__ void fr_reduce(const u32 *c, unsigned long long *counters)
{
#pragma unroll
    for (u32 k = 0; k <= FRC_ROWS; k++) {
        u32 v = c[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
        if ((threadIdx.x & 63u) == 0 && v) atomicAdd(&counters[k], (unsigned long long)v);
    }
}

// PASS 0: count the rows of every piece (A.kept) and the counters; 1: write the rows, report malformed records.  The record step
// is k_bam_walk's: every byte read lies inside [s, s + 4 + bs) with bs >= 32, which the step checks against A.N first.
template <int PASS>
__global__ void __launch_bounds__(64) k_fr_walk(const WalkArgs A, const FrArgs F)
{
    const u64 c = (u64)blockIdx.x * 64u + threadIdx.x;
    u32 cn[FRC_ROWS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (c < A.npieces) {
        u64 s = A.spec[c];
        const u64 cend = (c + 1u) * WALK_PIECE;
        const u8 *__restrict__ D = A.D;
        u32 nrows = 0;
        u64 w = PASS == 1 ? A.kept_base[c] : 0;
        while (s < cend && s < A.N) {
            u32 err = 0, bs = 0;
            if (s + 4u > A.N) {
                err = REC_ERR_EOF;
            } else {
                bs = ld32u(D + s);
                if (bs < 32u) err = REC_ERR_BS;
                else if (s + 4u + bs > A.N) err = REC_ERR_EOF;
            }
            const u8 *rec = D + s + 4;
            u32 l_name = 0, n_cig = 0;
            int ref = -1;
            if (!err) {
                ref = (int)ld32u(rec);
                l_name = rec[8];
                n_cig = ld16u(rec + 12);
                if (32ull + l_name + 4ull * n_cig > bs) err = REC_ERR_SHORT;
                else if (ref >= A.nref) err = REC_ERR_REF;
            }
            if (err) {
                if (PASS == 1) atomicMin(A.first_error, (unsigned long long)((s << 4) | err));
                break;
            }
            const u32 mapq = rec[9], flag = ld16u(rec + 14);
            if (!((flag & A.flag_exclude) || mapq < A.mapq_min || ref < 0 || (F.use && !F.use[ref]))) {
                const u32 l_seq = ld32u(rec + 16);
                const u8 *cig = rec + 32u + l_name;
                u32 n = n_cig;
                long_cigar(rec, bs, l_name, n_cig, l_seq, cig, n);
                if (cigar_qlen(cig, n)) {
                    const int pos1 = (int)(ld32u(rec + 4) + 1u), mref = (int)ld32u(rec + 20), mpos1 = (int)(ld32u(rec + 24) + 1u);
                    const int tlen = (int)ld32u(rec + 28);
                    int start1 = 0;
                    u32 size = 0, orient = 0;
                    const u32 k = fr_classify(flag, mref == ref, pos1, mpos1, tlen, F.max_size, start1, size, orient);
                    cn[FRC_READS]++;
                    if (k != FR_NOT_PAIRED) cn[FRC_PAIRED]++;
                    if (k >= FR_MATE_UNMAPPED && k < FR_ROW) cn[k + 1u]++;
                    if (k == FR_ROW && !(F.fr_only && orient)) {
                        if (PASS == 1) {
                            A.o_ref[w] = ref;
                            A.o_pos[w] = start1;
                            A.o_len[w] = (int)size;
                            A.o_rev[w] = (u8)orient;
                            w++;
                        }
                        nrows++;
                    }
                }
            }
            s += 4ull + bs;
        }
        cn[FRC_ROWS] = nrows;
        if (PASS == 0) A.kept[c] = nrows;
    }
    if (PASS == 0) fr_reduce(cn, F.counters);
}

// fields 7-9 of every record line, once per line table
__global__ void __launch_bounds__(256) k_sam_mates(const u8 *__restrict__ D, u64 beg, const u64 *__restrict__ nl, u64 nrec,
                                                   int *__restrict__ o_mpos, int *__restrict__ o_tlen, u8 *__restrict__ o_same,
                                                   unsigned long long *__restrict__ first_err)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= nrec) return;
    DevSrc s{D, ~0ull, make_uint4(0, 0, 0, 0)};
    samtext::Mates m;
    m.mate_pos1 = m.tlen = 0;
    m.same = 0;
    const u32 e = samtext::parse_mates(s, i ? nl[i - 1] + 1u : beg, nl[i], m);
    if (e) atomicMin(first_err, (unsigned long long)((i << 8) | e));
    o_mpos[i] = m.mate_pos1;
    o_tlen[i] = m.tlen;
    o_same[i] = (u8)m.same;
}

struct FrSam {
    const int *ref, *pos, *mpos, *tlen;
    const u32 *qlen, *fm;
    const u8 *same;
    u64 nrec;
    u32 mapq_min, flag_exclude;
};

// line i under the run's filter and the pair rule; true: it is a row
__device__ __forceinline__ bool fr_sam_row(const FrSam &S, const FrArgs &F, u64 i, u32 *cn, int &start1, u32 &size, u32 &orient)
{
    if (i >= S.nrec || !sam_keep(S.ref, S.qlen, S.fm, i, S.mapq_min, S.flag_exclude, -1)) return false;
    if (F.use && !F.use[S.ref[i]]) return false;
    const u32 k = fr_classify(S.fm[i] & 0xffffu, S.same[i] != 0, S.pos[i], S.mpos[i], S.tlen[i], F.max_size, start1, size, orient);
    cn[FRC_READS]++;
    if (k != FR_NOT_PAIRED) cn[FRC_PAIRED]++;
    if (k >= FR_MATE_UNMAPPED && k < FR_ROW) cn[k + 1u]++;
    if (k != FR_ROW || (F.fr_only && orient)) return false;
    cn[FRC_ROWS]++;
    return true;
}

__global__ void __launch_bounds__(256) k_fr_sam_keep(const FrSam S, const FrArgs F, u32 *__restrict__ bcnt)
{
    u32 cn[FRC_ROWS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int start1;
    u32 size, orient;
    const bool k = fr_sam_row(S, F, (u64)blockIdx.x * 256u + threadIdx.x, cn, start1, size, orient);
    const int n = __syncthreads_count(k);
    if (threadIdx.x == 0) bcnt[blockIdx.x] = (u32)n;
    fr_reduce(cn, F.counters);
}

__global__ void __launch_bounds__(256) k_fr_sam_compact(const FrSam S, const FrArgs F, const u64 *__restrict__ bbase, int *__restrict__ o_ref,
                                                        int *__restrict__ o_pos, int *__restrict__ o_len, u8 *__restrict__ o_rev)
{
    __shared__ u32 s_wave[4];
    const u32 t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    const u64 i = (u64)blockIdx.x * 256u + t;
    u32 cn[FRC_ROWS + 1] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    int start1 = 0;
    u32 size = 0, orient = 0;
    const bool k = fr_sam_row(S, F, i, cn, start1, size, orient);
    const u64 m = __ballot(k);
    if (lane == 0) s_wave[wave] = (u32)__popcll(m);
    __syncthreads();
    if (!k) return;
    u64 o = bbase[blockIdx.x] + (u64)__popcll(m & ((1ull << lane) - 1ull));
    for (u32 w = 0; w < wave; w++) o += s_wave[w];
    o_ref[o] = S.ref[i];
    o_pos[o] = start1;
    o_len[o] = (int)size;
    o_rev[o] = (u8)orient;
}

// H[o][s - 1] += 1 for every row (s = len[i] in 1 .. max_size, o = rev[i] in 0 .. 2: the row filter gives nothing else, and a row
// outside is skipped, never counted elsewhere).  Sizes pile up on a few hundred values: a row of size <= FR_LDS adds to a 32-bit
// LDS cell of its orientation (3 * FR_LDS cells, 48 KB), and the table is flushed with one 64-bit global atomic per non-zero cell.
// Global atomics on one address are taken one after the other (about 1 ns each when measured here: 0.74 M of them, from RF and
// TANDEM rows that an earlier form sent past the LDS table, took 0.8 ms), and the flushes of all workgroups land on the same few
// hundred addresses, so there are few workgroups -- at most FR_GRID, of 1024 lanes, striding over the rows -- and each flushes
// once.  Flush bound: a cell holds at most the rows of its workgroup, n / gridDim.x + 1024, and the launch keeps n / gridDim.x
// below 2^31.  A row above FR_LDS (few, and spread over many sizes) is combined with the lanes of its wave that hold the same
// cell -- one 64-bit global atomic per distinct cell and wave.
__global__ void __launch_bounds__(1024) k_fr_hist(const int *__restrict__ len, const u8 *__restrict__ rev, u64 n, u32 max_size,
                                                  unsigned long long *__restrict__ H)
{
    __shared__ u32 s_h[3u * FR_LDS];
    const u32 t = threadIdx.x, top = max_size < FR_LDS ? max_size : FR_LDS;
    for (u32 i = t; i < 3u * top; i += 1024u) s_h[i] = 0;
    __syncthreads();
    for (u64 i0 = (u64)blockIdx.x * 1024u; i0 < n; i0 += (u64)gridDim.x * 1024u) {      // (the same trip count in every lane)
        const u64 i = i0 + t;
        u32 cell = ~0u;                                  // (o * max_size + s - 1 of a row that goes to the global table)
        if (i < n) {
            const u32 s = (u32)len[i], o = rev[i];
            if (s >= 1u && s <= max_size && o < 3u) {
                if (s <= top) atomicAdd(&s_h[o * top + (s - 1u)], 1u);
                else cell = o * max_size + (s - 1u);
            }
        }
        u64 todo = __ballot(cell != ~0u);
        while (todo) {                                   // (the same in every lane of the wave)
            const u32 lead = (u32)__builtin_ctzll(todo);
            const u32 c0 = (u32)__shfl((int)cell, (int)lead, 64);
            const u64 same = __ballot(cell == c0);
            if ((t & 63u) == lead) atomicAdd(&H[c0], (unsigned long long)__popcll(same));
            todo &= ~same;
        }
    }
    __syncthreads();
    for (u32 i = t; i < 3u * top; i += 1024u)
        if (s_h[i]) atomicAdd(&H[(i / top) * max_size + i % top], (unsigned long long)s_h[i]);
}

namespace {

struct FrEvents {
    hipEvent_t a = nullptr, z = nullptr;
    ~FrEvents()
    {
        if (a) (void)hipEventDestroy(a);
        if (z) (void)hipEventDestroy(z);
    }
};

int fr_check_handle(pmx_dbam *b, const char *who)
{
    if (!b) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    if (b->bed) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": the input has no mate fields");
    return 0;
}

int fr_check_size(u32 max_size, const char *who)
{
    if (max_size >= 1u && max_size <= PMX_FRAGMENTS_MAX_SIZE) return 0;
    return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": max_size is " + std::to_string(max_size) + ": it must lie in [1, " +
                                          std::to_string(PMX_FRAGMENTS_MAX_SIZE) + "]");
}

// the mate table of the SAM lines the handle holds now: parsed the first time a pair call needs it
int fr_sam_mates(pmx_dbam *b)
{
    if (b->d_smpos || b->sam_lines == 0) return 0;
    const u64 n = b->sam_lines;
    hipStream_t st = b->stream;
    DevAlloc d_err, mpos, tlen, same;
    HIPOK(hipMalloc(&d_err.p, 8));
    HIPOK(hipMalloc(&mpos.p, 4 * n));
    HIPOK(hipMalloc(&tlen.p, 4 * n));
    HIPOK(hipMalloc(&same.p, n));
    HIPOK(hipMemsetAsync(d_err.p, 0xff, 8, st));
    hipLaunchKernelGGL(k_sam_mates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, b->d_out, b->data_beg, b->d_nl, n, mpos.as<int>(),
                       tlen.as<int>(), same.as<u8>(), d_err.as<unsigned long long>());
    HIPOK(hipGetLastError());
    unsigned long long fe = 0;
    HIPOK(hipMemcpyAsync(&fe, d_err.p, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (fe != ~0ull)
        return fail(PMX_DBAM_ERR_FORMAT, "line " + std::to_string(b->sam_line0 + (fe >> 8) + 1) + ": " + samtext::err_text((u32)(fe & 255u)));
    b->d_smpos = mpos.as<int>();
    b->d_stlen = tlen.as<int>();
    b->d_ssame = same.as<u8>();
    mpos.p = tlen.p = same.p = nullptr;
    if (b->st) stream_note(*b);
    return 0;
}

// The rows of what the handle holds now into R, after an attached mask; counters (FRC_MASKED + 1, may be null) of this call.
// A sibling of cx_filter: the same chain, scans and mask, rows instead of reads.
int fr_filter(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, u32 max_size, const u8 *d_use, bool fr_only, CxRecs &R, u64 *counters)
{
    hipStream_t st = b->stream;
    R.n = 0;
    if (counters)
        for (u32 k = 0; k <= FRC_MASKED; k++) counters[k] = 0;
    u64 totals[2] = {0, 0};
    DevAlloc d_kept, d_base, d_tot, d_c;
    HIPOK(hipMalloc(&d_tot.p, 16));
    HIPOK(hipMalloc(&d_c.p, 8 * (FRC_ROWS + 1)));
    HIPOK(hipMemsetAsync(d_c.p, 0, 8 * (FRC_ROWS + 1), st));
    FrArgs F;
    F.max_size = max_size;
    F.fr_only = fr_only ? 1u : 0u;
    F.use = d_use;
    F.counters = d_c.as<unsigned long long>();
    unsigned long long hc[FRC_ROWS + 1];
    auto finish = [&]() -> int {      // the mask on the rows, the counters of the call
        u64 m = totals[0];
        if (int rc = rm_filter(b, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(), R.rev.as<u8>(), m, &m)) return rc;
        R.n = m;
        if (counters) {
            for (u32 k = 0; k <= FRC_ROWS; k++) counters[k] = hc[k];
            counters[FRC_MASKED] = totals[0] - m;
        }
        return 0;
    };
    if (b->sam && b->sam_lines > 0) {
        if (int rc = fr_sam_mates(b)) return rc;
        const u64 n = b->sam_lines, nb = (n + 255) / 256;
        HIPOK(hipMalloc(&d_kept.p, 4 * nb));
        HIPOK(hipMalloc(&d_base.p, 8 * nb));
        const FrSam S{b->d_sref, b->d_spos, b->d_smpos, b->d_stlen, b->d_sqlen, b->d_sfm, b->d_ssame, n, mapq_min, flag_exclude};
        hipLaunchKernelGGL(k_fr_sam_keep, dim3((unsigned)nb), dim3(256), 0, st, S, F, d_kept.as<u32>());
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_kept.as<u32>(), d_kept.as<u32>(), nb, d_base.as<u64>(), d_tot.as<u64>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(totals, d_tot.p, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(hc, d_c.p, sizeof hc, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (int rc = R.alloc(totals[0])) return rc;
        hipLaunchKernelGGL(k_fr_sam_compact, dim3((unsigned)nb), dim3(256), 0, st, S, F, d_base.as<u64>(), R.ref.as<int>(), R.pos.as<int>(),
                           R.len.as<int>(), R.rev.as<u8>());
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(st));
        return finish();
    }
    if (!b->sam && b->npieces > 0) {
        const u64 np = b->npieces;
        WalkArgs A;
        A.D = b->d_out + b->data_beg;
        A.N = b->N - b->data_beg;
        A.nref = (int)b->ref_names.size();
        A.want_ref = -1;
        A.o_ref = A.o_pos = A.o_len = nullptr;
        A.o_rev = nullptr;
        if (!b->chain_ready) {   // (as cx_filter: the chain's counts are decode's scratch)
            A.mapq_min = 0;
            A.flag_exclude = 0;
            if (int rc = walk_chain(b, A)) return rc;
        }
        DevAlloc d_err;
        HIPOK(hipMalloc(&d_kept.p, 4 * np));
        HIPOK(hipMalloc(&d_base.p, 8 * np));
        HIPOK(hipMalloc(&d_err.p, 8));
        A.mapq_min = mapq_min;
        A.flag_exclude = flag_exclude;
        A.npieces = np;
        A.spec = b->d_spec;          // (read only: the verified piece starts)
        A.end = nullptr;
        A.cnt = nullptr;
        A.kept = d_kept.as<u32>();
        A.kept_base = d_base.as<u64>();
        A.first_error = d_err.as<unsigned long long>();
        A.nmis = nullptr;
        const dim3 wg((unsigned)((np + 63) / 64));
        hipLaunchKernelGGL(k_fr_walk<0>, wg, dim3(64), 0, st, A, F);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, st, d_kept.as<u32>(), d_kept.as<u32>(), np, d_base.as<u64>(), d_tot.as<u64>());
        HIPOK(hipGetLastError());
        HIPOK(hipMemcpyAsync(totals, d_tot.p, 16, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(hc, d_c.p, sizeof hc, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (int rc = R.alloc(totals[0])) return rc;
        A.o_ref = R.ref.as<int>();
        A.o_pos = R.pos.as<int>();
        A.o_len = R.len.as<int>();
        A.o_rev = R.rev.as<u8>();
        HIPOK(hipMemsetAsync(d_err.p, 0xff, 8, st));
        hipLaunchKernelGGL(k_fr_walk<1>, wg, dim3(64), 0, st, A, F);
        HIPOK(hipGetLastError());
        unsigned long long fe = 0;
        HIPOK(hipMemcpyAsync(&fe, d_err.p, 8, hipMemcpyDeviceToHost, st));
        HIPOK(hipStreamSynchronize(st));
        if (fe != ~0ull) return record_error(fe);
        return finish();
    }
    return 0;
}

int fr_use_to_device(pmx_dbam *b, const uint8_t *use_ref, DevAlloc &d)
{
    const u64 nref = b->ref_names.size();
    if (!use_ref || nref == 0) return 0;
    std::vector<u8> u(nref);
    for (u64 r = 0; r < nref; r++) u[r] = use_ref[r] ? 1 : 0;
    HIPOK(hipMalloc(&d.p, nref));
    HIPOK(hipMemcpy(d.p, u.data(), nref, hipMemcpyHostToDevice));
    return 0;
}

int fragments_begin_impl(pmx_dbam *b, u32 max_size, const uint8_t *use_ref)
{
    const char *who = "pmx_dbam_fragments_begin";
    if (int rc = fr_check_handle(b, who)) return rc;
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipStreamSynchronize(b->stream));
    b->fr = Fragments{};
    if (int rc = fr_check_size(max_size, who)) return rc;
    DevAlloc use;
    if (int rc = fr_use_to_device(b, use_ref, use)) return rc;
    HIPOK(hipMalloc(&b->fr.hist.p, 8ull * 3u * max_size));
    HIPOK(hipMemsetAsync(b->fr.hist.p, 0, 8ull * 3u * max_size, b->stream));
    HIPOK(hipStreamSynchronize(b->stream));
    b->fr.use = std::move(use);
    b->fr.max = max_size;
    if (b->st) stream_note(*b);
    return 0;
}

int fragments_add_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, uint64_t *rows_added)
{
    const char *who = "pmx_dbam_fragments_add";
    if (int rc = fr_check_handle(b, who)) return rc;
    if (!rows_added) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": null output");
    *rows_added = 0;
    if (!b->fr.on()) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": no table: call pmx_dbam_fragments_begin first");
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    CxRecs R;
    u64 c[PMX_FRAGMENTS_COUNTERS];
    const double t0 = now_s();
    if (int rc = fr_filter(b, mapq_min, flag_exclude, b->fr.max, b->fr.use.as<u8>(), false, R, c)) return rc;
    b->fr.t[0] += now_s() - t0;
    if (R.n) {
        FrEvents ev;                             // (HIP events around the one kernel: pmx_dbam_fragments_timings)
        HIPOK(hipEventCreate(&ev.a));
        HIPOK(hipEventCreate(&ev.z));
        HIPOK(hipEventRecord(ev.a, st));
        const u64 grid = std::max<u64>(std::min<u64>((R.n + 1023) / 1024, FR_GRID), (R.n >> 31) + 1u);
        hipLaunchKernelGGL(k_fr_hist, dim3((unsigned)grid), dim3(1024), 0, st, R.len.as<int>(), R.rev.as<u8>(), R.n, b->fr.max,
                           b->fr.hist.as<unsigned long long>());
        HIPOK(hipGetLastError());
        HIPOK(hipEventRecord(ev.z, st));
        HIPOK(hipStreamSynchronize(st));         // (R is freed on return)
        float ms = 0;
        HIPOK(hipEventElapsedTime(&ms, ev.a, ev.z));
        b->fr.t[1] += 1e-3 * (double)ms;
    }
    for (u32 k = 0; k < PMX_FRAGMENTS_COUNTERS; k++) b->fr.c[k] += c[k];
    *rows_added = R.n;
    return 0;
}

int fragments_tables_impl(pmx_dbam *b, uint64_t *hist, uint64_t *counters)
{
    const char *who = "pmx_dbam_fragments_tables";
    if (int rc = fr_check_handle(b, who)) return rc;
    if (!hist || !counters) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": null output");
    if (!b->fr.on()) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": no table: call pmx_dbam_fragments_begin first");
    HIPOK(hipSetDevice(b->device));
    HIPOK(hipMemcpyAsync(hist, b->fr.hist.p, 8ull * 3u * b->fr.max, hipMemcpyDeviceToHost, b->stream));
    HIPOK(hipStreamSynchronize(b->stream));
    for (u32 k = 0; k < PMX_FRAGMENTS_COUNTERS; k++) counters[k] = b->fr.c[k];
    return 0;
}

int64_t fragments_rows_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, u32 max_size, const uint8_t *use_ref, int64_t cap, int32_t *ref_id,
                            int32_t *start1, int32_t *size, uint8_t *orient)
{
    const char *who = "pmx_dbam_fragments_rows";
    if (int rc = fr_check_handle(b, who)) return rc;
    if (int rc = fr_check_size(max_size, who)) return rc;
    if (cap < 0 || (cap > 0 && (!ref_id || !start1 || !size || !orient))) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": null output");
    HIPOK(hipSetDevice(b->device));
    DevAlloc use;
    if (int rc = fr_use_to_device(b, use_ref, use)) return rc;
    CxRecs R;
    if (int rc = fr_filter(b, mapq_min, flag_exclude, max_size, use.as<u8>(), false, R, nullptr)) return rc;
    if (cap == 0 || R.n == 0) return (int64_t)R.n;
    if ((u64)cap < R.n) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": cap is below the number of rows");
    hipStream_t st = b->stream;
    HIPOK(hipMemcpyAsync(ref_id, R.ref.p, 4 * R.n, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(start1, R.pos.p, 4 * R.n, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(size, R.len.p, 4 * R.n, hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(orient, R.rev.p, R.n, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return (int64_t)R.n;
}

// the FR rows piled at their own extent: orientation FR is 0, so the rows are forward reads of `size` bases to k_cv_marks
int coverage_add_fragments_impl(pmx_dbam *b, u32 mapq_min, u32 flag_exclude, u32 max_size, uint64_t *added_out)
{
    const char *who = "pmx_dbam_coverage_add_fragments";
    if (int rc = fr_check_handle(b, who)) return rc;
    if (!added_out) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": null output");
    *added_out = 0;
    if (int rc = fr_check_size(max_size, who)) return rc;
    if (!b->cv.on()) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": no table: call pmx_dbam_coverage_begin first");
    if (b->cv.ext) return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": the table was begun with an extend: begin it with 0");
    HIPOK(hipSetDevice(b->device));
    hipStream_t st = b->stream;
    CxRecs R;
    if (int rc = fr_filter(b, mapq_min, flag_exclude, max_size, nullptr, true, R, nullptr)) return rc;
    if (R.n == 0) return 0;
    if (b->cv.reads + R.n >= CV_MAX_READS)
        return fail(PMX_DBAM_ERR_INVALID, std::string(who) + ": 2^31 reads or more: the depth is a 32-bit count");
    DevAlloc d_added;
    HIPOK(hipMalloc(&d_added.p, 8));
    HIPOK(hipMemsetAsync(d_added.p, 0, 8, st));
    hipLaunchKernelGGL(k_cv_marks, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, R.ref.as<int>(), R.pos.as<int>(), R.len.as<int>(),
                       R.rev.as<u8>(), R.n, b->cv.tab.as<long long>(), (u32)b->ref_names.size(), 0u, b->cv.table.as<int>(),
                       d_added.as<unsigned long long>());
    HIPOK(hipGetLastError());
    unsigned long long added = 0;
    HIPOK(hipMemcpyAsync(&added, d_added.p, 8, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    b->cv.reads += added;
    *added_out = added;
    return 0;
}

}  // namespace

extern "C" {

int pmx_dbam_fragments_begin(pmx_dbam *b, uint32_t max_size, const uint8_t *use_ref)
{
    return guarded("pmx_dbam_fragments_begin", [&] { return fragments_begin_impl(b, max_size, use_ref); });
}

int pmx_dbam_fragments_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t *rows_added)
{
    return guarded("pmx_dbam_fragments_add", [&] { return fragments_add_impl(b, mapq_min, flag_exclude, rows_added); });
}

int pmx_dbam_fragments_timings(pmx_dbam *b, double seconds[2])
{
    if (!b || !seconds) return fail(PMX_DBAM_ERR_INVALID, "pmx_dbam_fragments_timings: null argument");
    seconds[0] = b->fr.t[0];
    seconds[1] = b->fr.t[1];
    return 0;
}

int pmx_dbam_fragments_tables(pmx_dbam *b, uint64_t *hist, uint64_t counters[PMX_FRAGMENTS_COUNTERS])
{
    return guarded("pmx_dbam_fragments_tables", [&] { return fragments_tables_impl(b, hist, counters); });
}

int64_t pmx_dbam_fragments_rows(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint32_t max_size, const uint8_t *use_ref, int64_t cap,
                                int32_t *ref_id, int32_t *start1, int32_t *size, uint8_t *orient)
{
    return guarded("pmx_dbam_fragments_rows",
                   [&] { return fragments_rows_impl(b, mapq_min, flag_exclude, max_size, use_ref, cap, ref_id, start1, size, orient); });
}

int pmx_dbam_coverage_add_fragments(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint32_t max_size, uint64_t *added)
{
    return guarded("pmx_dbam_coverage_add_fragments", [&] { return coverage_add_fragments_impl(b, mapq_min, flag_exclude, max_size, added); });
}

}  // extern "C"
