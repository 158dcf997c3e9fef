// bigBed on the device (include/pymasc_amd_ingest.h, pmx_dbw_* with a bigBed file; DESIGN.md 7.12).  Included by bam_device.hip
// behind bigwig_device.inc, whose whole-file pass (bw_decode_all) runs it in place of k_bw_sections.
//
// A data block holds records  chromId u32, chromStart u32, chromEnd u32, rest of the BED line, NUL  (io/bigbed_parse.h).  Where
// record k+1 starts is a serial chain: one byte behind the first NUL at or beyond start_k + 12 -- and the 12 binary bytes may hold
// zeros themselves (chromId 0, start 256, ...), so the NULs alone do not give the starts.  One wavefront walks one block with a
// wave-uniform cursor: it loads a 64-byte window (a byte per lane) at cursor + 12, takes the mask of its zero bytes with one
// ballot, and resolves as many records as the mask reaches with scalar bit arithmetic; a new window is loaded only when the next
// NUL search leaves the current one.  The starts collect in a VGPR (lane k: the k-th start of the batch); at 64, or at the end of
// the block, every lane decodes one record, checks it, and the kept ones are written with ballot / popcount compaction at the
// block's place -- the output code of k_bw_sections.  The first bad record of the block (in record order) decides its status,
// as bigbed::walk_block decides on the host.

template <bool WRITE>
__global__ void __launch_bounds__(256)
k_bb_records(const u8 *__restrict__ base, const BwSpan *__restrict__ spans, u32 nblk, const u32 *__restrict__ chrom_lens, u32 nlens,
             float threshold, u32 *__restrict__ status, u32 *__restrict__ cnt, u32 *__restrict__ blk_chrom, const u64 *__restrict__ place,
             u32 *__restrict__ o_begin, u32 *__restrict__ o_end, float *__restrict__ o_value)
{
    const u32 m = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (m >= nblk) return;
    if (status[m]) return;
    const u64 off = ((u64)RFL((u32)(spans[m].off >> 32)) << 32) | RFL((u32)spans[m].off);
    const u8 *d = base + off;
    const u32 n = RFL(spans[m].size);     // (clamped to the block's share of the buffer: no load below reaches past it)
    const bool pass = !(threshold > 0.f && !(1.0f >= threshold));   // every record's value is 1
    u64 w = WRITE ? place[m] : 0;
    u32 total = 0, err = 0, first = 0, nlist = 0, my = 0, cur = 0, wbase = 0;
    u64 chrom_len = 0, zmask = 0;
    bool have_first = false, have_window = false;
    for (;;) {
        // the chain: up to 64 record starts (all wave-uniform but `my`)
        u32 serr = 0;
        while (nlist < 64u && cur < n) {
            if (n - cur < bigbed::RECORD_MIN) {
                serr = bigbed::BB_ERR_TRUNCATED;
                break;
            }
            u32 q = cur + 12u;      // the first NUL at or beyond q ends the record
            bool found = false;
            while (q < n) {
                if (!have_window || q < wbase || q - wbase >= 64u) {
                    wbase = q;
                    have_window = true;
                    const u32 at = q + lane;
                    zmask = __ballot(at < n && d[at] == 0);
                }
                const u64 mk = zmask >> (q - wbase);
                if (mk) {
                    q += (u32)__builtin_ctzll(mk);
                    found = true;
                    break;
                }
                q = wbase + 64u;
            }
            if (!found) {
                serr = bigbed::BB_ERR_NO_NUL;
                break;
            }
            if (lane == nlist) my = cur;
            nlist++;
            cur = q + 1u;
        }
        // the batch: one record per lane (each start has >= 13 bytes of the block behind it)
        if (nlist) {
            const bool act = lane < nlist;
            u32 c = 0, b = 0, e = 0;
            if (act) {
                c = ld32u(d + my);
                b = ld32u(d + my + 4);
                e = ld32u(d + my + 8);
            }
            if (!have_first) {      // (lane 0 holds the block's first record)
                first = RFL(c);
                have_first = true;
                chrom_len = first < nlens ? chrom_lens[first] : 0u;
            }
            const u32 lerr = !act ? 0u : e < b ? (u32)bigbed::BB_ERR_RANGE : c != first ? (u32)bigbed::BB_ERR_CHROM : 0u;
            const u64 em = __ballot(lerr != 0u);
            if (em) {
                err = RFL(__shfl((int)lerr, (int)__builtin_ctzll(em), 64));
                break;
            }
            const bool keep = act && !((u64)b >= chrom_len || e == 0u) && pass;
            const u64 mk = __ballot(keep);
            if (WRITE && keep) {
                const u64 at = w + (u64)__popcll(mk & ((1ull << lane) - 1ull));
                o_begin[at] = b;
                o_end[at] = e;
                o_value[at] = 1.0f;
            }
            const u32 k = (u32)__popcll(mk);
            w += k;
            total += k;
            nlist = 0;
        }
        if (serr) {
            err = serr;
            break;
        }
        if (cur >= n) break;
    }
    if (!WRITE && lane == 0) {
        if (err) status[m] = err;
        else {
            cnt[m] = total;
            if (have_first) blk_chrom[m] = first;
        }
    }
}

namespace {

void bb_launch_records(bool write, dim3 grid, hipStream_t s, const u8 *base, const BwSpan *spans, u32 nblk, const u32 *chrom_lens,
                       u32 nlens, float threshold, u32 *status, u32 *cnt, u32 *blk_chrom, const u64 *place, u32 *o_begin, u32 *o_end,
                       float *o_value)
{
    if (write)
        hipLaunchKernelGGL(k_bb_records<true>, grid, dim3(256), 0, s, base, spans, nblk, chrom_lens, nlens, threshold, status, cnt, blk_chrom,
                           place, o_begin, o_end, o_value);
    else
        hipLaunchKernelGGL(k_bb_records<false>, grid, dim3(256), 0, s, base, spans, nblk, chrom_lens, nlens, threshold, status, cnt,
                           blk_chrom, place, o_begin, o_end, o_value);
}

}  // namespace
