// BAM -> filtered (ref_id, pos, query length, strand) arrays for the MI355X calculator.
//
// Replaces the reference's per-read Python loop (PyMaSC/handler/calc.py:140-153 iterating a pysam.AlignmentFile,
// handler/read.py:62-155 filtering and extracting) with a windowed, multi-threaded native reader:
//
//   file (mmap) --scan BGZF headers--> window of <= WINDOW_BLOCKS blocks --parallel raw-inflate + CRC32-->
//   contiguous uncompressed bytes (+ the partial record carried from the previous window)
//   --serial hop over block_size fields--> record offsets --parallel decode + filter--> compact arrays
//
// A producer thread runs that pipeline one window ahead of the consumer (pmx_bam_next_batch), so the serial hops
// and the caller's own work (numpy, host->device copies, kernels) overlap the inflation of the next window.
//
// Formats: SAM/BAM spec v1 section 4.1 (BGZF: gzip members with a 'BC' extra subfield holding BSIZE, <= 64 KiB of
// payload each) and 4.2 (BAM header and alignment records, little endian).  pysam/htslib are absent from this
// image; what they would have returned for the fields used here is fixed by the spec, and the parity test replays
// the reference's own BAM <-> SAM twin (tests/data/ENCFF000RMB-test.{bam,sam}).
#include "../../../include/pymasc_amd_io.h"
#include "bai_index.h"
#include "io_common.h"

#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_map>
#include <vector>

namespace {

constexpr uint32_t WINDOW_BLOCKS = 1024;       // <= 64 MiB of uncompressed data per window
constexpr size_t QUEUE_DEPTH = 2;              // decoded windows waiting for the consumer
constexpr size_t BGZF_HEADER = 18, BGZF_FOOTER = 8;

struct Block {
    const uint8_t *cdata;   // raw deflate stream
    uint32_t clen;
    uint32_t isize;         // uncompressed size (footer)
    uint32_t crc;
    size_t out_off;
};

// Byte buffer that grows without zero-filling (std::vector::resize would memset every window).
struct RawBuf {
    uint8_t *p = nullptr;
    size_t n = 0, cap = 0;
    ~RawBuf() { free(p); }
    uint8_t *data() { return p; }
    const uint8_t *data() const { return p; }
    size_t size() const { return n; }
    void resize(size_t m)
    {
        if (m > cap) {
            const size_t c = std::max(m, cap + cap / 2);
            uint8_t *q = (uint8_t *)realloc(p, c);
            if (!q) throw pmx_io::Error(PMX_IO_ERR_OPEN, "out of memory");
            p = q;
            cap = c;
        }
        n = m;
    }
};

// decoded, filtered records of one window
struct Window {
    std::vector<int32_t> ref, pos, len;
    std::vector<uint8_t> rev;
    std::vector<uint16_t> flag;                  // (pmx_bam_next_mates only: the raw flag and the three mate fields)
    std::vector<int32_t> mref, mpos, tlen;
};

inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline int32_t le32s(const uint8_t *p) { return (int32_t)le32(p); }

}  // namespace

struct pmx_bam {
    pmx_io::MappedFile file;
    size_t next_off = 0;            // file offset of the next BGZF block to scan
    bool eof = false;
    int nthreads = 1;

    std::string text;
    std::vector<std::string> ref_names;
    std::vector<int64_t> ref_lens;

    RawBuf buf;                     // [carry | inflated window]
    size_t carry = 0;               // bytes of an incomplete record at the front of buf
    std::vector<Block> blocks;
    std::vector<size_t> rec_off;

    // consumer side: the window being handed out
    Window cur;
    size_t w_cursor = 0;

    // producer thread and its hand-over queue (started by the first pmx_bam_next_batch, when the filter is known)
    std::thread producer;
    std::mutex mu;
    std::condition_variable cv;
    std::deque<Window> queue;
    bool done = false, stop = false;
    int err_code = 0;
    std::string err_msg;

    bool filter_set = false;
    uint32_t mapq_min = 0, flag_exclude = 0;
    bool mates = false;             // the pass was begun by pmx_bam_next_mates: the windows carry the mate columns

    // .bai index: per reference the virtual file offsets [beg, end) of its records (SAM spec 5.2)
    using RefRange = pmx_bai::RefRange;
    std::vector<RefRange> index;
    bool have_index = false;
    // region mode (pmx_bam_fetch_ref): only records of want_ref, blocks up to the one holding the range's end
    int32_t want_ref = -1;
    size_t stop_block = SIZE_MAX;   // file offset of the last BGZF block that belongs to the region
    size_t skip = 0;                // bytes of the first inflated block that precede the region
    uint64_t data_beg = 0;          // virtual offset of the first alignment record (rewind target)
    bool pristine = true;           // nothing read since open: a rewind has nothing to do
    std::atomic<uint64_t> n_records{0}, n_kept{0}, bytes_out{0}, bytes_in{0};
    size_t hdr_len = 0;             // bytes of the BAM header at the front of the uncompressed stream
    // read-length histogram of the last pmx_bam_readlen_hist (length, count, first key), sorted by length, and its counters
    struct LenBin {
        int32_t len;
        uint64_t count, first;
    };
    std::vector<LenBin> rl_hist;
    uint64_t rl_counters[6] = {0, 0, 0, 0, 0, 0};
    bool rl_valid = false;
    uint32_t rl_mapq = 0;
    double t_scan = 0, t_alloc = 0, t_inflate = 0, t_walk = 0, t_decode = 0, t_concat = 0;   // PMX_IO_TIMING=1
};

namespace {

inline double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Parses the BGZF member at `off`; false at a clean end of file.  Throws on a malformed member.
bool scan_block(const uint8_t *base, size_t size, size_t off, Block &blk, size_t &next)
{
    if (off == size) return false;
    if (off + BGZF_HEADER + BGZF_FOOTER > size) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "truncated BGZF block header");
    const uint8_t *p = base + off;
    if (p[0] != 0x1f || p[1] != 0x8b || p[2] != 8 || !(p[3] & 4))
        throw pmx_io::Error(PMX_IO_ERR_FORMAT, "not a BGZF block (bad gzip magic / no extra field)");
    const uint32_t xlen = le16(p + 10);
    if (off + 12 + xlen + BGZF_FOOTER > size) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "truncated BGZF extra field");
    uint32_t bsize = 0;
    bool found = false;
    for (uint32_t x = 0; x + 4 <= xlen;) {
        const uint8_t *s = p + 12 + x;
        const uint32_t slen = le16(s + 2);
        if (s[0] == 'B' && s[1] == 'C' && slen == 2 && x + 6 <= xlen) {
            bsize = le16(s + 4);
            found = true;
            break;
        }
        x += 4 + slen;
    }
    if (!found) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "gzip member without the BGZF 'BC' subfield");
    const size_t total = (size_t)bsize + 1;
    if (total < 12 + xlen + BGZF_FOOTER || off + total > size)
        throw pmx_io::Error(PMX_IO_ERR_FORMAT, "truncated BGZF block");
    blk.cdata = p + 12 + xlen;
    blk.clen = (uint32_t)(total - 12 - xlen - BGZF_FOOTER);
    blk.crc = le32(p + total - 8);
    blk.isize = le32(p + total - 4);
    if (blk.isize > 65536) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BGZF block larger than 64 KiB");
    next = off + total;
    return true;
}

void inflate_block(const Block &blk, uint8_t *dst)
{
    if (blk.isize == 0) return;
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "zlib: inflateInit2 failed");
    zs.next_in = const_cast<Bytef *>(blk.cdata);
    zs.avail_in = blk.clen;
    zs.next_out = dst;
    zs.avail_out = blk.isize;
    const int rc = inflate(&zs, Z_FINISH);
    const bool ok = rc == Z_STREAM_END && zs.avail_out == 0;
    inflateEnd(&zs);
    if (!ok) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BGZF block does not inflate to its recorded size");
    if ((uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, blk.isize) != blk.crc)
        throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BGZF block CRC32 mismatch");
}

using pmx_io::parallel_for;

// Appends the next window of inflated bytes behind the carried partial record.  Returns false when no block is left.
bool load_window(pmx_bam &b, uint32_t max_blocks)
{
    b.blocks.clear();
    size_t out = b.carry;
    double t0 = now_s();
    while (b.blocks.size() < max_blocks) {
        Block blk;
        size_t next;
        if (b.next_off > b.stop_block || !scan_block(b.file.data, b.file.size, b.next_off, blk, next)) {
            b.eof = true;
            break;
        }
        blk.out_off = out;
        out += blk.isize;
        b.bytes_in += next - b.next_off;
        b.next_off = next;
        b.blocks.push_back(blk);
    }
    if (b.blocks.empty()) return false;
    double t1 = now_s();
    b.t_scan += t1 - t0;
    b.buf.resize(out);
    uint8_t *dst = b.buf.data();
    t0 = now_s();
    b.t_alloc += t0 - t1;
    const std::vector<Block> &blocks = b.blocks;
    parallel_for(b.nthreads, blocks.size(), 16, [&](size_t lo, size_t hi, size_t) {
        for (size_t i = lo; i < hi; i++) inflate_block(blocks[i], dst + blocks[i].out_off);
    });
    b.t_inflate += now_s() - t0;
    b.bytes_out += out - b.carry;
    return true;
}

// Query length as pysam's infer_query_length(): CIGAR operations that consume the query, hard clips excluded.
inline uint32_t query_length(const uint8_t *cig, uint32_t n)
{
    uint32_t q = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = le32(cig + 4 * i), op = v & 15u;
        // M=0 I=1 S=4 '='=7 X=8
        if ((0x193u >> op) & 1u) q += v >> 4;
    }
    return q;
}

// htslib moves a CIGAR of more than 65535 operations into the CG:B,I tag and leaves the placeholder
// "<l_seq>S<ref_len>N" (SAM spec 4.2.2); returns the real operations when `rec` is such a record.
bool long_cigar(const uint8_t *rec, uint32_t rec_len, uint32_t l_name, uint32_t n_cig, uint32_t l_seq,
                const uint8_t *&cig, uint32_t &n)
{
    if (n_cig != 2) return false;
    const uint8_t *c = rec + 32 + l_name;
    const uint32_t c0 = le32(c), c1 = le32(c + 4);
    if ((c0 & 15u) != 4 || (c0 >> 4) != l_seq || (c1 & 15u) != 3) return false;
    size_t p = 32 + (size_t)l_name + 8 + ((size_t)l_seq + 1) / 2 + l_seq;
    while (p + 3 <= rec_len) {
        const uint8_t t0 = rec[p], t1 = rec[p + 1], ty = rec[p + 2];
        p += 3;
        size_t sz;
        switch (ty) {
        case 'A': case 'c': case 'C': sz = 1; break;
        case 's': case 'S': sz = 2; break;
        case 'i': case 'I': case 'f': sz = 4; break;
        case 'Z': case 'H': {
            const void *z = memchr(rec + p, 0, rec_len - p);
            if (!z) return false;
            sz = (const uint8_t *)z - (rec + p) + 1;
            break;
        }
        case 'B': {
            if (p + 5 > rec_len) return false;
            const uint8_t sub = rec[p];
            const uint32_t cnt = le32(rec + p + 1);
            const size_t es = (sub == 'c' || sub == 'C') ? 1 : (sub == 's' || sub == 'S') ? 2 : 4;
            if (t0 == 'C' && t1 == 'G' && sub == 'I') {
                if (p + 5 + (size_t)cnt * 4 > rec_len) return false;
                cig = rec + p + 5;
                n = cnt;
                return true;
            }
            sz = 5 + (size_t)cnt * es;
            break;
        }
        default: return false;
        }
        p += sz;
    }
    return false;
}

using Decoded = Window;

void decode_range(const pmx_bam &b, size_t lo, size_t hi, Decoded &out)
{
    const uint8_t *buf = b.buf.data();
    const int32_t nref = (int32_t)b.ref_names.size();
    for (size_t i = lo; i < hi; i++) {
        const uint8_t *rec = buf + b.rec_off[i] + 4;          // past block_size
        const uint32_t rec_len = le32(rec - 4);
        const int32_t ref = le32s(rec);
        const int32_t pos = le32s(rec + 4);
        const uint32_t l_name = rec[8], mapq = rec[9];
        const uint32_t n_cig = le16(rec + 12), flag = le16(rec + 14);
        const uint32_t l_seq = le32(rec + 16);
        if (32 + (size_t)l_name + 4 * (size_t)n_cig > rec_len)
            throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BAM record shorter than its name and CIGAR");
        if (ref >= nref) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BAM record refers to an unknown reference id");
        if ((flag & b.flag_exclude) || mapq < b.mapq_min || ref < 0) continue;
        if (b.want_ref >= 0 && ref != b.want_ref) continue;
        const uint8_t *cig = rec + 32 + l_name;
        uint32_t n = n_cig;
        long_cigar(rec, rec_len, l_name, n_cig, l_seq, cig, n);
        const uint32_t q = query_length(cig, n);
        if (q == 0) continue;
        out.ref.push_back(ref);
        out.pos.push_back(pos + 1);
        out.len.push_back((int32_t)q);
        out.rev.push_back((flag & PMX_BAM_FLAG_REVERSE) ? 1 : 0);
        if (b.mates) {                                        // bytes 20-31 of the record: next_refID, next_pos, tlen
            out.flag.push_back((uint16_t)flag);
            out.mref.push_back(le32s(rec + 20));
            out.mpos.push_back((int32_t)(le32(rec + 24) + 1u));
            out.tlen.push_back(le32s(rec + 28));
        }
    }
}

// Decodes every complete record in buf into the window arrays and keeps the tail as carry.
void decode_window(pmx_bam &b, Window &w)
{
    const uint8_t *buf = b.buf.data();
    const size_t n = b.buf.size();
    b.rec_off.clear();
    size_t p = b.skip < n ? b.skip : n;   // region mode: the first block starts before the region
    b.skip -= p;
    double t0 = now_s();
    while (p + 4 <= n) {
        const uint32_t bs = le32(buf + p);
        if (bs < 32) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BAM record with block_size < 32");
        if (p + 4 + (size_t)bs > n) break;
        b.rec_off.push_back(p);
        p += 4 + (size_t)bs;
    }
    const size_t nrec = b.rec_off.size();
    const size_t grain = 1 << 16;
    const size_t chunks = (nrec + grain - 1) / grain;
    std::vector<Decoded> parts(chunks);
    double t1 = now_s();
    b.t_walk += t1 - t0;
    parallel_for(b.nthreads, nrec, grain, [&](size_t lo, size_t hi, size_t c) { decode_range(b, lo, hi, parts[c]); });
    t0 = now_s();
    b.t_decode += t0 - t1;
    size_t kept = 0;
    for (auto &d : parts) kept += d.ref.size();
    w.ref.resize(kept);
    w.pos.resize(kept);
    w.len.resize(kept);
    w.rev.resize(kept);
    if (b.mates) {
        w.flag.resize(kept);
        w.mref.resize(kept);
        w.mpos.resize(kept);
        w.tlen.resize(kept);
    }
    size_t o = 0;
    for (auto &d : parts) {
        const size_t k = d.ref.size();
        if (!k) continue;
        memcpy(w.ref.data() + o, d.ref.data(), k * 4);
        memcpy(w.pos.data() + o, d.pos.data(), k * 4);
        memcpy(w.len.data() + o, d.len.data(), k * 4);
        memcpy(w.rev.data() + o, d.rev.data(), k);
        if (b.mates) {
            memcpy(w.flag.data() + o, d.flag.data(), k * 2);
            memcpy(w.mref.data() + o, d.mref.data(), k * 4);
            memcpy(w.mpos.data() + o, d.mpos.data(), k * 4);
            memcpy(w.tlen.data() + o, d.tlen.data(), k * 4);
        }
        o += k;
    }
    b.n_records += nrec;
    b.n_kept += kept;
    // carry the incomplete tail to the front
    b.carry = n - p;
    if (b.carry) memmove(b.buf.data(), b.buf.data() + p, b.carry);
    b.buf.resize(b.carry);
    b.t_concat += now_s() - t0;
}

// Producer thread: windows -> queue, until end of file, an error or close().
void produce(pmx_bam *b)
{
    try {
        for (;;) {
            const bool region = b->want_ref >= 0;   // a region ends inside a block: what follows is the next reference
            if (b->eof) {
                if (b->carry && !region) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "file ends inside an alignment record");
                break;
            }
            const bool more = load_window(*b, WINDOW_BLOCKS);
            Window w;
            if (more || b->carry) decode_window(*b, w);
            if (!more && b->carry && !region)
                throw pmx_io::Error(PMX_IO_ERR_FORMAT, "file ends inside an alignment record");
            std::unique_lock<std::mutex> lk(b->mu);
            b->cv.wait(lk, [&] { return b->queue.size() < QUEUE_DEPTH || b->stop; });
            if (b->stop) return;
            if (!w.ref.empty()) {
                b->queue.push_back(std::move(w));
                b->cv.notify_all();
            }
        }
    } catch (const pmx_io::Error &e) {
        std::lock_guard<std::mutex> g(b->mu);
        b->err_code = e.code;
        b->err_msg = e.msg;
    } catch (const std::exception &e) {
        std::lock_guard<std::mutex> g(b->mu);
        b->err_code = PMX_IO_ERR_FORMAT;
        b->err_msg = e.what();
    }
    std::lock_guard<std::mutex> g(b->mu);
    b->done = true;
    b->cv.notify_all();
}

void parse_header(pmx_bam &b)
{
    // The header may span several BGZF blocks: inflate block by block until it is complete.
    std::vector<std::pair<size_t, size_t>> loaded;   // (file offset, uncompressed start) of the header's blocks
    auto need = [&](size_t upto) {
        while (b.buf.size() < upto) {
            loaded.emplace_back(b.next_off, b.buf.size());
            b.carry = b.buf.size();
            if (!load_window(b, 1)) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "file ends inside the BAM header");
        }
    };
    need(12);
    if (memcmp(b.buf.data(), "BAM\1", 4) != 0) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "not a BAM file (bad magic)");
    const uint32_t l_text = le32(b.buf.data() + 4);
    need(12 + (size_t)l_text);
    b.text.assign((const char *)b.buf.data() + 8, l_text);
    while (!b.text.empty() && b.text.back() == '\0') b.text.pop_back();
    size_t p = 8 + (size_t)l_text;
    const uint32_t n_ref = le32(b.buf.data() + p);
    p += 4;
    b.ref_names.reserve(n_ref);
    b.ref_lens.reserve(n_ref);
    for (uint32_t i = 0; i < n_ref; i++) {
        need(p + 4);
        const uint32_t l_name = le32(b.buf.data() + p);
        if (l_name == 0 || l_name > (1u << 20)) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "bad reference name length");
        need(p + 4 + l_name + 4);
        const char *nm = (const char *)b.buf.data() + p + 4;
        b.ref_names.emplace_back(nm, strnlen(nm, l_name));
        b.ref_lens.push_back((int64_t)le32(b.buf.data() + p + 4 + l_name));
        p += 4 + (size_t)l_name + 4;
    }
    b.hdr_len = p;
    for (const auto &blk : loaded)
        if (blk.second <= p) b.data_beg = ((uint64_t)blk.first << 16) | (uint64_t)(p - blk.second);
    // what follows the header stays in buf as the carry of the first record window
    const size_t rest = b.buf.size() - p;
    if (rest) memmove(b.buf.data(), b.buf.data() + p, rest);
    b.buf.resize(rest);
    b.carry = rest;
}

// ---- read-length histogram with the estimator's filter (PyMaSC core/readlen.pyx:estimate_readlen) ----------------
struct LenAcc {
    uint64_t count, first;
};
struct ReadlenPart {
    std::unordered_map<int32_t, LenAcc> h;
    uint64_t c[6] = {0, 0, 0, 0, 0, 0};   // nreads, nunmapped, ncounted, npaired, nread2, nnoqlen
};

// records [lo, hi) of rec_off (offsets into buf, whose first byte is at `base` of the uncompressed stream)
void readlen_range(const pmx_bam &b, const uint8_t *buf, const std::vector<size_t> &rec_off, uint64_t base, uint32_t mapq_min,
                   size_t lo, size_t hi, ReadlenPart &out)
{
    const int32_t nref = (int32_t)b.ref_names.size();
    int32_t last_q = -1;
    LenAcc *last = nullptr;
    for (size_t i = lo; i < hi; i++) {
        const uint8_t *rec = buf + rec_off[i] + 4;
        const uint32_t rec_len = le32(rec - 4);
        const int32_t ref = le32s(rec);
        const uint32_t l_name = rec[8], mapq = rec[9];
        const uint32_t n_cig = le16(rec + 12), flag = le16(rec + 14);
        const uint32_t l_seq = le32(rec + 16);
        if (32 + (size_t)l_name + 4 * (size_t)n_cig > rec_len)
            throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BAM record shorter than its name and CIGAR");
        if (ref >= nref) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BAM record refers to an unknown reference id");
        if (ref < 0) continue;                                    // reference_name is None: not even counted (readlen.pyx)
        out.c[0]++;
        if (flag & 0x1u) {
            out.c[3]++;
            if (flag & PMX_BAM_FLAG_READ2) out.c[4]++;
        }
        if (flag & PMX_BAM_FLAG_UNMAPPED) {
            out.c[1]++;
            continue;
        }
        if ((flag & PMX_BAM_FLAG_DUPLICATE) || mapq < mapq_min) continue;
        const uint8_t *cig = rec + 32 + l_name;
        uint32_t n = n_cig;
        long_cigar(rec, rec_len, l_name, n_cig, l_seq, cig, n);
        const uint32_t q = query_length(cig, n);
        if (q == 0 || q > 0x7fffffffu) {                          // infer_query_length() is None: kept apart
            out.c[5]++;
            continue;
        }
        out.c[2]++;
        const uint64_t key = base + rec_off[i];
        if ((int32_t)q != last_q) {
            auto it = out.h.emplace((int32_t)q, LenAcc{0, key}).first;   // (node-based: the pointer survives a rehash)
            last = &it->second;
            last_q = (int32_t)q;
        }
        last->count++;
        if (key < last->first) last->first = key;
    }
}

// One pass over the whole file with buffers of its own: the state of a pmx_bam_next_batch iteration is not touched.
void readlen_pass(pmx_bam &b, uint32_t mapq_min)
{
    RawBuf buf;
    std::vector<Block> blocks;
    std::vector<size_t> rec_off;
    std::unordered_map<int32_t, LenAcc> hist;
    uint64_t c[6] = {0, 0, 0, 0, 0, 0};
    size_t off = 0, carry = 0, skip = b.hdr_len;
    uint64_t base = 0;                                            // stream offset of buf[0]
    for (bool eof = false; !eof;) {
        blocks.clear();
        size_t out = carry;
        while (blocks.size() < WINDOW_BLOCKS) {
            Block blk;
            size_t next;
            if (!scan_block(b.file.data, b.file.size, off, blk, next)) {
                eof = true;
                break;
            }
            blk.out_off = out;
            out += blk.isize;
            off = next;
            blocks.push_back(blk);
        }
        buf.resize(out);
        uint8_t *dst = buf.data();
        parallel_for(b.nthreads, blocks.size(), 16, [&](size_t lo, size_t hi, size_t) {
            for (size_t i = lo; i < hi; i++) inflate_block(blocks[i], dst + blocks[i].out_off);
        });
        size_t p = skip < out ? skip : out;                       // the header (it may span windows)
        skip -= p;
        rec_off.clear();
        while (p + 4 <= out) {
            const uint32_t bs = le32(dst + p);
            if (bs < 32) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "BAM record with block_size < 32");
            if (p + 4 + (size_t)bs > out) break;
            rec_off.push_back(p);
            p += 4 + (size_t)bs;
        }
        const size_t grain = 1 << 16;
        std::vector<ReadlenPart> parts((rec_off.size() + grain - 1) / grain);
        parallel_for(b.nthreads, rec_off.size(), grain, [&](size_t lo, size_t hi, size_t k) {
            readlen_range(b, dst, rec_off, base, mapq_min, lo, hi, parts[k]);
        });
        for (const ReadlenPart &part : parts) {
            for (int k = 0; k < 6; k++) c[k] += part.c[k];
            for (const auto &kv : part.h) {
                auto it = hist.emplace(kv.first, kv.second);
                if (!it.second) {
                    it.first->second.count += kv.second.count;
                    if (kv.second.first < it.first->second.first) it.first->second.first = kv.second.first;
                }
            }
        }
        carry = out - p;
        if (eof && carry) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "file ends inside an alignment record");
        if (carry) memmove(dst, dst + p, carry);
        buf.resize(carry);
        base += p;
    }
    b.rl_hist.clear();
    b.rl_hist.reserve(hist.size());
    for (const auto &kv : hist) b.rl_hist.push_back({kv.first, kv.second.count, kv.second.first});
    std::sort(b.rl_hist.begin(), b.rl_hist.end(), [](const pmx_bam::LenBin &x, const pmx_bam::LenBin &y) { return x.len < y.len; });
    memcpy(b.rl_counters, c, sizeof c);
    b.rl_mapq = mapq_min;
    b.rl_valid = true;
}

}  // namespace

// Every BGZF member of data[0, size) inflated (and CRC-checked) on nthreads threads into `out`; for the SAM reader.
void pmx_io::bgzf_inflate_all(const uint8_t *data, size_t size, int nthreads, std::vector<uint8_t> &out, uint64_t &members)
{
    std::vector<Block> blocks;
    size_t off = 0, next, total = 0;
    Block blk;
    while (scan_block(data, size, off, blk, next)) {
        blk.out_off = total;
        total += blk.isize;
        blocks.push_back(blk);
        off = next;
    }
    out.resize(total);
    uint8_t *dst = out.data();
    parallel_for(nthreads, blocks.size(), 16, [&](size_t lo, size_t hi, size_t) {
        for (size_t i = lo; i < hi; i++) inflate_block(blocks[i], dst + blocks[i].out_off);
    });
    members = blocks.size();
}

size_t pmx_io::bgzf_inflate_prefix(const uint8_t *data, size_t size, size_t off, size_t want, std::vector<uint8_t> &out)
{
    Block blk;
    size_t next;
    while (out.size() < want && scan_block(data, size, off, blk, next)) {
        const size_t at = out.size();
        out.resize(at + blk.isize);
        inflate_block(blk, out.data() + at);
        off = next;
    }
    return off;
}

extern "C" {

int pmx_bam_open(const char *path, int nthreads, pmx_bam **out)
{
    if (!path || !out) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_open: NULL argument");
    *out = nullptr;
    pmx_bam *b = new pmx_bam();
    try {
        b->file.open(path);
        b->nthreads = pmx_io::pick_threads(nthreads);
        parse_header(*b);
    } catch (const pmx_io::Error &e) {
        delete b;
        return pmx_io::fail(e.code, std::string(path) + ": " + e.msg);
    } catch (const std::exception &e) {
        delete b;
        return pmx_io::fail(PMX_IO_ERR_OPEN, std::string(path) + ": " + e.what());
    }
    *out = b;
    return PMX_IO_OK;
}

void pmx_bam_close(pmx_bam *b)
{
    if (!b) return;
    if (b->producer.joinable()) {
        {
            std::lock_guard<std::mutex> g(b->mu);
            b->stop = true;
        }
        b->cv.notify_all();
        b->producer.join();
    }
    if (getenv("PMX_IO_TIMING"))
        fprintf(stderr, "[pmx_bam] scan %.3f alloc %.3f inflate %.3f walk %.3f decode %.3f concat %.3f s (%d threads)\n",
                b->t_scan, b->t_alloc, b->t_inflate, b->t_walk, b->t_decode, b->t_concat, b->nthreads);
    delete b;
}

int32_t pmx_bam_nref(const pmx_bam *b) { return b ? (int32_t)b->ref_names.size() : 0; }

const char *pmx_bam_ref_name(const pmx_bam *b, int32_t i)
{
    if (!b || i < 0 || (size_t)i >= b->ref_names.size()) return nullptr;
    return b->ref_names[i].c_str();
}

int64_t pmx_bam_ref_len(const pmx_bam *b, int32_t i)
{
    if (!b || i < 0 || (size_t)i >= b->ref_lens.size()) return -1;
    return b->ref_lens[i];
}

const char *pmx_bam_header_text(const pmx_bam *b, uint32_t *len)
{
    if (!b) return nullptr;
    if (len) *len = (uint32_t)b->text.size();
    return b->text.c_str();
}

// pmx_bam_next_batch, and with `mates` pmx_bam_next_mates: the pass is one or the other from its first call on
static int64_t next_batch(pmx_bam *b, bool mates, uint32_t mapq_min, uint32_t flag_exclude, int64_t cap, int32_t *ref_id, int32_t *pos1,
                          int32_t *read_len, uint8_t *reverse, uint16_t *flag, int32_t *mate_ref, int32_t *mate_pos1, int32_t *tlen)
{
    if (!b->filter_set) {
        b->mapq_min = mapq_min;
        b->flag_exclude = flag_exclude;
        b->mates = mates;
        b->filter_set = true;
    } else if (b->mapq_min != mapq_min || b->flag_exclude != flag_exclude || b->mates != mates) {
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_next_batch: the filter must not change between calls");
    }
    b->pristine = false;
    if (!b->producer.joinable() && !b->done) b->producer = std::thread(produce, b);
    while (b->w_cursor == b->cur.ref.size()) {
        std::unique_lock<std::mutex> lk(b->mu);
        b->cv.wait(lk, [&] { return !b->queue.empty() || b->done; });
        if (b->queue.empty()) {      // done: end of file or a failure
            if (b->err_code) return pmx_io::fail(b->err_code, b->err_msg);
            return 0;
        }
        b->cur = std::move(b->queue.front());
        b->queue.pop_front();
        b->w_cursor = 0;
        b->cv.notify_all();
    }
    const size_t n = std::min<size_t>((size_t)cap, b->cur.ref.size() - b->w_cursor);
    const size_t c = b->w_cursor;
    memcpy(ref_id, b->cur.ref.data() + c, n * 4);
    memcpy(pos1, b->cur.pos.data() + c, n * 4);
    memcpy(read_len, b->cur.len.data() + c, n * 4);
    memcpy(reverse, b->cur.rev.data() + c, n);
    if (mates) {
        memcpy(flag, b->cur.flag.data() + c, n * 2);
        memcpy(mate_ref, b->cur.mref.data() + c, n * 4);
        memcpy(mate_pos1, b->cur.mpos.data() + c, n * 4);
        memcpy(tlen, b->cur.tlen.data() + c, n * 4);
    }
    b->w_cursor += n;
    return (int64_t)n;
}

int64_t pmx_bam_next_batch(pmx_bam *b, uint32_t mapq_min, uint32_t flag_exclude, int64_t cap,
                           int32_t *ref_id, int32_t *pos1, int32_t *read_len, uint8_t *reverse)
{
    if (!b || cap <= 0 || !ref_id || !pos1 || !read_len || !reverse)
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_next_batch: NULL argument or cap <= 0");
    return next_batch(b, false, mapq_min, flag_exclude, cap, ref_id, pos1, read_len, reverse, nullptr, nullptr, nullptr, nullptr);
}

int64_t pmx_bam_next_mates(pmx_bam *b, uint32_t mapq_min, uint32_t flag_exclude, int64_t cap, int32_t *ref_id, int32_t *pos1,
                           int32_t *read_len, uint8_t *reverse, uint16_t *flag, int32_t *mate_ref, int32_t *mate_pos1, int32_t *tlen)
{
    if (!b || cap <= 0 || !ref_id || !pos1 || !read_len || !reverse || !flag || !mate_ref || !mate_pos1 || !tlen)
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_next_mates: NULL argument or cap <= 0");
    return next_batch(b, true, mapq_min, flag_exclude, cap, ref_id, pos1, read_len, reverse, flag, mate_ref, mate_pos1, tlen);
}

int pmx_bam_index_load(pmx_bam *b, const char *bai_path)
{
    if (!b) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_index_load: NULL handle");
    try {
        pmx_io::MappedFile f;
        f.open(bai_path);
        const uint8_t *d = f.data;
        const size_t n = f.size;
        std::vector<pmx_bai::RefRange> idx;
        std::string err;
        if (!pmx_bai::parse(d, n, b->ref_names.size(), idx, err)) throw pmx_io::Error(PMX_IO_ERR_FORMAT, err);
        b->index.swap(idx);
        b->have_index = true;
    } catch (const pmx_io::Error &e) {
        return pmx_io::fail(e.code, std::string(bai_path ? bai_path : "") + ": " + e.msg);
    }
    return PMX_IO_OK;
}

int pmx_bam_has_index(const pmx_bam *b) { return b && b->have_index ? 1 : 0; }

int pmx_bam_fetch_ref(pmx_bam *b, int32_t ref_id)
{
    if (!b) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_fetch_ref: NULL handle");
    if (ref_id >= 0 && !b->have_index) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_fetch_ref: no index loaded");
    if (ref_id < -1 || (ref_id >= 0 && (size_t)ref_id >= b->index.size()))
        return pmx_io::fail(PMX_IO_ERR_NOTFOUND, "pmx_bam_fetch_ref: reference id out of range");
    if (ref_id < 0 && b->pristine) return PMX_IO_OK;
    b->pristine = false;
    if (b->producer.joinable()) {     // retire the running pipeline
        {
            std::lock_guard<std::mutex> g(b->mu);
            b->stop = true;
        }
        b->cv.notify_all();
        b->producer.join();
    }
    b->queue.clear();
    b->cur = Window();
    b->w_cursor = 0;
    b->stop = false;
    b->err_code = 0;
    b->err_msg.clear();
    b->carry = 0;
    b->buf.resize(0);
    b->filter_set = false;
    b->want_ref = ref_id;
    if (ref_id < 0) {                 // back to one pass over the whole file
        b->eof = false;
        b->done = false;
        b->next_off = (size_t)(b->data_beg >> 16);
        b->skip = (size_t)(b->data_beg & 0xffffu);
        b->stop_block = SIZE_MAX;
        return PMX_IO_OK;
    }
    const pmx_bam::RefRange &rr = b->index[ref_id];
    if (!rr.has) {                    // a reference without records
        b->eof = true;
        b->done = true;
        return PMX_IO_OK;
    }
    b->eof = false;
    b->done = false;
    b->next_off = (size_t)(rr.beg >> 16);
    b->skip = (size_t)(rr.beg & 0xffffu);
    b->stop_block = (size_t)(rr.end >> 16);
    if (b->next_off >= b->file.size)
        return pmx_io::fail(PMX_IO_ERR_FORMAT, "pmx_bam_fetch_ref: the index points past the end of the file");
    return PMX_IO_OK;
}

int pmx_bam_counters(const pmx_bam *b, uint64_t *records, uint64_t *kept, uint64_t *bytes_out, uint64_t *bytes_in)
{
    if (!b) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_counters: NULL handle");
    if (records) *records = b->n_records.load();
    if (kept) *kept = b->n_kept.load();
    if (bytes_out) *bytes_out = b->bytes_out.load();
    if (bytes_in) *bytes_in = b->bytes_in.load();
    return PMX_IO_OK;
}

int64_t pmx_bam_readlen_hist(pmx_bam *b, uint32_t mapq_min, int64_t cap, int32_t *lengths, uint64_t *counts, uint64_t *first)
{
    if (!b) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_readlen_hist: NULL handle");
    if (lengths && (cap < 0 || !counts || !first))
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_readlen_hist: NULL argument or cap < 0");
    if (!b->rl_valid || b->rl_mapq != mapq_min) {
        b->rl_valid = false;
        try {
            readlen_pass(*b, mapq_min);
        } catch (const pmx_io::Error &e) {
            return pmx_io::fail(e.code, e.msg);
        } catch (const std::exception &e) {
            return pmx_io::fail(PMX_IO_ERR_OPEN, std::string("pmx_bam_readlen_hist: ") + e.what());
        }
    }
    if (!lengths) return (int64_t)b->rl_hist.size();
    const int64_t m = std::min<int64_t>(cap, (int64_t)b->rl_hist.size());
    for (int64_t i = 0; i < m; i++) {
        lengths[i] = b->rl_hist[(size_t)i].len;
        counts[i] = b->rl_hist[(size_t)i].count;
        first[i] = b->rl_hist[(size_t)i].first;
    }
    return m;
}

int pmx_bam_readlen_counters(const pmx_bam *b, uint64_t c[6])
{
    if (!b || !c) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_readlen_counters: NULL argument");
    if (!b->rl_valid) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bam_readlen_counters: no pmx_bam_readlen_hist yet");
    memcpy(c, b->rl_counters, sizeof b->rl_counters);
    return PMX_IO_OK;
}

}  // extern "C"
