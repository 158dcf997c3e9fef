// BigWig (bbi) on the device (include/pymasc_amd_ingest.h, pmx_dbw_*; SURVEY.md §8 row f2).  Included by bam_device.hip.
//
// Replaces PyMaSC/reader/bigwig.pyx:147-177 (BigWigReader.fetch: the intervals of one chromosome with value >= threshold) the way
// the BAM side replaces pysam: the file goes to HBM as it is; the host reads the 64-byte header, the chromosome B+ tree and, per
// fetch, walks the R-tree for the chromosome's data blocks (offsets and sizes: a few KB of index); the blocks -- zlib streams of
// unknown length -- are inflated by k_bgzf_inflate (one wavefront each, `open_size`), their Adler-32 checked (k_bw_adler), their
// sections (bedGraph / variableStep / fixedStep items) decoded and filtered by k_bw_sections, and the intervals land in device
// arrays in index order, where pmx_bits_set_regions_dev_ex (include/pymasc_amd.h) builds the mappability vector from them.
// Same intervals as pmx_track_fetch (libpymasc_io.so, the checker), bit for bit.
//
// A bigBed file (io/bigbed_parse.h, DESIGN.md 7.12) takes the same path up to the decode: its blocks hold BED records, walked by
// k_bb_records (bigbed_device.inc) in place of k_bw_sections.

#include "../io/bigbed_parse.h"

enum { BW_OK = 0, BW_ERR_HEADER = 20, BW_ERR_TYPE = 21, BW_ERR_ITEMS = 22, BW_ERR_ADLER = 23 };

// Adler-32 of a block's output against the four bytes behind its DEFLATE stream (RFC 1950): A = 1 + sum d_i, B = n + sum (n - i) d_i
__global__ void __launch_bounds__(256)
k_bw_adler(const u8 *__restrict__ out, const DMember *__restrict__ mem, const u32 *__restrict__ out_size, u32 nmem, u32 *__restrict__ status)
{
    const u32 m = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (m >= nmem) return;
    if (status[m]) return;
    const u32 n = out_size[m];
    const u8 *p = out + mem[m].out_off;
    const u32 per = (n + 63u) / 64u, lo = lane * per < n ? lane * per : n, hi = lo + per < n ? lo + per : n;
    u64 a = 0, b = 0;
    for (u32 i = lo; i < hi; i++) {
        const u64 d = p[i];
        a += d;
        b += (u64)(n - i) * d;
    }
    for (u32 o = 32; o; o >>= 1) {
        a += ((u64)(u32)__shfl_xor((int)(u32)(a >> 32), (int)o, 64) << 32) | (u32)__shfl_xor((int)(u32)a, (int)o, 64);
        b += ((u64)(u32)__shfl_xor((int)(u32)(b >> 32), (int)o, 64) << 32) | (u32)__shfl_xor((int)(u32)b, (int)o, 64);
    }
    const u32 A = (u32)((1u + a) % 65521u), B = (u32)((n + b) % 65521u);
    if (lane == 0 && ((B << 16) | A) != mem[m].crc) status[m] = BW_ERR_ADLER;
}

struct BwSpan {
    u64 off;    // of the section's bytes in `base` (the inflated blocks, or the file itself when it is not compressed)
    u32 size, pad;
};

// One wavefront per data block: 24-byte section header + items -> the intervals that overlap the chromosome and pass the
// threshold (bigwig.pyx:147-177), counted (WRITE = false) or written in item order at the block's place (WRITE = true)
// (every block is described by an explicit (offset, size) pair -- for inflated blocks k_bw_spans writes them -- and the size is clamped
// to the block's share of the buffer: whatever the bytes say, no lane reads outside it)
__global__ void __launch_bounds__(256) k_bw_spans(const u32 *__restrict__ out_size, u64 stride, u32 nblk, BwSpan *__restrict__ spans)
{
    const u32 m = blockIdx.x * 256u + threadIdx.x;
    if (m >= nblk) return;
    BwSpan s;
    s.off = (u64)m * stride;
    s.size = out_size[m] < (u32)stride ? out_size[m] : (u32)stride;
    s.pad = 0;
    spans[m] = s;
}

template <bool WRITE>
__global__ void __launch_bounds__(256)
k_bw_sections(const u8 *__restrict__ base, const BwSpan *__restrict__ spans, u32 nblk, const u32 *__restrict__ chrom_lens, u32 nlens,
              float threshold, u32 *__restrict__ status, u32 *__restrict__ cnt, u32 *__restrict__ blk_chrom, const u64 *__restrict__ place,
              u32 *__restrict__ o_begin, u32 *__restrict__ o_end, float *__restrict__ o_value)
{
    const u32 m = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (m >= nblk) return;
    if (status[m]) return;
    // A wavefront works on ONE block: everything the section header says is the same in every lane, and saying so (readfirstlane)
    // makes the dispatch on the item type a scalar branch.  It is also what makes the kernel RIGHT with this compiler: with the
    // header fields as per-lane values the three-way dispatch compiled to a load through a register pair that the fixedStep path
    // never set -- a memory fault at whatever the previous kernel had left there (0x1e00000000: the inflate kernel's 30 distance
    // codes), on files of fixedStep sections only; found with PMX_DBW_DEBUG=1 (a synchronisation and a pause behind every launch).
    const u64 off = ((u64)RFL((u32)(spans[m].off >> 32)) << 32) | RFL((u32)spans[m].off);
    const u8 *d = base + off;
    const u32 n = RFL(spans[m].size);
    u32 err = 0;
    if (n < 24u) err = BW_ERR_HEADER;
    u32 chrom = 0, start = 0, step = 0, span = 0, type = 0, count = 0, item = 0;
    if (!err) {
        chrom = RFL(ld32u(d));
        start = RFL(ld32u(d + 4));
        step = RFL(ld32u(d + 12));
        span = RFL(ld32u(d + 16));
        type = RFL(d[20]);
        count = RFL(ld16u(d + 22));
        item = type == 1u ? 12u : type == 2u ? 8u : type == 3u ? 4u : 0u;
        if (!item) err = BW_ERR_TYPE;
        else if (24ull + (u64)count * item > n) err = BW_ERR_ITEMS;
        if (err) count = 0;
    }
    if (err) {
        if (lane == 0) status[m] = err;
        return;
    }
    // (every chromosome of the file in one pass: a block belongs to the chromosome its header names; one the chromosome tree does not
    // know has length 0 and keeps nothing)
    const u64 chrom_len = chrom < nlens ? RFL(chrom_lens[chrom]) : 0u;
    if (!WRITE && lane == 0) blk_chrom[m] = chrom;
    u64 w = WRITE ? place[m] : 0;
    u32 total = 0;
    for (u32 i0 = 0; i0 < count; i0 += 64u) {
        const u32 i = i0 + lane;
        bool keep = false;
        u32 b = 0, e = 0;
        float v = 0.f;
        if (i < count) {
            const u8 *p = d + 24u + (u64)i * item;
            u32 vb;
            if (type == 1u) {
                b = ld32u(p);
                e = ld32u(p + 4);
                vb = ld32u(p + 8);
            } else if (type == 2u) {
                b = ld32u(p);
                vb = ld32u(p + 4);
                e = b + span;
            } else {
                b = start + i * step;
                e = b + span;
                vb = ld32u(p);
            }
            v = __uint_as_float(vb);
            keep = !((u64)b >= chrom_len || e == 0u) && !(threshold > 0.f && !(v >= threshold));
        }
        const u64 mk = __ballot(keep);
        if (WRITE && keep) {
            const u64 at = w + (u64)__popcll(mk & ((1ull << lane) - 1ull));
            o_begin[at] = b;
            o_end[at] = e;
            o_value[at] = v;
        }
        const u32 k = (u32)__popcll(mk);
        w += k;
        total += k;
    }
    if (!WRITE && lane == 0) cnt[m] = total;
}

// are the fetched intervals non-empty, ascending and disjoint (begin_i < end_i <= begin_(i+1))?  what the calculator asks before it
// BUILDS the mappability vector from them instead of OR-ing into a cleared one (pymasc_amd.h: PMX_REGIONS_SORTED)
__global__ void __launch_bounds__(256) k_bw_order(const u32 *__restrict__ begin, const u32 *__restrict__ end, u64 n, u32 *__restrict__ bad)
{
    const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (!(begin[i] < end[i]) || (i + 1 < n && begin[i + 1] < end[i])) atomicOr(bad, 1u);
}

// ---------------------------------------------------------------------------------------------------------------
struct pmx_dbw {
    int device = 0;
    hipStream_t stream = nullptr;
    u64 fsize = 0;
    std::vector<u8> host;              // the file (header and index are read from here)
    u8 *d_file = nullptr;
    u64 chrom_tree_off = 0, index_off = 0;
    u32 uncompress_buf = 0;
    bool bigbed = false;            // a bigBed file: data blocks of BED records (k_bb_records)
    std::vector<std::string> names;
    std::vector<u32> ids;
    std::vector<int64_t> sizes;
    // the last fetch
    u32 *d_begin = nullptr, *d_end = nullptr;
    float *d_value = nullptr;
    u64 n = 0, total = 0;           // intervals of the chromosome fetched last / of the whole file
    size_t cur = 0;
    bool sorted = true;
    bool have = false;              // the arrays hold the file decoded at `have_threshold`
    float have_threshold = 0;
    std::vector<std::pair<u64, u64>> range;   // per chromosome: its intervals in the arrays
    std::vector<int> order;         // per chromosome: -1 not asked yet, 1 ascending and disjoint, 0 not
    std::vector<void *> retired;    // arrays of an earlier threshold
    // a text track (pmx_dtt_open, text_track_device.inc): every chromosome's lines in per-chromosome order, each in file order
    bool text = false;
    u32 *t_b = nullptr, *t_e = nullptr;
    float *t_v = nullptr;
    u64 *t_cbase = nullptr;         // [nchrom + 1]: where each chromosome's lines start
    u64 t_n = 0, text_lines = 0, text_heads = 0, text_slow = 0;   // data lines, lines, chromosome blocks, values strtod decided
    // a k-mer track (pmx_dkm_open, kmer_track_device.inc): the runs of every record in d_begin / d_end / d_value, made at open
    bool kmer = false;
    std::vector<std::pair<u64, u64>> km_range;   // per record: its runs in the arrays
    u64 km_kmers = 0, km_resolved = 0;           // k-mers sorted; elements of colliding runs resolved on the host
    u32 km_passes = 0;
};

namespace {

constexpr u32 BW_MAGIC = 0x888FFC26u, BW_CHROM_TREE_MAGIC = 0x78CA8C91u, BW_RTREE_MAGIC = 0x2468ACE0u;

struct BwErr {
    int code;
    std::string msg;
};
struct BwCursor {
    const pmx_dbw &w;
    const u8 *at(u64 off, u64 n) const
    {
        if (off > w.fsize || n > w.fsize - off)
            throw BwErr{PMX_DBAM_ERR_FORMAT, std::string(w.bigbed ? "bigBed" : "BigWig") + " structure points past the end of the file"};
        return w.host.data() + off;
    }
    u32 r8(u64 off) const { return *at(off, 1); }
    u32 r16(u64 off) const { return h16(at(off, 2)); }
    u32 r32(u64 off) const { return h32(at(off, 4)); }
    u64 r64(u64 off) const { return (u64)h32(at(off, 8)) | ((u64)h32(at(off + 4, 4)) << 32); }
};

void bw_walk_chrom_tree(pmx_dbw &w, const BwCursor &c, u64 node, u32 key_size, u32 val_size, int depth)
{
    if (depth > 32) throw BwErr{PMX_DBAM_ERR_FORMAT, "chromosome tree too deep"};
    const bool leaf = c.r8(node) != 0;
    const u32 count = c.r16(node + 2);
    u64 p = node + 4;
    for (u32 i = 0; i < count; i++) {
        const char *key = (const char *)c.at(p, key_size);
        if (leaf) {
            if (val_size < 8) throw BwErr{PMX_DBAM_ERR_FORMAT, "chromosome tree value size < 8"};
            w.names.emplace_back(key, strnlen(key, key_size));
            w.ids.push_back(c.r32(p + key_size));
            w.sizes.push_back((int64_t)c.r32(p + key_size + 4));
            p += key_size + val_size;
        } else {
            bw_walk_chrom_tree(w, c, c.r64(p + key_size), key_size, val_size, depth + 1);
            p += key_size + 8;
        }
    }
}

struct BwBlock {
    u64 offset, size;
};
void bw_walk_rtree(const BwCursor &c, u64 node, u32 cid, std::vector<BwBlock> &out, int depth)
{
    if (depth > 64) throw BwErr{PMX_DBAM_ERR_FORMAT, "R-tree too deep"};
    const bool leaf = c.r8(node) != 0;
    const u32 count = c.r16(node + 2);
    u64 p = node + 4;
    for (u32 i = 0; i < count; i++) {
        const u32 c0 = c.r32(p), c1 = c.r32(p + 8);
        const bool hit = c0 <= cid && cid <= c1;
        if (leaf) {
            if (hit) out.push_back(BwBlock{c.r64(p + 16), c.r64(p + 24)});
            p += 32;
        } else {
            if (hit) bw_walk_rtree(c, c.r64(p + 16), cid, out, depth + 1);
            p += 24;
        }
    }
}

int bw_open(pmx_dbw &w, const char *path, int nthreads)
{
    const int fd = open(path, O_RDONLY);
    if (fd < 0) return fail(PMX_DBAM_ERR_OPEN, std::string("cannot open ") + path);
    struct Closer {
        int fd;
        ~Closer() { close(fd); }
    } closer{fd};
    struct stat st;
    if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) return fail(PMX_DBAM_ERR_OPEN, std::string("not a regular file: ") + path);
    w.fsize = (u64)st.st_size;
    if (w.fsize < 64) return fail(PMX_DBAM_ERR_FORMAT, std::string(path) + ": not a BigWig file (shorter than its header)");
    w.host.resize(w.fsize);
    {   // the file -> host memory on several threads, then ONE copy to the device (a mappability track is tens to hundreds of MB)
        const int T = (int)std::max<u64>(1, std::min<u64>((u64)nthreads, w.fsize >> 22));
        std::vector<std::thread> th;
        std::vector<int> bad((size_t)T, 0);
        for (int ti = 0; ti < T; ti++)
            th.emplace_back([&, ti] {
                const u64 lo = w.fsize * (u64)ti / (u64)T, hi = w.fsize * (u64)(ti + 1) / (u64)T;
                u64 done = lo;
                while (done < hi) {
                    const ssize_t r = pread(fd, w.host.data() + done, hi - done, (off_t)done);
                    if (r <= 0) {
                        bad[(size_t)ti] = 1;
                        return;
                    }
                    done += (u64)r;
                }
            });
        for (auto &x : th) x.join();
        for (int v : bad)
            if (v) return fail(PMX_DBAM_ERR_OPEN, std::string("read error on ") + path);
    }
    try {
        const BwCursor c{w};
        const u32 magic = c.r32(0);
        if (magic == __builtin_bswap32(BW_MAGIC)) throw BwErr{PMX_DBAM_ERR_FORMAT, "byte-swapped (big-endian) BigWig files are not supported"};
        if (magic == __builtin_bswap32(bigbed::MAGIC)) throw BwErr{PMX_DBAM_ERR_FORMAT, bigbed::ERR_SWAPPED};
        if (magic != BW_MAGIC && magic != bigbed::MAGIC) throw BwErr{PMX_DBAM_ERR_FORMAT, "not a BigWig file (bad magic)"};
        w.bigbed = magic == bigbed::MAGIC;
        if (w.bigbed && c.r16(32) < 3) throw BwErr{PMX_DBAM_ERR_FORMAT, bigbed::ERR_FIELDS};
        w.chrom_tree_off = c.r64(8);
        w.index_off = c.r64(24);
        w.uncompress_buf = c.r32(52);
        if (w.uncompress_buf > (1u << 30)) throw BwErr{PMX_DBAM_ERR_FORMAT, "implausible uncompressBufSize"};
        const u64 t = w.chrom_tree_off;
        if (c.r32(t) != BW_CHROM_TREE_MAGIC) throw BwErr{PMX_DBAM_ERR_FORMAT, "bad chromosome tree magic"};
        const u32 key_size = c.r32(t + 8), val_size = c.r32(t + 12);
        const u64 item_count = c.r64(t + 16);
        if (key_size == 0 || key_size > 4096) throw BwErr{PMX_DBAM_ERR_FORMAT, "bad chromosome tree key size"};
        if (item_count) bw_walk_chrom_tree(w, c, t + 32, key_size, val_size, 0);
        if (c.r32(w.index_off) != BW_RTREE_MAGIC) throw BwErr{PMX_DBAM_ERR_FORMAT, "bad R-tree index magic"};
    } catch (const BwErr &e) {
        return fail(e.code, std::string(path) + ": " + e.msg);
    }
    HIPOK(hipMalloc((void **)&w.d_file, w.fsize + IN_PAD));
    HIPOK(hipMemsetAsync(w.d_file + w.fsize, 0, IN_PAD, w.stream));
    HIPOK(hipMemcpyAsync(w.d_file, w.host.data(), w.fsize, hipMemcpyHostToDevice, w.stream));
    HIPOK(hipStreamSynchronize(w.stream));
    return 0;
}

const char *bw_err_text(u32 code)
{
    switch (code) {
    case BW_ERR_HEADER: return "BigWig data block shorter than its header";
    case BW_ERR_TYPE: return "BigWig data block of unknown type";
    case BW_ERR_ITEMS: return "BigWig data block shorter than its items";
    case BW_ERR_ADLER: return "BigWig data block does not inflate (Adler-32 mismatch)";
    }
    return "BigWig data block does not inflate";
}

struct DevBuf {   // frees what a fetch allocated however it ends
    std::vector<void *> p;
    ~DevBuf()
    {
        for (void *x : p)
            if (x) (void)hipFree(x);
    }
    template <class T>
    hipError_t get(T **out, size_t bytes)
    {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 16));
        if (e == hipSuccess) p.push_back(q);
        *out = (T *)q;
        return e;
    }
};

}  // namespace

extern "C" {

static int dbw_open_impl(const char *path, int device, int nthreads, pmx_dbw **out);
int pmx_dbw_open(const char *path, int device, int nthreads, pmx_dbw **out)
{
    try {   // (an exception must not leave the C ABI)
        return dbw_open_impl(path, device, nthreads, out);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dbw_open: ") + e.what());
    }
}
static int dbw_open_impl(const char *path, int device, int nthreads, pmx_dbw **out)
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
    if (hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking) != hipSuccess) {
        delete w;
        return fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    }
    const int rc = bw_open(*w, path, nthreads);
    if (rc) {
        const std::string keep = g_err;
        pmx_dbw_close(w);
        g_err = keep;
        return rc;
    }
    *out = w;
    return 0;
}

void pmx_dbw_close(pmx_dbw *w)
{
    if (!w) return;
    (void)hipSetDevice(w->device);
    if (w->stream) (void)hipStreamSynchronize(w->stream);
    for (void *p : {(void *)w->d_file, (void *)w->d_begin, (void *)w->d_end, (void *)w->d_value, (void *)w->t_b, (void *)w->t_e,
                    (void *)w->t_v, (void *)w->t_cbase})
        if (p) (void)hipFree(p);
    for (void *p : w->retired) (void)hipFree(p);
    if (w->stream) (void)hipStreamDestroy(w->stream);
    delete w;
}

int32_t pmx_dbw_nchrom(const pmx_dbw *w) { return w ? (int32_t)w->names.size() : 0; }
int pmx_dbw_kind(const pmx_dbw *w) { return !w ? 0 : w->kmer ? 2 : w->bigbed ? 1 : 0; }
const char *pmx_dbw_chrom_name(const pmx_dbw *w, int32_t i)
{
    return (w && i >= 0 && (size_t)i < w->names.size()) ? w->names[(size_t)i].c_str() : nullptr;
}
int64_t pmx_dbw_chrom_len(const pmx_dbw *w, int32_t i) { return (w && i >= 0 && (size_t)i < w->sizes.size()) ? w->sizes[(size_t)i] : -1; }

}  // extern "C" (reopened behind the whole-file pass)

// The whole file in one pass, once per threshold: every data block inflated by ONE launch, every section decoded by one, the
// intervals of all chromosomes in one set of arrays in index order (chromosome by chromosome); a fetch then only looks up the
// chromosome's range.  (The first version worked chromosome by chromosome: ~10 allocations, 6 launches and 4 synchronisations per
// fetch -- 36 ms for the 24 chromosomes of an hg38-shaped track against 15 ms of the host reader on 16 threads.)
namespace {

// (ends on any input, as the host walk does: a child lies strictly after its parent and inside the file, and at most
// file size / 32 leaf items are read -- io/bigbed_parse.h)
void bw_walk_all(const BwCursor &c, u64 node, std::vector<BwBlock> &out, int depth)
{
    if (depth > 64) throw BwErr{PMX_DBAM_ERR_FORMAT, "R-tree too deep"};
    const bool leaf = c.r8(node) != 0;
    const u32 count = c.r16(node + 2);
    u64 p = node + 4;
    if (leaf && out.size() + count > c.w.fsize / 32) throw BwErr{PMX_DBAM_ERR_FORMAT, bigbed::ERR_RTREE_ITEMS};
    for (u32 i = 0; i < count; i++) {
        if (leaf) {
            out.push_back(BwBlock{c.r64(p + 16), c.r64(p + 24)});
            p += 32;
        } else {
            const u64 child = c.r64(p + 16);
            if (child <= node || child >= c.w.fsize) throw BwErr{PMX_DBAM_ERR_FORMAT, bigbed::ERR_RTREE_CHILD};
            bw_walk_all(c, child, out, depth + 1);
            p += 24;
        }
    }
}

// bigbed_device.inc: k_bb_records<write> over the blocks, launched on `s` (hipGetLastError tells whether the launch failed)
void bb_launch_records(bool write, dim3 grid, hipStream_t s, const u8 *base, const BwSpan *spans, u32 nblk, const u32 *chrom_lens,
                       u32 nlens, float threshold, u32 *status, u32 *cnt, u32 *blk_chrom, const u64 *place, u32 *o_begin, u32 *o_end,
                       float *o_value);

int bw_decode_all(pmx_dbw *w, float threshold)
{
    std::vector<BwBlock> blocks;
    try {
        const BwCursor c{*w};
        bw_walk_all(c, w->index_off + 48, blocks, 0);
        for (const BwBlock &b : blocks) (void)c.at(b.offset, b.size);
    } catch (const BwErr &e) {
        return fail(e.code, e.msg);
    }
    // (the previous threshold's arrays may still be read by a consumer: kept until close)
    for (void *p : {(void *)w->d_begin, (void *)w->d_end, (void *)w->d_value})
        if (p) w->retired.push_back(p);
    w->d_begin = w->d_end = nullptr;
    w->d_value = nullptr;
    w->range.assign(w->names.size(), std::pair<u64, u64>(0, 0));
    w->order.assign(w->names.size(), -1);
    w->have = true;
    w->have_threshold = threshold;
    const u32 nb = (u32)blocks.size();
    if (!nb) return 0;
    const bool dbg = getenv("PMX_DBW_DEBUG") != nullptr;
#define BW_STEP(what)                                                                                  \
    if (dbg) {                                                                                         \
        const hipError_t e_ = hipStreamSynchronize(w->stream);                                         \
        fprintf(stderr, "[pmx_dbw] %s: %s (blocks %u, bound %u)\n", what, hipGetErrorString(e_), nb, w->uncompress_buf); \
        fflush(stderr);                                                                                \
        usleep(300000); /* (a memory fault is reported asynchronously: give it time to arrive before the next launch) */ \
    }
    DevBuf tmp;
    const bool z = w->uncompress_buf > 0;
    const u64 stride = ((u64)w->uncompress_buf + 255u) & ~255ull;
    u32 *d_status = nullptr, *d_size = nullptr, *d_cnt = nullptr, *d_bchrom = nullptr, *d_lens = nullptr;
    u64 *d_place = nullptr, *d_tot = nullptr;
    DMember *d_mem = nullptr;
    BwSpan *d_spans = nullptr;
    u8 *d_out = nullptr;
    u32 max_id = 0;
    for (u32 id : w->ids) max_id = std::max(max_id, id);
    if (max_id > (1u << 24)) return fail(PMX_DBAM_ERR_FORMAT, "implausible chromosome id in the chromosome tree");
    std::vector<u32> lens((size_t)max_id + 1, 0u);
    for (size_t i = 0; i < w->ids.size(); i++) lens[w->ids[i]] = (u32)std::min<int64_t>(w->sizes[i], 0xffffffffll);
    HIPOK(tmp.get(&d_status, 4ull * nb));
    HIPOK(tmp.get(&d_cnt, 4ull * nb));
    HIPOK(tmp.get(&d_bchrom, 4ull * nb));
    HIPOK(tmp.get(&d_place, 8ull * nb));
    HIPOK(tmp.get(&d_tot, 16));
    HIPOK(tmp.get(&d_lens, 4ull * lens.size()));
    HIPOK(tmp.get(&d_spans, sizeof(BwSpan) * nb));
    HIPOK(hipMemsetAsync(d_status, 0, 4ull * nb, w->stream));
    HIPOK(hipMemsetAsync(d_cnt, 0, 4ull * nb, w->stream));   // (a block that fails is not counted)
    HIPOK(hipMemsetAsync(d_bchrom, 0xff, 4ull * nb, w->stream));
    HIPOK(hipMemcpyAsync(d_lens, lens.data(), 4ull * lens.size(), hipMemcpyHostToDevice, w->stream));
    std::vector<DMember> mem;
    std::vector<BwSpan> sp;
    if (z) {
        mem.resize(nb);
        for (u32 i = 0; i < nb; i++) {
            const BwBlock &b = blocks[i];
            const u8 *p = w->host.data() + b.offset;
            // zlib wrapper (RFC 1950): CMF / FLG in front, Adler-32 (big-endian) behind the DEFLATE stream
            if (b.size < 6 || (p[0] & 15u) != 8u || ((u32)p[0] * 256u + p[1]) % 31u != 0u || (p[1] & 32u))
                return fail(PMX_DBAM_ERR_FORMAT, w->bigbed ? bigbed::ERR_INFLATE : "BigWig data block does not inflate");
            const u8 *q = p + b.size - 4;
            mem[i].in_off = b.offset + 2;
            mem[i].out_off = (u64)i * stride;
            mem[i].clen = (u32)(b.size - 6);
            mem[i].isize = w->uncompress_buf;
            mem[i].crc = ((u32)q[0] << 24) | ((u32)q[1] << 16) | ((u32)q[2] << 8) | q[3];
            mem[i].open_size = 1;
        }
        HIPOK(tmp.get(&d_mem, sizeof(DMember) * nb));
        HIPOK(tmp.get(&d_size, 4ull * nb));
        HIPOK(tmp.get(&d_out, stride * nb + 64));
        HIPOK(hipMemcpyAsync(d_mem, mem.data(), sizeof(DMember) * nb, hipMemcpyHostToDevice, w->stream));
        hipLaunchKernelGGL(k_bgzf_inflate, dim3(nb), dim3(64), 0, w->stream, w->d_file, d_out, d_mem, nb, d_status, d_size);
        HIPOK(hipGetLastError());
        BW_STEP("inflate")
        hipLaunchKernelGGL(k_bw_adler, dim3((nb + 3) / 4), dim3(256), 0, w->stream, d_out, d_mem, d_size, nb, d_status);
        HIPOK(hipGetLastError());
        hipLaunchKernelGGL(k_bw_spans, dim3((nb + 255) / 256), dim3(256), 0, w->stream, d_size, stride, nb, d_spans);
        HIPOK(hipGetLastError());
    } else {
        sp.resize(nb);
        for (u32 i = 0; i < nb; i++) {
            if (blocks[i].size > 0xffffffffull)
                return fail(PMX_DBAM_ERR_FORMAT, w->bigbed ? "bigBed data block larger than 4 GB" : "BigWig data block larger than 4 GB");
            sp[i].off = blocks[i].offset;
            sp[i].size = (u32)blocks[i].size;
            sp[i].pad = 0;
        }
        HIPOK(hipMemcpyAsync(d_spans, sp.data(), sizeof(BwSpan) * nb, hipMemcpyHostToDevice, w->stream));
    }
    BW_STEP("adler / spans")
    const u8 *base = z ? d_out : w->d_file;
    const dim3 grid((nb + 3) / 4);
    if (w->bigbed)
        bb_launch_records(false, grid, w->stream, base, d_spans, nb, d_lens, (u32)lens.size(), threshold, d_status, d_cnt, d_bchrom, d_place,
                          nullptr, nullptr, nullptr);
    else
        hipLaunchKernelGGL(k_bw_sections<false>, grid, dim3(256), 0, w->stream, base, d_spans, nb, d_lens, (u32)lens.size(), threshold,
                           d_status, d_cnt, d_bchrom, d_place, (u32 *)nullptr, (u32 *)nullptr, (float *)nullptr);
    HIPOK(hipGetLastError());
    BW_STEP(w->bigbed ? "records (count)" : "sections (count)")
    hipLaunchKernelGGL(k_bam_scan, dim3(1), dim3(1024), 0, w->stream, d_cnt, d_cnt, (u64)nb, d_place, d_tot);
    HIPOK(hipGetLastError());
    std::vector<u32> status(nb), cnt(nb), bchrom(nb);
    std::vector<u64> place(nb);
    u64 tot[2] = {0, 0};
    HIPOK(hipMemcpyAsync(status.data(), d_status, 4ull * nb, hipMemcpyDeviceToHost, w->stream));
    HIPOK(hipMemcpyAsync(cnt.data(), d_cnt, 4ull * nb, hipMemcpyDeviceToHost, w->stream));
    HIPOK(hipMemcpyAsync(bchrom.data(), d_bchrom, 4ull * nb, hipMemcpyDeviceToHost, w->stream));
    HIPOK(hipMemcpyAsync(place.data(), d_place, 8ull * nb, hipMemcpyDeviceToHost, w->stream));
    HIPOK(hipMemcpyAsync(tot, d_tot, 16, hipMemcpyDeviceToHost, w->stream));
    HIPOK(hipStreamSynchronize(w->stream));   // (mem / sp / lens are locals)
    for (u32 i = 0; i < nb; i++)
        if (status[i]) {
            if (w->bigbed)
                return fail(PMX_DBAM_ERR_FORMAT, status[i] >= bigbed::BB_ERR_TRUNCATED ? bigbed::err_text(status[i])
                                                 : status[i] == BW_ERR_ADLER ? bigbed::ERR_ADLER : bigbed::ERR_INFLATE);
            return fail(PMX_DBAM_ERR_FORMAT, status[i] >= BW_ERR_HEADER ? bw_err_text(status[i]) : "BigWig data block does not inflate");
        }
    // the range of every chromosome: its blocks are consecutive in index order (a chromosome whose blocks are not -- an index that is
    // not sorted by chromosome -- cannot be served from one range and is refused)
    std::vector<int> by_id((size_t)max_id + 1, -1);
    for (size_t i = 0; i < w->ids.size(); i++) by_id[w->ids[i]] = (int)i;
    std::vector<char> closed(w->names.size(), 0);
    int cur = -1;
    for (u32 i = 0; i < nb; i++) {
        const int k = bchrom[i] <= max_id ? by_id[bchrom[i]] : -1;
        if (k != cur) {
            if (cur >= 0) closed[(size_t)cur] = 1;
            cur = k;
            if (k >= 0) {
                if (closed[(size_t)k])
                    return fail(PMX_DBAM_ERR_FORMAT, w->bigbed ? "bigBed index is not sorted by chromosome" : "BigWig index is not sorted by chromosome");
                w->range[(size_t)k].first = place[i];
                w->range[(size_t)k].second = place[i];
            }
        }
        if (k >= 0) w->range[(size_t)k].second = place[i] + cnt[i];
    }
    if (tot[0]) {
        HIPOK(hipMalloc((void **)&w->d_begin, 4 * tot[0]));
        HIPOK(hipMalloc((void **)&w->d_end, 4 * tot[0]));
        HIPOK(hipMalloc((void **)&w->d_value, 4 * tot[0]));
        if (w->bigbed)
            bb_launch_records(true, grid, w->stream, base, d_spans, nb, d_lens, (u32)lens.size(), threshold, d_status, d_cnt, d_bchrom,
                              d_place, w->d_begin, w->d_end, w->d_value);
        else
            hipLaunchKernelGGL(k_bw_sections<true>, grid, dim3(256), 0, w->stream, base, d_spans, nb, d_lens, (u32)lens.size(), threshold,
                               d_status, d_cnt, d_bchrom, d_place, w->d_begin, w->d_end, w->d_value);
        HIPOK(hipGetLastError());
        HIPOK(hipStreamSynchronize(w->stream));
    }
    w->total = tot[0];
    return 0;
#undef BW_STEP
}

}  // namespace

static int tt_decode_all(pmx_dbw *w, float threshold);   // text_track_device.inc
static int km_select(pmx_dbw *w, float threshold);       // kmer_track_device.inc

extern "C" {

static int64_t dbw_fetch_impl(pmx_dbw *w, const char *chrom, float threshold);
int64_t pmx_dbw_fetch(pmx_dbw *w, const char *chrom, float threshold)
{
    try {
        return dbw_fetch_impl(w, chrom, threshold);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dbw_fetch: ") + e.what());
    }
}
static int64_t dbw_fetch_impl(pmx_dbw *w, const char *chrom, float threshold)
{
    if (!w || !chrom) return fail(PMX_DBAM_ERR_INVALID, "null argument");
    HIPOK(hipSetDevice(w->device));
    size_t k = 0;
    while (k < w->names.size() && w->names[k] != chrom) k++;
    if (k == w->names.size()) return fail(PMX_DBAM_ERR_NOTFOUND, std::string("unknown chromosome: ") + chrom);
    if (!(threshold > 0.f)) threshold = 0.f;
    if (!w->have || w->have_threshold != threshold) {
        w->have = false;
        const int rc = w->kmer ? km_select(w, threshold) : w->text ? tt_decode_all(w, threshold) : bw_decode_all(w, threshold);
        if (rc) return rc;
    }
    w->cur = k;
    const u64 n = w->range[k].second - w->range[k].first;
    if (n && w->order[k] < 0) {   // ascending and disjoint?  (asked once per chromosome)
        u32 *d_bad = nullptr, bad = 0;
        HIPOK(hipMalloc((void **)&d_bad, 4));
        hipError_t e = hipMemsetAsync(d_bad, 0, 4, w->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_bw_order, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, w->stream, w->d_begin + w->range[k].first,
                               w->d_end + w->range[k].first, n, d_bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, w->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(w->stream);
        (void)hipFree(d_bad);
        if (e != hipSuccess) return fail(PMX_DBAM_ERR_DEVICE, std::string("pmx_dbw_fetch: ") + hipGetErrorString(e));
        w->order[k] = bad ? 0 : 1;
    }
    w->n = n;
    w->sorted = n ? w->order[k] == 1 : true;
    return (int64_t)n;
}

int pmx_dbw_device_arrays(const pmx_dbw *w, const uint32_t **d_begin, const uint32_t **d_end, const float **d_value)
{
    if (!w) return fail(PMX_DBAM_ERR_INVALID, "null handle");
    const u64 o = (w->have && w->cur < w->range.size()) ? w->range[w->cur].first : 0;
    if (d_begin) *d_begin = w->d_begin ? w->d_begin + o : nullptr;
    if (d_end) *d_end = w->d_end ? w->d_end + o : nullptr;
    if (d_value) *d_value = w->d_value ? w->d_value + o : nullptr;
    return 0;
}

int pmx_dbw_sorted(const pmx_dbw *w) { return (w && w->sorted) ? 1 : 0; }

int pmx_dbw_copy(pmx_dbw *w, int64_t first, int64_t n, uint32_t *begin, uint32_t *end, float *value)
{
    if (!w || first < 0 || n < 0 || (u64)(first + n) > w->n) return fail(PMX_DBAM_ERR_INVALID, "range outside the fetched intervals");
    if (n == 0) return 0;
    HIPOK(hipSetDevice(w->device));
    first += (int64_t)w->range[w->cur].first;
    if (begin) HIPOK(hipMemcpyAsync(begin, w->d_begin + first, 4 * (size_t)n, hipMemcpyDeviceToHost, w->stream));
    if (end) HIPOK(hipMemcpyAsync(end, w->d_end + first, 4 * (size_t)n, hipMemcpyDeviceToHost, w->stream));
    if (value) HIPOK(hipMemcpyAsync(value, w->d_value + first, 4 * (size_t)n, hipMemcpyDeviceToHost, w->stream));
    HIPOK(hipStreamSynchronize(w->stream));
    return 0;
}

}  // extern "C"
