// bigBed mappability tracks -> intervals.  Shared by the host reader (io/bigwig_reader.cpp, libpymasc_io.so) and the device
// reader (ingest/bigbed_device.inc, libpymasc_ingest.so): one set of record rules, one set of error codes and messages, so both
// readers refuse the same block for the same reason.
//
//   header      the bbi header of a BigWig file with magic 0x8789F2EB; fieldCount (offset 32) >= 3.  Zoom levels, autoSql,
//               the total summary and the extension / extra indices are not read
//   blocks      the R-tree's leaves, zlib streams when uncompressBufSize > 0, each holding whole records of ONE chromosome
//   record      chromId u32, chromStart u32, chromEnd u32, then the rest of the BED line up to and including a NUL
//               (bed3: the NUL alone); record k+1 starts right behind record k's NUL
//   value       every record is [chromStart, chromEnd) with value 1.0, whatever its other fields say (text BED, 7.10)
//   keep        as a BigWig item: dropped when chromStart >= the chromosome's size or chromEnd == 0, and when threshold > 0 and
//               1.0 < threshold
//   errors      the first bad record of a block (in record order) decides: fewer than 13 bytes left, no NUL before the block
//               ends, chromEnd < chromStart, a chromId other than the block's first record's
//
// The R-tree walk of both bbi readers (BigWig and bigBed) ends on any input: a child must lie strictly after its parent and
// inside the file, and the leaf items may not outnumber file size / 32 (a leaf item is 32 bytes).
#ifndef PMX_BIGBED_PARSE_H
#define PMX_BIGBED_PARSE_H

#include <cstdint>
#include <cstring>

namespace bigbed {

constexpr uint32_t MAGIC = 0x8789F2EBu;
constexpr uint32_t RECORD_MIN = 13;     // 12 binary bytes and the NUL of an empty rest

// per-block status codes (the device writes them to status[m]; above the BigWig and inflate codes)
enum : uint32_t {
    BB_OK = 0,
    BB_ERR_TRUNCATED = 40,   // fewer than 13 bytes left for a record
    BB_ERR_NO_NUL = 41,      // the rest of the BED line has no NUL before the block ends
    BB_ERR_RANGE = 42,       // chromEnd < chromStart
    BB_ERR_CHROM = 43,       // a record of another chromosome than the block's first
};

inline const char *err_text(uint32_t code)
{
    switch (code) {
    case BB_ERR_TRUNCATED: return "bigBed record does not fit in its data block (fewer than 13 bytes left)";
    case BB_ERR_NO_NUL: return "bigBed record does not fit in its data block (no NUL before the block ends)";
    case BB_ERR_RANGE: return "bigBed record ends before it starts";
    case BB_ERR_CHROM: return "bigBed data block holds records of more than one chromosome";
    }
    return "bigBed data block is malformed";
}

constexpr const char *ERR_SWAPPED = "byte-swapped (big-endian) bigBed files are not supported";
constexpr const char *ERR_FIELDS = "bigBed fieldCount below 3";
constexpr const char *ERR_INFLATE = "bigBed data block does not inflate";
constexpr const char *ERR_ADLER = "bigBed data block does not inflate (Adler-32 mismatch)";

// the R-tree rules of both bbi readers
constexpr const char *ERR_RTREE_CHILD = "R-tree child does not lie after its parent inside the file";
constexpr const char *ERR_RTREE_ITEMS = "R-tree has more leaf items than the file has room for";

// The records of one (inflated) block, in order: f(chrom, start, end) for each good record until the first bad one, whose code
// is returned (BB_OK when every record is good).  The host reader's decoder and the rule k_bb_records implements.
template <class F>
inline uint32_t walk_block(const uint8_t *d, uint64_t n, F &&f)
{
    uint64_t p = 0;
    uint32_t first = 0;
    while (p < n) {
        if (n - p < RECORD_MIN) return BB_ERR_TRUNCATED;
        const void *z = memchr(d + p + 12, 0, (size_t)(n - p - 12));
        if (!z) return BB_ERR_NO_NUL;
        uint32_t c, s, e;
        memcpy(&c, d + p, 4);
        memcpy(&s, d + p + 4, 4);
        memcpy(&e, d + p + 8, 4);
        if (e < s) return BB_ERR_RANGE;
        if (p == 0) first = c;
        else if (c != first) return BB_ERR_CHROM;
        f(c, s, e);
        p = (uint64_t)((const uint8_t *)z - d) + 1;
    }
    return BB_OK;
}

}  // namespace bigbed

#endif
