// The .bai index (SAM spec 5.2) as per-reference ranges of virtual file offsets [beg, end).  Header-only, without zlib or
// anything else of libpymasc_io.so: the host reader (bam_reader.cpp, pmx_bam_index_load) and the device ingest
// (ingest/bam_device.hip, pmx_dbam_open_indexed) include the same parser, so the two cannot read an index differently.
#ifndef PMX_BAI_INDEX_H
#define PMX_BAI_INDEX_H

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace pmx_bai {

struct RefRange {
    bool has = false;           // the reference has records
    uint64_t beg = 0, end = 0;  // virtual offsets: coffset << 16 | uoffset
};

// Parses the index in d[0, n).  The range of a reference is the pseudo-bin 37450 {ref_beg, ref_end} when present, otherwise
// the minimum begin and the maximum end over the chunks of all its bins.  Returns false with `err` set when the index is
// truncated, has a bad magic or lists another number of references than `n_ref_header`.
inline bool parse(const uint8_t *d, size_t n, size_t n_ref_header, std::vector<RefRange> &out, std::string &err)
{
    auto le32 = [&](size_t q) { return (uint32_t)d[q] | ((uint32_t)d[q + 1] << 8) | ((uint32_t)d[q + 2] << 16) | ((uint32_t)d[q + 3] << 24); };
    auto le64 = [&](size_t q) { return (uint64_t)le32(q) | ((uint64_t)le32(q + 4) << 32); };
    auto have = [&](size_t p, size_t k) { return p <= n && k <= n - p; };
    if (!have(0, 8)) {
        err = "truncated BAM index";
        return false;
    }
    if (memcmp(d, "BAI\1", 4) != 0) {
        err = "not a BAM index (bad magic)";
        return false;
    }
    const uint32_t n_ref = le32(4);
    if (n_ref != n_ref_header) {
        err = "BAM index lists a different number of references than the BAM header";
        return false;
    }
    std::vector<RefRange> idx(n_ref);
    size_t p = 8;
    for (uint32_t r = 0; r < n_ref; r++) {
        if (!have(p, 4)) {
            err = "truncated BAM index";
            return false;
        }
        const uint32_t n_bin = le32(p);
        p += 4;
        uint64_t lo = UINT64_MAX, hi = 0;
        bool pseudo = false;
        for (uint32_t k = 0; k < n_bin; k++) {
            if (!have(p, 8)) {
                err = "truncated BAM index";
                return false;
            }
            const uint32_t bin = le32(p), n_chunk = le32(p + 4);
            p += 8;
            if (!have(p, (size_t)n_chunk * 16)) {
                err = "truncated BAM index";
                return false;
            }
            if (bin == 37450 && n_chunk >= 1) {          // pseudo-bin: [ref_beg, ref_end) then the read counts
                idx[r].beg = le64(p);
                idx[r].end = le64(p + 8);
                pseudo = true;
            } else {
                for (uint32_t c = 0; c < n_chunk; c++) {
                    const uint64_t cb = le64(p + 16 * (size_t)c), ce = le64(p + 16 * (size_t)c + 8);
                    if (cb < lo) lo = cb;
                    if (ce > hi) hi = ce;
                }
            }
            p += (size_t)n_chunk * 16;
        }
        if (!have(p, 4)) {
            err = "truncated BAM index";
            return false;
        }
        const uint32_t n_intv = le32(p);
        p += 4;
        if (!have(p, (size_t)n_intv * 8)) {
            err = "truncated BAM index";
            return false;
        }
        p += (size_t)n_intv * 8;
        if (pseudo) {
            idx[r].has = idx[r].end > idx[r].beg;
        } else if (hi > lo) {
            idx[r].has = true;
            idx[r].beg = lo;
            idx[r].end = hi;
        }
    }
    out.swap(idx);
    return true;
}

}  // namespace pmx_bai
#endif
