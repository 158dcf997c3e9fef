// The one host track handle (include/pymasc_amd_io.h, pmx_track): what every kind of mappability track shares -- the chromosome
// dictionary, the kind, the sorted flag of the last fetch -- with the interval source behind a virtual fetch.  track.cpp holds
// the pmx_track_* accessors (name lookup, argument checks, error wrapping); bigwig_reader.cpp decodes and caches, a text track
// and a k-mer track are both a StoredTrack filled at open.
#ifndef PMX_IO_TRACK_H
#define PMX_IO_TRACK_H

#include <memory>
#include <string>
#include <vector>

#include "io_common.h"

struct pmx_track {
    std::vector<std::string> names;
    std::vector<int64_t> sizes;
    int kind = 0;                            // 0 BigWig (and text tracks), 1 bigBed, 2 k-mer: pmx_dbw_kind's numbering
    bool sorted = true;                      // begin < end and end <= the next begin over what the last fetch delivered
    virtual ~pmx_track() {}
    // The intervals of chromosome c with value >= threshold (threshold <= 0: every one): their number when begin is NULL,
    // otherwise up to cap of them written; sets `sorted` through a Sorted.  May throw pmx_io::Error.
    virtual int64_t fetch(size_t c, float threshold, int64_t cap, uint32_t *begin, uint32_t *end, float *value) = 0;
};

namespace pmx_io {

// The one definition of pmx_track_sorted, fed the intervals of a fetch in order.
struct Sorted {
    bool ok = true;
    uint32_t prev_end = 0;
    void add(uint32_t b, uint32_t e)
    {
        if (!(b < e) || b < prev_end) ok = false;
        prev_end = e;
    }
};

// Per chromosome begin / end / value in file order.  A k-mer track leaves v empty: every value is 1.0.
struct StoredTrack : pmx_track {
    std::vector<std::vector<uint32_t>> b, e;
    std::vector<std::vector<float>> v;
    int64_t fetch(size_t c, float threshold, int64_t cap, uint32_t *begin, uint32_t *end, float *value) override;
};

// The frame of every pmx_*_open: the argument check under the function's name `fn`, then make() (a std::unique_ptr of the
// track; it throws pmx_io::Error); an error gets the path in front.
template <class Make>
int open_track(const char *fn, const char *path, pmx_track **out, Make make)
{
    if (!path || !out) return fail(PMX_IO_ERR_INVALID, std::string(fn) + ": NULL argument");
    *out = nullptr;
    try {
        *out = make().release();
    } catch (const Error &e) {
        return fail(e.code, std::string(path) + ": " + e.msg);
    } catch (const std::exception &e) {
        return fail(PMX_IO_ERR_OPEN, std::string(path) + ": " + e.what());
    }
    return PMX_IO_OK;
}

}  // namespace pmx_io
#endif
