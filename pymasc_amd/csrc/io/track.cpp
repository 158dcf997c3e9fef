// The pmx_track_* accessors (include/pymasc_amd_io.h) over the base of track.h, and the fetch loop of the tracks that are stored
// whole at open (text tracks, k-mer tracks).
#include "track.h"

namespace pmx_io {

int64_t StoredTrack::fetch(size_t c, float threshold, int64_t cap, uint32_t *begin, uint32_t *end, float *value)
{
    const std::vector<uint32_t> &B = b[c], &E = e[c];
    const float *V = v.empty() ? nullptr : v[c].data();
    int64_t n = 0;
    Sorted s;
    for (size_t i = 0; i < B.size(); i++) {
        const float x = V ? V[i] : 1.0f;
        if (threshold > 0.f && !(x >= threshold)) continue;
        if (begin) {
            if (n >= cap) break;
            begin[n] = B[i];
            end[n] = E[i];
            if (value) value[n] = x;
        }
        s.add(B[i], E[i]);
        n++;
    }
    sorted = s.ok;
    return n;
}

}  // namespace pmx_io

extern "C" {

void pmx_track_close(pmx_track *t) { delete t; }

int32_t pmx_track_nchrom(const pmx_track *t) { return t ? (int32_t)t->names.size() : 0; }

const char *pmx_track_chrom_name(const pmx_track *t, int32_t i)
{
    if (!t || i < 0 || (size_t)i >= t->names.size()) return nullptr;
    return t->names[(size_t)i].c_str();
}

int64_t pmx_track_chrom_len(const pmx_track *t, int32_t i)
{
    if (!t || i < 0 || (size_t)i >= t->sizes.size()) return -1;
    return t->sizes[(size_t)i];
}

int pmx_track_kind(const pmx_track *t) { return t ? t->kind : 0; }

int pmx_track_sorted(const pmx_track *t) { return (t && t->sorted) ? 1 : 0; }

int64_t pmx_track_fetch(pmx_track *t, const char *chrom, float threshold, int64_t cap, uint32_t *begin, uint32_t *end,
                        float *value)
{
    if (!t || !chrom) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_track_fetch: NULL argument");
    if (begin && (!end || cap < 0)) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_track_fetch: end is NULL or cap < 0");
    size_t c = 0;
    while (c < t->names.size() && t->names[c] != chrom) c++;
    if (c == t->names.size()) return pmx_io::fail(PMX_IO_ERR_NOTFOUND, std::string("unknown chromosome: ") + chrom);
    try {
        return t->fetch(c, threshold, cap, begin, end, value);
    } catch (const pmx_io::Error &e) {
        return pmx_io::fail(e.code, e.msg);
    } catch (const std::exception &e) {
        return pmx_io::fail(PMX_IO_ERR_FORMAT, e.what());
    }
}

}  // extern "C"
