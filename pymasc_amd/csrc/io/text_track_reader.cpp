// Text mappability tracks -- bedGraph, BED, WIG; plain, BGZF or gzip -- -> the intervals a BigWig reader gives
// (include/pymasc_amd_io.h, pmx_ttrack_open; the handle is track.h's StoredTrack).  The host twin of the device reader (ingest/text_track_device.inc) and its
// checker: the same rules (io/text_track_parse.h), every value through (float)strtod.  The whole text is read at open:
//
//   file (mmap; gzip / BGZF: every member inflated with zlib) --kind from the first lines (track type=, a WIG declaration,
//   the .bed suffix)--> one line at a time: the WIG block state, the chromosome of every data line (a name seen before is
//   found by its bytes) --> per chromosome: begin / end / value in file order, and the largest end (chromsizes)
#include "../../../include/pymasc_amd_io.h"
#include "io_common.h"
#include "text_track_parse.h"
#include "track.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

void parse_text(pmx_io::StoredTrack &t, const uint8_t *text, uint64_t N, const std::string &path)
{
    using namespace ttrack;
    uint32_t kind = 0;                   // bedGraph, BED or WIG (the handle's kind stays 0: a text track answers as a BigWig)
    if (detect_kind(text, N, true, path, kind) != 0) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "cannot tell the kind of track");
    PtrSrc s{text};
    std::unordered_map<std::string, uint32_t> ids;
    uint64_t line = 0, p = 0;
    bool seen_data = false, seen_track = false;
    // the current WIG block
    uint32_t decl = L_SKIP, start = 0, step = 0, span = 1, chrom = 0, decl_nlen = 0;
    uint64_t k = 0, decl_name = 0;
    bool have_chrom = false;             // (a chromosome is named by its first data line: a block without lines adds none)
    auto chrom_of = [&](uint64_t name, uint32_t nlen) -> uint32_t {
        std::string key((const char *)text + name, nlen);
        auto it = ids.find(key);
        if (it != ids.end()) return it->second;
        const uint32_t id = (uint32_t)t.names.size();
        ids.emplace(key, id);
        t.names.push_back(key);
        t.sizes.push_back(0);
        t.b.emplace_back();
        t.e.emplace_back();
        t.v.emplace_back();
        return id;
    };
    for (; p < N; line++) {
        const uint8_t *q = (const uint8_t *)memchr(text + p, '\n', (size_t)(N - p));
        const uint64_t end = q ? (uint64_t)(q - text) : N;
        Line L;
        uint32_t err = parse_line(s, p, end, kind, L);
        if (!err && L.type == L_TRACK) {
            if (seen_data) err = TT_ERR_LATE_TRACK;
            else if (seen_track) err = TT_ERR_TRACK;
            seen_track = true;
        }
        if (!err && (L.type == L_VAR || L.type == L_FIXED)) {
            seen_data = true;
            decl = L.type;
            start = L.b;
            step = L.e;
            span = L.span;
            decl_name = L.name;
            decl_nlen = L.nlen;
            have_chrom = false;
            k = 0;
        } else if (!err && L.type == L_DATA) {
            seen_data = true;
            uint32_t c = 0, b = L.b, e = L.e;
            if (kind == KIND_WIG) {
                if (decl == L_SKIP) err = TT_ERR_NODECL;
                else err = wig_interval(decl, L.nfields, L.b, start, step, span, k++, b, e);
                if (!err && !have_chrom) {
                    chrom = chrom_of(decl_name, decl_nlen);
                    have_chrom = true;
                }
                c = chrom;
            } else {
                c = chrom_of(L.name, L.nlen);
            }
            if (!err) {
                const float v = (kind == KIND_BED) ? 1.0f : slow_value((const char *)text + L.voff, L.vlen);
                t.b[c].push_back(b);
                t.e[c].push_back(e);
                t.v[c].push_back(v);
                t.sizes[c] = std::max<int64_t>(t.sizes[c], e);
            }
        }
        if (err) throw pmx_io::Error(PMX_IO_ERR_FORMAT, line_error(line, err));
        p = end + 1;
    }
}

}  // namespace

extern "C" {

int pmx_ttrack_open(const char *path, int nthreads, pmx_track **out)
{
    (void)nthreads;
    return pmx_io::open_track("pmx_ttrack_open", path, out, [&]() {
        std::unique_ptr<pmx_io::StoredTrack> t(new pmx_io::StoredTrack);
        pmx_io::MappedFile f;
        f.open(path);
        if (ttrack::detect_compression(f.data, f.size) == ttrack::COMP_PLAIN) {
            parse_text(*t, f.data, f.size, path);
        } else {
            std::vector<uint8_t> text;
            std::string err;
            if (!ttrack::inflate_gzip(f.data, f.size, text, err)) throw pmx_io::Error(PMX_IO_ERR_FORMAT, err);
            f.close();
            parse_text(*t, text.data(), text.size(), path);
        }
        return t;
    });
}

}  // extern "C"
