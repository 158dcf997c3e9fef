// BED read files (tagAlign: BED6, one line per read) -> the per-record fields of the SAM parse table.  Shared by the host
// reader (io/sam_reader.cpp pmx_bed_open, libpymasc_io.so) and the device reader (ingest/bed_reads_device.inc, libpymasc_ingest.so):
// one set of rules, one set of error codes and messages, so both readers reject the same line for the same reason.
//
//   lines       '\n'-terminated (the last one may lack it); a '\r' before the '\n' is dropped; fields are runs of bytes separated
//               by runs of TABs or spaces (io/text_track_parse.h); blank lines, '#' lines and "browser" lines carry no read and
//               may stand anywhere; at most one "track" line, before the first read
//   read        chrom start end name score strand [...]: >= 6 fields, those after the sixth ignored; chrom a name of the
//               chromosome sizes (byte for byte); 0 <= start < end < 2^31, end - start < 2^28; name ignored; score a
//               non-negative decimal (MAPQ = min(score, 255)) or '.' (MAPQ 255); strand '+' or '-'
//   record      ref = the name's index in the sizes, pos1 = start + 1, qlen = end - start, flag 16 for '-' else 0
#ifndef PMX_BED_READS_PARSE_H
#define PMX_BED_READS_PARSE_H

#include <cstdint>

#include "sam_parse.h"

namespace bedreads {

enum { L_SKIP = 0, L_TRACK = 1, L_READ = 2 };

enum {
    BR_OK = 0,
    BR_ERR_FIELDS = 1,      // fewer than 6 fields
    BR_ERR_CHROM = 2,       // not a name of the chromosome sizes
    BR_ERR_COORD = 3,       // start or end is not a decimal below 2^31
    BR_ERR_RANGE = 4,       // end <= start
    BR_ERR_SPAN = 5,        // end - start >= 2^28
    BR_ERR_SCORE = 6,       // neither a non-negative decimal nor '.'
    BR_ERR_STRAND = 7,      // neither '+' nor '-'
    BR_ERR_TRACK = 8,       // a second track line
    BR_ERR_LATE_TRACK = 9,  // a track line after the first read
    BR_NERR
};

inline const char *err_text(uint32_t code)
{
    switch (code) {
    case BR_ERR_FIELDS: return "fewer than 6 fields (chrom start end name score strand)";
    case BR_ERR_CHROM: return "chrom is not a chromosome of the chromosome sizes";
    case BR_ERR_COORD: return "start or end is not a decimal below 2^31";
    case BR_ERR_RANGE: return "end is not greater than start";
    case BR_ERR_SPAN: return "end - start is not below 2^28";
    case BR_ERR_SCORE: return "score is neither a non-negative decimal nor '.'";
    case BR_ERR_STRAND: return "strand is neither '+' nor '-'";
    case BR_ERR_TRACK: return "more than one track line";
    case BR_ERR_LATE_TRACK: return "track line after the first read";
    }
    return "malformed line";
}

PMX_SAM_HD bool is_ws(uint8_t c) { return c == ' ' || c == '\t'; }

// [a, b) -> v, saturated at `sat`: false unless 1+ decimal digits
template <class Src>
PMX_SAM_HD bool dec_sat(Src &s, uint64_t a, uint64_t b, uint32_t sat, uint32_t &v)
{
    if (b <= a) return false;
    uint64_t x = 0;
    for (uint64_t p = a; p < b; p++) {
        const uint8_t c = s.at(p);
        if (c < '0' || c > '9') return false;
        x = x * 10u + (uint32_t)(c - '0');
        if (x > sat) x = sat;
    }
    v = (uint32_t)x;
    return true;
}

template <class Src>
PMX_SAM_HD bool token_is(Src &s, uint64_t a, uint64_t b, const char *w)
{
    uint64_t p = a;
    for (; *w; w++, p++)
        if (p >= b || s.at(p) != (uint8_t)*w) return false;
    return p == b;
}

// Src: at(i) = byte i of the text.  [beg, end) is the line without its '\n'.  Returns BR_OK or a BR_ERR_* code; *type says
// what the line is (L_READ: r holds the record).  The track-line rules need the lines before this one: the caller applies them.
template <class Src>
PMX_SAM_HD uint32_t parse_line(Src &s, uint64_t beg, uint64_t end, const samtext::Names &nm, uint32_t &type, samtext::Rec &r)
{
    type = L_SKIP;
    if (end > beg && s.at(end - 1) == '\r') end--;
    uint64_t p = beg;
    while (p < end && is_ws(s.at(p))) p++;
    if (p == end || s.at(p) == '#') return BR_OK;
    // the first six fields (scalars: a lane's fields stay in registers)
    uint64_t a[6] = {0, 0, 0, 0, 0, 0}, b[6] = {0, 0, 0, 0, 0, 0};
    uint32_t n = 0;
    while (p < end && n < 6) {
        const uint64_t q = p;
        while (p < end && !is_ws(s.at(p))) p++;
        for (uint32_t k = 0; k < 6; k++)
            if (k == n) a[k] = q, b[k] = p;
        n++;
        while (p < end && is_ws(s.at(p))) p++;
    }
    if (token_is(s, a[0], b[0], "browser")) return BR_OK;
    if (token_is(s, a[0], b[0], "track")) {
        type = L_TRACK;
        return BR_OK;
    }
    type = L_READ;
    if (n < 6) return BR_ERR_FIELDS;
    {                                                         // chrom
        const uint64_t len = b[0] - a[0];
        uint32_t h = samtext::NAME_HASH_INIT;
        for (uint64_t i = a[0]; i < b[0]; i++) h = samtext::name_hash_step(h, s.at(i));
        r.ref = -1;
        for (uint32_t k = h & nm.mask, probe = 0; probe <= nm.mask; probe++, k = (k + 1u) & nm.mask) {
            const int32_t id = nm.slot[k];
            if (id < 0) break;
            const uint32_t o = nm.off[id];
            if (nm.off[id + 1] - o != len) continue;
            uint64_t i = 0;
            while (i < len && nm.bytes[o + i] == s.at(a[0] + i)) i++;
            if (i == len) {
                r.ref = id;
                break;
            }
        }
        if (r.ref < 0) return BR_ERR_CHROM;
    }
    uint32_t start = 0, stop = 0, score = 0;
    if (!dec_sat(s, a[1], b[1], 0x80000000u, start) || !dec_sat(s, a[2], b[2], 0x80000000u, stop) || start >= 0x80000000u ||
        stop >= 0x80000000u)
        return BR_ERR_COORD;
    if (stop <= start) return BR_ERR_RANGE;
    if (stop - start >= (1u << 28)) return BR_ERR_SPAN;
    if (b[4] - a[4] == 1 && s.at(a[4]) == '.') score = 255;
    else if (!dec_sat(s, a[4], b[4], 255u, score)) return BR_ERR_SCORE;
    if (b[5] - a[5] != 1 || (s.at(a[5]) != '+' && s.at(a[5]) != '-')) return BR_ERR_STRAND;
    r.pos1 = (int32_t)(start + 1u);
    r.qlen = stop - start;
    r.flag = s.at(a[5]) == '-' ? 0x10u : 0u;
    r.mapq = score;
    return BR_OK;
}

// The sort key of a line: ref << 31 | start for a read; a line without a read sorts after every read of `nref` references
PMX_SAM_HD uint64_t sort_key(int32_t ref, int32_t pos1, uint32_t nref)
{
    return ref >= 0 ? ((uint64_t)(uint32_t)ref << 31) | (uint64_t)(uint32_t)(pos1 - 1) : (uint64_t)nref << 31;
}

}  // namespace bedreads

#include <algorithm>
#include <string>
#include <vector>

namespace bedreads {

// The name table of samtext::Names for the chromosome sizes' names (host code; the device reader uploads it)
inline void name_table(const std::vector<std::string> &names, std::vector<uint8_t> &bytes, std::vector<uint32_t> &off,
                       std::vector<int32_t> &slot)
{
    bytes.clear();
    off.assign(1, 0);
    for (const std::string &s : names) {
        bytes.insert(bytes.end(), s.begin(), s.end());
        off.push_back((uint32_t)bytes.size());
    }
    uint32_t slots = 2;
    while (slots < 2u * names.size()) slots <<= 1;
    slot.assign(slots, -1);
    for (size_t i = 0; i < names.size(); i++) {
        uint32_t x = samtext::NAME_HASH_INIT;
        for (unsigned char c : names[i]) x = samtext::name_hash_step(x, c);
        uint32_t k = x & (slots - 1);
        while (slot[k] >= 0) k = (k + 1u) & (slots - 1);
        slot[k] = (int32_t)i;
    }
}

// The track-line rules over the track lines (0-based line numbers, ascending) and the first read line (~0: none): the first
// offending line and its code, or code 0
inline uint32_t track_error(const std::vector<uint64_t> &tracks, uint64_t first_read, uint64_t &line)
{
    for (size_t k = 0; k < tracks.size(); k++) {
        if (tracks[k] > first_read) return line = tracks[k], BR_ERR_LATE_TRACK;
        if (k > 0) return line = tracks[k], BR_ERR_TRACK;
    }
    return 0;
}

inline std::string line_error(uint64_t line0, uint32_t code)
{
    return "line " + std::to_string(line0 + 1) + ": " + err_text(code);
}

// Sizes given by the caller: names unique and non-empty, lengths in 1..2^31-1.  Empty string when they are usable.
inline std::string check_sizes(int32_t nref, const char *const *names, const int64_t *lengths, std::vector<std::string> &out_names,
                               std::vector<int64_t> &out_lens)
{
    if (nref <= 0 || !names || !lengths) return "no chromosome sizes given";
    if (nref >= (1 << 30)) return "too many chromosomes";
    out_names.clear();
    out_lens.clear();
    std::vector<std::string> sorted;
    for (int32_t i = 0; i < nref; i++) {
        if (!names[i] || !names[i][0]) return "chromosome sizes: an empty name";
        if (lengths[i] < 1 || lengths[i] > 2147483647LL) return std::string("chromosome sizes: the length of ") + names[i] + " is not in 1..2^31-1";
        out_names.emplace_back(names[i]);
        out_lens.push_back(lengths[i]);
    }
    sorted = out_names;
    std::sort(sorted.begin(), sorted.end());
    for (size_t i = 1; i < sorted.size(); i++)
        if (sorted[i] == sorted[i - 1]) return "chromosome sizes: " + sorted[i] + " is named twice";
    return "";
}

}  // namespace bedreads
#endif
