// SAM text (SAM spec v1 section 1) -> the fields the calculator and the read-length estimator use.  Shared by the host reader
// (io/sam_reader.cpp, libpymasc_io.so) and the device reader (ingest/sam_device.inc, libpymasc_ingest.so): one set of rules,
// one set of error codes and messages, so both readers reject the same line for the same reason.
//
//   header      the '@' lines before the first record; @SQ SN / LN give the references in header order
//   record      >= 11 TAB-separated fields; FLAG, RNAME, POS, MAPQ and CIGAR are parsed, SEQ / QUAL are not looked at
//   line ends   '\n'; a '\r' before it is dropped; the last line may lack its '\n'; one empty line at the very end is allowed
#ifndef PMX_SAM_PARSE_H
#define PMX_SAM_PARSE_H

#include <cstdint>

#if defined(__HIPCC__)
#define PMX_SAM_HD __host__ __device__ __forceinline__
#else
#define PMX_SAM_HD inline
#endif

namespace samtext {

enum {
    SAM_OK = 0,
    SAM_ERR_FIELDS = 1,      // fewer than 11 fields
    SAM_ERR_FLAG = 2,
    SAM_ERR_RNAME = 3,       // not '*' and not an @SQ name
    SAM_ERR_POS = 4,
    SAM_ERR_MAPQ = 5,
    SAM_ERR_CIGAR = 6,
    SAM_ERR_EMPTY = 7,       // an empty line before the end of the file
    SAM_ERR_LATE_HEADER = 8, // an '@' line after the first record
    SAM_ERR_PNEXT = 9,       // (parse_mates)
    SAM_ERR_TLEN = 10,       // (parse_mates)
    SAM_NERR
};

inline const char *err_text(uint32_t code)
{
    switch (code) {
    case SAM_ERR_FIELDS: return "fewer than 11 TAB-separated fields";
    case SAM_ERR_FLAG: return "FLAG is not a decimal in 0..65535";
    case SAM_ERR_RNAME: return "RNAME is neither '*' nor a reference of an @SQ line";
    case SAM_ERR_POS: return "POS is not a decimal in 0..2147483647";
    case SAM_ERR_MAPQ: return "MAPQ is not a decimal in 0..255";
    case SAM_ERR_CIGAR: return "CIGAR is neither '*' nor (<length < 2^28><op in MIDNSHP=X>)+";
    case SAM_ERR_EMPTY: return "empty line";
    case SAM_ERR_LATE_HEADER: return "header line after the first alignment record";
    case SAM_ERR_PNEXT: return "PNEXT is not a decimal in 0..2147483647";
    case SAM_ERR_TLEN: return "TLEN is not a decimal in -2147483648..2147483647";
    }
    return "malformed alignment line";
}

// FNV-1a over a reference name: the slot of the open-addressing name table (a power of two >= 2x the references)
PMX_SAM_HD uint32_t name_hash_step(uint32_t h, uint8_t c) { return (h ^ c) * 16777619u; }
constexpr uint32_t NAME_HASH_INIT = 2166136261u;

// The @SQ names: concatenated bytes, offsets [nref + 1], slots [mask + 1] holding a reference id or -1.
struct Names {
    const uint8_t *bytes;
    const uint32_t *off;
    const int32_t *slot;
    uint32_t mask;
};

struct Rec {
    int32_t ref;        // -1: RNAME '*'
    int32_t pos1;       // POS (1-based; 0 when unavailable)
    uint32_t qlen;      // sum of the M / I / S / = / X lengths (pysam infer_query_length; 0 for '*'), modulo 2^32 as in BAM
    uint32_t flag, mapq;
};

// Src: at(i) = byte i of the text.  [beg, end) is the line without its '\n'.  Returns SAM_OK or a SAM_ERR_* code.
template <class Src>
PMX_SAM_HD uint32_t parse_line(Src &s, uint64_t beg, uint64_t end, const Names &nm, Rec &r)
{
    if (end > beg && s.at(end - 1) == '\r') end--;
    if (end == beg) return SAM_ERR_EMPTY;
    if (s.at(beg) == '@') return SAM_ERR_LATE_HEADER;
    uint64_t p = beg;
    while (p < end && s.at(p) != '\t') p++;                  // QNAME
    if (p == end) return SAM_ERR_FIELDS;
    p++;
    // a decimal field ending at a TAB: 0 ok, 1 missing TAB (too few fields), 2 malformed
    auto dec = [&](uint32_t maxv, uint32_t &v) -> uint32_t {
        uint64_t x = 0;
        const uint64_t a = p;
        uint32_t bad = 0;
        for (; p < end; p++) {
            const uint8_t c = s.at(p);
            if (c == '\t') break;
            if (c < '0' || c > '9' || x > maxv) {
                bad = 1;
                continue;
            }
            x = x * 10u + (uint32_t)(c - '0');
        }
        if (p == end) return 1;
        p++;
        v = (uint32_t)x;
        return (bad || p - 1 == a || x > maxv) ? 2 : 0;
    };
    uint32_t v, e;
    if ((e = dec(65535u, v))) return e == 1 ? SAM_ERR_FIELDS : SAM_ERR_FLAG;
    r.flag = v;
    {                                                         // RNAME
        const uint64_t a = p;
        uint32_t h = NAME_HASH_INIT;
        while (p < end && s.at(p) != '\t') h = name_hash_step(h, s.at(p++));
        if (p == end) return SAM_ERR_FIELDS;
        const uint64_t len = p - a;
        p++;
        if (len == 1 && s.at(a) == '*') {
            r.ref = -1;
        } else {
            r.ref = -2;
            for (uint32_t k = h & nm.mask, probe = 0; probe <= nm.mask; probe++, k = (k + 1u) & nm.mask) {
                const int32_t id = nm.slot[k];
                if (id < 0) break;
                const uint32_t o = nm.off[id];
                if (nm.off[id + 1] - o != len) continue;
                uint64_t i = 0;
                while (i < len && nm.bytes[o + i] == s.at(a + i)) i++;
                if (i == len) {
                    r.ref = id;
                    break;
                }
            }
            if (r.ref == -2) return SAM_ERR_RNAME;
        }
    }
    if ((e = dec(2147483647u, v))) return e == 1 ? SAM_ERR_FIELDS : SAM_ERR_POS;
    r.pos1 = (int32_t)v;
    if ((e = dec(255u, v))) return e == 1 ? SAM_ERR_FIELDS : SAM_ERR_MAPQ;
    r.mapq = v;
    {                                                         // CIGAR
        uint32_t q = 0, n = 0, ndig = 0, nops = 0;
        bool bad = false;
        if (p + 1 < end && s.at(p) == '*' && s.at(p + 1) == '\t') {
            p++;
        } else {
            for (; p < end; p++) {
                const uint8_t c = s.at(p);
                if (c == '\t') break;
                if (c >= '0' && c <= '9') {
                    if (n >= (1u << 28) / 10u + 1u) bad = true;
                    else n = n * 10u + (uint32_t)(c - '0');
                    ndig++;
                    continue;
                }
                // M=0 I=1 D=2 N=3 S=4 H=5 P=6 '='=7 X=8
                int op = c == 'M' ? 0 : c == 'I' ? 1 : c == 'D' ? 2 : c == 'N' ? 3 : c == 'S' ? 4 : c == 'H' ? 5 : c == 'P' ? 6
                       : c == '=' ? 7 : c == 'X' ? 8 : -1;
                if (op < 0 || ndig == 0 || n >= (1u << 28)) bad = true;
                else if ((0x193u >> op) & 1u) q += n;
                n = 0;
                ndig = 0;
                nops++;
            }
            if (p < end && (ndig || nops == 0)) bad = true;
        }
        if (p == end) return SAM_ERR_FIELDS;
        p++;
        if (bad) return SAM_ERR_CIGAR;
        r.qlen = q;
    }
    for (int k = 0; k < 4; k++) {                             // RNEXT, PNEXT, TLEN, SEQ: QUAL must follow
        while (p < end && s.at(p) != '\t') p++;
        if (p == end) return SAM_ERR_FIELDS;
        p++;
    }
    return SAM_OK;
}

// The mate fields of a line that parse_line accepted (fields 7-9: RNEXT, PNEXT, TLEN), read only by the pair counts
// (DESIGN.md 7.21).  same: RNEXT is '=' or byte-equal to RNAME; [rnext, rnext + rnext_len) is RNEXT in the text.
struct Mates {
    int32_t mate_pos1;  // PNEXT (1-based; 0 when unavailable)
    int32_t tlen;       // TLEN, signed
    uint32_t same;
    uint64_t rnext, rnext_len;
};

template <class Src>
PMX_SAM_HD uint32_t parse_mates(Src &s, uint64_t beg, uint64_t end, Mates &m)
{
    if (end > beg && s.at(end - 1) == '\r') end--;
    uint64_t p = beg, f[9];                                   // f[k]: the start of field k + 1; f[k + 1] - 1 its end
    f[0] = beg;
    for (int k = 1; k < 9; k++) {                             // (>= 11 fields: parse_line has seen them)
        while (p < end && s.at(p) != '\t') p++;
        if (p == end) return SAM_ERR_FIELDS;
        f[k] = ++p;
    }
    uint64_t e9 = f[8];
    while (e9 < end && s.at(e9) != '\t') e9++;
    const uint64_t a2 = f[2], n2 = f[3] - 1 - a2, a6 = f[6], n6 = f[7] - 1 - a6;
    m.rnext = a6;
    m.rnext_len = n6;
    m.same = n6 == 1 && s.at(a6) == '=';
    if (!m.same && n6 == n2 && !(n6 == 1 && s.at(a6) == '*')) {
        uint64_t i = 0;
        while (i < n6 && s.at(a2 + i) == s.at(a6 + i)) i++;
        m.same = i == n6;
    }
    // a decimal in [a, e): at most `lim`
    auto dec = [&](uint64_t a, uint64_t e, uint64_t lim, uint64_t &v) -> bool {
        if (a == e) return false;
        uint64_t x = 0;
        for (uint64_t i = a; i < e; i++) {
            const uint8_t c = s.at(i);
            if (c < '0' || c > '9') return false;
            x = x * 10u + (uint32_t)(c - '0');
            if (x > lim) return false;
        }
        v = x;
        return true;
    };
    uint64_t v = 0;
    if (!dec(f[7], f[8] - 1, 2147483647u, v)) return SAM_ERR_PNEXT;
    m.mate_pos1 = (int32_t)v;
    uint64_t a = f[8];
    const bool neg = a < e9 && s.at(a) == '-';
    if (neg || (a < e9 && s.at(a) == '+')) a++;
    if (!dec(a, e9, neg ? 2147483648u : 2147483647u, v)) return SAM_ERR_TLEN;
    m.tlen = neg ? (int32_t)(0u - (uint32_t)v) : (int32_t)v;
    return SAM_OK;
}

}  // namespace samtext

#include <string>
#include <unordered_set>
#include <vector>

namespace samtext {

// The header of a SAM text (host code: the device reader parses it from the stream's prefix too).
struct Header {
    std::string text;                   // the header lines as they are in the file
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    uint64_t data_beg = 0;              // offset of the first line that is not a header line
    uint64_t lines = 0;                 // header lines
    // the name table of Names
    std::vector<uint8_t> bytes;
    std::vector<uint32_t> off;
    std::vector<int32_t> slot;
};

// Parses the header in t[0, n).  complete: t holds the whole text (else the header may continue past n).  Returns 0, 1 when
// the header runs past n and the text is not complete (give more), or -1 with `err` set ("line N: ...").
inline int parse_header(const char *t, uint64_t n, bool complete, Header &h, std::string &err)
{
    h = Header();
    uint64_t p = 0, line = 0;
    std::unordered_set<std::string> seen;
    while (p < n && t[p] == '@') {
        uint64_t e = p;
        while (e < n && t[e] != '\n') e++;
        if (e == n && !complete) return 1;
        line++;
        uint64_t le = e;
        if (le > p && t[le - 1] == '\r') le--;
        const std::string ln(t + p, le - p);
        if (ln.compare(0, 4, "@SQ\t") == 0) {
            std::string sn;
            bool have_sn = false, have_ln = false, ln_ok = true;
            int64_t len = 0;
            size_t a = 4;
            while (a <= ln.size()) {
                size_t b = ln.find('\t', a);
                if (b == std::string::npos) b = ln.size();
                const std::string f = ln.substr(a, b - a);
                if (f.compare(0, 3, "SN:") == 0 && !have_sn) {
                    sn = f.substr(3);
                    have_sn = true;
                } else if (f.compare(0, 3, "LN:") == 0 && !have_ln) {
                    have_ln = true;
                    const std::string d = f.substr(3);
                    ln_ok = !d.empty() && d.size() <= 10;
                    for (char c : d) ln_ok = ln_ok && c >= '0' && c <= '9';
                    if (ln_ok) len = std::stoll(d);
                    ln_ok = ln_ok && len >= 1 && len <= 2147483647LL;
                }
                a = b + 1;
            }
            const std::string where = "line " + std::to_string(line) + ": ";
            if (!have_sn || sn.empty()) return err = where + "@SQ line without SN", -1;
            if (!have_ln) return err = where + "@SQ line without LN", -1;
            if (!ln_ok) return err = where + "@SQ LN is not a decimal in 1..2147483647", -1;
            if (!seen.insert(sn).second) return err = where + "duplicate @SQ SN " + sn, -1;
            h.names.push_back(sn);
            h.lens.push_back(len);
        }
        p = e < n ? e + 1 : n;
    }
    if (p == n && !complete) return 1;
    if (h.names.empty()) return err = "no @SQ lines in the SAM header", -1;
    h.text.assign(t, p);
    h.data_beg = p;
    h.lines = line;
    h.off.push_back(0);
    for (const std::string &s : h.names) {
        h.bytes.insert(h.bytes.end(), s.begin(), s.end());
        h.off.push_back((uint32_t)h.bytes.size());
    }
    uint32_t slots = 2;
    while (slots < 2u * h.names.size()) slots <<= 1;
    h.slot.assign(slots, -1);
    for (size_t i = 0; i < h.names.size(); i++) {
        uint32_t x = NAME_HASH_INIT;
        for (unsigned char c : h.names[i]) x = name_hash_step(x, c);
        uint32_t k = x & (slots - 1);
        while (h.slot[k] >= 0) k = (k + 1u) & (slots - 1);
        h.slot[k] = (int32_t)i;
    }
    return 0;
}

inline Names names_of(const Header &h)
{
    return Names{h.bytes.data(), h.off.data(), h.slot.data(), (uint32_t)h.slot.size() - 1u};
}

// "line N: reason" of the record error (code) on record line `rec` (0-based among the lines after the header)
inline std::string line_error(const Header &h, uint64_t rec, uint32_t code)
{
    return "line " + std::to_string(h.lines + rec + 1) + ": " + err_text(code);
}

}  // namespace samtext
#endif
