// Text mappability tracks (bedGraph, BED, WIG) -> intervals.  Shared by the host reader (io/text_track_reader.cpp,
// libpymasc_io.so) and the device reader (ingest/text_track_device.inc, libpymasc_ingest.so): one set of line and number
// rules, one set of error codes and messages, so both readers reject the same line for the same reason.
//
//   lines       '\n'-terminated (the last one may lack it); a trailing '\r' is dropped; fields are runs of bytes separated by
//               runs of TABs or spaces; blank lines, '#' lines and "browser" lines are skipped anywhere
//   track       at most one "track" line, before the first data line; type=bedGraph / type=wiggle_0 decide the kind
//   bedGraph    chrom start end value (exactly four fields), 0-based half-open
//   BED         chrom start end [...] (at least three fields; the value is 1)
//   WIG         variableStep chrom=C [span=S] / fixedStep chrom=C start=P step=T [span=S] declarations, then "pos value"
//               (variableStep, pos 1-based) or "value" (fixedStep) lines: the BigWig item types 2 and 3 written as text
//   numbers     coordinates: unsigned decimals below 2^32; values: [+-] digits [. digits] [e [+-] digits], stored as
//               (float)strtod(text) -- what bedGraphToBigWig / wigToBigWig store; nan, inf and hex are refused
#ifndef PMX_TEXT_TRACK_PARSE_H
#define PMX_TEXT_TRACK_PARSE_H

#include <cstdint>

#if defined(__HIPCC__)
#define PMX_TT_HD __host__ __device__ __forceinline__
#else
#define PMX_TT_HD inline
#endif

namespace ttrack {

enum { KIND_BEDGRAPH = 0, KIND_BED = 1, KIND_WIG = 2 };
enum { L_SKIP = 0, L_TRACK = 1, L_VAR = 2, L_FIXED = 3, L_DATA = 4 };

enum {
    TT_OK = 0,
    TT_ERR_FIELDS = 1,      // the wrong number of fields for the kind of track
    TT_ERR_COORD = 2,       // a coordinate that is not a decimal below 2^32 (or a WIG interval that ends beyond it)
    TT_ERR_VALUE = 3,       // a value that is not a decimal number
    TT_ERR_RANGE = 4,       // end <= start
    TT_ERR_NODECL = 5,      // a WIG data line before any declaration
    TT_ERR_DECL = 6,        // a malformed variableStep / fixedStep line
    TT_ERR_TRACK = 7,       // a second track line
    TT_ERR_LATE_TRACK = 8,  // a track line after the first data line
    TT_ERR_NAME = 9,        // a chromosome name longer than 255 bytes
    TT_ERR_BLOCK = 10,      // a "pos value" line in a fixedStep block, or a "value" line in a variableStep block
    TT_NERR
};

constexpr uint32_t MAX_NAME = 255;

inline const char *err_text(uint32_t code)
{
    switch (code) {
    case TT_ERR_FIELDS: return "malformed line: wrong number of fields";
    case TT_ERR_COORD: return "bad number: a coordinate is not a decimal below 2^32";
    case TT_ERR_VALUE: return "bad number: the value is not a decimal number";
    case TT_ERR_RANGE: return "malformed line: end is not greater than start";
    case TT_ERR_NODECL: return "data line before any WIG declaration";
    case TT_ERR_DECL: return "malformed variableStep / fixedStep declaration";
    case TT_ERR_TRACK: return "more than one track line";
    case TT_ERR_LATE_TRACK: return "track line after the first data line";
    case TT_ERR_NAME: return "malformed line: chromosome name longer than 255 bytes";
    case TT_ERR_BLOCK: return "malformed line: wrong number of fields for its WIG block";
    }
    return "malformed line";
}

PMX_TT_HD uint32_t hash_step(uint32_t h, uint8_t c) { return (h ^ c) * 16777619u; }
constexpr uint32_t HASH_INIT = 2166136261u;

PMX_TT_HD bool is_ws(uint8_t c) { return c == ' ' || c == '\t'; }

// One parsed line.  Data lines: b / e (bedGraph, BED), pos in b (WIG "pos value"), the value and its token; declarations:
// b = start, e = step, span; the chromosome of data lines and declarations: name offset / length / hash.
struct Line {
    uint32_t type, nfields;
    uint32_t b, e, span;
    float v;
    bool slow;              // the value lies outside the exact fast path: (float)strtod of [voff, voff + vlen) decides
    uint64_t name, voff;
    uint32_t nlen, vlen, hash;
};

// [a, b) -> *out: 1-10 decimal digits, value < 2^32
template <class Src>
PMX_TT_HD bool parse_u32(Src &s, uint64_t a, uint64_t b, uint32_t &out)
{
    if (b <= a || b - a > 10) return false;
    uint64_t x = 0;
    for (uint64_t p = a; p < b; p++) {
        const uint8_t c = s.at(p);
        if (c < '0' || c > '9') return false;
        x = x * 10u + (uint32_t)(c - '0');
    }
    if (x > 0xffffffffull) return false;
    out = (uint32_t)x;
    return true;
}

// 10^k for 0 <= k <= 22: every product is exact in a double (5^22 < 2^53)
PMX_TT_HD double pow10_exact(int k)
{
    double p = 1.0;
    for (int i = 0; i < k; i++) p *= 10.0;
    return p;
}

// [a, b) -> *v.  false: not a decimal number.  Clinger's fast path: at most 15 significant digits and a decimal exponent within
// +-22 make m * 10^e (or m / 10^-e) ONE correctly rounded operation on exact doubles, which is what strtod returns; the cast to
// float is then the same as (float)strtod.  Anything else sets *slow, and the caller takes (float)strtod of the token.
template <class Src>
PMX_TT_HD bool parse_value(Src &s, uint64_t a, uint64_t b, float &v, bool &slow)
{
    uint64_t p = a;
    bool neg = false;
    slow = false;
    if (p < b && (s.at(p) == '+' || s.at(p) == '-')) neg = s.at(p++) == '-';
    uint64_t m = 0;
    int sig = 0, e10 = 0, ndig = 0;
    bool dropped = false, dot = false;
    for (; p < b; p++) {
        const uint8_t c = s.at(p);
        if (c == '.') {
            if (dot) return false;
            dot = true;
            continue;
        }
        if (c < '0' || c > '9') break;
        ndig++;
        if (m == 0 && c == '0') {               // a leading zero: not significant
            if (dot) e10--;
            continue;
        }
        if (sig < 19) {
            m = m * 10u + (uint32_t)(c - '0');
            sig++;
            if (dot) e10--;
        } else {
            if (c != '0') dropped = true;
            sig++;
            if (!dot) e10++;
        }
    }
    if (ndig == 0) return false;
    if (p < b) {
        if (s.at(p) != 'e' && s.at(p) != 'E') return false;
        p++;
        bool eneg = false;
        if (p < b && (s.at(p) == '+' || s.at(p) == '-')) eneg = s.at(p++) == '-';
        if (p == b) return false;
        int x = 0;
        for (; p < b; p++) {
            const uint8_t c = s.at(p);
            if (c < '0' || c > '9') return false;
            if (x < 100000) x = x * 10 + (int)(c - '0');
        }
        e10 += eneg ? -x : x;
    }
    if (m == 0) {
        v = neg ? -0.0f : 0.0f;
        return true;
    }
    while (sig > 15 && !dropped && sig <= 19 && m % 10u == 0) {   // trailing zeros of the mantissa
        m /= 10u;
        sig--;
        e10++;
    }
    if (sig > 15 || dropped || e10 < -22 || e10 > 22) {
        slow = true;
        v = 0.0f;
        return true;
    }
    double d = (double)m;
    d = e10 < 0 ? d / pow10_exact(-e10) : d * pow10_exact(e10);
    v = (float)(neg ? -d : d);
    return true;
}

// Does the token [a, b) spell `w`?
template <class Src>
PMX_TT_HD bool token_is(Src &s, uint64_t a, uint64_t b, const char *w)
{
    uint64_t p = a;
    for (; *w; w++, p++)
        if (p >= b || s.at(p) != (uint8_t)*w) return false;
    return p == b;
}

// Src: at(i) = byte i of the text.  [beg, end) is the line without its '\n'.  kind: KIND_*.  Returns TT_OK or a TT_ERR_* code;
// L.type says what the line is.  A WIG data line is only split here (its interval needs its declaration: wig_interval).
template <class Src>
PMX_TT_HD uint32_t parse_line(Src &s, uint64_t beg, uint64_t end, uint32_t kind, Line &L)
{
    L.type = L_SKIP;
    L.nfields = 0;
    L.b = L.e = 0;
    L.span = 1;
    L.v = 0.0f;
    L.slow = false;
    L.name = L.voff = 0;
    L.nlen = L.vlen = 0;
    L.hash = HASH_INIT;
    if (end > beg && s.at(end - 1) == '\r') end--;
    uint64_t p = beg;
    while (p < end && is_ws(s.at(p))) p++;
    if (p == end || s.at(p) == '#') return TT_OK;
    // the first three fields and the last one (scalars, not an array: a lane's fields stay in registers)
    uint64_t a0 = 0, b0 = 0, a1 = 0, b1 = 0, a2 = 0, b2 = 0, la = 0, lb = 0;
    uint32_t n = 0;
    while (p < end) {
        const uint64_t a = p;
        while (p < end && !is_ws(s.at(p))) p++;
        if (n == 0) a0 = a, b0 = p;
        else if (n == 1) a1 = a, b1 = p;
        else if (n == 2) a2 = a, b2 = p;
        la = a;
        lb = p;
        n++;
        while (p < end && is_ws(s.at(p))) p++;
    }
    L.nfields = n;
    if (token_is(s, a0, b0, "browser")) return TT_OK;
    if (token_is(s, a0, b0, "track")) {
        L.type = L_TRACK;
        return TT_OK;
    }
    if (kind == KIND_WIG) {
        const bool var = token_is(s, a0, b0, "variableStep"), fixed = token_is(s, a0, b0, "fixedStep");
        if (var || fixed) {
            L.type = var ? L_VAR : L_FIXED;
            // key=value tokens after the keyword: chrom, span, and for fixedStep start and step; each at most once
            uint32_t seen = 0;                  // bit 0 chrom, 1 start, 2 step, 3 span
            uint64_t q = b0;
            while (q < end) {
                while (q < end && is_ws(s.at(q))) q++;
                if (q == end) break;
                const uint64_t a = q;
                while (q < end && !is_ws(s.at(q))) q++;
                uint64_t eq = a;
                while (eq < q && s.at(eq) != '=') eq++;
                if (eq == q) return TT_ERR_DECL;
                uint32_t bit;
                if (token_is(s, a, eq, "chrom")) bit = 1;
                else if (token_is(s, a, eq, "start") && fixed) bit = 2;
                else if (token_is(s, a, eq, "step") && fixed) bit = 4;
                else if (token_is(s, a, eq, "span")) bit = 8;
                else return TT_ERR_DECL;
                if (seen & bit) return TT_ERR_DECL;
                seen |= bit;
                if (bit == 1) {
                    if (q == eq + 1) return TT_ERR_DECL;
                    if (q - eq - 1 > MAX_NAME) return TT_ERR_NAME;
                    L.name = eq + 1;
                    L.nlen = (uint32_t)(q - eq - 1);
                    for (uint64_t i = eq + 1; i < q; i++) L.hash = hash_step(L.hash, s.at(i));
                } else {
                    uint32_t x;
                    if (!parse_u32(s, eq + 1, q, x) || x == 0) return TT_ERR_COORD;
                    if (bit == 2) L.b = x;
                    else if (bit == 4) L.e = x;
                    else L.span = x;
                }
            }
            if (!(seen & 1) || (fixed && (seen & 6) != 6)) return TT_ERR_DECL;
            return TT_OK;
        }
        L.type = L_DATA;
        if (n == 2) {
            uint32_t pos;
            if (!parse_u32(s, a0, b0, pos) || pos == 0) return TT_ERR_COORD;
            L.b = pos;
        } else if (n != 1) {
            return TT_ERR_FIELDS;
        }
        L.voff = la;
        L.vlen = (uint32_t)(lb - la);
        if (!parse_value(s, la, lb, L.v, L.slow)) return TT_ERR_VALUE;
        return TT_OK;
    }
    L.type = L_DATA;
    if (kind == KIND_BEDGRAPH ? n != 4 : n < 3) return TT_ERR_FIELDS;
    if (b0 - a0 > MAX_NAME) return TT_ERR_NAME;
    L.name = a0;
    L.nlen = (uint32_t)(b0 - a0);
    for (uint64_t i = a0; i < b0; i++) L.hash = hash_step(L.hash, s.at(i));
    if (!parse_u32(s, a1, b1, L.b) || !parse_u32(s, a2, b2, L.e)) return TT_ERR_COORD;
    if (L.e <= L.b) return TT_ERR_RANGE;
    if (kind == KIND_BEDGRAPH) {
        L.voff = la;
        L.vlen = (uint32_t)(lb - la);
        if (!parse_value(s, la, lb, L.v, L.slow)) return TT_ERR_VALUE;
    } else {
        L.v = 1.0f;
    }
    return TT_OK;
}

// The interval of a WIG data line: a "pos value" line (pos in L.b) of a variableStep block, or line k (from 0) of a fixedStep
// block.  decl: L_VAR / L_FIXED; start, step, span from the declaration.
PMX_TT_HD uint32_t wig_interval(uint32_t decl, uint32_t nfields, uint32_t pos, uint32_t start, uint32_t step, uint32_t span, uint64_t k,
                                uint32_t &b, uint32_t &e)
{
    if (decl == L_VAR ? nfields != 2 : nfields != 1) return TT_ERR_BLOCK;
    const uint64_t b64 = decl == L_VAR ? (uint64_t)pos - 1u : (uint64_t)start - 1u + k * (uint64_t)step;
    const uint64_t e64 = b64 + span;
    if (k > 0xffffffffull || e64 > 0xffffffffull) return TT_ERR_COORD;
    b = (uint32_t)b64;
    e = (uint32_t)e64;
    return TT_OK;
}

}  // namespace ttrack

#include <cctype>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <zlib.h>

namespace ttrack {

// ---- host only: compression, the kind of track, the slow values -------------------------------------------------------

enum { COMP_PLAIN = 0, COMP_BGZF = 1, COMP_GZIP = 2 };

// From the first bytes: BGZF (gzip with the BC extra subfield, SAM spec 4.1), other gzip, or plain text
inline int detect_compression(const uint8_t *p, uint64_t n)
{
    if (n < 2 || p[0] != 0x1f || p[1] != 0x8b) return COMP_PLAIN;
    if (n >= 18 && p[2] == 8 && (p[3] & 4) && p[10] + 256u * p[11] >= 6u && p[12] == 'B' && p[13] == 'C' && p[14] == 2 && p[15] == 0)
        return COMP_BGZF;
    return COMP_GZIP;
}

inline uint64_t count_lines(const std::vector<uint8_t> &t)
{
    uint64_t n = 0;
    for (uint8_t c : t) n += c == '\n';
    return n;
}

// Every gzip member of p[0, n) (BGZF or plain, one or several concatenated) inflated with zlib into out.  false with err set
// ("line N: truncated gzip stream" / "line N: corrupt gzip stream": N = the line the text breaks off in).
inline bool inflate_gzip(const uint8_t *p, uint64_t n, std::vector<uint8_t> &out, std::string &err)
{
    out.clear();
    z_stream z;
    memset(&z, 0, sizeof z);
    if (inflateInit2(&z, 15 + 16) != Z_OK) {
        err = "zlib inflateInit2 failed";
        return false;
    }
    std::vector<uint8_t> buf(1u << 20);
    uint64_t off = 0;
    bool in_member = false;
    const char *why = nullptr;
    for (;;) {
        if (z.avail_in == 0) {
            if (off >= n) break;
            const uint64_t c = n - off < (1ull << 30) ? n - off : (1ull << 30);
            z.next_in = const_cast<Bytef *>(p + off);
            z.avail_in = (uInt)c;
            off += c;
        }
        z.next_out = buf.data();
        z.avail_out = (uInt)buf.size();
        const int rc = inflate(&z, Z_NO_FLUSH);
        out.insert(out.end(), buf.data(), buf.data() + (buf.size() - z.avail_out));
        if (rc == Z_STREAM_END) {             // a member ends; another may follow
            in_member = false;
            inflateReset(&z);
        } else if (rc == Z_OK || rc == Z_BUF_ERROR) {
            in_member = true;
        } else {
            why = "corrupt gzip stream";
            break;
        }
    }
    inflateEnd(&z);
    if (!why && in_member) why = "truncated gzip stream";
    if (why) {
        err = "line " + std::to_string(count_lines(out) + 1) + ": " + why;
        return false;
    }
    return true;
}

inline bool iends_with(const std::string &s, const char *suf)
{
    const size_t k = strlen(suf);
    if (s.size() < k) return false;
    for (size_t i = 0; i < k; i++)
        if (tolower((unsigned char)s[s.size() - k + i]) != suf[i]) return false;
    return true;
}

// The kind of a text track from its first lines (t[0, n); complete: the whole text) and its path.  Returns 0 when decided, 1
// when the lines that decide run past n (give more text).
struct PtrSrc {
    const uint8_t *t;
    uint8_t at(uint64_t i) const { return t[i]; }
};

inline int detect_kind(const uint8_t *t, uint64_t n, bool complete, const std::string &path, uint32_t &kind)
{
    std::string name = path;
    if (iends_with(name, ".gz")) name.resize(name.size() - 3);
    else if (iends_with(name, ".bgz")) name.resize(name.size() - 4);
    // (ENCODE's peak formats are BED6+4 / BED6+3 / BED12+3: read as BED, by their first three columns)
    const bool bed = iends_with(name, ".bed") || iends_with(name, ".narrowpeak") || iends_with(name, ".broadpeak") || iends_with(name, ".gappedpeak");
    const uint32_t by_name = bed ? KIND_BED : KIND_BEDGRAPH;
    PtrSrc s{t};
    uint64_t p = 0;
    while (p < n) {
        uint64_t e = p;
        while (e < n && t[e] != '\n') e++;
        if (e == n && !complete) return 1;
        Line L;
        (void)parse_line(s, p, e, KIND_WIG, L);
        if (L.type == L_TRACK) {
            uint64_t q = p;
            while (q < e) {                       // type=... among the track line's fields
                while (q < e && is_ws(t[q])) q++;
                const uint64_t a = q;
                while (q < e && !is_ws(t[q])) q++;
                uint64_t b = q;
                if (b > a && t[b - 1] == '\r') b--;
                if (token_is(s, a, b, "type=bedGraph")) return kind = KIND_BEDGRAPH, 0;
                if (token_is(s, a, b, "type=wiggle_0")) return kind = KIND_WIG, 0;
            }
        } else if (L.type != L_SKIP) {
            kind = (L.type == L_VAR || L.type == L_FIXED) ? KIND_WIG : by_name;
            return 0;
        }
        p = e + 1;
    }
    if (!complete) return 1;
    kind = by_name;
    return 0;
}

// (float)strtod of a value token the fast path left alone (the syntax is already checked)
inline float slow_value(const char *p, size_t n)
{
    std::string tok(p, n);
    return (float)strtod(tok.c_str(), nullptr);
}

inline std::string line_error(uint64_t line0, uint32_t code)
{
    return "line " + std::to_string(line0 + 1) + ": " + err_text(code);
}

}  // namespace ttrack
#endif
