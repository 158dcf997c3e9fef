// Genome FASTA -> the exact k-mer uniqueness track.  Shared by the host generator (io/kmer_track.cpp,
// libpymasc_io.so, the checker) and the device generator (ingest/kmer_track_device.inc, libpymasc_ingest.so): one set of line
// rules, one packed layout of the genome, one k-mer order and one set of error texts.
//
//   lines       '\n'-terminated (the last one may lack it); a trailing '\r' is dropped; blank lines are ignored
//   header      ">name ...": the name runs to the first space or tab; the records keep the file order
//   sequence    ASCII letters only; uppercased, A C G T are bases and every other letter (N, IUPAC codes, X) is masked
//   errors      "line N: <reason>" (N 1-based in the decompressed text), the first by line (then by code): a non-blank line
//               before the first header, an empty name, a duplicate name, a record with no bases (at its header), a byte of a
//               sequence line that is not an ASCII letter
//   the rule    a k-mer at 0-based position p of record c exists when p + k <= len(c) and its k bases are valid; (c, p) is
//               uniquely mappable when F != revcomp(F) and no other existing position has F or revcomp(F) as its k-mer
//
// Positions: the records are laid end to end, each behind one masked separator position, and one more separator closes the
// genome: the base p of record r is at r + 1 + (bases of the records before r) + p, so no window of valid bases crosses a
// record.  Packed: 2 bits per base (A C G T = 0 1 2 3), 32 positions per u64 word, position q at bits 2 (q % 32); valid: one bit
// per position, 32 per u32 word.  Both arrays hold two words more than the positions need (loads stay inside them).
#ifndef PMX_FASTA_PARSE_H
#define PMX_FASTA_PARSE_H

#include <cstdint>
#include <string>

#if defined(__HIPCC__)
#define PMX_FA_HD __host__ __device__ __forceinline__
#else
#define PMX_FA_HD inline
#endif

namespace fasta {

enum { L_BLANK = 0, L_HEADER = 1, L_SEQ = 2 };

enum {
    FA_OK = 0,
    FA_ERR_BEFORE = 1,      // a non-blank line before the first header
    FA_ERR_NONAME = 2,      // a header with an empty name
    FA_ERR_DUP = 3,         // a name seen before
    FA_ERR_EMPTY = 4,       // a record with no bases (reported at its header)
    FA_ERR_BYTE = 5,        // a sequence byte that is not an ASCII letter
};

constexpr uint32_t K_MIN = 16, K_MAX = 1024;

inline const char *err_text(uint32_t code)
{
    switch (code) {
    case FA_ERR_BEFORE: return "sequence before the first header";
    case FA_ERR_NONAME: return "empty sequence name";
    case FA_ERR_DUP: return "duplicate sequence name";
    case FA_ERR_EMPTY: return "record with no bases";
    case FA_ERR_BYTE: return "sequence byte that is not a letter";
    default: return "malformed FASTA";
    }
}

inline std::string line_error(uint64_t line0, uint32_t code)
{
    return "line " + std::to_string(line0 + 1) + ": " + err_text(code);
}

inline const char *too_large_text() { return "the genome has 2^32 or more bases: not supported"; }
inline const char *no_record_text() { return "no FASTA record"; }
inline std::string bad_k_text(long long k)
{
    return "k = " + std::to_string(k) + ": the k-mer length must lie in [" + std::to_string(K_MIN) + ", " + std::to_string(K_MAX) + "]";
}

// Genomes whose positions (bases + one separator per record + the closing one) do not fit in u32
PMX_FA_HD bool too_large(uint64_t bases, uint64_t records) { return bases >= (1ull << 32) || bases + records + 1 >= 0xffffffffull - 64; }

PMX_FA_HD bool is_letter(uint8_t c) { return (uint8_t)((c | 0x20u) - 'a') < 26u; }

// 0..3 for A C G T (any case), 4 for every other letter
PMX_FA_HD uint32_t base_code(uint8_t c)
{
    switch (c | 0x20u) {
    case 'a': return 0;
    case 'c': return 1;
    case 'g': return 2;
    case 't': return 3;
    default: return 4;
    }
}

// One line [p, e) ('\n' excluded) of a text read through s.at(i): its type, the end of its body ('\r' dropped) and, for a
// header, the end of its name.  The only error found here is an empty name; the letters are checked where they are packed.
template <class S>
PMX_FA_HD uint32_t classify(S &s, uint64_t p, uint64_t e, uint32_t &type, uint64_t &body_end, uint64_t &name_end)
{
    if (e > p && s.at(e - 1) == '\r') e--;
    body_end = name_end = e;
    if (e == p) {
        type = L_BLANK;
        return FA_OK;
    }
    if (s.at(p) != '>') {
        type = L_SEQ;
        return FA_OK;
    }
    type = L_HEADER;
    uint64_t q = p + 1;
    while (q < e) {
        const uint8_t c = s.at(q);
        if (c == ' ' || c == '\t') break;
        q++;
    }
    name_end = q;
    return q == p + 1 ? FA_ERR_NONAME : FA_OK;
}

// n <= 32 bases from position q: base q + j at bits 2j
PMX_FA_HD uint64_t get_bases(const uint64_t *P, uint64_t q, uint32_t n)
{
    const uint64_t w = q >> 5;
    const uint32_t s = (uint32_t)(q & 31u);
    uint64_t x = P[w] >> (2u * s);
    if (s) x |= P[w + 1] << (64u - 2u * s);
    return n >= 32u ? x : (x & ((1ull << (2u * n)) - 1ull));
}

// the reverse complement of the n bases of x (base j at bits 2j)
PMX_FA_HD uint64_t revcomp(uint64_t x, uint32_t n)
{
    x = ~x;                                                                   // complement: 3 - c
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    x = (x >> 32) | (x << 32);
    return n >= 32u ? x : (x >> (64u - 2u * n));
}

// Word i (< (k + 31) / 32) of the k-mer at q: bases [32 i, 32 i + 32) of F (rev false) or of R = revcomp(F) (rev true)
PMX_FA_HD uint64_t kmer_word(const uint64_t *P, uint64_t q, uint32_t k, uint32_t i, bool rev)
{
    const uint32_t n = k - 32u * i < 32u ? k - 32u * i : 32u;
    if (!rev) return get_bases(P, q + 32ull * i, n);
    return revcomp(get_bases(P, q + (k - 32u * i - n), n), n);
}

// every position of [q, q + k) is valid (q + k <= npos)
PMX_FA_HD bool window_valid(const uint32_t *V, uint64_t q, uint32_t k, uint64_t npos)
{
    if (q + k > npos) return false;
    uint64_t a = q;
    const uint64_t e = q + k;
    while (a < e) {
        const uint32_t s = (uint32_t)(a & 31u), n = (uint32_t)((e - a) < (uint64_t)(32u - s) ? (e - a) : (uint64_t)(32u - s));
        const uint32_t m = n == 32u ? 0xffffffffu : (((1u << n) - 1u) << s);
        if ((V[a >> 5] & m) != m) return false;
        a += n;
    }
    return true;
}

// -1 / 0 / 1: F against R of the k-mer at q, word by word (0: a palindrome)
PMX_FA_HD int strand_order(const uint64_t *P, uint64_t q, uint32_t k)
{
    const uint32_t nw = (k + 31u) / 32u;
    for (uint32_t i = 0; i < nw; i++) {
        const uint64_t f = kmer_word(P, q, k, i, false), r = kmer_word(P, q, k, i, true);
        if (f != r) return f < r ? -1 : 1;
    }
    return 0;
}

// The canonical k-mer (the smaller of F and R, word by word) of q: word i
PMX_FA_HD uint64_t canon_word(const uint64_t *P, uint64_t q, uint32_t k, uint32_t i, bool rev) { return kmer_word(P, q, k, i, rev); }

// The same k-mer, in either orientation, at a and b
PMX_FA_HD bool same_kmer(const uint64_t *P, uint64_t a, uint64_t b, uint32_t k)
{
    const uint32_t nw = (k + 31u) / 32u;
    bool fw = true, rc = true;
    for (uint32_t i = 0; i < nw && (fw || rc); i++) {
        const uint64_t x = kmer_word(P, a, k, i, false);
        fw = fw && x == kmer_word(P, b, k, i, false);
        rc = rc && x == kmer_word(P, b, k, i, true);
    }
    return fw || rc;
}

PMX_FA_HD uint64_t mix64(uint64_t x)
{
    x ^= x >> 30;
    x *= 0xbf58476d1ce4e5b9ull;
    x ^= x >> 27;
    x *= 0x94d049bb133111ebull;
    x ^= x >> 31;
    return x;
}

}  // namespace fasta
#endif
