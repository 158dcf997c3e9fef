// The exact k-mer uniqueness track of a genome FASTA on host threads (include/pymasc_amd_io.h, pmx_kmer_open).
// The host twin of the device generator (ingest/kmer_track_device.inc) and its checker, by another method: no hashing.
//
//   file (mmap; gzip / BGZF: every member inflated with zlib) --the rules of io/fasta_parse.h, one line at a time--> the
//   packed genome (2 bits and a valid bit per position, a separator in front of every record) --> every position whose k-mer
//   exists and is no palindrome, with the strand of its canonical k-mer --> the positions sorted on nthreads threads by the
//   canonical packed k-mer, compared word by word --> the groups of size one are the unique positions --> per record, its runs
//   of unique positions as [p, q) with value 1.0 (track.h's StoredTrack without a value vector)
#include "../../../include/pymasc_amd_io.h"
#include "fasta_parse.h"
#include "io_common.h"
#include "text_track_parse.h"
#include "track.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <unordered_set>
#include <vector>

namespace {

struct Genome {
    std::vector<uint64_t> P;                 // 2 bits per position
    std::vector<uint32_t> V;                 // 1 valid bit per position
    std::vector<uint64_t> start;             // the position of each record's first base
    uint64_t npos = 0;
};

void put(Genome &g, uint64_t q, uint32_t code)
{
    if ((q >> 5) + 2 >= g.V.size()) {
        const size_t n = std::max<size_t>(1024, 2 * g.V.size());
        g.P.resize(n, 0);
        g.V.resize(n, 0);
    }
    if (code < 4u) {
        g.P[q >> 5] |= (uint64_t)code << (2u * (q & 31u));
        g.V[q >> 5] |= 1u << (q & 31u);
    }
}

void parse_fasta(pmx_io::StoredTrack &t, Genome &g, const uint8_t *text, uint64_t N)
{
    using namespace fasta;
    ttrack::PtrSrc s{text};
    std::unordered_set<std::string> seen;
    uint64_t err = ~0ull;                    // line << 8 | code, the smallest
    auto flag = [&](uint64_t line, uint32_t code) { err = std::min<uint64_t>(err, line << 8 | code); };
    uint64_t q = 0, bases = 0, head_line = 0, rec_bases = 0;
    bool in_rec = false;
    auto close_rec = [&]() {
        if (in_rec) {
            if (rec_bases == 0) flag(head_line, FA_ERR_EMPTY);
            t.sizes.push_back((int64_t)rec_bases);
        }
    };
    uint64_t line = 0;
    for (uint64_t p = 0; p < N; line++) {
        const uint8_t *nl = (const uint8_t *)memchr(text + p, '\n', (size_t)(N - p));
        const uint64_t end = nl ? (uint64_t)(nl - text) : N;
        uint32_t type = 0;
        uint64_t body = 0, name_end = 0;
        const uint32_t e = classify(s, p, end, type, body, name_end);
        if (e) flag(line, e);
        if (type == L_HEADER) {
            close_rec();
            std::string name((const char *)text + p + 1, (size_t)(name_end - p - 1));
            if (!e && !seen.insert(name).second) flag(line, FA_ERR_DUP);
            t.names.push_back(name);
            in_rec = true;
            head_line = line;
            rec_bases = 0;
            put(g, q++, 4);                   // the record's separator
            g.start.push_back(q);
        } else if (type == L_SEQ) {
            if (!in_rec) {
                flag(line, FA_ERR_BEFORE);
            } else if (err == ~0ull) {        // (after an error the genome is not needed: only earlier errors can win)
                for (uint64_t i = p; i < body; i++) {
                    const uint8_t c = text[i];
                    if (!is_letter(c)) {
                        flag(line, FA_ERR_BYTE);
                        break;
                    }
                    put(g, q++, base_code(c));
                }
            } else {
                for (uint64_t i = p; i < body; i++)
                    if (!is_letter(text[i])) {
                        flag(line, FA_ERR_BYTE);
                        break;
                    }
            }
            rec_bases += body - p;
            bases += body - p;
        }
        p = end + 1;
    }
    close_rec();
    if (err != ~0ull) throw pmx_io::Error(PMX_IO_ERR_FORMAT, line_error(err >> 8, (uint32_t)(err & 255u)));
    if (t.names.empty()) throw pmx_io::Error(PMX_IO_ERR_FORMAT, no_record_text());
    if (too_large(bases, t.names.size())) throw pmx_io::Error(PMX_IO_ERR_FORMAT, too_large_text());
    put(g, q++, 4);                           // the closing separator
    g.npos = q;
    const size_t words = (size_t)((q >> 5) + 3);
    g.P.resize(words, 0);
    g.V.resize(words, 0);
}

void generate(pmx_io::StoredTrack &t, const Genome &g, uint32_t k, int nthreads)
{
    using namespace fasta;
    const uint64_t npos = g.npos;
    const uint32_t nw = (k + 31u) / 32u;
    const uint64_t *P = g.P.data();
    // the positions with a k-mer that is no palindrome, and the strand of their canonical k-mer
    std::vector<uint64_t> rev((npos + 63) / 64, 0);
    const size_t grain = 1u << 20;
    const size_t nchunks = (size_t)((npos + grain - 1) / grain);
    std::vector<std::vector<uint32_t>> part(nchunks);
    pmx_io::parallel_for(nthreads, (size_t)npos, grain, [&](size_t lo, size_t hi, size_t c) {
        std::vector<uint32_t> &v = part[c];
        for (size_t q = lo; q < hi; q++) {
            if (!window_valid(g.V.data(), q, k, npos)) continue;
            const int o = strand_order(P, q, k);
            if (o == 0) continue;
            v.push_back((uint32_t)q);
            if (o > 0) __atomic_fetch_or(&rev[q >> 6], 1ull << (q & 63u), __ATOMIC_RELAXED);
        }
    });
    std::vector<uint32_t> pos;
    for (auto &v : part) {
        pos.insert(pos.end(), v.begin(), v.end());
        std::vector<uint32_t>().swap(v);
    }
    auto is_rev = [&](uint32_t q) { return (rev[q >> 6] >> (q & 63u)) & 1u; };
    auto cmp3 = [&](uint32_t a, uint32_t b) -> int {
        const bool ra = is_rev(a), rb = is_rev(b);
        for (uint32_t i = 0; i < nw; i++) {
            const uint64_t x = canon_word(P, a, k, i, ra), y = canon_word(P, b, k, i, rb);
            if (x != y) return x < y ? -1 : 1;
        }
        return 0;
    };
    auto less = [&](uint32_t a, uint32_t b) { return cmp3(a, b) < 0; };
    // sorted in pieces on the threads, then merged pairwise
    const size_t n = pos.size();
    const size_t pieces = std::max<size_t>(1, std::min<size_t>((size_t)nthreads, n / 4096 + 1));
    std::vector<size_t> cut(pieces + 1);
    for (size_t i = 0; i <= pieces; i++) cut[i] = n * i / pieces;
    pmx_io::parallel_for((int)pieces, pieces, 1, [&](size_t lo, size_t, size_t) { std::sort(pos.begin() + cut[lo], pos.begin() + cut[lo + 1], less); });
    for (size_t width = 1; width < pieces; width *= 2) {
        const size_t pairs = (pieces + 2 * width - 1) / (2 * width);
        pmx_io::parallel_for(nthreads, pairs, 1, [&](size_t lo, size_t, size_t) {
            const size_t a = 2 * width * lo, m = std::min(pieces, a + width), e = std::min(pieces, a + 2 * width);
            if (m < e) std::inplace_merge(pos.begin() + cut[a], pos.begin() + cut[m], pos.begin() + cut[e], less);
        });
    }
    // groups of one: unique
    std::vector<uint64_t> uniq((npos + 63) / 64, 0);
    for (size_t i = 0; i < n;) {
        size_t j = i + 1;
        while (j < n && cmp3(pos[i], pos[j]) == 0) j++;
        if (j == i + 1) uniq[pos[i] >> 6] |= 1ull << (pos[i] & 63u);
        i = j;
    }
    std::vector<uint32_t>().swap(pos);
    // per record: the runs of unique positions
    t.b.resize(t.names.size());
    t.e.resize(t.names.size());
    for (size_t r = 0; r < t.names.size(); r++) {
        const uint64_t s = g.start[r], len = (uint64_t)t.sizes[r];
        uint64_t p = 0;
        while (p < len) {
            const uint64_t q = s + p;
            if (!((uniq[q >> 6] >> (q & 63u)) & 1u)) {
                p++;
                continue;
            }
            uint64_t e = p;
            while (e < len && ((uniq[(s + e) >> 6] >> ((s + e) & 63u)) & 1u)) e++;
            t.b[r].push_back((uint32_t)p);
            t.e[r].push_back((uint32_t)e);
            p = e;
        }
    }
}

}  // namespace

extern "C" {

int pmx_kmer_open(const char *path, int32_t k, int nthreads, pmx_track **out)
{
    if (path && out && (k < (int32_t)fasta::K_MIN || k > (int32_t)fasta::K_MAX)) {
        *out = nullptr;
        return pmx_io::fail(PMX_IO_ERR_INVALID, fasta::bad_k_text(k));
    }
    return pmx_io::open_track("pmx_kmer_open", path, out, [&]() {
        std::unique_ptr<pmx_io::StoredTrack> t(new pmx_io::StoredTrack);
        t->kind = 2;
        Genome g;
        {
            pmx_io::MappedFile f;
            f.open(path);
            if (ttrack::detect_compression(f.data, f.size) == ttrack::COMP_PLAIN) {
                parse_fasta(*t, g, f.data, f.size);
            } else {
                std::vector<uint8_t> text;
                std::string err;
                if (!ttrack::inflate_gzip(f.data, f.size, text, err)) throw pmx_io::Error(PMX_IO_ERR_FORMAT, err);
                f.close();
                parse_fasta(*t, g, text.data(), text.size());
            }
        }
        generate(*t, g, (uint32_t)k, pmx_io::pick_threads(nthreads));
        return t;
    });
}

}  // extern "C"
