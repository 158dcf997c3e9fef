// SAM text (plain, or BGZF-compressed as bgzip writes it) -> the arrays the BAM reader yields (include/pymasc_amd_io.h,
// pmx_sam_*).  The host twin of the device reader (ingest/sam_device.inc) and its checker: the same rules (io/sam_parse.h),
// the same records, read-length histogram and counters; the first-occurrence key of a length is its line's byte offset in the
// text.  The whole text is indexed and parsed at open, on the reader's threads:
//
//   file (mmap; BGZF: every member inflated on the threads) --header on this thread--> line starts (memchr, one part of the
//   text per thread) --parse (one chunk of lines per task)--> per-record table (ref, pos1, qlen, flag | mapq << 16)
//   --pmx_sam_decode: filter + compaction--> the kept arrays, copied out by pmx_sam_fetch
#include "../../../include/pymasc_amd_io.h"
#include "bed_reads_parse.h"
#include "io_common.h"
#include "sam_parse.h"
#include "text_track_parse.h"

#include <algorithm>
#include <cstring>
#include <numeric>
#include <string>
#include <unordered_map>
#include <vector>

struct pmx_sam {
    pmx_io::MappedFile file;
    std::vector<uint8_t> inflated;  // the text of a BGZF file
    const uint8_t *t = nullptr;     // the text
    uint64_t N = 0, members = 0;
    int nthreads = 1;
    bool header_only = false;       // pmx_sam_open_header: no record was read
    samtext::Header h;
    std::vector<uint64_t> nl;       // end ('\n' or the end of the text) of every record line
    std::vector<uint64_t> ls;       // a BED read file put in order (pmx_bed_open): the start of each record's line
    uint64_t nrec = 0;
    std::vector<int32_t> ref, pos;
    std::vector<uint32_t> qlen, fm;  // fm = flag | mapq << 16
    std::vector<int32_t> o_ref, o_pos, o_len;
    std::vector<uint8_t> o_rev;
    uint64_t n_kept = 0;
    // pmx_sam_fetch_mates: the last decode's filter, and the mate columns of its kept records, parsed when first asked for
    uint32_t d_mapq = 0, d_flags = 0;
    int32_t d_want = -1;
    bool bed = false, mates_valid = false;
    std::vector<uint16_t> m_flag;
    std::vector<int32_t> m_ref, m_pos, m_tlen;
    struct LenBin {
        int32_t len;
        uint64_t count, first;
    };
    std::vector<LenBin> rl_hist;
    uint64_t rl_counters[6] = {0, 0, 0, 0, 0, 0};
    bool rl_valid = false;
    uint32_t rl_mapq = 0;

    uint64_t line_start(uint64_t i) const { return !ls.empty() ? ls[i] : i ? nl[i - 1] + 1 : h.data_beg; }
};

namespace {

struct HostSrc {
    const uint8_t *t;
    uint8_t at(uint64_t i) const { return t[i]; }
};

using pmx_io::parallel_for;

// s.nl: the end of every line after the header
void index_lines(pmx_sam &s)
{
    const uint64_t beg = s.h.data_beg, N = s.N;
    // line ends: one part of the text per thread
    const uint64_t T = (uint64_t)std::max(1, s.nthreads), span = N - beg;
    std::vector<std::vector<uint64_t>> parts(T);
    parallel_for((int)T, T, 1, [&](size_t lo, size_t, size_t) {
        const uint64_t a = beg + span * lo / T, b = beg + span * (lo + 1) / T;
        const uint8_t *p = s.t + a, *e = s.t + b;
        while (p < e) {
            const void *q = memchr(p, '\n', (size_t)(e - p));
            if (!q) break;
            parts[lo].push_back((uint64_t)((const uint8_t *)q - s.t));
            p = (const uint8_t *)q + 1;
        }
    });
    size_t total = 0;
    for (auto &v : parts) total += v.size();
    s.nl.reserve(total + 1);
    for (auto &v : parts) s.nl.insert(s.nl.end(), v.begin(), v.end());
    if (N > beg && s.t[N - 1] != '\n') s.nl.push_back(N);    // the last line without its '\n'
}

void index_and_parse(pmx_sam &s)
{
    index_lines(s);
    uint64_t n = s.nl.size();
    if (n) {                                                  // one empty line at the very end is allowed
        const uint64_t a = s.line_start(n - 1);
        uint64_t e = s.nl[n - 1];
        if (e > a && s.t[e - 1] == '\r') e--;
        if (e == a) n--;
    }
    s.nrec = n;
    s.ref.resize(n);
    s.pos.resize(n);
    s.qlen.resize(n);
    s.fm.resize(n);
    const size_t grain = 1 << 16, chunks = (n + grain - 1) / grain;
    std::vector<uint64_t> first_err(chunks, ~0ull);           // line index << 8 | code
    const samtext::Names nm = samtext::names_of(s.h);
    parallel_for(s.nthreads, n, grain, [&](size_t lo, size_t hi, size_t c) {
        HostSrc src{s.t};
        for (size_t i = lo; i < hi; i++) {
            samtext::Rec r;
            const uint32_t e = samtext::parse_line(src, s.line_start(i), s.nl[i], nm, r);
            if (e) {
                first_err[c] = ((uint64_t)i << 8) | e;
                return;
            }
            s.ref[i] = r.ref;
            s.pos[i] = r.pos1;
            s.qlen[i] = r.qlen;
            s.fm[i] = r.flag | (r.mapq << 16);
        }
    });
    const uint64_t fe = chunks ? *std::min_element(first_err.begin(), first_err.end()) : ~0ull;
    if (fe != ~0ull) throw pmx_io::Error(PMX_IO_ERR_FORMAT, samtext::line_error(s.h, fe >> 8, (uint32_t)(fe & 255u)));
}

// the filter of pmx_bam_next_batch (pymasc_amd_io.h) on record i
inline bool keep(const pmx_sam &s, size_t i, uint32_t mapq_min, uint32_t flag_exclude, int32_t want_ref)
{
    const uint32_t flag = s.fm[i] & 0xffffu, mapq = s.fm[i] >> 16;
    return !(flag & flag_exclude) && mapq >= mapq_min && s.ref[i] >= 0 && (want_ref < 0 || s.ref[i] == want_ref) && s.qlen[i] != 0;
}

// A BED read file (pmx_bed_open): every line parsed by io/bed_reads_parse.h, the track-line rules, then the table put in
// (reference, start) order by std::stable_sort when the file is not in that order already; lines without a read sort last and
// are dropped
void bed_parse_sort(pmx_sam &s)
{
    index_lines(s);
    const uint64_t n = s.nl.size();
    if (n >= 0xffffffffull) throw pmx_io::Error(PMX_IO_ERR_FORMAT, "more than 2^32 - 2 lines");
    const uint32_t nref = (uint32_t)s.h.names.size();
    s.ref.resize(n);
    s.pos.resize(n);
    s.qlen.resize(n);
    s.fm.resize(n);
    std::vector<uint64_t> key(n);
    const size_t grain = 1 << 16, chunks = (n + grain - 1) / grain;
    std::vector<uint64_t> first_err(chunks, ~0ull), first_read(chunks, ~0ull), unsorted(chunks, 0);
    std::vector<std::vector<uint64_t>> tracks(chunks);
    const samtext::Names nm = samtext::names_of(s.h);
    parallel_for(s.nthreads, n, grain, [&](size_t lo, size_t hi, size_t c) {
        HostSrc src{s.t};
        for (size_t i = lo; i < hi; i++) {
            samtext::Rec r;
            r.ref = -1;
            r.pos1 = 0;
            r.qlen = r.flag = r.mapq = 0;
            uint32_t type;
            const uint32_t e = bedreads::parse_line(src, s.line_start(i), s.nl[i], nm, type, r);
            if (type == bedreads::L_READ && first_read[c] == ~0ull) first_read[c] = i;
            if (type == bedreads::L_TRACK) tracks[c].push_back(i);
            if (e) {
                first_err[c] = ((uint64_t)i << 8) | e;
                return;
            }
            s.ref[i] = r.ref;
            s.pos[i] = r.pos1;
            s.qlen[i] = r.qlen;
            s.fm[i] = r.flag | (r.mapq << 16);
            key[i] = bedreads::sort_key(r.ref, r.pos1, nref);
            if (i > lo && key[i] < key[i - 1]) unsorted[c] = 1;
        }
    });
    uint64_t fe = chunks ? *std::min_element(first_err.begin(), first_err.end()) : ~0ull;
    const uint64_t fr = chunks ? *std::min_element(first_read.begin(), first_read.end()) : ~0ull;
    std::vector<uint64_t> tr;
    for (const auto &v : tracks) tr.insert(tr.end(), v.begin(), v.end());
    uint64_t tline = 0;
    if (const uint32_t tc = bedreads::track_error(tr, fr, tline))
        if ((tline << 8 | tc) < fe) fe = tline << 8 | tc;
    if (fe != ~0ull) throw pmx_io::Error(PMX_IO_ERR_FORMAT, bedreads::line_error(fe >> 8, (uint32_t)(fe & 255u)));
    bool sorted = true;
    for (size_t c = 0; c < chunks && sorted; c++)
        sorted = !unsorted[c] && (c == 0 || key[c * grain] >= key[c * grain - 1]);
    const uint64_t none = (uint64_t)nref << 31;
    uint64_t reads = 0;
    for (uint64_t k : key) reads += k < none;
    if (!sorted) {
        std::vector<std::pair<uint64_t, uint32_t>> kv(n);
        for (uint64_t i = 0; i < n; i++) kv[i] = {key[i], (uint32_t)i};
        std::stable_sort(kv.begin(), kv.end(), [](const std::pair<uint64_t, uint32_t> &x, const std::pair<uint64_t, uint32_t> &y) {
            return x.first < y.first;
        });
        std::vector<int32_t> ref(reads), pos(reads);
        std::vector<uint32_t> qlen(reads), fm(reads);
        std::vector<uint64_t> ls(reads);
        parallel_for(s.nthreads, reads, grain, [&](size_t lo, size_t hi, size_t) {
            for (size_t i = lo; i < hi; i++) {
                const uint32_t j = kv[i].second;
                ref[i] = s.ref[j];
                pos[i] = s.pos[j];
                qlen[i] = s.qlen[j];
                fm[i] = s.fm[j];
                ls[i] = s.line_start(j);
            }
        });
        s.ref.swap(ref);
        s.pos.swap(pos);
        s.qlen.swap(qlen);
        s.fm.swap(fm);
        s.ls.swap(ls);
    }
    s.nrec = reads;                 // (in order, the lines without a read are behind the reads)
}

}  // namespace

extern "C" {

int pmx_bed_open(const char *path, int nthreads, int32_t nref, const char *const *names, const int64_t *lengths, pmx_sam **out)
{
    if (!path || !out) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_bed_open: NULL argument");
    *out = nullptr;
    pmx_sam *s = new pmx_sam();
    s->bed = true;
    try {
        const std::string why = bedreads::check_sizes(nref, names, lengths, s->h.names, s->h.lens);
        if (!why.empty()) throw pmx_io::Error(PMX_IO_ERR_INVALID, why);
        bedreads::name_table(s->h.names, s->h.bytes, s->h.off, s->h.slot);
        s->file.open(path);
        s->nthreads = pmx_io::pick_threads(nthreads);
        const uint8_t *d = s->file.data;
        const size_t n = s->file.size;
        const int comp = ttrack::detect_compression(d, n);
        if (comp == ttrack::COMP_PLAIN) {
            s->t = d;
            s->N = n;
        } else {
            bool ok = false;
            if (comp == ttrack::COMP_BGZF) {
                try {
                    pmx_io::bgzf_inflate_all(d, n, s->nthreads, s->inflated, s->members);
                    ok = true;
                } catch (const pmx_io::Error &) {   // the words of the gzip path below: where the text breaks off
                }
                s->members = 0;                     // (as the device reader counts: 0 for every BED file)
            }
            std::string err;
            if (!ok && !ttrack::inflate_gzip(d, n, s->inflated, err)) throw pmx_io::Error(PMX_IO_ERR_FORMAT, err);
            s->t = s->inflated.data();
            s->N = s->inflated.size();
        }
        bed_parse_sort(*s);
    } catch (const pmx_io::Error &e) {
        delete s;
        return pmx_io::fail(e.code, std::string(path) + ": " + e.msg);
    } catch (const std::exception &e) {
        delete s;
        return pmx_io::fail(PMX_IO_ERR_OPEN, std::string(path) + ": " + e.what());
    }
    *out = s;
    return PMX_IO_OK;
}

int pmx_sam_open(const char *path, int nthreads, pmx_sam **out)
{
    if (!path || !out) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_open: NULL argument");
    *out = nullptr;
    pmx_sam *s = new pmx_sam();
    try {
        s->file.open(path);
        s->nthreads = pmx_io::pick_threads(nthreads);
        const uint8_t *d = s->file.data;
        const size_t n = s->file.size;
        if (n >= 2 && d[0] == 0x1f && d[1] == 0x8b) {
            if (n < 4 || d[2] != 8 || !(d[3] & 4))
                throw pmx_io::Error(PMX_IO_ERR_FORMAT, "gzip-compressed SAM that is not BGZF: recompress it with bgzip");
            pmx_io::bgzf_inflate_all(d, n, s->nthreads, s->inflated, s->members);
            s->t = s->inflated.data();
            s->N = s->inflated.size();
        } else {
            s->t = d;
            s->N = n;
        }
        std::string err;
        if (samtext::parse_header((const char *)s->t, s->N, true, s->h, err) != 0) throw pmx_io::Error(PMX_IO_ERR_FORMAT, err);
        index_and_parse(*s);
    } catch (const pmx_io::Error &e) {
        delete s;
        return pmx_io::fail(e.code, std::string(path) + ": " + e.msg);
    } catch (const std::exception &e) {
        delete s;
        return pmx_io::fail(PMX_IO_ERR_OPEN, std::string(path) + ": " + e.what());
    }
    *out = s;
    return PMX_IO_OK;
}

int pmx_sam_open_header(const char *path, pmx_sam **out)
{
    if (!path || !out) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_open_header: NULL argument");
    *out = nullptr;
    pmx_sam *s = new pmx_sam();
    s->header_only = true;
    try {
        s->file.open(path);
        const uint8_t *d = s->file.data;
        const size_t n = s->file.size;
        std::string err;
        int rc;
        if (n >= 2 && d[0] == 0x1f && d[1] == 0x8b) {
            if (n < 4 || d[2] != 8 || !(d[3] & 4))
                throw pmx_io::Error(PMX_IO_ERR_FORMAT, "gzip-compressed SAM that is not BGZF: recompress it with bgzip");
            // members inflated in order until the text holds the first record line (or the file ends), as pmx_dsam_open
            // reads its header from a growing prefix
            size_t off = 0;
            for (size_t want = (size_t)1 << 20;; want *= 2) {
                off = pmx_io::bgzf_inflate_prefix(d, n, off, want, s->inflated);
                rc = samtext::parse_header((const char *)s->inflated.data(), s->inflated.size(), off == n, s->h, err);
                if (rc != 1) break;
            }
            std::vector<uint8_t>().swap(s->inflated);
        } else {
            rc = samtext::parse_header((const char *)d, n, true, s->h, err);     // reads the '@' lines only
        }
        if (rc != 0) throw pmx_io::Error(PMX_IO_ERR_FORMAT, err);
        s->file.close();
    } catch (const pmx_io::Error &e) {
        delete s;
        return pmx_io::fail(e.code, std::string(path) + ": " + e.msg);
    } catch (const std::exception &e) {
        delete s;
        return pmx_io::fail(PMX_IO_ERR_OPEN, std::string(path) + ": " + e.what());
    }
    *out = s;
    return PMX_IO_OK;
}

void pmx_sam_close(pmx_sam *s) { delete s; }

int32_t pmx_sam_nref(const pmx_sam *s) { return s ? (int32_t)s->h.names.size() : 0; }

const char *pmx_sam_ref_name(const pmx_sam *s, int32_t i)
{
    if (!s || i < 0 || (size_t)i >= s->h.names.size()) return nullptr;
    return s->h.names[(size_t)i].c_str();
}

int64_t pmx_sam_ref_len(const pmx_sam *s, int32_t i)
{
    if (!s || i < 0 || (size_t)i >= s->h.lens.size()) return -1;
    return s->h.lens[(size_t)i];
}

const char *pmx_sam_header_text(const pmx_sam *s, uint32_t *len)
{
    if (!s) return nullptr;
    if (len) *len = (uint32_t)s->h.text.size();
    return s->h.text.c_str();
}

int64_t pmx_sam_decode(pmx_sam *s, uint32_t mapq_min, uint32_t flag_exclude, int32_t want_ref)
{
    if (!s) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_decode: NULL handle");
    if (s->header_only) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_decode: the file was opened for its header only");
    try {
        const size_t n = s->nrec, grain = 1 << 16, chunks = (n + grain - 1) / grain;
        std::vector<uint64_t> base(chunks + 1, 0);
        parallel_for(s->nthreads, n, grain, [&](size_t lo, size_t hi, size_t c) {
            uint64_t k = 0;
            for (size_t i = lo; i < hi; i++) k += keep(*s, i, mapq_min, flag_exclude, want_ref);
            base[c + 1] = k;
        });
        for (size_t c = 0; c < chunks; c++) base[c + 1] += base[c];
        const uint64_t kept = base[chunks];
        s->o_ref.resize(kept);
        s->o_pos.resize(kept);
        s->o_len.resize(kept);
        s->o_rev.resize(kept);
        parallel_for(s->nthreads, n, grain, [&](size_t lo, size_t hi, size_t c) {
            uint64_t o = base[c];
            for (size_t i = lo; i < hi; i++)
                if (keep(*s, i, mapq_min, flag_exclude, want_ref)) {
                    s->o_ref[o] = s->ref[i];
                    s->o_pos[o] = s->pos[i];
                    s->o_len[o] = (int32_t)s->qlen[i];
                    s->o_rev[o] = (s->fm[i] & PMX_BAM_FLAG_REVERSE) ? 1 : 0;
                    o++;
                }
        });
        s->n_kept = kept;
        s->d_mapq = mapq_min;
        s->d_flags = flag_exclude;
        s->d_want = want_ref;
        s->mates_valid = false;
    } catch (const pmx_io::Error &e) {
        return pmx_io::fail(e.code, e.msg);
    } catch (const std::exception &e) {
        return pmx_io::fail(PMX_IO_ERR_OPEN, std::string("pmx_sam_decode: ") + e.what());
    }
    return (int64_t)s->n_kept;
}

int pmx_sam_fetch(pmx_sam *s, int64_t first, int64_t n, int32_t *ref_id, int32_t *pos1, int32_t *read_len, uint8_t *reverse)
{
    if (!s || first < 0 || n < 0 || (uint64_t)(first + n) > s->n_kept)
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_fetch: range outside the kept records");
    if (ref_id) memcpy(ref_id, s->o_ref.data() + first, 4 * (size_t)n);
    if (pos1) memcpy(pos1, s->o_pos.data() + first, 4 * (size_t)n);
    if (read_len) memcpy(read_len, s->o_len.data() + first, 4 * (size_t)n);
    if (reverse) memcpy(reverse, s->o_rev.data() + first, (size_t)n);
    return PMX_IO_OK;
}

// the mate columns of the kept records of the last decode: fields 7-9 by samtext::parse_mates, RNEXT through the @SQ names
static void parse_kept_mates(pmx_sam &s)
{
    const uint64_t kept = s.n_kept;
    s.m_flag.resize(kept);
    s.m_ref.resize(kept);
    s.m_pos.resize(kept);
    s.m_tlen.resize(kept);
    std::unordered_map<std::string, int32_t> ids;
    for (size_t r = 0; r < s.h.names.size(); r++) ids.emplace(s.h.names[r], (int32_t)r);
    HostSrc src{s.t};
    uint64_t o = 0;
    for (size_t i = 0; i < s.nrec; i++) {
        if (!keep(s, i, s.d_mapq, s.d_flags, s.d_want)) continue;
        samtext::Mates m;
        const uint32_t e = samtext::parse_mates(src, s.line_start(i), s.nl[i], m);
        if (e) throw pmx_io::Error(PMX_IO_ERR_FORMAT, samtext::line_error(s.h, i, e));
        int32_t mr = s.ref[i];
        if (!m.same) {
            const auto it = ids.find(std::string((const char *)s.t + m.rnext, (size_t)m.rnext_len));
            mr = it == ids.end() ? -1 : it->second;
        }
        s.m_flag[o] = (uint16_t)(s.fm[i] & 0xffffu);
        s.m_ref[o] = mr;
        s.m_pos[o] = m.mate_pos1;
        s.m_tlen[o] = m.tlen;
        o++;
    }
    s.mates_valid = true;
}

int pmx_sam_fetch_mates(pmx_sam *s, int64_t first, int64_t n, uint16_t *flag, int32_t *mate_ref, int32_t *mate_pos1, int32_t *tlen)
{
    if (!s) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_fetch_mates: NULL handle");
    if (s->bed) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_fetch_mates: the input has no mate fields");
    if (first < 0 || n < 0 || (uint64_t)(first + n) > s->n_kept)
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_fetch_mates: range outside the kept records");
    try {
        if (!s->mates_valid) parse_kept_mates(*s);
    } catch (const pmx_io::Error &e) {
        return pmx_io::fail(e.code, e.msg);
    } catch (const std::exception &e) {
        return pmx_io::fail(PMX_IO_ERR_OPEN, std::string("pmx_sam_fetch_mates: ") + e.what());
    }
    if (flag) memcpy(flag, s->m_flag.data() + first, 2 * (size_t)n);
    if (mate_ref) memcpy(mate_ref, s->m_ref.data() + first, 4 * (size_t)n);
    if (mate_pos1) memcpy(mate_pos1, s->m_pos.data() + first, 4 * (size_t)n);
    if (tlen) memcpy(tlen, s->m_tlen.data() + first, 4 * (size_t)n);
    return PMX_IO_OK;
}

int pmx_sam_counters(const pmx_sam *s, uint64_t *records, uint64_t *kept, uint64_t *bytes_out, uint64_t *bytes_in,
                     uint64_t *members)
{
    if (!s) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_counters: NULL handle");
    if (records) *records = s->nrec;
    if (kept) *kept = s->n_kept;
    if (bytes_out) *bytes_out = s->N;
    if (bytes_in) *bytes_in = s->file.size;
    if (members) *members = s->members;
    return PMX_IO_OK;
}

int64_t pmx_sam_readlen_hist(pmx_sam *s, uint32_t mapq_min, int64_t cap, int32_t *lengths, uint64_t *counts, uint64_t *first)
{
    if (!s) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_readlen_hist: NULL handle");
    if (s->header_only) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_readlen_hist: the file was opened for its header only");
    if (lengths && (cap < 0 || !counts || !first))
        return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_readlen_hist: NULL argument or cap < 0");
    if (!s->rl_valid || s->rl_mapq != mapq_min) {
        s->rl_valid = false;
        try {
            struct Part {
                std::unordered_map<int32_t, std::pair<uint64_t, uint64_t>> h;   // length -> (count, first key)
                uint64_t c[6] = {0, 0, 0, 0, 0, 0};
            };
            const size_t n = s->nrec, grain = 1 << 16;
            std::vector<Part> parts((n + grain - 1) / grain);
            parallel_for(s->nthreads, n, grain, [&](size_t lo, size_t hi, size_t k) {
                Part &out = parts[k];
                for (size_t i = lo; i < hi; i++) {     // the rules of pmx_bam_readlen_hist
                    if (s->ref[i] < 0) continue;
                    const uint32_t flag = s->fm[i] & 0xffffu, mapq = s->fm[i] >> 16, q = s->qlen[i];
                    out.c[0]++;
                    if (flag & 0x1u) {
                        out.c[3]++;
                        if (flag & PMX_BAM_FLAG_READ2) out.c[4]++;
                    }
                    if (flag & PMX_BAM_FLAG_UNMAPPED) {
                        out.c[1]++;
                        continue;
                    }
                    if ((flag & PMX_BAM_FLAG_DUPLICATE) || mapq < mapq_min) continue;
                    if (q == 0 || q > 0x7fffffffu) {
                        out.c[5]++;
                        continue;
                    }
                    out.c[2]++;
                    const uint64_t key = s->line_start(i);
                    auto it = out.h.emplace((int32_t)q, std::make_pair((uint64_t)0, key)).first;
                    it->second.first++;
                    it->second.second = std::min(it->second.second, key);   // (a BED file put in order: lines out of order)
                }
            });
            std::unordered_map<int32_t, std::pair<uint64_t, uint64_t>> hist;
            uint64_t c[6] = {0, 0, 0, 0, 0, 0};
            for (const Part &p : parts) {                // (chunks in file order: the first key of a length is the first chunk's)
                for (int k = 0; k < 6; k++) c[k] += p.c[k];
                for (const auto &kv : p.h) {
                    auto it = hist.emplace(kv.first, kv.second);
                    if (!it.second) {
                        it.first->second.first += kv.second.first;
                        it.first->second.second = std::min(it.first->second.second, kv.second.second);
                    }
                }
            }
            s->rl_hist.clear();
            for (const auto &kv : hist) s->rl_hist.push_back({kv.first, kv.second.first, kv.second.second});
            std::sort(s->rl_hist.begin(), s->rl_hist.end(), [](const pmx_sam::LenBin &x, const pmx_sam::LenBin &y) { return x.len < y.len; });
            memcpy(s->rl_counters, c, sizeof c);
            s->rl_mapq = mapq_min;
            s->rl_valid = true;
        } catch (const pmx_io::Error &e) {
            return pmx_io::fail(e.code, e.msg);
        } catch (const std::exception &e) {
            return pmx_io::fail(PMX_IO_ERR_OPEN, std::string("pmx_sam_readlen_hist: ") + e.what());
        }
    }
    if (!lengths) return (int64_t)s->rl_hist.size();
    const int64_t m = std::min<int64_t>(cap, (int64_t)s->rl_hist.size());
    for (int64_t i = 0; i < m; i++) {
        lengths[i] = s->rl_hist[(size_t)i].len;
        counts[i] = s->rl_hist[(size_t)i].count;
        first[i] = s->rl_hist[(size_t)i].first;
    }
    return m;
}

int pmx_sam_readlen_counters(const pmx_sam *s, uint64_t c[6])
{
    if (!s || !c) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_readlen_counters: NULL argument");
    if (!s->rl_valid) return pmx_io::fail(PMX_IO_ERR_INVALID, "pmx_sam_readlen_counters: no pmx_sam_readlen_hist yet");
    memcpy(c, s->rl_counters, sizeof s->rl_counters);
    return PMX_IO_OK;
}

}  // extern "C"
