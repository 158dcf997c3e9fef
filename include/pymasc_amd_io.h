/* pymasc_amd_io.h -- C ABI of the host-side readers that feed the MI355X calculator.
 *
 * libpymasc_io.so is plain host code (C++17 + zlib + threads, no HIP): it turns the two input formats of the
 * reference into the flat arrays the GPU entry points of pymasc_amd.h take --
 *
 *   BAM  -> (ref_id, 1-based position, query length, strand) of the reads that pass the reference's filter,
 *           in file order; consumed by pmx_bits_set_positions[_dev] after the calculator's duplicate rules.
 *           Replaces the per-read pysam loop of PyMaSC/handler/calc.py:140-153 + handler/read.py:62-155.
 *   BigWig -> (begin, end, value) intervals of one chromosome with value >= threshold; consumed by
 *           pmx_bits_set_regions[_dev].  Replaces PyMaSC/reader/bigwig.pyx:147-177 (BigWigReader.fetch, itself a
 *           wrapper over the absent third-party libBigWig submodule).  bigBed, text and k-mer tracks give the same.
 *
 * All functions return PMX_IO_OK (0) or a negative error code unless stated; the message of the last error of the
 * calling thread is pmx_io_last_error().  Handles are not thread-safe; the library runs its own worker threads.
 */
#ifndef PYMASC_AMD_IO_H
#define PYMASC_AMD_IO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_IO_OK            0
#define PMX_IO_ERR_OPEN     -1   /* cannot open / map the file */
#define PMX_IO_ERR_FORMAT   -2   /* not the expected format, truncated or corrupt (bad magic, CRC, sizes) */
#define PMX_IO_ERR_INVALID  -3   /* bad argument */
#define PMX_IO_ERR_NOTFOUND -4   /* unknown chromosome */

const char *pmx_io_last_error(void);
int pmx_io_version(void);

/* ---- BAM (SAM spec v1 section 4; BGZF section 4.1) -------------------------------------------------------- */
typedef struct pmx_bam pmx_bam;

/* Opens and memory-maps a BGZF-compressed BAM file and parses its header.  nthreads <= 0: one per core (max 16). */
int pmx_bam_open(const char *path, int nthreads, pmx_bam **out);
void pmx_bam_close(pmx_bam *b);

/* Reference dictionary = pysam's AlignmentFile.references / .lengths (reader/bam.py:137-153). */
int32_t pmx_bam_nref(const pmx_bam *b);
const char *pmx_bam_ref_name(const pmx_bam *b, int32_t i);
int64_t pmx_bam_ref_len(const pmx_bam *b, int32_t i);
/* The SAM header text (not NUL-terminated in the file; a terminator is appended here). */
const char *pmx_bam_header_text(const pmx_bam *b, uint32_t *len);

/* SAM flag bits the reference's filter looks at (handler/read.py:62-90) */
#define PMX_BAM_FLAG_UNMAPPED  0x4u
#define PMX_BAM_FLAG_REVERSE   0x10u
#define PMX_BAM_FLAG_READ2     0x80u
#define PMX_BAM_FLAG_DUPLICATE 0x400u
#define PMX_BAM_DEFAULT_EXCLUDE (PMX_BAM_FLAG_READ2 | PMX_BAM_FLAG_UNMAPPED | PMX_BAM_FLAG_DUPLICATE)

/* Next batch of alignment records in file order that pass the filter:
 *   skipped:  flag & flag_exclude, mapq < mapq_min          (ReadFilter.should_skip_read, read.py:62-90)
 *             ref_id < 0 (reference_name is None, read.py:131-133)
 *             query length 0 (infer_query_length() is None, read.py:139-141)
 *   pos1[i]     = reference_start + 1                                            (read.py:138)
 *   read_len[i] = sum of the CIGAR operations M, I, S, =, X (pysam infer_query_length; a CIGAR moved to the CG:B,I
 *                 tag because it has > 65535 operations is followed there, as htslib does on reading)
 *   reverse[i]  = flag & 0x10 != 0                                               (read.py:144)
 * Returns the number of records written (<= cap), 0 at end of file, or a negative error code.  The filter
 * arguments must not change between calls on one handle. */
int64_t pmx_bam_next_batch(pmx_bam *b, uint32_t mapq_min, uint32_t flag_exclude, int64_t cap,
                           int32_t *ref_id, int32_t *pos1, int32_t *read_len, uint8_t *reverse);
/* pmx_bam_next_batch with four raw columns more (version >= 8): flag[i] = the record's flag, mate_ref[i] =
 * next_refID, mate_pos1[i] = next_pos + 1, tlen[i] = tlen.  The checker of the device pair counts: the pair rule itself is applied
 * by the caller.  A pass over the file is made of calls of one of the two functions only. */
int64_t pmx_bam_next_mates(pmx_bam *b, uint32_t mapq_min, uint32_t flag_exclude, int64_t cap, int32_t *ref_id, int32_t *pos1,
                           int32_t *read_len, uint8_t *reverse, uint16_t *flag, int32_t *mate_ref, int32_t *mate_pos1, int32_t *tlen);

/* .bai index (SAM spec 5.2): what the reference's multi-process mode requires (reader/bam.py:246-262) and uses
 * through pysam's fetch(chrom) (handler/worker.py:106-132).  After pmx_bam_fetch_ref, pmx_bam_next_batch yields
 * the records of that reference only (same filter, same fields) and returns 0 at the end of the reference; it
 * may be called again for another reference, or with ref_id = -1 to go back to one pass over the whole file
 * (no index needed for that).  A reference without records is an empty range, not an error. */
int pmx_bam_index_load(pmx_bam *b, const char *bai_path);
int pmx_bam_has_index(const pmx_bam *b);
int pmx_bam_fetch_ref(pmx_bam *b, int32_t ref_id);

/* Counters since open: alignment records decoded, records that passed the filter, uncompressed bytes inflated,
 * compressed bytes consumed. */
int pmx_bam_counters(const pmx_bam *b, uint64_t *records, uint64_t *kept, uint64_t *bytes_out, uint64_t *bytes_in);

/* Read-length histogram with the ESTIMATOR's filter, which is not the one above (PyMaSC core/readlen.pyx:estimate_readlen,
 * readlen.pyx:139-162), over every alignment record of the file in file order:
 *   ref_id < 0                        skipped, not counted anywhere                     (readlen.pyx:140-142)
 *   otherwise nreads; flag & 0x1 -> npaired, and with flag & 0x80 also nread2      (readlen.pyx:144-148)
 *   flag & 0x4                        nunmapped, nothing else                           (readlen.pyx:155-156)
 *   !(flag & 0x400), mapq >= mapq_min counted at its query length (as read_len above; read2, secondary, supplementary
 *                                     and QC-fail records included)                     (readlen.pyx:157-162)
 *   ... query length 0 or no CIGAR    nnoqlen instead (infer_query_length() is None; the reference fails on it)
 * One pass on the reader's threads with buffers of its own: a pmx_bam_next_batch iteration in progress is not disturbed.
 * Two-call protocol like pmx_track_fetch: lengths == NULL returns the number of distinct counted lengths; otherwise fills up
 * to cap entries sorted by length -- counts[i], first[i] = offset in the uncompressed stream (header included) of the first
 * counted record of that length: the same key as pmx_dbam_readlen_hist's.  The result is kept for the next call with the same
 * mapq_min. */
int64_t pmx_bam_readlen_hist(pmx_bam *b, uint32_t mapq_min, int64_t cap, int32_t *lengths, uint64_t *counts, uint64_t *first);
/* c = {nreads, nunmapped, ncounted, npaired, nread2, nnoqlen} of the last pmx_bam_readlen_hist */
int pmx_bam_readlen_counters(const pmx_bam *b, uint64_t c[6]);

/* ---- SAM text (SAM spec v1 section 1), plain or BGZF-compressed (bgzip) ---------------------------------------
 * The host twin of pmx_dsam_open (pymasc_amd_ingest.h) and its checker: the same parsing rules, the same
 * records, read-length histogram and counters as that reader, and as the BAM readers give for the BAM twin of the file.
 * pmx_sam_open reads the whole text (a BGZF file inflated on the reader's threads; a gzip file that is not BGZF is refused),
 * parses the header ('@' lines before the first record; @SQ SN / LN in header order = the references) and every record line
 * (FLAG, RNAME, POS, MAPQ, CIGAR; >= 11 fields); a malformed line is PMX_IO_ERR_FORMAT with "line N: <reason>" (1-based).
 * nthreads <= 0: one per core (max 16).  There is no index: a SAM file is read whole. */
typedef struct pmx_sam pmx_sam;
int pmx_sam_open(const char *path, int nthreads, pmx_sam **out);
/* The header only: the '@' lines of plain text, or of the BGZF members inflated in order until the first record line, parsed
 * with pmx_sam_open's rules; no record is read.  nref / ref_name / ref_len / header_text answer as after pmx_sam_open;
 * pmx_sam_decode and pmx_sam_readlen_hist are PMX_IO_ERR_INVALID on such a handle. */
int pmx_sam_open_header(const char *path, pmx_sam **out);
void pmx_sam_close(pmx_sam *s);
int32_t pmx_sam_nref(const pmx_sam *s);
const char *pmx_sam_ref_name(const pmx_sam *s, int32_t i);
int64_t pmx_sam_ref_len(const pmx_sam *s, int32_t i);
const char *pmx_sam_header_text(const pmx_sam *s, uint32_t *len);
/* The records that pass pmx_bam_next_batch's filter (want_ref >= 0: that reference only), in file order: returns their number;
 * pmx_sam_fetch copies records [first, first + n) of them.  May be called again with another filter. */
int64_t pmx_sam_decode(pmx_sam *s, uint32_t mapq_min, uint32_t flag_exclude, int32_t want_ref);
int pmx_sam_fetch(pmx_sam *s, int64_t first, int64_t n, int32_t *ref_id, int32_t *pos1, int32_t *read_len, uint8_t *reverse);
/* Parallel to pmx_sam_fetch (version >= 8): flag, and the mate fields of records [first, first + n) of the last
 * decode by the rules of io/sam_parse.h (parse_mates): mate_ref = the record's own id when RNEXT is '=' or its own name, the named
 * reference's id otherwise, -1 for '*' or a name no @SQ line has; mate_pos1 = PNEXT; tlen = TLEN.  The fields are parsed on the
 * first call after a decode: a PNEXT or TLEN that is not a decimal integer is PMX_IO_ERR_FORMAT, "line N: <reason>".  A handle of
 * pmx_bed_open: PMX_IO_ERR_INVALID, "the input has no mate fields". */
int pmx_sam_fetch_mates(pmx_sam *s, int64_t first, int64_t n, uint16_t *flag, int32_t *mate_ref, int32_t *mate_pos1, int32_t *tlen);
/* alignment lines, records kept by the last decode, text bytes, file bytes, BGZF members (0 for plain SAM) */
int pmx_sam_counters(const pmx_sam *s, uint64_t *records, uint64_t *kept, uint64_t *bytes_out, uint64_t *bytes_in,
                     uint64_t *members);
/* pmx_bam_readlen_hist's rules and protocol; first[i] = byte offset in the text of the line of the first counted record */
int64_t pmx_sam_readlen_hist(pmx_sam *s, uint32_t mapq_min, int64_t cap, int32_t *lengths, uint64_t *counts, uint64_t *first);
int pmx_sam_readlen_counters(const pmx_sam *s, uint64_t c[6]);

/* ---- BED read files: tagAlign / bedtools bamtobed, BED6 with one line per read (version >= 4) ----------
 * The host twin of pmx_dbed_open (pymasc_amd_ingest.h) and its checker.  `path` is plain text, BGZF or gzip (one or several
 * members; told from the bytes).  A BED file has no header: the references are the nref chromosome sizes given (names unique
 * and non-empty, lengths in 1..2^31-1; their order is the reference order).  Every line is parsed by the rules of
 * io/bed_reads_parse.h: "chrom start end name score strand" gives ref = chrom's index, pos1 = start + 1, query length =
 * end - start, flag 16 for '-' (else 0), MAPQ = min(score, 255) ('.': 255); blank, '#', "browser" and one leading "track"
 * line carry no read.  A malformed line: PMX_IO_ERR_FORMAT, "line N: <reason>" (1-based in the decompressed text).  The records
 * are delivered sorted stably by (reference, start), ties in file order: a file out of that order is put in it with
 * std::stable_sort.  The handle is a pmx_sam: nref / ref_name / ref_len (the sizes), header_text (empty), decode, fetch,
 * counters (records = reads; members = BGZF members, 0 for plain text and other gzip), readlen_hist (first[i] = byte offset
 * of the line of the first counted record, whatever the sort did), readlen_counters and close work on it. */
int pmx_bed_open(const char *path, int nthreads, int32_t nref, const char *const *names, const int64_t *lengths, pmx_sam **out);

/* ---- Mappability tracks: one handle for every kind ------------------------------------------------------------------
 * pmx_bigwig_open, pmx_ttrack_open and pmx_kmer_open each return a pmx_track (version >= 7; as pmx_dbw is the one track handle
 * of pymasc_amd_ingest.h), read through the accessors below. */
typedef struct pmx_track pmx_track;
void pmx_track_close(pmx_track *t);

/* Chromosome dictionary = BigWigReader.chromsizes (reader/bigwig.pyx:60-75), in the order each open states. */
int32_t pmx_track_nchrom(const pmx_track *t);
const char *pmx_track_chrom_name(const pmx_track *t, int32_t i);
int64_t pmx_track_chrom_len(const pmx_track *t, int32_t i);

/* All intervals of `chrom`, in the order each open states, whose float32 value is >= threshold (threshold <= 0: every
 * interval), as BigWigReader.fetch yields them (bigwig.pyx:147-177): begin 0-based inclusive, end exclusive.
 * Two-call protocol: with begin == NULL returns the number of intervals; otherwise fills up to cap entries and
 * returns the number written.  value may be NULL.  PMX_IO_ERR_NOTFOUND for a chromosome the dictionary does not hold (the
 * reference raises KeyError). */
int64_t pmx_track_fetch(pmx_track *t, const char *chrom, float threshold, int64_t cap, uint32_t *begin, uint32_t *end,
                        float *value);
/* 1 when the intervals the last fetch delivered are non-empty, ascending and disjoint (begin_i < end_i, end_i <= begin_(i+1)),
 * when there were none, and before the first fetch */
int pmx_track_sorted(const pmx_track *t);
/* 0 BigWig (a text track too, as on the device), 1 bigBed, 2 k-mer track: pmx_dbw_kind's numbering */
int pmx_track_kind(const pmx_track *t);

/* ---- BigWig (bbi): chromosomes in the file's B+ tree order, intervals in index order (ascending for a valid file) ------
 * bigBed (version >= 5): pmx_bigwig_open also takes a bigBed file (magic 0x8789F2EB; fieldCount >= 3).  Its
 * records, decoded by the rules of io/bigbed_parse.h, are the intervals [chromStart, chromEnd) with value 1.0 in index order;
 * fetch keeps them as it keeps BigWig items.  A malformed record, end < start, a block of two chromosomes, a block that does not
 * inflate or fails its Adler-32: PMX_IO_ERR_FORMAT with bigbed_parse.h's message. */
int pmx_bigwig_open(const char *path, pmx_track **out);

/* ---- Text tracks: bedGraph, BED, WIG -------------------------------------------------------
 * The host twin of pmx_dtt_open (pymasc_amd_ingest.h) and its checker.  `path` is plain text, BGZF or gzip (one or several
 * members; told from the bytes).  The kind: a track line's type=bedGraph / type=wiggle_0, else a WIG declaration as the first
 * data line, else a .bed suffix (after .gz / .bgz) means BED, else bedGraph.  The whole text is read and parsed at open by the
 * rules of io/text_track_parse.h; values are (float)strtod of their text.  A malformed line, a bad number, a WIG data line
 * before any declaration, a second track line or a truncated gzip stream: PMX_IO_ERR_FORMAT, "line N: <reason>" (1-based).
 * nthreads is unused (one thread).  The chromosomes are those that have lines, in the order of their first line; chrom_len =
 * the largest end of its lines (an extent, not a chromosome size); fetch delivers the lines in file order. */
int pmx_ttrack_open(const char *path, int nthreads, pmx_track **out);

/* ---- Genome FASTA -> k-mer uniqueness track (version >= 6) ------------------------------------------
 * The host twin of pmx_dkm_open (pymasc_amd_ingest.h) and its checker, by another method: no hashing.  `path` is a genome
 * FASTA, plain, BGZF or gzip (told from the bytes), read by the rules of io/fasta_parse.h.  Position p of record c is uniquely
 * mappable when its k-mer F exists (p + k <= len(c), k valid bases A C G T of any case), F != revcomp(F), and no other existing
 * position has F or revcomp(F) as its k-mer.  The positions are sorted on nthreads threads by the canonical packed k-mer
 * (min(F, R), compared word by word) and the groups of size one are unique.  The track of a record is its maximal runs of
 * unique positions, [p, q) with value 1.0, ascending and disjoint.  k outside [16, 1024]: PMX_IO_ERR_INVALID.  A malformed
 * file: PMX_IO_ERR_FORMAT, "line N: <reason>" (1-based, in the decompressed text), or the genome-size message.
 * The chromosomes are every record in file order with its length in bases. */
int pmx_kmer_open(const char *path, int32_t k, int nthreads, pmx_track **out);

#ifdef __cplusplus
}
#endif
#endif
