/* pymasc_amd_ingest.h -- C ABI of the DEVICE-side BAM ingest.
 *
 * libpymasc_ingest.so (pymasc_amd/csrc/ingest/bam_device.hip, hipcc, gfx950) does on the GPU what libpymasc_io.so
 * (include/pymasc_amd_io.h) does with zlib on host threads: it replaces the per-read pysam loop of the reference,
 * PyMaSC/handler/calc.py:140-153 + handler/read.py:62-155, for a whole BAM file at once:
 *
 *   host    the compressed file is read into page-locked staging buffers and copied to HBM as it is; the host only
 *           hops over the BGZF member headers (SAM spec 4.1: BSIZE, CRC32, ISIZE) -- no zlib in this library;
 *   k_bgzf_inflate   one wavefront per BGZF member: DEFLATE (RFC 1951; stored / fixed / dynamic blocks), Huffman tables
 *           and a 4-KB window of recent output in LDS, matches further back read from the member's own output in HBM;
 *   k_bgzf_crc       CRC-32 of every member's output (64 slices per member combined with x^(8n) mod P), compared with
 *           the member's footer together with ISIZE;
 *   k_bam_spec / k_bam_walk   the chain of alignment records (block_size hops) of the inflated stream, found in
 *           parallel: every 16-KB piece guesses its first record, walks to its end, and the guesses are VERIFIED against
 *           the neighbour's end (pieces whose guess was wrong are walked again until the chain closes: the result is the
 *           exact chain, not a heuristic); the walk applies the reference's read filter and extracts the fields;
 *   result  (ref_id, 1-based position, query length, strand) of the reads that pass, in file order, in device memory
 *           (pmx_dbam_device_arrays) or copied to the host (pmx_dbam_fetch): the arrays pmx_bam_next_batch yields.
 *
 * Same filter and fields as pmx_bam_next_batch (pymasc_amd_io.h), bit for bit; the host reader stays as the checker
 * (tests/test_gpu_ingest.py).  All functions return 0 or a negative PMX_IO_ERR_* code (same values as pymasc_amd_io.h);
 * the message of the calling thread's last error is pmx_dbam_last_error().  A handle is not thread-safe.
 */
#ifndef PYMASC_AMD_INGEST_H
#define PYMASC_AMD_INGEST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_DBAM_OK            0
#define PMX_DBAM_ERR_OPEN     -1   /* cannot open / read the file, or out of (device) memory */
#define PMX_DBAM_ERR_FORMAT   -2   /* not a BAM file, truncated or corrupt (gzip magic, DEFLATE, CRC32, ISIZE, records) */
#define PMX_DBAM_ERR_INVALID  -3   /* bad argument */
#define PMX_DBAM_ERR_NOTFOUND -4   /* unknown chromosome (pmx_dbw_fetch) */
#define PMX_DBAM_ERR_DEVICE   -5   /* a HIP call failed */

typedef struct pmx_dbam pmx_dbam;

const char *pmx_dbam_last_error(void);
int pmx_dbam_version(void);

/* Reads `path` (a BGZF-compressed BAM file), inflates ALL of it on GPU `device`, checks every member's CRC32 and ISIZE
 * and parses the BAM header.  nthreads: host threads that read the file into the staging buffers (<= 0: up to 16).
 * The inflated stream stays in device memory until pmx_dbam_close.  Replaces pysam.AlignmentFile(path)
 * (reader/bam.py:84-126). */
int pmx_dbam_open(const char *path, int device, int nthreads, pmx_dbam **out);
void pmx_dbam_close(pmx_dbam *b);

/* Indexed reading (version >= 2): only the chromosomes a caller chooses are read, copied and inflated.
 * pmx_dbam_open_indexed reads, copies and inflates only the BGZF members that hold the BAM header (from offset 0 until the
 * parsed header is complete) and loads the .bai index (bai_path, or NULL: <path>.bai, then <stem>.bai), checked against the
 * header.  nref / ref_name / ref_len / header_text work as after pmx_dbam_open; pmx_dbam_decode finds no records until
 * pmx_dbam_select.  A missing or truncated index, a bad magic or another number of references: PMX_DBAM_ERR_FORMAT. */
int pmx_dbam_open_indexed(const char *path, const char *bai_path, int device, int nthreads, pmx_dbam **out);
/* Reads, copies and inflates only the members that hold the records of refs[0..n) (their [beg, end) virtual offsets from the
 * index, SAM spec 5.2: the pseudo-bin 37450 when present, else min / max over the chunks of all bins -- the rule of
 * pmx_bam_index_load); afterwards the handle behaves like a pmx_dbam_open handle of a file that holds the header and just those
 * records, in file order (decode, fetch, runs, readlen_hist, inflated: over that stream).  May be called again with another
 * set: the stream is replaced.  A reference id out of range: PMX_DBAM_ERR_INVALID; a chosen reference without records
 * contributes nothing.  PMX_DBAM_ERR_FORMAT, and a handle without records, for an offset outside the file or not at a member
 * start, a range that begins after it ends or inside the header, a range start the verified record chain does not pass through
 * (stale or shifted index), and a record of a reference that was not chosen. */
int pmx_dbam_select(pmx_dbam *b, const int32_t *refs, int32_t n);

/* SAM text (version >= 3): `path` is a SAM file, plain or BGZF-compressed (bgzip; a gzip file that is not BGZF is
 * PMX_DBAM_ERR_FORMAT).  The text goes to HBM as the BAM open sends the file (BGZF: the same member scan, k_bgzf_inflate and
 * k_bgzf_crc); the header is parsed on the host from the stream's prefix; k_sam_count / k_sam_lines index the lines and
 * k_sam_parse parses every record line into a table in HBM by the rules of DESIGN.md 7.4 (the rules of pmx_sam_open,
 * pymasc_amd_io.h, which is its checker).  A malformed line: PMX_DBAM_ERR_FORMAT, "line N: <reason>" as pmx_sam_open words it.
 * The handle is a pmx_dbam whose stream is the text: nref / ref_name / ref_len / header_text, decode (a filter + compaction
 * over the table: the records, fields and order of the BAM twin), device_arrays, fetch, runs, readlen_hist (first[i] = byte
 * offset in the text of the line of the first counted record), readlen_counters, counters (records = alignment lines,
 * bytes_out = text bytes, bytes_in = file bytes, members = 0 for plain SAM, rewalked = 0), timings ([4] line index,
 * [5] parse + the last filter) and inflated (the text) work on it; pmx_dbam_select returns PMX_DBAM_ERR_INVALID (no index). */
int pmx_dsam_open(const char *path, int device, int nthreads, pmx_dbam **out);

/* Stream reading (version >= 4): `fd` is read in BOUNDED WINDOWS -- a pipe, a FIFO, a socket, a character
 * device or a regular file; it is never sized (fstat) or seeked, and the caller keeps it (it is not closed).  The format comes
 * from the first bytes: BGZF whose first member inflates to "BAM\1" is BAM, to text is BGZF SAM; text starting with '@' is plain
 * SAM; gzip that is not BGZF is PMX_DBAM_ERR_FORMAT.  The open reads and inflates the first window(s), as far as the header
 * needs; nref / ref_name / ref_len / header_text work at once.  window_bytes: compressed bytes per window (0: 64 MiB); a window
 * is whole BGZF members within window_bytes compressed AND 4 * window_bytes inflated (at least one member), or that many bytes
 * of plain text.  nthreads is unused (one reader thread reads ahead).  Device memory depends on window_bytes only: the buffers
 * grow only for a record or line longer than a window. */
int pmx_dbam_open_stream(int fd, int device, int nthreads, uint64_t window_bytes, pmx_dbam **out);
/* Makes the next window current: decode, device_arrays, runs, fetch, counters, readlen_hist and inflated then work on it (its
 * records: from the record its first byte starts -- the first after the header, or the one the last window carried -- up to the
 * last record that ends inside it; the rest is carried to the front of the next window by a device-to-device copy).  While the
 * caller works on this window, a host thread reads the next one from fd.  Returns the window's record bytes (> 0), 0 at the end
 * of the stream, or a negative error code: a stream that ends inside a member or a record, a CRC / ISIZE / DEFLATE error, a
 * malformed record or SAM line are PMX_DBAM_ERR_FORMAT, with the messages of pmx_dbam_open / pmx_dsam_open; a read error is
 * PMX_DBAM_ERR_OPEN.  readlen_hist's first-occurrence keys are offsets in the whole inflated stream. */
int64_t pmx_dbam_stream_next(pmx_dbam *b);
/* out = {windows made current, compressed bytes taken from fd, largest carried tail (bytes), peak device bytes the handle has
 * held between calls (window buffers, compressed window, member table, record chain, kept-record arrays, histogram and SAM
 * line tables; not pmx_dbam_runs' transient table), window_bytes, inflated budget}.  PMX_DBAM_ERR_INVALID for a handle that
 * was not opened by pmx_dbam_open_stream. */
int pmx_dbam_stream_info(const pmx_dbam *b, uint64_t out[6]);

/* Reference dictionary = pysam's AlignmentFile.references / .lengths (reader/bam.py:137-153). */
int32_t pmx_dbam_nref(const pmx_dbam *b);
const char *pmx_dbam_ref_name(const pmx_dbam *b, int32_t i);
int64_t pmx_dbam_ref_len(const pmx_dbam *b, int32_t i);
const char *pmx_dbam_header_text(const pmx_dbam *b, uint32_t *len);

/* Walks every alignment record on the device and keeps those that pass the reference's filter
 * (ReadFilter.should_skip_read, handler/read.py:62-90; reference_name None, read.py:131-133; query length 0,
 * read.py:139-141) -- exactly the records, fields and order of pmx_bam_next_batch; want_ref >= 0 keeps the records of
 * that reference only (what AlignmentFile.fetch(chrom) yields a worker, handler/worker.py:106-132).
 * Returns the number of kept records or a negative error code; may be called again with another filter. */
int64_t pmx_dbam_decode(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, int32_t want_ref);

/* The kept records of the last pmx_dbam_decode in device memory: int32 ref_id[n], int32 pos1[n], int32 read_len[n],
 * uint8 reverse[n] (valid until the next decode / close). */
int pmx_dbam_device_arrays(const pmx_dbam *b, const int32_t **d_ref_id, const int32_t **d_pos1, const int32_t **d_read_len,
                           const uint8_t **d_reverse);
/* ... and copied to host arrays: records [first, first + n). */
int pmx_dbam_fetch(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref_id, int32_t *pos1, int32_t *read_len, uint8_t *reverse);

/* The kept records as RUNS of one reference each, in file order (a coordinate-sorted file: one run per chromosome):
 * start[r] = index of the run's first record in the arrays above, ref_id[r], and the positions of its first and last record
 * (what the calculator's order check needs on the host; everything inside a run is checked by the device feeders).
 * Two-call protocol: with start == NULL returns the number of runs, else fills up to cap entries and returns the number
 * written.  More than 65536 runs (an unsorted file): PMX_DBAM_ERR_INVALID -- take the arrays through pmx_dbam_fetch then. */
int64_t pmx_dbam_runs(pmx_dbam *b, int64_t cap, int64_t *start, int32_t *ref_id, int32_t *first_pos1, int32_t *last_pos1);

/* Read-length histogram with the ESTIMATOR's filter (PyMaSC core/readlen.pyx:139-162; not the filter of pmx_dbam_decode):
 * exactly what pmx_bam_readlen_hist (pymasc_amd_io.h) gives -- records with ref_id < 0 invisible; nreads, npaired, nread2;
 * unmapped ones in nunmapped only; the others counted at their query length when not duplicates and mapq >= mapq_min (read2,
 * secondary, supplementary, QC-fail included); query length 0 in nnoqlen.  One more walk over the verified record chain already
 * in HBM (no second inflate), with tables of its own: the arrays of the last pmx_dbam_decode are left as they are, and the
 * order of the two calls does not matter.  Malformed records: the error codes and messages of pmx_dbam_decode.
 * Two-call protocol like pmx_dbam_runs: lengths == NULL returns the number of distinct counted lengths; otherwise fills up to
 * cap entries sorted by length -- counts[i], first[i] = byte offset in the inflated stream (header included) of the first
 * counted record of that length (the file-order key MODE's tie rule needs; the same key as pmx_bam_readlen_hist's).
 * The result is kept for the next call with the same mapq_min. */
int64_t pmx_dbam_readlen_hist(pmx_dbam *b, uint32_t mapq_min, int64_t cap, int32_t *lengths, uint64_t *counts, uint64_t *first);
/* c = {nreads, nunmapped, ncounted, npaired, nread2, nnoqlen} of the last pmx_dbam_readlen_hist */
int pmx_dbam_readlen_counters(const pmx_dbam *b, uint64_t c[6]);

/* Library complexity (version >= 9): how often each key (ref_id, pos1, read_len, reverse) occurs among the
 * records that pass mapq_min / flag_exclude (the filter of pmx_dbam_decode; ENCODE's NRF / PBC1 / PBC2 keep flagged duplicates:
 * pass PMX_BAM_DEFAULT_EXCLUDE & ~PMX_BAM_FLAG_DUPLICATE).  The four fields are compared in full.  One more walk + filter over
 * the record chain (or the SAM / BED parse table) already in HBM, with arrays of its own: the arrays of the last pmx_dbam_decode,
 * its counters and pmx_dbam_runs are left as they are, and the order of the calls does not matter.  Equal keys are brought
 * together by the stable LSD radix sort of pmx_dbed_open over the digits of the key (a digit that is the same in every key is
 * skipped), so the input need not be sorted and a pile of reads on one position costs what any other reads cost.
 * per_ref[4 * r + {0, 1, 2, 3}] = {reads, distinct keys, keys seen once, keys seen twice} of reference r (a key never spans two
 * references: the whole is their sum); hist[k] = keys seen exactly k times for 1 <= k < PMX_COMPLEXITY_BINS - 1, the last bin =
 * keys seen at least that often, hist[0] = the largest multiplicity.  use_ref: nref bytes, 0 = the reference is left out of every
 * output; NULL = every reference.  Device memory: at most 40 bytes per kept read, transient (freed before the call returns).
 * A stream handle: a call counts the current window, once (a second call for the same window reports zeros), except that the
 * kept records of the window's last (ref_id, pos1) are held back in device memory (13 bytes each, part of pmx_dbam_stream_info's
 * peak) and counted with the next window; a call after pmx_dbam_stream_next has returned 0 counts what is still held back, and
 * the calls after it report zeros: the caller adds the calls up.  A stream must be in (ref_id, pos1) order: a kept record below
 * its predecessor is PMX_DBAM_ERR_INVALID, "stream is not sorted by position".  Malformed records: the codes and messages of
 * pmx_dbam_decode; a NULL output: PMX_DBAM_ERR_INVALID; 2^32 - 1 kept reads or more: PMX_DBAM_ERR_OPEN. */
#define PMX_COMPLEXITY_BINS 32
int pmx_dbam_complexity(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, const uint8_t *use_ref, uint64_t *per_ref,
                        uint64_t hist[PMX_COMPLEXITY_BINS]);

/* Excluded regions (version >= 10): attaches a BED mask to the handle.  offsets[nref + 1] (host memory) delimit each
 * reference's lines in begin[] / end[] (0-based, half-open; host OR device memory, the pointer decides): the lines of reference r are
 * [offsets[r], offsets[r + 1]), in any order, overlapping or abutting.  They are clipped to the reference's length (a line that
 * is empty then is dropped), sorted by begin within a reference and merged ON THE DEVICE (a line that overlaps or abuts the
 * running maximum of the ends in front of it joins that group); the merged intervals stay in HBM with the handle.  From then on
 * every pmx_dbam_decode -- of a BAM, indexed BAM, SAM or BED handle, and of every window of a stream -- leaves out, after its own
 * filter, the records whose extent [pos1, pos1 + read_len - 1] overlaps a merged interval (b, e) of their reference:
 * b + 1 <= pos1 + read_len - 1 and pos1 <= e.  The kept records are compacted in file order, so that device_arrays, fetch, runs and
 * counters' `kept` describe the stream as if the dropped records had never been in the file; pmx_dbam_complexity counts the same
 * records.  readlen_hist is not affected.  offsets = begin = end = NULL detaches the mask.  nref must be pmx_dbam_nref. */
int pmx_dbam_set_exclude(pmx_dbam *b, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end);
/* The merged intervals in (reference, begin) order.  Two-call protocol like pmx_dbam_runs: ref_id == NULL returns their number. */
int64_t pmx_dbam_exclude_intervals(pmx_dbam *b, int64_t cap, int32_t *ref_id, uint32_t *begin, uint32_t *end);
/* *dropped = records the last pmx_dbam_decode left out because of the mask; *intervals = merged intervals attached. */
int pmx_dbam_excluded(const pmx_dbam *b, uint64_t *dropped, uint64_t *intervals);

/* Read counts per genome bin (version >= 11): the table behind the fingerprint and the Jensen-Shannon distance.
 * A chosen reference of length len has floor(len / bin_size) bins; bin j (0-based) covers the 1-based positions
 * j * bin_size + 1 .. (j + 1) * bin_size, the tail shorter than a bin has none; the chosen references' bins lie end to end in
 * header order.  A read covers [pos1, pos1 + L - 1] when forward and [pos1 + read_len - L, pos1 + read_len - 1] when reverse (its
 * 5' end stays put), with L = extend, or read_len when extend is 0; the extent is clipped to [1, len] and the read adds 1 to every
 * bin it overlaps.
 * pmx_dbam_bincount_begin allocates one zeroed uint32 per bin and 16 bytes per reference in device memory (part of
 * pmx_dbam_stream_info's peak); they replace any earlier table and stay until the next begin or close.  use_ref: nref bytes, 0 =
 * the reference has no bins; NULL = every reference.  bin_size 0, no bin at all, or 2^31 bins or more: PMX_DBAM_ERR_INVALID.
 * pmx_dbam_bincount_add counts what the handle holds now -- the whole file, the selection of an indexed handle, the current
 * window of a stream -- at mapq_min / flag_exclude (the filter of pmx_dbam_decode), less the reads an attached mask leaves out:
 * the walk + filter of pmx_dbam_complexity, with arrays of its own (13 bytes per kept read, freed before the call returns), so
 * the arrays, counters and runs of the last pmx_dbam_decode are left as they are.  Calls add up in the table: a stream is
 * counted by one call per window (a read is counted in the window that decodes it, so nothing is held back and no order is
 * asked for), and a second call on the same records doubles every bin.  *reads_added = the reads of this call that added to at
 * least one bin.
 * pmx_dbam_bincount_hist: hist[k] = bins that hold exactly k reads, for k < PMX_BINCOUNT_HIST; totals = {bins, the sum of all
 * bins, reads that added to a bin since begin}.  The values of the bins at or above PMX_BINCOUNT_HIST come in `tail`, in any
 * order (two-call protocol like pmx_dbam_runs: tail == NULL returns their number, else up to cap are written and their number
 * is returned; hist and totals are filled by both calls).  The table is not cleared.
 * pmx_dbam_bincount_copy: the bins [first, first + n) copied to the host.
 * add / hist / copy before begin, a NULL output, and a range outside the table: PMX_DBAM_ERR_INVALID. */
#define PMX_BINCOUNT_HIST 4096
int pmx_dbam_bincount_begin(pmx_dbam *b, uint32_t bin_size, uint32_t extend, const uint8_t *use_ref);
int pmx_dbam_bincount_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t *reads_added);
int64_t pmx_dbam_bincount_hist(pmx_dbam *b, uint64_t hist[PMX_BINCOUNT_HIST], uint64_t totals[3], int64_t cap, uint32_t *tail);
int pmx_dbam_bincount_copy(pmx_dbam *b, int64_t first, int64_t n, uint32_t *counts);

/* Reads per peak line and reads in peaks (version >= 12): FRiP's counts.  The lines come per reference as for
 * pmx_dbam_set_exclude (offsets[nref + 1] in host memory; begin[] / end[] 0-based, half-open, in host OR device memory), in any
 * order, overlapping, nested, abutting or repeated, and EVERY line keeps a count of its own.  A line is clipped to its reference's
 * length; one that is empty then stays in the table with the count 0.  A read's extent is pmx_dbam_bincount's with `extend`,
 * clipped to [1, len]: [lo, hi].  The read is IN the line (b, e) when b + 1 <= hi and lo <= e.
 * pmx_dbam_peakcount_begin clips, sorts and scans the lines on the device with the mask's kernels and keeps, per line, the sorted
 * key, the clipped end, the running maximum of the ends, the input place and one zeroed uint32 (28 bytes per line, part of
 * pmx_dbam_stream_info's peak); they replace any earlier table and stay until the next begin or close.  use_ref: nref bytes, 0 =
 * reads of that reference are not counted and its lines add nothing to the union; NULL = every reference.
 * pmx_dbam_peakcount_add counts what the handle holds now -- the whole file, the selection of an indexed handle, the current
 * window of a stream -- through the walk + filter of pmx_dbam_bincount_add (arrays of its own, an attached mask applied); calls
 * add up.  out = {reads counted, reads in at least one line} of this call; a read on a chosen reference is counted whether or not
 * it touches a line.
 * pmx_dbam_peakcount_copy: the counts of the lines [first, first + n) in INPUT order.
 * pmx_dbam_peakcount_totals: totals = {reads counted, reads in at least one line, bases of the clipped, merged lines on chosen
 * references, lines} since begin; per_ref[2 * r + {0, 1}] = the first two for reference r (2 * nref values).
 * add / copy / totals before begin, a NULL output, and a range outside the table: PMX_DBAM_ERR_INVALID. */
int pmx_dbam_peakcount_begin(pmx_dbam *b, int32_t nref, const int64_t *offsets, const uint32_t *begin, const uint32_t *end,
                             uint32_t extend, const uint8_t *use_ref);
int pmx_dbam_peakcount_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t out[2]);
int pmx_dbam_peakcount_copy(pmx_dbam *b, int64_t first, int64_t n, uint32_t *counts);
int pmx_dbam_peakcount_totals(pmx_dbam *b, uint64_t totals[4], uint64_t *per_ref);

/* The fragment pileup as a bedGraph track (version >= 13).  The reads are pmx_dbam_bincount_add's (the filter, the
 * chosen references, less the reads an attached exclude mask drops) with its extent: L = extend, or the read's own length at 0; a
 * forward read covers [pos1, pos1 + L - 1], a reverse read [pos1 + read_len - L, pos1 + read_len - 1], clipped to [1, len] of the
 * reference; a read with nothing left adds nothing.  depth[r][p] = the kept reads whose clipped extent holds position p, a 32-bit
 * count.  Per chosen reference, in header order, the maximal intervals of constant depth > 0 are the runs (start0, end0, depth),
 * 0-based and half-open; reads that abut at equal depth form one run; depth 0 is no run.
 * begin: one zeroed int32 slot per base of every chosen reference (use_ref[nref], NULL: all) plus one closing slot each (each
 * reference begins on a multiple of 4 slots): 4 bytes per chosen base, 12.4 GB for hg38.  It replaces any earlier pileup and
 * stays with the handle until finish, the next begin or close; it counts towards pmx_dbam_stream_info's peak.  No chosen reference:
 * PMX_DBAM_ERR_INVALID; out of device memory: PMX_DBAM_ERR_OPEN, with the size asked for.
 * add: the kept records of what the handle holds now (the arrays of the last decode stay untouched) each add +1 at the slot of
 * their first position and -1 behind their last; *reads_added = the reads that added.  Calls add up (the windows of a stream);
 * 2^31 reads or more since begin: PMX_DBAM_ERR_INVALID.
 * finish: the table becomes the runs (tiles of PMX_COVERAGE_TILE slots: sums, scans, a compaction of the non-zero slots, a second
 * one of the entries of depth > 0) and is freed; totals = reads, runs, covered bases = sum (end0 - start0), fragment bases =
 * sum depth * (end0 - start0), the largest depth.  The runs (16 bytes each) stay until the next begin or close.
 * runs: runs [first, first + n) copied to the host.  text: the bytes of their bedGraph lines "chrom\tstart0\tend0\tdepth\n",
 * formatted on the device; with buf NULL only their number is returned (then call again with that much room, as for
 * pmx_dbam_bincount_hist); a cap that is too small: PMX_DBAM_ERR_INVALID.  Returns the number of bytes.
 * add / finish without a table, runs / text before finish, a NULL output and a range outside the runs: PMX_DBAM_ERR_INVALID. */
#define PMX_COVERAGE_TILE 4096u
int pmx_dbam_coverage_begin(pmx_dbam *b, uint32_t extend, const uint8_t *use_ref);
int pmx_dbam_coverage_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t *reads_added);
int pmx_dbam_coverage_finish(pmx_dbam *b, uint64_t totals[5]);
int pmx_dbam_coverage_runs(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *depth);
int64_t pmx_dbam_coverage_text(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap);

/* The pileup as the parts of a bigWig file (version >= 17): the bytes of its data sections and of its zoom
 * records, computed from the runs finish left, with a table per call that says where every section begins and ends, so that the
 * host builds the R-trees without parsing a byte.  All four are legal only between finish and the next begin
 * (PMX_DBAM_ERR_INVALID otherwise), and follow text: a NULL buffer returns the size, a cap that is too small is
 * PMX_DBAM_ERR_INVALID, out of device memory is PMX_DBAM_ERR_OPEN with the bytes asked for.
 * ranges: first[k] = the first run of the k-th chosen reference in header order (a reference without a run: that of the next),
 * first[chosen] = the number of runs.  Returns chosen + 1; with first NULL only that.
 * sections: runs [first, first + n), which must be runs of ONE reference, as bedGraph sections (type 1) of `items` runs (1 .. 65535;
 * the last one shorter): a 24-byte header (chrom_id, start, end, 0, 0, type 1, 0, itemCount), then (start0, end0, float32 depth) per
 * run; a depth is exact up to 2^24 and rounded to nearest above.  Returns the bytes, 24 per section + 12 per run;
 * table[section][5] = chrom_id, start, chrom_id, end, bytes.
 * zoom_begin: dense bins of z0 * 4^k bases for levels k < `levels` (at most PMX_COVERAGE_ZOOM_LEVELS) over every chosen
 * reference; chrom_id[nref] gives every chosen reference its id, 0 .. chosen - 1 each once, and the bins lie in id order.  Bin j of
 * a reference covers [j * z, min((j + 1) * z, len)).  Per bin, as integers: the covered bases (depth > 0), the smallest and
 * largest depth, the sum of the depth and of its square over those bases.  Level 0 is filled from the runs, level k + 1 from four
 * bins of level k.  out[0] = the sum of depth^2 over all covered bases, out[1] = the smallest depth (0 without a run).  28 bytes
 * per bin of level 0 and about a third again, counted towards pmx_dbam_stream_info's peak, until the last level is pulled, the
 * next zoom_begin, begin or close.  max_depth * fragment_bases >= 2^64 (a 64-bit sum of squares could be inexact):
 * PMX_DBAM_ERR_INVALID and no bins.
 * zoom_records: the bins of `level` with a covered base, in (id, start) order, as 32-byte records (chrom_id, start, end,
 * validCount u32, then min, max, sum, sumSquares as float32, rounded to nearest even), in sections of `items` records that may
 * hold two references; table[section][5] = first id, first start, last id, last end, bytes.  Returns the bytes.  Pulling
 * the last level frees the bins. */
#define PMX_COVERAGE_ZOOM_LEVELS 10u
int64_t pmx_dbam_coverage_ranges(pmx_dbam *b, int64_t *first, int64_t cap);
int64_t pmx_dbam_coverage_sections(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                   uint32_t *table, int64_t table_cap);
int pmx_dbam_coverage_zoom_begin(pmx_dbam *b, uint32_t z0, uint32_t levels, const uint32_t *chrom_id, uint64_t out[2]);
int64_t pmx_dbam_coverage_zoom_records(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                       int64_t table_cap);

/* The pileup as a signal track (version >= 19): the mean depth per bin of B bases times a scale factor, float32,
 * equal neighbours merged; made of the runs finish left, so every call here is legal only between finish and the next begin
 * (PMX_DBAM_ERR_INVALID otherwise), and all but `signal` only after a `signal`.
 * The definitions.  Reference r of length len has the bins j = 0 .. ceil(len / B) - 1; bin j covers [j * B, min((j + 1) * B, len)) and
 * has the width w_j (only the last bin can be short); S_j is the integer sum of the depth over its bases (below 2^47: exact as u64
 * and as float64); B is 1 .. 65536.  v_j = f32((f64(S_j) * scale) / f64(w_j)): one float64 multiply, one float64 divide, one
 * conversion to float32, each rounded to nearest even.  Consecutive bins of one reference are one run when they have the same S and
 * the same width (the rule is on S, not on v: two S that round to one float32 stay two runs); bins with S = 0 are in no run; a run
 * is (ref, start0, end0, v), in header order.  With B = 1 the signal runs are the depth runs with v = f32(f64(depth) * scale).
 * signal: makes the signal runs, kept on the handle beside the depth runs (16 bytes each) and replaced by the next signal, begin or
 * close; totals = runs, covered bases (the runs' widths summed), the smallest and the largest v (0 without a run).  scale must be
 * finite and at least 2^-64 (no value is a float32 denormal) with scale * max_depth < 2^40 (v * 10^6 < 2^63), bin 1 .. 65536:
 * PMX_DBAM_ERR_INVALID otherwise.  For B > 1 a dense u64 table, 8 bytes per bin of every chosen reference, is held inside the call
 * and counted towards pmx_dbam_stream_info's peak; out of device memory: PMX_DBAM_ERR_OPEN with the bytes asked for.  A failure
 * leaves no signal.
 * signal_runs / _text / _ranges / _sections / _zoom_begin / _zoom_records / _sections_z / _zoom_records_z: their depth twins over the
 * signal runs, with the same rules for a NULL buffer, a short cap and out of memory.  What differs:
 * - runs: the fourth column is the float32 v.
 * - text: the value is the decimal expansion of the exact value of v rounded to six decimals, ties to even, without trailing zeros
 *   and without a trailing '.' ("0.0000004" is "0"); made in integers.  With scale 1 and B = 1 the lines equal pmx_dbam_coverage_text's.
 * - sections: the third word of an item is v; sums[section][2] = the section's runs in order, acc += f64(ov) * f64(v) and
 *   acc += f64(ov) * (f64(v) * f64(v)) from 0.0, ov = end0 - start0 (what the total summary adds up, in file order, on the host).
 * - zoom_begin: a bin of level 0 takes the signal runs that overlap it in ascending start order, each by ov bases: validCount =
 *   sum ov, min and max over v, and the two sums above as float64; a bin of level k + 1 adds its up to four bins of level k in
 *   index order the same way.  Every multiply and add is rounded on its own (no fused multiply-add), so the records do not depend
 *   on scheduling.  out[0] = out[1] = 0: the signal's summary needs nothing from here.  The bins replace the depth's, and the
 *   depth's zoom_begin replaces these; zoom_records of the other kind: PMX_DBAM_ERR_INVALID.
 * - zoom_records: min and max as they are, the two sums rounded to float32. */
int pmx_dbam_coverage_signal(pmx_dbam *b, uint32_t bin, double scale, double totals[4]);
int pmx_dbam_coverage_signal_runs(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, float *value);
int64_t pmx_dbam_coverage_signal_text(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap);
int64_t pmx_dbam_coverage_signal_ranges(pmx_dbam *b, int64_t *first, int64_t cap);
int64_t pmx_dbam_coverage_signal_sections(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                          uint32_t *table, int64_t table_cap, double *sums);
int pmx_dbam_coverage_signal_zoom_begin(pmx_dbam *b, uint32_t z0, uint32_t levels, const uint32_t *chrom_id, uint64_t out[2]);
int64_t pmx_dbam_coverage_signal_zoom_records(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                              int64_t table_cap);
int64_t pmx_dbam_coverage_signal_sections_z(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                            uint32_t *table, int64_t table_cap, uint32_t *zsizes, double *sums);
int64_t pmx_dbam_coverage_signal_zoom_records_z(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                                int64_t table_cap, uint32_t *zsizes);

/* Treatment against control (version >= 20): two pileups as one signal track.  `b` (the treatment) and `c` (the
 * control) must both be in the runs state (between finish and the next begin), on the same device, with equal chosen references (the
 * same names and lengths in the same order): PMX_DBAM_ERR_INVALID otherwise, with the condition that failed.  c == b is legal: with
 * a_t == a_c it gives a track of zeros (ones, for ratio) over b's covered bins.
 * The definitions.  S_t[j] and S_c[j] are the integer depth sums per bin of B bases, with the bins, the widths w_j and the bound on S
 * of pmx_dbam_coverage_signal; B is 1 .. 65536.  Per bin, in float64, each operation rounded to nearest even on its own (no fused
 * multiply-add):
 *   t = (f64(S_t) * a_t) / f64(w)        c = (f64(S_c) * a_c) / f64(w)
 *   op 2, subtract: v = f32(t - c)
 *   op 1, ratio:    v = f32((t + p) / (c + p))
 *   op 0, log2:     v = f32(lg2((t + p) / (c + p)))
 * lg2(x) of a positive normal float64 is a stated algorithm, not a library call:
 *   1. (m, e) = frexp(x), with m in [0.5, 1) (the exponent field, taken with integer operations).
 *   2. If m < C, with C = 0.7071067811865476 (the float64 of sqrt(1/2)), then m = 2 m and e = e - 1.
 *   3. f = m - 1.0; s = f / (2.0 + f); z = s * s.
 *   4. P = c_10; for k = 9 .. 0: P = P * z + c_k, with c_k = 1.0 / (2 k + 1) computed as a float64 division (c_0 = 1.0); the
 *      multiply and the add are rounded separately.
 *   5. ln = (2.0 * s) * P; lg2 = f64(e) + ln * 1.4426950408889634.
 * Consecutive bins of one reference are one run when they have the same S_t, the same S_c and the same width (the rule is on the
 * sums, not on v: (3, 3) and (5, 5) both give log2 = 0 and stay two runs); bins with S_t = 0 and S_c = 0 are in no run; a bin that
 * only the control covers is in a run.  A run is (ref, start0, end0, v), in header order.  totals = runs, covered bases, the smallest
 * and the largest v as signed floats (0 without a run).
 * Refused with PMX_DBAM_ERR_INVALID: an op other than 0, 1, 2; a bin outside 1 .. 65536; a factor, or for log2 / ratio p, below
 * 2^-64 or not finite; a * max_depth >= 2^40 for either track; p >= 2^40; for ratio (a_t * max_depth_t + p) / p >= 2^40 (below that
 * |v| * 10^6 < 2^63 and the text is integer arithmetic).  subtract ignores p.
 * The call waits for c's stream, then works on b's.  The runs are kept on b in the signal slot -- the same four columns, replaced by
 * the next signal, compare, begin or close -- and all eight pmx_dbam_coverage_signal_* consumers serve them: the text of a negative v
 * is '-' followed by the text of |v|, written only when round(|v| * 10^6) is not 0 ("0", never "-0"); min and max of a zoom record
 * are signed.  c is not changed.  Two dense u64 tables, 16 bytes per bin of every chosen reference, are held inside the call for
 * B = 1 as for any other bin (two run lists do not line up), counted towards pmx_dbam_stream_info's peak and freed before the call
 * returns: B = 1 on a large genome (hg38: 49 GB) runs out of device memory and returns PMX_DBAM_ERR_OPEN with the bytes asked for;
 * the table is not tiled.  A failure leaves no signal. */
int pmx_dbam_coverage_compare(pmx_dbam *b, pmx_dbam *c, uint32_t bin, int op, double a_t, double a_c, double pseudo, double totals[4]);

/* The treatment scored against the control (version >= 22): -log10 of a Poisson upper tail per bin against a local
 * lambda, as one signal track.  The definitions are this project's own; nothing here was compared with MACS2.  `b` and `c` are
 * checked as pmx_dbam_coverage_compare checks them (both in the runs state, one device, equal chosen references; c == b is legal).
 * The definitions.  Everything is integer arithmetic or float64, each float64 operation rounded to nearest even on its own (no
 * fused multiply-add).  S_t[j] and S_c[j] are the integer depth sums per bin of B bases (1 .. 65536) with the bins and the widths w_j
 * of pmx_dbam_coverage_signal; reference r has the bins 0 .. n_r - 1 and the length len_r.  a_c is a float64 factor; the treatment is
 * not scaled, because the score counts reads.  small (W_s) and large (W_l) are two window sizes in bases, each 0 (off) .. 2^31 - 1.
 *   k        k[j] = S_t[j] / w_j, an integer division.
 *   window   For W > 0: h = (W / B) / 2 bins; lo = max(0, j - h) and hi = min(n_r - 1, j + h), inside the bin range of j's own
 *            reference (a window never crosses into another reference); N = sum S_c[lo .. hi] as u64;
 *            D = min(len_r, (hi + 1) * B) - lo * B; c_W = (f64(N) * a_c) / f64(D).  h = 0 gives the bin's own value; a window that is
 *            off contributes nothing.
 *   lambda   c_0 = (f64(S_c[j]) * a_c) / f64(w_j); l_bg = (f64(sum of every S_c) * a_c) / f64(sum of the chosen lengths);
 *            l[j] = max(l_bg, c_0, c_Ws, c_Wl).  A control without a covered base is refused, so l > 0 and normal everywhere.
 *   ln, F    ln(x) = lg2(x) * 0.6931471805599453 with lg2 the stated algorithm of pmx_dbam_coverage_compare.  F[0] = F[1] = 0.0,
 *            F[i] = F[i - 1] + ln(f64(i)), a sequential sum: the caller computes it once for max_depth_t + 1 entries and hands it in
 *            as lnfact[n_lnfact] (more entries are legal; only the first max_depth_t + 1 are read).
 *   score    If f64(k) <= l then v = 0.0: the bin is not enriched, and equality counts as not enriched.  Otherwise S = 1.0, T = 1.0
 *            and for i = 1, 2, ...: r = l / f64(k + i); T = T * r; S' = S + T; stop when S' == S, else S = S' (the ratio is below
 *            1 and falling, so the loop ends).  Then A = f64(k) * ln(l); C = (l - A) + F[k];
 *            v = f32(C * 0.4342944819032518 - lg2(S) * 0.3010299956639812): -log10 of P(X >= k | l), with 0 <= v < 2^40.
 *   runs     A bin with S_t = 0 is in no run.  A kept bin begins a run when it is the first bin of its reference, when the bin
 *            before it is not kept, or when k or the bits of l differ from the bin before: the rule is on (k, l), not on v and not
 *            on the width.  A run is (ref, start0, end0, v), in header order.  totals: as pmx_dbam_coverage_signal's four.
 * Refused with PMX_DBAM_ERR_INVALID: a bin outside 1 .. 65536; a window above 2^31 - 1; n_lnfact <= max_depth_t (or lnfact NULL);
 * max_depth_t > 2^20; a_c below 2^-64, not finite, or a_c * max_depth_c >= 2^40; a control without a covered base.
 * The call waits for c's stream, then works on b's.  The runs are kept on b in the signal slot, marked as a p-score track until the
 * next signal, compare, poisson, begin or close, and all eight pmx_dbam_coverage_signal_* consumers and pmx_dbam_coverage_call serve
 * them; pmx_dbam_coverage_call_text on a p-score track writes the peak's value text in column 8 as well, in place of -1.  c is not
 * changed.  Inside the call 24 bytes per bin of every chosen reference (S_t, the inclusive u64 prefix sum of S_c, l), 12 per 256
 * bins, 8 per entry of F read and 20 per boundary of a run are held, counted towards pmx_dbam_stream_info's peak and freed before
 * the call returns; out of memory for the tables is PMX_DBAM_ERR_OPEN with the bytes asked for (B = 1 on a large genome: the table
 * is not tiled).  A failure leaves no signal. */
int pmx_dbam_coverage_poisson(pmx_dbam *b, pmx_dbam *c, uint32_t bin, double a_c, uint32_t small, uint32_t large, const double *lnfact,
                              uint64_t n_lnfact, double totals[4]);

/* Peaks called from the signal track (version >= 21): a threshold caller over the signal runs on the handle, the
 * result of pmx_dbam_coverage_signal or pmx_dbam_coverage_compare.  The definitions are this project's own; nothing here was
 * compared with MACS2.
 * The input.  The signal runs (ref, start0, end0, v), in header order; within a reference they ascend and do not overlap, and the
 * bases in no run are uncovered.  cutoff is a finite float64 (negative is legal), max_gap an integer 0 .. 2^31 - 1, min_length an
 * integer 1 .. 2^31 - 1: PMX_DBAM_ERR_INVALID otherwise.  Values compare as floats: f64(v) against cutoff and f64(v) against f64(v');
 * -0.0 equals 0.0.
 * Passing.  A run passes when f64(v) >= cutoff.  Equality passes.
 * Chains.  Take the passing runs of one reference in order.  Two consecutive passing runs a, b are linked when
 * b.start0 - a.end0 <= max_gap, whatever lies between them (failing runs or uncovered bases).  Runs of different references are never
 * linked.  A candidate is a maximal chain: its start is the first run's start0, its end the last run's end0.
 * Peaks.  A candidate is a peak when end - start >= min_length.  Peaks are in header order, then ascending.
 * Per peak.  value: the largest v of its passing runs, float32.  summit = s + (e - s) / 2 (integer division), where (s, e) is the
 * FIRST passing run with that value; the position is 0-based.  runs: the number of its passing runs.  Only integers, a maximum and a
 * first-argmax appear, so every reduction is associative and the result does not depend on scheduling; a mean or an area over the
 * peak would be a float sum in some order and is left out.
 * totals = passing runs, candidates, peaks, peak bases (end - start summed over the peaks), passing bases (the widths of the passing
 * runs inside peaks).
 * The narrowPeak line of peak number n, 1-based in file order (first + i + 1 of a pull), no header line:
 *   chrom TAB start TAB end TAB peak_<n> TAB score TAB . TAB value TAB -1 TAB -1 TAB (summit - start) LF
 * score = trunc(min(max(f64(value) * 10.0, 0.0), 1000.0)), the product exact in float64; value is written as the signal's text
 * writes it: six decimals, ties to even, '-' only when the rounded micro-count is not 0.  On a p-score track (the signal slot filled
 * by pmx_dbam_coverage_poisson, version >= 22) the first -1, column 8, is the value's text as well.
 * call without a signal on the handle is PMX_DBAM_ERR_INVALID (call signal or compare first).  The peak table (reference, start, end,
 * summit, value, runs: 24 bytes per peak) is kept on the handle, counted towards pmx_dbam_stream_info's peak, and dropped by the next
 * call, signal, compare, begin or close; call_rows and call_text after one of those are PMX_DBAM_ERR_INVALID.  The signal runs and
 * the depth runs are not changed.  Inside call 12 bytes per 256 signal runs and 4 per passing run, candidate and peak are held and
 * freed before it returns; a failure leaves no peak table and the signal as it was.  Refused: 2^32 signal runs or more.
 * call_rows copies the peaks [first, first + n); call_text formats their lines on the device (buf NULL: the size; a cap below it:
 * PMX_DBAM_ERR_INVALID), with the range rules of pmx_dbam_coverage_signal_runs / _text. */
int pmx_dbam_coverage_call(pmx_dbam *b, double cutoff, uint32_t max_gap, uint32_t min_length, uint64_t totals[5]);
int pmx_dbam_coverage_call_rows(pmx_dbam *b, int64_t first, int64_t n, int32_t *ref, uint32_t *start, uint32_t *end, uint32_t *summit,
                                float *value, uint32_t *runs);
int64_t pmx_dbam_coverage_call_text(pmx_dbam *b, int64_t first, int64_t n, uint8_t *buf, int64_t cap);

/* Benjamini-Hochberg q-scores for the p-score track (version >= 23): the correction over every base of the chosen
 * genome, made on the device from the runs pmx_dbam_coverage_poisson left in the signal slot.  The definitions are this project's own;
 * nothing here was compared with MACS2.  Everything is integer arithmetic or float64, and every float64 operation is rounded to nearest
 * even on its own (no fused multiply-add).
 *   input      The runs (ref, start0, end0, v) of a p-score track, v float32: +0.0 or the float32 of a positive number, so v >= 0 and
 *              never a NaN.  A track whose smallest value is negative is refused.
 *   tests      N = the sum of the lengths of the chosen references, u64 (the L of pmx_dbam_coverage_poisson's l_bg).  Every base of
 *              the chosen genome is one test; a base in no run has p = 1 and counts in N only.
 *   distinct   u_1 > u_2 > ... > u_m are the distinct values of the runs, compared as floats.  W_i = the sum of end0 - start0 over
 *              the runs with the value u_i, u64.
 *   rank       r_1 = 1, r_i = 1 + W_1 + ... + W_(i-1), u64.  r_i <= N always.
 *   raw score  x_i = f64(u_i) + (lg2(f64(r_i)) - lg2(f64(N))) * 0.3010299956639812, with lg2 the stated algorithm of
 *              pmx_dbam_coverage_compare.  r_i and N are below 2^53, so the conversions are exact.
 *   monotone   Q_i = max(0.0, min(x_1 .. x_i)) and q_i = f32(Q_i).  min and max are associative and exact and the sums are integers,
 *              so no result depends on scheduling or on the order of the sort.  q is non-increasing in i, hence non-decreasing in the
 *              p-score.
 *   table      m rows (u_i, W_i, q_i), descending in u.
 *   cutoff     pcut(X) for a finite float64 X: f64(u_i) of the largest i with f64(q_i) >= X, the smallest p-score whose q-score
 *              reaches X; 2^40 when no row reaches X (v < 2^40, so pmx_dbam_coverage_call then finds nothing); X <= 0 gives f64(u_m).
 *   lookup     The q-score of a peak is q_i of the row with u_i == its value.  A peak's value is the value of one of its runs, so the
 *              row exists: a miss is an internal error (PMX_DBAM_ERR_DEVICE), not a -1.
 * pmx_dbam_coverage_qvalue builds the table: totals = m, N, the covered bases (the sum of every W), the bases with q > 0.  The runs go
 * through one key pass, a stable radix sort over the 8-bit digits that differ, a u64 prefix sum, a compaction of the heads and a
 * prefix minimum.  PMX_DBAM_ERR_INVALID: no signal, a signal that is not a p-score track, 2^32 runs or more.  A track with 0 runs
 * gives an empty table and is legal.  The table (16 bytes per row) is kept on the handle beside the signal runs, counted towards
 * pmx_dbam_stream_info's peak, and dropped with them by the next signal, compare, poisson, begin or close; qvalue again replaces it.
 * qvalue drops a peak table that is there: call again.  Inside the call 40 bytes per run, 3072 per 8192 runs, 64, and 16 per row are
 * held besides, counted the same way and freed before it returns; out of memory is PMX_DBAM_ERR_OPEN with the bytes asked for.  A
 * failure leaves no table and the signal as it was.
 * qvalue_rows copies the rows [first, first + n) (p = u, bases = W, q), with the range rules of pmx_dbam_coverage_signal_runs.
 * qvalue_cutoff gives pcut(X) by a search on the device; a non-finite X is PMX_DBAM_ERR_INVALID.  Both without a table:
 * PMX_DBAM_ERR_INVALID.
 * While the handle holds a table, pmx_dbam_coverage_call_text writes the text of the peak's q-score in column 9, in place of the
 * second -1; column 8 is as above.  Without a table every byte is as above; call and call_rows are the same either way. */
int pmx_dbam_coverage_qvalue(pmx_dbam *b, uint64_t totals[4]);
int pmx_dbam_coverage_qvalue_rows(pmx_dbam *b, int64_t first, int64_t n, float *p, uint64_t *bases, float *q);
int pmx_dbam_coverage_qvalue_cutoff(pmx_dbam *b, double X, double *pcut);

/* A DEFLATE encoder on the device (version >= 18): independent chunks of at most PMX_DEFLATE_MAX_CHUNK bytes, each
 * turned into one complete zlib stream (RFC 1950 around RFC 1951): the header 0x78 with a 32-KB window and no dictionary, DEFLATE
 * blocks of which the last is marked final, the big-endian Adler-32 of the raw bytes.  Matches have length 4 .. 258 and distance
 * 1 .. 32768 (greedy parse, the nearest earlier position with the same four bytes); per chunk the smallest of one dynamic block
 * (code lengths of at most 15 bits built on the device, 7 for the code-length alphabet), one fixed block and stored blocks is
 * written, so a stream of n raw bytes is never longer than pmx_ddeflate_bound(n) = n + 5 * max(1, ceil(n / 65535)) + 6; n == 0 is
 * a valid stream.  The same bytes give the same stream on every call.  The streams decode to the raw bytes; they are not the bytes
 * zlib's own encoder writes.
 * pmx_ddeflate: all pointers are host pointers; chunk i is src[offsets[i], offsets[i + 1]) for i < n.  The n streams are written end
 * to end into dst[cap] and their lengths into sizes[n]; returns their total.  A NULL pointer, a negative n or cap, descending
 * offsets, a chunk above the maximum (all before any launch) and a cap below the total: PMX_DBAM_ERR_INVALID; out of device
 * memory: PMX_DBAM_ERR_OPEN with the bytes asked for.  Device memory: the raw bytes, 4 bytes of tokens per raw byte, a slot of
 * `bound` per chunk, then the streams.
 * sections_z / zoom_records_z: pmx_dbam_coverage_sections / _zoom_records with every section compressed before it leaves the device.
 * `table` is exactly what the raw call gives (column 4 stays the RAW size of the section, what uncompressBufSize needs);
 * zsizes[section] = the length of its stream, and buf holds the streams end to end.  With buf NULL the return value is an upper
 * bound of the bytes (the sum of the sections' bounds), with a buffer the bytes written; a cap below them is PMX_DBAM_ERR_INVALID.
 * A raw section must fit a chunk: more than 5459 items (sections_z) or 2048 items (zoom_records_z) is PMX_DBAM_ERR_INVALID.
 * The scratch counts towards pmx_dbam_stream_info's peak and is freed with the call; pulling the last level frees the bins. */
#define PMX_DEFLATE_MAX_CHUNK 65536u
uint64_t pmx_ddeflate_bound(uint64_t n);
int64_t pmx_ddeflate(int device, const uint8_t *src, const uint64_t *offsets, int64_t n, uint8_t *dst, int64_t cap, uint32_t *sizes);
int64_t pmx_dbam_coverage_sections_z(pmx_dbam *b, int64_t first, int64_t n, uint32_t chrom_id, uint32_t items, uint8_t *buf, int64_t cap,
                                     uint32_t *table, int64_t table_cap, uint32_t *zsizes);
int64_t pmx_dbam_coverage_zoom_records_z(pmx_dbam *b, uint32_t level, uint32_t items, uint8_t *buf, int64_t cap, uint32_t *table,
                                         int64_t table_cap, uint32_t *zsizes);

/* Counters: alignment records walked and records kept by the last decode, uncompressed / compressed bytes of the file,
 * BGZF members, and how many 16-KB pieces had to be walked again because their guessed first record was wrong.  An indexed
 * handle: bytes_out is the length of its stream (header + selected records), bytes_in and members count only the members
 * that were read (the header's and the selected references', each once). */
int pmx_dbam_counters(const pmx_dbam *b, uint64_t *records, uint64_t *kept, uint64_t *bytes_out, uint64_t *bytes_in,
                      uint64_t *members, uint64_t *rewalked);
/* Wall-clock seconds of the phases of open + the last decode: [0] file -> HBM (read + copies + member scan), [1] inflate,
 * [2] CRC32, [3] header, [4] record chain (guess + walk + verification), [5] filter + field extraction + write. */
int pmx_dbam_timings(const pmx_dbam *b, double t[6]);

/* Test hook: the inflated stream (bytes [first, first + n)) copied to the host. */
int pmx_dbam_inflated(pmx_dbam *b, uint64_t first, uint64_t n, uint8_t *dst);

/* ---- BigWig (bbi) on the device -----------------------------------------------------------
 * What pmx_bigwig_open / pmx_track_fetch (pymasc_amd_io.h) do with zlib on host threads, with the data blocks inflated (the
 * BGZF kernel, for zlib streams of unknown length), Adler-32-checked and decoded by HIP kernels; the host reads the header, the chromosome B+ tree and
 * the R-tree (a few KB per chromosome).  Replaces PyMaSC/reader/bigwig.pyx:129-177 (pyBigWig). */
typedef struct pmx_dbw pmx_dbw;
int pmx_dbw_open(const char *path, int device, int nthreads, pmx_dbw **out);
void pmx_dbw_close(pmx_dbw *w);
/* Chromosome dictionary = BigWigReader.chromsizes (reader/bigwig.pyx:60-75), in the file's B+ tree order. */
int32_t pmx_dbw_nchrom(const pmx_dbw *w);
const char *pmx_dbw_chrom_name(const pmx_dbw *w, int32_t i);
int64_t pmx_dbw_chrom_len(const pmx_dbw *w, int32_t i);
/* All intervals of `chrom` in index order (ascending position for a valid file) whose float32 value is >= threshold
 * (threshold <= 0: every interval), as BigWigReader.fetch yields them (bigwig.pyx:147-177) -- the intervals, values and order
 * of pmx_track_fetch.  They stay in device memory (begin[n], end[n] uint32, value[n] float32; every fetch has arrays of its own,
 * valid until close).  Returns n, PMX_DBAM_ERR_NOTFOUND for an unknown chromosome, or another negative error code. */
int64_t pmx_dbw_fetch(pmx_dbw *w, const char *chrom, float threshold);
int pmx_dbw_device_arrays(const pmx_dbw *w, const uint32_t **d_begin, const uint32_t **d_end, const float **d_value);
/* 1 when the intervals of the last fetch are non-empty, ascending and disjoint (begin_i < end_i <= begin_(i+1): BigWig order) */
int pmx_dbw_sorted(const pmx_dbw *w);
int pmx_dbw_copy(pmx_dbw *w, int64_t first, int64_t n, uint32_t *begin, uint32_t *end, float *value);
/* bigBed on the device (version >= 7): pmx_dbw_open also takes a bigBed file, read by the rules of pmx_bigwig_open
 * (pymasc_amd_io.h, its checker).  Its blocks are inflated and Adler-32-checked as a BigWig's; k_bb_records walks each block's
 * record chain (one wavefront per block) and writes [chromStart, chromEnd) with value 1.0.  pmx_dbw_kind: 0 BigWig (or a text
 * track), 1 bigBed, 2 a k-mer track of pmx_dkm_open (version >= 8). */
int pmx_dbw_kind(const pmx_dbw *w);

/* Text tracks on the device (version >= 5): `path` is a bedGraph, BED or WIG file, plain, BGZF or gzip, read by
 * the rules of pmx_ttrack_open (pymasc_amd_io.h, its checker).  Plain text is copied to HBM through the staging buffers; BGZF goes
 * through the member scan, k_bgzf_inflate and k_bgzf_crc; other gzip is inflated on the host with zlib (one DEFLATE stream
 * cannot be split) and copied.  k_sam_count / k_bam_scan / k_sam_lines index the lines, k_tt_parse parses one line per lane
 * (values by Clinger's fast path; the rest re-parsed with strtod on the host), WIG lines find their declaration by a scan over the
 * line table, and the lines are put into per-chromosome order on the device.  A malformed line: PMX_DBAM_ERR_FORMAT with
 * pmx_ttrack_open's message.  The handle is a pmx_dbw: nchrom / chrom_name / chrom_len (the chromosomes with lines, in the order
 * of their first line; chrom_len = the largest end), fetch (the lines of a chromosome with value >= threshold, in file order),
 * device_arrays, sorted, copy and close work on it. */
int pmx_dtt_open(const char *path, int device, int nthreads, pmx_dbw **out);

/* BED read files on the device (version >= 6): `path` is a tagAlign / BED6 file with one read per line, plain,
 * BGZF or gzip, read by the rules of pmx_bed_open (pymasc_amd_io.h, its checker) with the nref chromosome sizes given (their
 * order is the reference order).  The text reaches HBM as a text track's does (pmx_dtt_open); k_sam_count / k_bam_scan /
 * k_sam_lines index the lines, k_bed_parse parses one line per lane into the SAM parse table, and a file that is not in
 * (reference, start) order is put in it by a stable LSD radix sort of the keys ref << 31 | start on the device (passes whose
 * digit is the same in every key skipped), ties in file order.  A malformed line: PMX_DBAM_ERR_FORMAT with pmx_bed_open's
 * message.  The handle is a pmx_dbam: nref / ref_name / ref_len (the sizes), header_text (empty), decode, device_arrays, fetch,
 * runs, readlen_hist (first-occurrence keys: byte offsets of lines in the text), readlen_counters, counters (members 0) and
 * timings work on it; pmx_dbam_select is PMX_DBAM_ERR_INVALID. */
int pmx_dbed_open(const char *path, int device, int nthreads, int32_t nref, const char *const *names, const int64_t *lengths,
                  pmx_dbam **out);

/* The k-mer uniqueness track of a genome FASTA on the device (version >= 8): `path` is a FASTA file, plain, BGZF
 * or gzip, read by the rules of pmx_kmer_open (pymasc_amd_io.h, its checker), and the track is pmx_kmer_open's, interval for
 * interval.  The text reaches HBM as a text track's does (pmx_dtt_open) and is indexed by k_sam_count / k_bam_scan / k_sam_lines;
 * k_fa_class / k_fa_list / k_fa_pack pack the genome at 2 bits and a valid bit per position and the text is freed.  One lane per
 * position hashes its k-mer strand-symmetrically (h = min(H(F), H(R)), any k in [16, 1024]; no k-mer or a palindrome: never
 * unique, never sorted).  A histogram of the top 16 kept hash bits plans passes of at most budget_bytes / 24 k-mers (0: half of
 * the free device memory less 4 GiB); each pass recomputes the hashes of its bins and LSD-radix-sorts (hash, position) with a
 * multi-workgroup scan.  A run of equal hashes of one element is unique; in a longer run every element is compared with the
 * run's first (a segmented max-scan finds it); a run with a mismatch is resolved exactly on the host by sorting the canonical
 * packed k-mers of its elements.  hash_bits < 64 keeps only the low bits of the hash (a test knob that forces collisions).
 * The handle is a pmx_dbw: nchrom / chrom_name / chrom_len (every record in file order, its length in bases), fetch (the
 * record's unique runs, value 1.0; none above threshold 1), device_arrays, sorted, copy and close work on it; only the intervals
 * (12 bytes each) stay in device memory.  k outside [16, 1024], hash_bits outside [1, 64]: PMX_DBAM_ERR_INVALID; a malformed
 * file: PMX_DBAM_ERR_FORMAT with pmx_kmer_open's message; one hash bin larger than the budget: PMX_DBAM_ERR_OPEN. */
int pmx_dkm_open(const char *path, int32_t k, int device, int nthreads, int64_t budget_bytes, int32_t hash_bits, pmx_dbw **out);

/* GC bias (version >= 14): the reads against the genome's windows, per G + C content of the window.
 * The genome handle: pmx_dgc_open is the first stage of pmx_dkm_open and nothing else -- the FASTA (plain, BGZF, gzip) reaches HBM
 * and is packed at 2 bits and a valid bit per position, with pmx_dkm_open's rules and error messages ("line N: <reason>", 2^32
 * bases) -- and the handle keeps the packed genome with the records' names, lengths and first positions, in file order. */
typedef struct pmx_dgc pmx_dgc;
int pmx_dgc_open(const char *path, int device, int nthreads, pmx_dgc **out);
void pmx_dgc_close(pmx_dgc *g);
int32_t pmx_dgc_nrec(const pmx_dgc *g);
const char *pmx_dgc_rec_name(const pmx_dgc *g, int32_t i);
int64_t pmx_dgc_rec_len(const pmx_dgc *g, int32_t i);
/* The window: W = `window`, 1 <= W <= 1024.  A chosen reference of length len has a window at every 1-based start s with
 * s + W - 1 <= len, covering [s, s + W - 1].  A window is BLOCKED when any of its positions is not A C G T (either case) or lies
 * inside a merged interval of the handle's attached mask (pmx_dbam_set_exclude: excluded regions act as runs of N).  g(s) = the
 * G / C among the W bases of an unblocked window, an integer in 0 .. W.  N[g] = the unblocked windows of the chosen references
 * with that g.
 * The reads are pmx_dbam_bincount_add's (mapq_min / flag_exclude, the chosen references, less the reads an attached mask leaves
 * out; reads on other references are ignored entirely).  A forward read is placed at s = pos1, a reverse read at
 * s = pos1 + read_len - W (its window ends on its 5' base; it is not clipped).  s < 1 or s + W - 1 > len: the read counts in
 * off_end; otherwise, a blocked window: in blocked; otherwise F[g(s)] += 1.
 * pmx_dbam_gcbias_begin matches every chosen reference (use_ref[nref], NULL: all) to the record of the same name, which must
 * have the same length (the FASTA's order is free, other records are ignored; the first reference without one:
 * PMX_DBAM_ERR_INVALID, named); builds a GC bit and a blocked bit per position of the chosen references, laid end to end with one
 * blocked separator behind each (0.25 bytes per chosen base, about 0.78 GB for hg38; part of pmx_dbam_stream_info's peak);
 * computes N and zeroes F and the counters.  The genome is not referenced after begin returns: it may be closed, and one genome
 * serves any number of handles.  The table replaces any earlier one and stays until the next begin or close; a mask attached
 * later does not change it.  A chosen reference shorter than W has no windows, and all its reads are off_end.
 * pmx_dbam_gcbias_add counts what the handle holds now (the arrays, counters and runs of the last pmx_dbam_decode stay
 * untouched); out = {reads placed, off_end, blocked} of this call.  Calls add up in F (the windows of a stream); N never changes.
 * pmx_dbam_gcbias_tables returns W + 1 and, with cap >= W + 1, fills windows[] = N and reads[] = F; totals = {sum N, sum F,
 * off_end, blocked} since begin.
 * add / tables without begin, a NULL output, window 0 or above 1024, a genome on another device, no chosen reference:
 * PMX_DBAM_ERR_INVALID. */
int pmx_dbam_gcbias_begin(pmx_dbam *b, const pmx_dgc *genome, uint32_t window, const uint8_t *use_ref);
int pmx_dbam_gcbias_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t out[3]);
int64_t pmx_dbam_gcbias_tables(pmx_dbam *b, uint64_t *windows, uint64_t *reads, int64_t cap, uint64_t totals[4]);

/* Paired-end fragment sizes and the pair pileup (version >= 15).  A pair is counted at its read1 record, from that
 * record's own fields (flag, next_refID / RNEXT, next_pos / PNEXT, tlen / TLEN): nothing is matched, nothing is held back between
 * a stream's windows.
 * The pair rule.  A record that passes mapq_min / flag_exclude with ref_id >= 0, a query length > 0 and a chosen reference counts
 * in `reads`; with flag 0x1 also in `paired`, and then in exactly one of (the first that holds): mate_unmapped (flag 0x8);
 * mate_elsewhere (BAM: next_refID != refID; SAM: RNEXT is neither '=' nor byte-equal to RNAME); no_size (tlen 0 or -2^31, or
 * mate_pos1 = next_pos + 1 = PNEXT <= 0); else it is a fragment of size = |tlen|, start1 = min(pos1, mate_pos1) and orientation
 * TANDEM (2) when bits 0x10 and 0x20 agree, FR (0) when the read is forward and tlen > 0 or reverse and tlen < 0, RF (1) otherwise.
 * size > max_size: over[orientation], and no further.  Otherwise a row (ref_id, start1, size, orientation), counted in `rows`; an
 * attached mask (pmx_dbam_set_exclude) drops the rows whose extent [start1, start1 + size - 1] overlaps a region: `masked`.
 * H[o][s - 1] = the rows left of orientation o and size s.  paired = mate_unmapped + mate_elsewhere + no_size + sum(over) + rows;
 * rows - masked = sum(H).
 * pmx_dbam_fragments_begin allocates and zeroes H (8 * 3 * max_size bytes) and the counters, 1 <= max_size <= 65536; use_ref[nref]
 * chooses references (NULL: all).  They stay until the next begin or close.  pmx_dbam_fragments_add counts what the handle holds
 * now (the arrays of the last pmx_dbam_decode stay untouched); *rows_added = the rows it added to H.  pmx_dbam_fragments_tables
 * copies H (3 * max_size, [o][s - 1]) and the counters since begin.
 * pmx_dbam_fragments_rows: the rows of what the handle holds now, after the mask, in record order; cap 0 returns their number, a
 * cap >= it fills the arrays and returns it.
 * pmx_dbam_coverage_add_fragments: between pmx_dbam_coverage_begin(b, 0, use_ref) and _finish, marks the FR rows at their own
 * extent (clipped to the reference as a read's is); *added = the rows marked.
 * A SAM handle parses PNEXT and TLEN the first time one of these is called: a field that is not a decimal integer (TLEN may be
 * signed) is PMX_DBAM_ERR_FORMAT, "line N: <reason>".  A BED read handle: PMX_DBAM_ERR_INVALID, "the input has no mate fields".
 * add / tables before begin, max_size out of range, a NULL output: PMX_DBAM_ERR_INVALID. */
#define PMX_FRAGMENTS_MAX_SIZE 65536u
#define PMX_FRAGMENTS_COUNTERS 10   /* reads, paired, mate_unmapped, mate_elsewhere, no_size, over FR / RF / TANDEM, rows, masked */
int pmx_dbam_fragments_begin(pmx_dbam *b, uint32_t max_size, const uint8_t *use_ref);
int pmx_dbam_fragments_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t *rows_added);
int pmx_dbam_fragments_tables(pmx_dbam *b, uint64_t *hist, uint64_t counters[PMX_FRAGMENTS_COUNTERS]);
/* seconds = {the row filter of the adds since begin (wall clock: walk, scan, write, mask), k_fr_hist of them (HIP events)} */
int pmx_dbam_fragments_timings(pmx_dbam *b, double seconds[2]);
int64_t pmx_dbam_fragments_rows(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint32_t max_size, const uint8_t *use_ref,
                                int64_t cap, int32_t *ref_id, int32_t *start1, int32_t *size, uint8_t *orient);
int pmx_dbam_coverage_add_fragments(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint32_t max_size, uint64_t *added);

/* The strand-aware read profile around anchor sites (version >= 16): TSS enrichment's counts.  An anchor is
 * (reference, a, s): a 1-based position a and a strand s (+ or -).  Anchors may repeat, and each counts separately.  The reads are
 * pmx_dbam_bincount_add's (the filter, the chosen references, less the reads an attached exclude mask drops); N is their number.  A
 * read's extent [lo, hi] is pmx_dbam_bincount's with `extend` (0: the read's own length; 1: its 5' base only), clipped to [1, len].
 * With the flank F (1 .. PMX_TSS_MAX_FLANK) and W = 2F + 1, a read on an anchor's reference covers, for that anchor, the offsets
 * o = s * (p - a) for p in [lo, hi] with |o| <= F.  For every such o, same[o + F] += 1 when the read's strand equals the anchor's,
 * opposite[o + F] += 1 otherwise.  pairs = the (read, anchor) pairs with at least one such offset; n_near = the reads in at least
 * one pair, once each.
 * pmx_dbam_tss_begin takes n anchors in host memory (ref[] the reference's index, pos1[] = a, reverse[] non-zero for a - anchor),
 * in any order.  A reference outside the header, a < 1, a beyond its reference's length, F outside 1 .. PMX_TSS_MAX_FLANK or more
 * than PMX_TSS_MAX_ANCHORS anchors: PMX_DBAM_ERR_INVALID, and the handle holds no table of this family.  use_ref: nref bytes, 0 =
 * reads of that reference are not counted and its anchors are dropped; NULL = every reference.  The kept anchors are sorted by
 * (reference, a) on the device (12 bytes each) beside a zeroed table of signed 64-bit differences [2][W + 1] (part of
 * pmx_dbam_stream_info's peak); they replace any earlier table and stay until the next begin or close.
 * pmx_dbam_tss_add counts what the handle holds now, as pmx_dbam_peakcount_add does; calls add up.  out = {N, n_near} of this call.
 * pmx_dbam_tss_copy: profile[0 .. W) = same, profile[W .. 2W) = opposite: the prefix sums of the differences.  A negative sum or a
 * row that does not close at 0: PMX_DBAM_ERR_DEVICE, and nothing is written.
 * pmx_dbam_tss_totals: totals = {N, n_near, anchors kept, pairs} since begin.
 * add / copy / totals before begin and a NULL output: PMX_DBAM_ERR_INVALID. */
#define PMX_TSS_MAX_FLANK 4095u
#define PMX_TSS_MAX_ANCHORS (1u << 20)
int pmx_dbam_tss_begin(pmx_dbam *b, int64_t n, const int32_t *ref, const uint32_t *pos1, const uint8_t *reverse, uint32_t flank,
                       uint32_t extend, const uint8_t *use_ref);
int pmx_dbam_tss_add(pmx_dbam *b, uint32_t mapq_min, uint32_t flag_exclude, uint64_t out[2]);
int pmx_dbam_tss_copy(pmx_dbam *b, uint64_t *profile);
int pmx_dbam_tss_totals(pmx_dbam *b, uint64_t totals[4]);

#ifdef __cplusplus
}
#endif
#endif
