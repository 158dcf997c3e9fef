// Windowed stream reading (pmx_dbam_open_stream / pmx_dbam_stream_next, include/pymasc_amd_ingest.h; DESIGN.md 7.9).  Included
// at the end of bam_device.hip, after sam_device.inc: a stream handle is a pmx_dbam whose stream is the CURRENT WINDOW, so
// decode / fetch / runs / readlen_hist / counters work on it unchanged.
//
//   host     a reader thread fills one of two page-locked buffers from the fd (read(2): a pipe, a FIFO, a socket or a file,
//            never seeked or sized) while the window before is inflated, decoded and fed; the member scan takes whole BGZF
//            members up to window_bytes compressed and 4 * window_bytes inflated (ISIZE is read before anything is inflated)
//   device   the carried tail of the last window is copied to the front of the other window buffer, the members are inflated
//            and CRC-checked behind it (k_bgzf_inflate / k_bgzf_crc, as the whole-file open does), and the record chain
//            (k_bam_spec / k_bam_walk) finds where the last whole record ends: a record that runs past the window's end is
//            no error here but the CARRY point.  SAM text is cut after the window's last '\n'.
// Buffers are allocated for the window budget once and grow only for a record (or line) longer than a window: the device
// bytes depend on window_bytes, never on the length of the input.

namespace {

constexpr u64 STREAM_DEFAULT_WINDOW = 64ull << 20;
constexpr u64 STREAM_MEMBER_MAX = 65536 + 64;   // the bytes of the largest BGZF member (BSIZE + 1 <= 65536) and some
enum { SFMT_UNKNOWN = 0, SFMT_BAM = 1, SFMT_SAM = 2, SFMT_SAM_BGZF = 3 };

struct StreamState {
    int fd = -1;
    u64 window = 0, infl = 0, target = 0;
    int fmt = SFMT_UNKNOWN;
    bool gz = false, header = false, primed = false, done = false;
    // host: two page-locked buffers; the reader thread fills hb[1 - hcur] while hb[hcur] is taken
    u8 *hb[2] = {nullptr, nullptr};
    int hcur = 1;
    u64 hlen = 0;
    bool eof = false;
    std::thread reader;
    bool reading = false;
    u64 rd_len = 0;
    bool rd_eof = false;
    int rd_errno = 0;
    // device: two window buffers (tail + this window's output), the compressed members, their table and status
    u8 *d_win[2] = {nullptr, nullptr};
    u64 wcap[2] = {0, 0};
    int wcur = 0;
    u64 full = 0;          // bytes in d_win[wcur]: the carried tail + this window's output
    u64 base = 0;          // offset of d_win[wcur][0] in the whole inflated stream
    u64 in_cap = 0, mcap = 0;
    DMember *d_mem = nullptr;
    u32 *d_st = nullptr;
    std::vector<DMember> mem;
    samtext::Header sh;
    u64 sam_hdr_lines = 0, lines_before = 0;
    // stream_info
    u64 windows = 0, bytes_in = 0, max_tail = 0, peak = 0;
    // pmx_dbam_complexity (complexity_device.inc): the kept records of the last counted window's last (ref_id, pos1), counted with
    // the next window; the window counted last; whether pmx_dbam_stream_next has reported the end
    int *cx_ref = nullptr, *cx_pos = nullptr, *cx_len = nullptr;
    u8 *cx_rev = nullptr;
    u64 cx_n = 0, cx_window = ~0ull;
    bool cx_end = false;
};

// len bytes (or until the end of the stream) into hb[x] behind `have` bytes already there
void stream_fill(StreamState *s, int x, u64 have)
{
    u64 len = have;
    bool eof = false;
    int err = 0;
    while (len < s->target) {
        const ssize_t r = read(s->fd, s->hb[x] + len, (size_t)(s->target - len));
        if (r < 0) {
            if (errno == EINTR) continue;
            err = errno;
            break;
        }
        if (r == 0) {
            eof = true;
            break;
        }
        len += (u64)r;
    }
    s->rd_len = len;
    s->rd_eof = eof;
    s->rd_errno = err;
}

void stream_join(StreamState *s)
{
    if (s->reading) {
        s->reader.join();
        s->reading = false;
    }
}

// the bytes of device memory the handle holds now
u64 stream_held(const pmx_dbam &b)
{
    const StreamState *s = b.st;
    u64 h = s->wcap[0] + s->wcap[1] + s->in_cap + s->mcap * (sizeof(DMember) + 4);
    if (b.d_spec) h += b.chain_cap * 32 + 28;
    h += b.out_cap * 13;
    if (b.d_rl) h += 8 * (2u * RL_SHORT + RL_NCNT + 1u);
    if (b.sam) h += b.sam_lines * 24 + b.sam_nb_cap * 12 + 16;
    h += s->cx_n * 13;
    h += b.bc.held() + b.pk.held() + b.cv.held() + b.gc.held() + b.fr.held() + b.ts.held();
    h += b.d_smpos ? b.sam_lines * 9 : 0;
    return h;
}
void stream_note(pmx_dbam &b) { b.st->peak = std::max(b.st->peak, stream_held(b)); }

int dev_grow(u8 *&p, u64 &cap, u64 need, hipStream_t st, u64 keep)
{
    if (need <= cap) return 0;
    const u64 c = std::max<u64>(need, cap + cap / 2);
    u8 *q = nullptr;
    HIPOK(hipMalloc((void **)&q, c));
    if (p) {
        if (keep) HIPOK(hipMemcpyAsync(q, p, keep, hipMemcpyDeviceToDevice, st));
        HIPOK(hipStreamSynchronize(st));
        HIPOK(hipFree(p));
    }
    p = q;
    cap = c;
    return 0;
}

// Where the last whole BAM record of d_out[data_beg, full) ends: the record chain over the window, with a write pass that keeps
// nothing (mapq_min 256) and so only reports the first record that is malformed or runs past the end.  The verified chain stays
// for decode / readlen_hist over [data_beg, carry).
int stream_carry_bam(pmx_dbam &b, u64 full, u64 &carry)
{
    const u64 beg = b.data_beg;
    carry = beg;
    if (full <= beg) return 0;
    b.N = full;
    b.npieces = (full - beg + WALK_PIECE - 1) / WALK_PIECE;
    b.respec = true;
    b.chain_ready = false;
    WalkArgs A;
    A.D = b.d_out + beg;
    A.N = full - beg;
    A.nref = (int)b.ref_names.size();
    A.mapq_min = 256;
    A.flag_exclude = 0;
    A.want_ref = -1;
    A.o_ref = A.o_pos = A.o_len = nullptr;
    A.o_rev = nullptr;
    if (int rc = walk_chain(&b, A)) return rc;
    HIPOK(hipMemsetAsync(b.d_first_error, 0xff, 8, b.stream));
    hipLaunchKernelGGL(k_bam_walk<2>, dim3((unsigned)((b.npieces + 63) / 64)), dim3(64), 0, b.stream, A);
    HIPOK(hipGetLastError());
    unsigned long long fe = 0;
    HIPOK(hipMemcpyAsync(&fe, b.d_first_error, 8, hipMemcpyDeviceToHost, b.stream));
    HIPOK(hipStreamSynchronize(b.stream));
    // (the chain before the first bad record is exact; pieces behind it lie inside that record, so its offset is the minimum)
    if (fe == ~0ull) carry = full;
    else if ((fe & 15ull) == REC_ERR_EOF) carry = beg + (fe >> 4);
    else return record_error(fe);
    return 0;
}

// behind the last '\n' of d_out[data_beg, full), or data_beg when there is none
int stream_carry_sam(pmx_dbam &b, u64 full, u64 &carry)
{
    carry = b.data_beg;
    std::vector<u8> h;
    for (u64 hi = full; hi > b.data_beg;) {
        const u64 lo = hi - std::min<u64>(hi - b.data_beg, 65536);
        h.resize(hi - lo);
        HIPOK(hipMemcpy(h.data(), b.d_out + lo, hi - lo, hipMemcpyDeviceToHost));
        for (u64 i = hi - lo; i-- > 0;)
            if (h[i] == '\n') {
                carry = lo + i + 1;
                return 0;
            }
        hi = lo;
    }
    return 0;
}

void sam_free_table(pmx_dbam &b)
{
    for (void *p : {(void *)b.d_nl, (void *)b.d_sref, (void *)b.d_spos, (void *)b.d_sqlen, (void *)b.d_sfm, (void *)b.d_smpos,
                    (void *)b.d_stlen, (void *)b.d_ssame})
        if (p) (void)hipFree(p);
    b.d_smpos = b.d_stlen = nullptr;
    b.d_ssame = nullptr;
    b.d_nl = nullptr;
    b.d_sref = b.d_spos = nullptr;
    b.d_sqlen = b.d_sfm = nullptr;
    b.sam_lines = 0;
}

// Makes the next window current: > 0 its record bytes, 0 at the end of the stream, or an error code.
int64_t stream_advance(pmx_dbam &b)
{
    StreamState *s = b.st;
    if (s->done) return 0;
    // what is left of the last window: its tail [N, full) moves to the front of the next window buffer
    u64 tail_at = b.N, tail = s->full - b.N;
    if (!s->header) tail_at = 0, tail = s->full;   // (no header yet: everything so far is kept)
    for (;;) {
        // 1. the bytes the reader thread has read
        stream_join(s);
        s->hcur = 1 - s->hcur;
        s->hlen = s->rd_len;
        s->eof = s->rd_eof;
        if (s->rd_errno) return fail(PMX_DBAM_ERR_OPEN, std::string("read error on the input stream: ") + strerror(s->rd_errno));
        u8 *H = s->hb[s->hcur];
        if (s->fmt == SFMT_UNKNOWN && !s->gz && s->windows == 0 && s->full == 0) {   // the first bytes decide
            if (s->hlen == 0) return fail(PMX_DBAM_ERR_FORMAT, "truncated BGZF block header");
            if (H[0] == 0x1f && s->hlen >= 2 && H[1] == 0x8b) {
                if (s->hlen < 4 || H[2] != 8 || !(H[3] & 4))
                    return fail(PMX_DBAM_ERR_FORMAT, "gzip-compressed input that is not BGZF: recompress it with bgzip");
                s->gz = true;
            } else if (H[0] == '@') {
                s->fmt = SFMT_SAM;
            } else {
                return fail(PMX_DBAM_ERR_FORMAT, "not a BGZF block (bad gzip magic / no extra field)");
            }
        }
        // 2. what this window takes: whole members within both budgets (at least one), or the raw text
        s->mem.clear();
        u64 p = 0, isum = 0;
        if (s->gz) {
            while (p < s->hlen) {
                FileMember m;
                const char *err = parse_member(H + p, s->hlen - p, m);
                if (err) {
                    if (!s->eof && strncmp(err, "truncated", 9) == 0) break;
                    char where[64];
                    snprintf(where, sizeof where, " (stream offset %llu)", (unsigned long long)(s->bytes_in + p));
                    return fail(PMX_DBAM_ERR_FORMAT, std::string(err) + where);
                }
                if (!s->mem.empty() && (p + m.total > s->window || isum + m.isize > s->infl)) break;
                DMember d;
                d.in_off = p + m.hlen;
                d.clen = m.total - m.hlen - 8;
                d.isize = m.isize;
                d.crc = m.crc;
                d.out_off = tail + isum;
                d.open_size = 0;
                s->mem.push_back(d);
                isum += m.isize;
                p += m.total;
            }
        } else {
            p = isum = s->hlen;
        }
        const bool last = s->eof && p == s->hlen;   // nothing more will come after this window
        // 3. the next window buffer: the tail in front, then room for this window's output
        const int nw = 1 - s->wcur;
        if (int rc = dev_grow(s->d_win[nw], s->wcap[nw], tail + isum + 64, b.stream, 0)) return rc;
        if (tail) HIPOK(hipMemcpyAsync(s->d_win[nw], s->d_win[s->wcur] + tail_at, tail, hipMemcpyDeviceToDevice, b.stream));
        const double t0 = now_s();
        if (s->gz) {
            const u32 n = (u32)s->mem.size();
            if (int rc = dev_grow(b.d_in, s->in_cap, p + IN_PAD, b.stream, 0)) return rc;
            if (n > s->mcap) {
                if (s->d_mem) HIPOK(hipFree(s->d_mem));
                if (s->d_st) HIPOK(hipFree(s->d_st));
                s->d_mem = nullptr;
                s->d_st = nullptr;
                s->mcap = 0;
                HIPOK(hipMalloc((void **)&s->d_mem, sizeof(DMember) * n));
                HIPOK(hipMalloc((void **)&s->d_st, 4 * (u64)n));
                s->mcap = n;
            }
            if (p) HIPOK(hipMemcpyAsync(b.d_in, H, p, hipMemcpyHostToDevice, b.stream));
            HIPOK(hipMemsetAsync(b.d_in + p, 0, IN_PAD, b.stream));
            if (n) {
                HIPOK(hipMemcpyAsync(s->d_mem, s->mem.data(), sizeof(DMember) * n, hipMemcpyHostToDevice, b.stream));
                HIPOK(hipMemsetAsync(s->d_st, 0, 4 * (u64)n, b.stream));
                hipLaunchKernelGGL(k_bgzf_inflate, dim3(n), dim3(64), 0, b.stream, b.d_in, s->d_win[nw], s->d_mem, n, s->d_st, (u32 *)nullptr);
                HIPOK(hipGetLastError());
                hipLaunchKernelGGL(k_bgzf_crc, dim3((n + 3) / 4), dim3(256), 0, b.stream, s->d_win[nw], s->d_mem, n, s->d_st);
                HIPOK(hipGetLastError());
            }
        } else if (p) {
            HIPOK(hipMemcpyAsync(s->d_win[nw] + tail, H, p, hipMemcpyHostToDevice, b.stream));
        }
        HIPOK(hipMemsetAsync(s->d_win[nw] + tail + isum, 0, 64, b.stream));
        // 4. the bytes not taken go to the front of the other host buffer, and the reader thread fills it behind them while
        //    this window is inflated, decoded and fed (hb[hcur] is not written again before the copies above are waited for)
        const u64 rest = s->hlen - p;
        if (rest) memcpy(s->hb[1 - s->hcur], H + p, rest);
        s->bytes_in += p;
        b.members_read += s->mem.size();
        if (s->eof) {
            s->rd_len = rest;
            s->rd_eof = true;
            s->rd_errno = 0;
        } else {
            s->reader = std::thread(stream_fill, s, 1 - s->hcur, rest);
            s->reading = true;
        }
        std::vector<u32> status(s->mem.size());
        if (!status.empty()) HIPOK(hipMemcpyAsync(status.data(), s->d_st, 4 * status.size(), hipMemcpyDeviceToHost, b.stream));
        HIPOK(hipStreamSynchronize(b.stream));
        b.t[1] = now_s() - t0;
        for (size_t i = 0; i < status.size(); i++)
            if (status[i]) return fail(PMX_DBAM_ERR_FORMAT, std::string(inf_err_text(status[i])) + " (in a member of the input stream)");
        s->base += tail_at;
        b.stream_base = s->base;
        s->wcur = nw;
        s->full = tail + isum;
        b.d_out = s->d_win[nw];
        b.N = s->full;
        b.bytes_read = s->bytes_in;
        // 5. the header, from the first window(s)
        if (!s->header) {
            if (s->fmt == SFMT_UNKNOWN) {
                if (s->full < 4 && !last) {
                    tail_at = 0, tail = s->full;
                    continue;
                }
                u8 mg[4] = {0, 0, 0, 0};
                HIPOK(hipMemcpy(mg, b.d_out, std::min<u64>(4, s->full), hipMemcpyDeviceToHost));
                s->fmt = mg[0] == '@' ? SFMT_SAM_BGZF : SFMT_BAM;
            }
            b.sam = s->fmt != SFMT_BAM;
            int rc;
            if (s->fmt == SFMT_BAM) {
                rc = parse_header(b, !last);
            } else {
                rc = 1;
                std::vector<u8> pre;
                for (u64 L = std::min<u64>(s->full, 1u << 20);; L = std::min<u64>(s->full, 2 * L)) {
                    pre.resize(L);
                    if (L) HIPOK(hipMemcpy(pre.data(), b.d_out, L, hipMemcpyDeviceToHost));
                    std::string err;
                    s->sh = samtext::Header();
                    rc = samtext::parse_header((const char *)pre.data(), L, L == s->full && last, s->sh, err);
                    if (rc < 0) return fail(PMX_DBAM_ERR_FORMAT, err);
                    if (rc == 0 || L == s->full) break;
                }
                if (rc == 0) {
                    b.text = s->sh.text;
                    b.ref_names = s->sh.names;
                    b.ref_lens = s->sh.lens;
                    b.data_beg = s->sh.data_beg;
                    b.sam_hdr_lines = s->sam_hdr_lines = s->sh.lines;
                }
            }
            if (rc < 0) return rc;
            if (rc == 1) {   // the header runs past what was read: read more
                tail_at = 0, tail = s->full;
                continue;
            }
            s->header = true;
        } else {
            b.data_beg = 0;
        }
        // 6. the carry point
        u64 carry = b.data_beg;
        b.rl_valid = false;
        b.n_kept = b.n_records = 0;
        if (b.sam) {
            sam_free_table(b);
            if (int rc = stream_carry_sam(b, s->full, carry)) return rc;
            if (last) carry = s->full;   // (the last line may go without its '\n')
        } else {
            if (int rc = stream_carry_bam(b, s->full, carry)) return rc;
            if (last && carry < s->full) {
                b.N = b.data_beg;
                b.npieces = 0;
                return fail(PMX_DBAM_ERR_FORMAT, "file ends inside an alignment record");
            }
        }
        if (carry == b.data_beg && !last) {   // no whole record yet (one longer than the window): read more behind it
            if (s->full - carry > (1ull << 30)) return fail(PMX_DBAM_ERR_FORMAT, "alignment record or line longer than 1 GiB");
            b.npieces = 0;
            b.N = carry;
            tail_at = carry, tail = s->full - carry;   // (the header stays parsed; the next round copies the record to the front)
            continue;
        }
        b.N = carry;
        b.npieces = b.sam ? 0 : (carry > b.data_beg ? (carry - b.data_beg + WALK_PIECE - 1) / WALK_PIECE : 0);
        if (b.sam && carry > b.data_beg) {
            s->sh.lines = s->sam_hdr_lines + s->lines_before;   // (line numbers of errors count from the start of the stream)
            if (int rc = sam_index_parse(b, s->sh)) return rc;
            s->lines_before += b.sam_lines;
        }
        s->windows++;
        s->max_tail = std::max<u64>(s->max_tail, s->full - carry);
        if (last) s->done = carry == s->full;
        stream_note(b);
        if (carry == b.data_beg) {       // (the last window holds no record)
            s->done = true;
            return 0;
        }
        return (int64_t)(carry - b.data_beg);
    }
}

}  // namespace

static void stream_free(pmx_dbam *b)
{
    StreamState *s = b->st;
    if (!s) return;
    stream_join(s);
    for (int i = 0; i < 2; i++) {
        if (s->d_win[i]) (void)hipFree(s->d_win[i]);
        if (s->hb[i]) (void)hipHostFree(s->hb[i]);
    }
    if (s->d_mem) (void)hipFree(s->d_mem);
    if (s->d_st) (void)hipFree(s->d_st);
    for (void *p : {(void *)s->cx_ref, (void *)s->cx_pos, (void *)s->cx_len, (void *)s->cx_rev})
        if (p) (void)hipFree(p);
    b->d_out = nullptr;   // (it pointed into d_win)
    delete s;
    b->st = nullptr;
}

extern "C" {

static int stream_open_impl(int fd, int device, int nthreads, uint64_t window_bytes, pmx_dbam **out)
{
    if (fd < 0 || !out) return fail(PMX_DBAM_ERR_INVALID, "bad fd or null argument");
    *out = nullptr;
    (void)nthreads;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(PMX_DBAM_ERR_DEVICE, "no HIP device: the device ingest needs a GPU");
    if (device < 0 || device >= ndev) return fail(PMX_DBAM_ERR_INVALID, "no such device");
    HIPOK(hipSetDevice(device));
    pmx_dbam *b = new pmx_dbam;
    b->device = device;
    b->pipelined = false;
    b->st = new StreamState;
    StreamState *s = b->st;
    s->fd = fd;
    s->window = window_bytes ? window_bytes : STREAM_DEFAULT_WINDOW;
    s->infl = std::max<u64>(4 * s->window, 65536);
    s->target = s->window + STREAM_MEMBER_MAX;
    int rc = 0;
    if (hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&b->kstream, hipStreamNonBlocking) != hipSuccess)
        rc = fail(PMX_DBAM_ERR_DEVICE, "hipStreamCreate failed");
    for (int i = 0; i < 2 && !rc; i++)
        if (hipHostMalloc((void **)&s->hb[i], s->target, hipHostMallocDefault) != hipSuccess)
            rc = fail(PMX_DBAM_ERR_DEVICE, "hipHostMalloc of the stream buffers failed");
    if (!rc) {
        const double t0 = now_s();
        stream_fill(s, 0, 0);            // (hb[1 - hcur]: the first window's bytes)
        const int64_t r = stream_advance(*b);
        b->t[0] = now_s() - t0;
        if (r < 0) rc = (int)r;
        else s->primed = true;
    }
    if (rc) {
        const std::string keep = g_err;
        pmx_dbam_close(b);
        g_err = keep;
        return rc;
    }
    *out = b;
    return 0;
}

int pmx_dbam_open_stream(int fd, int device, int nthreads, uint64_t window_bytes, pmx_dbam **out)
{
    try {
        return stream_open_impl(fd, device, nthreads, window_bytes, out);
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dbam_open_stream: ") + e.what());
    }
}

int64_t pmx_dbam_stream_next(pmx_dbam *b)
{
    if (!b || !b->st) return fail(PMX_DBAM_ERR_INVALID, "not a stream handle");
    try {
        HIPOK(hipSetDevice(b->device));
        if (b->st->primed) {
            b->st->primed = false;
            const int64_t r0 = b->N > b->data_beg ? (int64_t)(b->N - b->data_beg) : 0;
            if (r0 == 0) b->st->cx_end = true;
            return r0;
        }
        const int64_t r = stream_advance(*b);
        if (r == 0) b->st->cx_end = true;
        return r;
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string("pmx_dbam_stream_next: ") + e.what());
    }
}

int pmx_dbam_stream_info(const pmx_dbam *b, uint64_t out[6])
{
    if (!b || !b->st || !out) return fail(PMX_DBAM_ERR_INVALID, "not a stream handle");
    StreamState *s = b->st;
    s->peak = std::max(s->peak, stream_held(*b));
    out[0] = s->windows;
    out[1] = s->bytes_in;
    out[2] = s->max_tail;
    out[3] = s->peak;
    out[4] = s->window;
    out[5] = s->infl;
    return 0;
}

}  // extern "C"
