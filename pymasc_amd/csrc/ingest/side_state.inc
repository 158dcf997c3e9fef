// What a handle holds for its side counts (DESIGN.md 7.20), and the guard of their entry points.  Included in bam_device.hip in front
// of struct pmx_dbam: one struct per family, whose destructor frees the family's device memory, so that dropping a table is
// `b->x = X{}` and pmx_dbam_close frees what is held with `delete b`.  on(): a table is held; held(): the device bytes of the family
// in pmx_dbam_stream_info's peak.

struct DevAlloc {   // a device allocation freed on every way out: moved, never copied
    void *p = nullptr;
    DevAlloc() = default;
    DevAlloc(const DevAlloc &) = delete;
    DevAlloc &operator=(const DevAlloc &) = delete;
    DevAlloc(DevAlloc &&o) noexcept : p(o.p) { o.p = nullptr; }
    DevAlloc &operator=(DevAlloc &&o) noexcept
    {
        if (this != &o) {
            if (p) (void)hipFree(p);
            p = o.p;
            o.p = nullptr;
        }
        return *this;
    }
    ~DevAlloc()
    {
        if (p) (void)hipFree(p);
    }
    template <class T> T *as() const { return (T *)p; }
};

// read counts per genome bin (pmx_dbam_bincount_*, bincount_device.inc): from begin to the next begin or close
struct Bincount {
    DevAlloc counts;                 // u32: one count per bin, the chosen references' bins end to end in header order
    DevAlloc tab;                    // long long, per reference: its first bin (-1: not chosen), its number of bins
    u64 bins = 0, reads = 0;         // bins; reads that added to a bin since begin
    u32 bin = 0, ext = 0;            // bin size, extend
    bool on() const { return counts.p != nullptr; }
    u64 held() const { return bins * 4; }
};

// reads per peak line (pmx_dbam_peakcount_*, peakcount_device.inc): from begin to the next begin or close
struct Peakcount {
    DevAlloc lines;                  // per line, in (reference, begin) order: key, pmax (8 bytes each), end, input line; counts by input line
    DevAlloc tab;                    // long long, per reference: its length, -1 when it is not chosen
    bool begun = false;              // between a begin that succeeded and the next one
    u64 n = 0, uni = 0;              // lines; bases of the merged lines on chosen references
    u32 ext = 0;                     // extend
    std::vector<u64> tot;            // N, n_in, then the same two per reference, summed over the calls of add
    bool on() const { return begun; }
    u64 held() const { return n * 28; }
};

// fragment pileup (pmx_dbam_coverage_*, coverage_device.inc): the table from begin to finish, the runs from finish to the next begin or close
enum { CV_NONE = 0, CV_TABLE = 1, CV_RUNS = 2 };
struct Coverage {
    DevAlloc table;                  // int: one slot per base of every chosen reference + a closing one: depth[p] - depth[p - 1]
    DevAlloc tab;                    // long long, per reference: its first slot (-1: not chosen), its length
    DevAlloc seg;                    // CvSeg, per chosen reference: first slot, first tile, slots, id; one more entry closes the tiles
    DevAlloc names;                  // u8: per reference the offset of its name (u32, one more closes them), then the names
    DevAlloc runs;                   // u8: reference, start, end, depth of every run (4 bytes each)
    int state = CV_NONE;             // nothing / a table / runs
    u64 slots = 0, tiles = 0, reads = 0, nruns = 0;   // slots; tiles; reads that added since begin; runs
    u64 bytes = 0;                   // device bytes the pileup holds now
    u32 nc = 0, ext = 0;             // chosen references; extend
    u64 tot[5] = {0, 0, 0, 0, 0};    // reads, runs, covered bases, fragment bases, largest depth
    std::vector<int> chosen;         // the chosen references, in header order
    std::vector<u64> ranges;         // runs state, once asked for: the first run of every chosen reference, one more entry closing them
    // the zoom bins of a bigWig file (pmx_dbam_coverage_zoom_*; DESIGN.md 7.18.1): from zoom_begin until the last level is pulled
    DevAlloc zbins;                  // per level: u64 sum, u64 sum of squares, u32 covered bases, u32 min, u32 max of every bin (28 bytes)
    DevAlloc ztab;                   // u64 per level and chromosome id: its first bin (one more closes a level); u32 id of every
                                     // reference; u32 length of every id
    u32 zlevels = 0, z0 = 0;         // levels; the reduction of level 0
    std::vector<u64> znb, zoff;      // per level: its bins; its first byte in zbins
    u64 zbytes = 0;                  // device bytes of zbins and ztab, counted in `bytes`
    bool zsg = false;                // the bins are the signal's: f64 sums and f32 bounds in the same 28 bytes
    // the signal track (pmx_dbam_coverage_signal, signal_device.inc; DESIGN.md 7.18.3) or the compared track (pmx_dbam_coverage_compare,
    // compare_device.inc; 7.18.4): from signal / compare until the next signal, compare, begin or close
    DevAlloc sruns;                  // u8: reference, start, end, float32 value of every signal run (the layout of `runs`)
    bool shave = false;              // a signal has been made of these runs
    bool spscore = false;            // its values are p-scores (pmx_dbam_coverage_poisson, poisson_device.inc; 7.18.6): call writes column 8
    u64 snruns = 0;                  // its runs
    u32 sbin = 0;                    // its bin
    double stot[4] = {0, 0, 0, 0};   // runs, covered bases, smallest and largest value
    std::vector<u64> sranges;        // `ranges` of the signal runs
    // the peaks called from the signal runs (pmx_dbam_coverage_call, call_device.inc; DESIGN.md 7.18.5): from call until the next
    // call, signal, compare, begin or close
    DevAlloc peaks;                  // u8: reference, start, end, summit, float32 value, passing runs of every peak (4 bytes each)
    bool phave = false;              // peaks have been called from these signal runs
    u64 npeaks = 0;                  // the peaks
    u64 ptot[5] = {0, 0, 0, 0, 0};   // passing runs, candidates, peaks, peak bases, passing bases
    // the q-scores of a p-score track (pmx_dbam_coverage_qvalue, qvalue_device.inc; DESIGN.md 7.18.7): from qvalue until the next
    // qvalue, signal, compare, poisson, begin or close
    DevAlloc qtab;                   // u8: per distinct value its covered bases (8 bytes), its float32 p-score, its float32 q-score
    bool qhave = false;              // the table has been made of these signal runs
    u64 qrows = 0;                   // its rows
    u64 qtot[4] = {0, 0, 0, 0};      // rows, tests, covered bases, bases with q > 0
    bool on() const { return state == CV_TABLE; }
    u64 held() const { return bytes; }
};

// GC bias (pmx_dbam_gcbias_*, gcbias_device.inc): from begin to the next begin or close
struct GcBias {
    DevAlloc gc, bl;                 // u64: one GC and one blocked bit per position of the chosen references, laid end to end
    DevAlloc tab;                    // long long, per reference: its first position in the bit vectors (-1: not chosen), its length
    DevAlloc f;                      // unsigned long long: F[0 .. window]
    u32 w = 0;                       // the window (0: no table)
    u64 words = 0;                   // words of each bit vector
    std::vector<u64> n;              // N[0 .. window], computed by begin
    u64 tot[3] = {0, 0, 0};          // reads placed, off_end, blocked since begin
    bool on() const { return w != 0; }
    u64 held() const { return words * 16; }
};

// fragment sizes (pmx_dbam_fragments_*, fragments_device.inc): from begin to the next begin or close
struct Fragments {
    DevAlloc hist;                   // unsigned long long: H[3][max]
    DevAlloc use;                    // u8, per reference: chosen (null: every reference)
    u32 max = 0;                     // max_size (0: no table)
    u64 c[PMX_FRAGMENTS_COUNTERS] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // the counters since begin
    double t[2] = {0, 0};            // seconds since begin: the row filter (wall clock), k_fr_hist (HIP events)
    bool on() const { return max != 0; }
    u64 held() const { return 24ull * max; }
};

// read profile around anchor sites (pmx_dbam_tss_*, tss_device.inc): from begin to the next begin or close
struct TssProfile {
    DevAlloc key, strand;            // per kept anchor, in (reference, a) order: u64 ref_id << 32 | a; u32 1 for a '-' anchor
    DevAlloc tab;                    // long long, per reference: its length, -1 when it is not chosen
    DevAlloc table;                  // long long [2][2 * flank + 2]: the differences of same / opposite, one closing entry per row
    bool begun = false;              // between a begin that succeeded and the next one
    u64 na = 0;                      // anchors on chosen references
    u32 flank = 0, ext = 0;          // flank, extend
    u64 tot[3] = {0, 0, 0};          // N, n_near, pairs, summed over the calls of add
    bool on() const { return begun; }
    u64 held() const { return begun ? na * 12 + 16ull * (2ull * flank + 2ull) : 0; }
};

// the body of an entry point: an exception (std::bad_alloc, ...) must not leave the C ABI
template <class F> auto guarded(const char *name, F &&f) -> decltype(f())
{
    try {
        return f();
    } catch (const std::exception &e) {
        return fail(PMX_DBAM_ERR_OPEN, std::string(name) + ": " + e.what());
    }
}
