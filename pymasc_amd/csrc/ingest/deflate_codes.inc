// The serial half of the DEFLATE encoder (deflate_device.inc; DESIGN.md 7.18.2): code lengths from symbol counts, canonical codes,
// and the code-length sequence of a dynamic block's header (RFC 1951 3.2.2, 3.2.7).  Plain C++ over caller-given arrays, a few
// hundred steps each, walked by one lane on the device; it compiles for the host as well, where a program can check it against zlib.

#ifndef DF_HD
#define DF_HD __host__ __device__ __forceinline__
#endif

#define DF_LL 286       // literal / length symbols that may be used (0 .. 285)
#define DF_D 30         // distance symbols
#define DF_CL 19        // symbols of the code-length alphabet
#define DF_NODES (2 * DF_LL)

// Code lengths of at most `maxbits` for the m used symbols order[0, m), given in ascending (count, symbol) order; len[] of the
// other symbols stays as it is.  The tree is the two-queue merge over the sorted leaves (a leaf wins a tie, so the result is a
// function of the counts alone); depths above maxbits are cut to it and the Kraft sum is repaired one unit of 2^-maxbits at a time:
// a leaf of the deepest level below maxbits moves one level down and takes a leaf of level maxbits up beside it.  The lengths
// are then dealt out again, the longest to the rarest symbol.  m == 1: length 1.  Work: node[2 m] (u32), up[2 m], dep[2 m] (u16).
DF_HD void df_lengths(const uint32_t *freq, const uint16_t *order, uint32_t m, uint32_t maxbits, uint8_t *len, uint32_t *node,
                      uint16_t *up, uint16_t *dep)
{
    if (m == 0) return;
    if (m == 1) {
        len[order[0]] = 1;
        return;
    }
    for (uint32_t i = 0; i < m; i++) node[i] = freq[order[i]];
    uint32_t leaf = 0, inner = m, next = m;         // the heads of the two queues; the node being made
    for (; next < 2 * m - 1; next++) {
        uint32_t sum = 0;
        for (int k = 0; k < 2; k++) {
            const bool take_leaf = leaf < m && (inner >= next || node[leaf] <= node[inner]);
            const uint32_t x = take_leaf ? leaf++ : inner++;
            sum += node[x];
            up[x] = (uint16_t)next;
        }
        node[next] = sum;
    }
    uint32_t count[16];
    for (uint32_t b = 0; b < 16; b++) count[b] = 0;
    dep[2 * m - 2] = 0;
    for (uint32_t x = 2 * m - 2; x-- > 0;) {
        dep[x] = (uint16_t)(dep[up[x]] + 1);
        if (x < m) count[dep[x] < maxbits ? dep[x] : maxbits]++;
    }
    uint32_t kraft = 0;                             // in units of 2^-maxbits; 2^maxbits for a complete code
    for (uint32_t b = 1; b <= maxbits; b++) kraft += count[b] << (maxbits - b);
    for (; kraft > (1u << maxbits); kraft--) {
        uint32_t b = maxbits - 1;
        while (count[b] == 0) b--;
        count[b]--;
        count[b + 1] += 2;
        count[maxbits]--;
    }
    uint32_t i = 0;
    for (uint32_t b = maxbits; b >= 1; b--)
        for (uint32_t c = count[b]; c > 0; c--) len[order[i++]] = (uint8_t)b;
}

// the bits of v in reverse order
DF_HD uint32_t df_reverse(uint32_t v, uint32_t bits)
{
    uint32_t r = 0;
    for (uint32_t k = 0; k < bits; k++, v >>= 1) r = (r << 1) | (v & 1u);
    return r;
}

// tab[s] = len[s] << 16 | the canonical code of s, bit-reversed (a code goes into the stream from its most significant bit on)
DF_HD void df_codes(const uint8_t *len, uint32_t n, uint32_t *tab)
{
    uint32_t count[16], next[16];
    for (uint32_t b = 0; b < 16; b++) count[b] = 0;
    for (uint32_t s = 0; s < n; s++) count[len[s]]++;
    count[0] = 0;
    uint32_t code = 0;
    for (uint32_t b = 1; b < 16; b++) {
        code = (code + count[b - 1]) << 1;
        next[b] = code;
    }
    for (uint32_t s = 0; s < n; s++) tab[s] = len[s] ? ((uint32_t)len[s] << 16) | df_reverse(next[len[s]]++, len[s]) : 0u;
}

// The n code lengths of the two alphabets as symbols of the code-length alphabet: seq[k] = symbol | extra bits' value << 8, with the
// runs of 16 (the previous length 3 .. 6 times more), 17 (3 .. 10 zeros) and 18 (11 .. 138 zeros); cfreq[19] counts the symbols.
// Returns the number of entries, at most n.
DF_HD uint32_t df_header_seq(const uint8_t *len, uint32_t n, uint16_t *seq, uint32_t *cfreq)
{
    for (uint32_t s = 0; s < DF_CL; s++) cfreq[s] = 0;
    uint32_t k = 0;
    for (uint32_t i = 0; i < n;) {
        const uint32_t v = len[i];
        uint32_t run = 1;
        while (i + run < n && len[i + run] == v) run++;
        i += run;
        if (v != 0) {                               // the length itself once, then what repeats it
            seq[k++] = (uint16_t)v;
            cfreq[v]++;
            run--;
        }
        while (run > 0) {
            if (v == 0 && run >= 11) {
                const uint32_t r = run < 138u ? run : 138u;
                seq[k++] = (uint16_t)(18u | (r - 11u) << 8);
                cfreq[18]++;
                run -= r;
            } else if (run >= 3) {
                const uint32_t r = v == 0 ? (run < 10u ? run : 10u) : (run < 6u ? run : 6u);
                seq[k++] = (uint16_t)((v == 0 ? 17u : 16u) | (r - 3u) << 8);
                cfreq[v == 0 ? 17 : 16]++;
                run -= r;
            } else {
                seq[k++] = (uint16_t)v;
                cfreq[v]++;
                run--;
            }
        }
    }
    return k;
}

// the order in which a dynamic block's header gives the lengths of the code-length alphabet
#define DF_CL_ORDER {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15}

// the used symbols of cfreq[19] in ascending (count, symbol) order; returns their number
DF_HD uint32_t df_cl_sort(const uint32_t *cfreq, uint16_t *order)
{
    uint32_t m = 0;
    for (uint32_t s = 0; s < DF_CL; s++) {
        if (!cfreq[s]) continue;
        uint32_t at = m++;
        for (; at > 0 && cfreq[order[at - 1]] > cfreq[s]; at--) order[at] = order[at - 1];
        order[at] = (uint16_t)s;
    }
    return m;
}

// length code and extra bits of a match length 3 .. 258 (RFC 1951 3.2.5): symbol 257 .. 285
DF_HD void df_len_code(uint32_t len, uint32_t &sym, uint32_t &nbits, uint32_t &extra)
{
    const uint32_t l = len - 3u;
    if (l < 8u) {
        sym = 257u + l, nbits = 0, extra = 0;
    } else if (len == 258u) {
        sym = 285u, nbits = 0, extra = 0;
    } else {
        nbits = 29u - (uint32_t)__builtin_clz(l);
        sym = 261u + 4u * nbits + ((l >> nbits) & 3u);
        extra = l & ((1u << nbits) - 1u);
    }
}

// distance code and extra bits of a distance 1 .. 32768
DF_HD void df_dist_code(uint32_t dist, uint32_t &sym, uint32_t &nbits, uint32_t &extra)
{
    const uint32_t d = dist - 1u;
    if (d < 4u) {
        sym = d, nbits = 0, extra = 0;
    } else {
        nbits = 30u - (uint32_t)__builtin_clz(d);
        sym = 2u * nbits + 2u + ((d >> nbits) & 1u);
        extra = d & ((1u << nbits) - 1u);
    }
}

DF_HD uint32_t df_len_extra_bits(uint32_t sym) { return sym < 265u || sym == 285u ? 0u : (sym - 261u) >> 2; }
DF_HD uint32_t df_dist_extra_bits(uint32_t sym) { return sym < 4u ? 0u : (sym - 2u) >> 1; }

// the fixed codes of RFC 1951 3.2.6 as a length: literal / length symbol s
DF_HD uint32_t df_fixed_len(uint32_t s) { return s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u; }

// the bits of a dynamic block's header behind its three block bits: 14 + 3 per declared code-length code + the sequence
DF_HD uint32_t df_header_bits(uint32_t hclen, const uint32_t *cfreq, const uint8_t *cl_len)
{
    uint32_t bits = 14u + 3u * hclen + 2u * cfreq[16] + 3u * cfreq[17] + 7u * cfreq[18];
    for (uint32_t s = 0; s < DF_CL; s++) bits += cfreq[s] * cl_len[s];
    return bits;
}

// the declared code-length codes: the order of the header cut behind its last used symbol, at least 4
DF_HD uint32_t df_hclen(const uint8_t *cl_len)
{
    const uint8_t ord[DF_CL] = DF_CL_ORDER;
    uint32_t n = DF_CL;
    while (n > 4u && cl_len[ord[n - 1u]] == 0) n--;
    return n;
}

// put(value, bits) appends to the stream: HLIT, HDIST, HCLEN, the code-length code's lengths, the sequence with its extra bits
template <class Put>
DF_HD void df_header_write(Put &&put, uint32_t hlit, uint32_t hdist, uint32_t hclen, const uint8_t *cl_len, const uint32_t *cl_tab,
                           const uint16_t *seq, uint32_t nseq)
{
    const uint8_t ord[DF_CL] = DF_CL_ORDER;
    put(hlit - 257u, 5u);
    put(hdist - 1u, 5u);
    put(hclen - 4u, 4u);
    for (uint32_t k = 0; k < hclen; k++) put((uint32_t)cl_len[ord[k]], 3u);
    for (uint32_t k = 0; k < nseq; k++) {
        const uint32_t s = seq[k] & 0xffu, x = seq[k] >> 8;
        put(cl_tab[s] & 0xffffu, cl_tab[s] >> 16);
        if (s >= 16u) put(x, s == 16u ? 2u : s == 17u ? 3u : 7u);
    }
}

// The code-length alphabet's own lengths (at most 7 bits) from cfreq[19].  zlib refuses an incomplete code here, so a single used
// symbol is given a partner of length 1.  order[19], node[38], up[38], dep[38]: work.
DF_HD void df_cl_lengths(const uint32_t *cfreq, uint8_t *cl_len, uint16_t *order, uint32_t *node, uint16_t *up, uint16_t *dep)
{
    for (uint32_t s = 0; s < DF_CL; s++) cl_len[s] = 0;
    const uint32_t m = df_cl_sort(cfreq, order);
    df_lengths(cfreq, order, m, 7u, cl_len, node, up, dep);
    if (m == 1) cl_len[order[0] == 0 ? 1 : 0] = 1;
}
