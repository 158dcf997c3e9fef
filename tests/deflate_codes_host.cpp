// TEST INFRASTRUCTURE: the serial half of the device DEFLATE encoder (pymasc_amd/csrc/ingest/deflate_codes.inc) compiled for the
// host, driven by lines on stdin; tests/test_deflate_codes.py builds it (plain, and with the address and undefined-behaviour
// sanitizers), feeds it and judges what it prints.  It judges nothing itself.  Every array a routine is given has exactly the size
// the routine is promised, on the heap, so that a step outside it is the sanitizer's to find.
//
//   L maxbits n f[0..n)     df_lengths over the used symbols in ascending (count, symbol) order
//                             -> "len[0..n)" and "tab[0..n)" (df_codes of them)
//   C f[0..19)              df_cl_lengths -> "len[0..19)", "tab[0..19)", "hclen"
//   S hlit n len[0..n)      df_header_seq -> "nseq seq[0..nseq)", "cfreq[0..19)", "cl[0..19)", "hclen header_bits"; with hlit > 0 also
//                           df_header_write of HLIT = hlit, HDIST = n - hlit -> "bits_written x<hex of the bytes>"
//   T                       df_len_code of 3 .. 258, df_dist_code of 1 .. 32768 (sym nbits extra each), df_len_extra_bits of
//                           257 .. 285, df_dist_extra_bits of 0 .. 29, df_fixed_len of 0 .. 287: one line each
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#ifndef DF_HD
#define DF_HD static inline
#endif
#include "deflate_codes.inc"

namespace {

template <class T>
std::unique_ptr<T[]> exact(size_t n)
{
    std::unique_ptr<T[]> p(new T[n ? n : 1]);
    std::fill(p.get(), p.get() + (n ? n : 1), T(0));
    return p;
}

template <class T>
void line(const T *v, size_t n)
{
    for (size_t i = 0; i < n; i++) std::printf(i ? " %lu" : "%lu", (unsigned long)v[i]);
    std::printf("\n");
}

void lengths(std::istringstream &in)
{
    uint32_t maxbits, n;
    in >> maxbits >> n;
    auto freq = exact<uint32_t>(n);
    for (uint32_t s = 0; s < n; s++) in >> freq[s];
    std::vector<uint16_t> used;
    for (uint32_t s = 0; s < n; s++)
        if (freq[s]) used.push_back((uint16_t)s);
    std::stable_sort(used.begin(), used.end(), [&](uint16_t a, uint16_t b) { return freq[a] < freq[b]; });
    const uint32_t m = (uint32_t)used.size();
    auto order = exact<uint16_t>(m);
    std::copy(used.begin(), used.end(), order.get());
    auto len = exact<uint8_t>(n);
    auto node = exact<uint32_t>(2 * m);
    auto up = exact<uint16_t>(2 * m), dep = exact<uint16_t>(2 * m);
    df_lengths(freq.get(), order.get(), m, maxbits, len.get(), node.get(), up.get(), dep.get());
    auto tab = exact<uint32_t>(n);
    df_codes(len.get(), n, tab.get());
    line(len.get(), n);
    line(tab.get(), n);
}

void cl_lengths(std::istringstream &in)
{
    auto cfreq = exact<uint32_t>(DF_CL);
    for (uint32_t s = 0; s < DF_CL; s++) in >> cfreq[s];
    auto cl = exact<uint8_t>(DF_CL);
    auto order = exact<uint16_t>(DF_CL);
    auto node = exact<uint32_t>(2 * DF_CL);
    auto up = exact<uint16_t>(2 * DF_CL), dep = exact<uint16_t>(2 * DF_CL);
    df_cl_lengths(cfreq.get(), cl.get(), order.get(), node.get(), up.get(), dep.get());
    auto tab = exact<uint32_t>(DF_CL);
    df_codes(cl.get(), DF_CL, tab.get());
    line(cl.get(), DF_CL);
    line(tab.get(), DF_CL);
    std::printf("%u\n", df_hclen(cl.get()));
}

void header(std::istringstream &in)
{
    uint32_t hlit, n;
    in >> hlit >> n;
    auto len = exact<uint8_t>(n);
    for (uint32_t i = 0; i < n; i++) {
        uint32_t v;
        in >> v;
        len[i] = (uint8_t)v;
    }
    auto seq = exact<uint16_t>(n);
    auto cfreq = exact<uint32_t>(DF_CL);
    const uint32_t nseq = df_header_seq(len.get(), n, seq.get(), cfreq.get());
    std::printf("%u", nseq);
    for (uint32_t k = 0; k < nseq; k++) std::printf(" %u", seq[k]);
    std::printf("\n");
    line(cfreq.get(), DF_CL);
    auto cl = exact<uint8_t>(DF_CL);
    auto order = exact<uint16_t>(DF_CL);
    auto node = exact<uint32_t>(2 * DF_CL);
    auto up = exact<uint16_t>(2 * DF_CL), dep = exact<uint16_t>(2 * DF_CL);
    df_cl_lengths(cfreq.get(), cl.get(), order.get(), node.get(), up.get(), dep.get());
    line(cl.get(), DF_CL);
    const uint32_t hclen = df_hclen(cl.get());
    std::printf("%u %u\n", hclen, df_header_bits(hclen, cfreq.get(), cl.get()));
    if (!hlit) return;
    auto tab = exact<uint32_t>(DF_CL);
    df_codes(cl.get(), DF_CL, tab.get());
    std::vector<uint8_t> bytes;
    uint64_t at = 0;
    auto put = [&](uint32_t value, uint32_t bits) {
        for (uint32_t b = 0; b < bits; b++, at++) {
            if (at / 8 >= bytes.size()) bytes.push_back(0);
            bytes[at / 8] |= (uint8_t)(((value >> b) & 1u) << (at % 8));
        }
    };
    df_header_write(put, hlit, n - hlit, hclen, cl.get(), tab.get(), seq.get(), nseq);
    std::printf("%lu x", (unsigned long)at);
    for (uint8_t b : bytes) std::printf("%02x", b);
    std::printf("\n");
}

void tables()
{
    for (uint32_t l = 3; l <= 258; l++) {
        uint32_t sym = ~0u, nbits = ~0u, extra = ~0u;
        df_len_code(l, sym, nbits, extra);
        std::printf(l > 3 ? " %u %u %u" : "%u %u %u", sym, nbits, extra);
    }
    std::printf("\n");
    for (uint32_t d = 1; d <= 32768; d++) {
        uint32_t sym = ~0u, nbits = ~0u, extra = ~0u;
        df_dist_code(d, sym, nbits, extra);
        std::printf(d > 1 ? " %u %u %u" : "%u %u %u", sym, nbits, extra);
    }
    std::printf("\n");
    for (uint32_t s = 257; s <= 285; s++) std::printf(s > 257 ? " %u" : "%u", df_len_extra_bits(s));
    std::printf("\n");
    for (uint32_t s = 0; s < 30; s++) std::printf(s ? " %u" : "%u", df_dist_extra_bits(s));
    std::printf("\n");
    for (uint32_t s = 0; s < 288; s++) std::printf(s ? " %u" : "%u", df_fixed_len(s));
    std::printf("\n");
}

}  // namespace

int main()
{
    std::string text;
    while (std::getline(std::cin, text)) {
        std::istringstream in(text);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "L")
            lengths(in);
        else if (what == "C")
            cl_lengths(in);
        else if (what == "S")
            header(in);
        else if (what == "T")
            tables();
        else {
            std::fprintf(stderr, "unknown command %s\n", what.c_str());
            return 2;
        }
        if (!in) {
            std::fprintf(stderr, "short line: %s\n", text.c_str());
            return 2;
        }
    }
    return 0;
}
