// pg_csv_cell.h -- the text of one allele-frequency cell and of a row's position, shared by the device formatter (pg_csv.hip)
// and its host checker (pg_host_csv_freq_rows, pg_hostmath.cpp).  The rule stands in for parse_f64_roundup_and_own(x, 6)
// (base/helpers.rs:103-117) on [0, 1] and NaN:
//   NaN -> "NaN";  t = x * 1e6 (one rounded multiply), k = t rounded half away from zero;  k == 0 -> "0";  otherwise the decimal of
//   k / 10^6, followed, when k % 10^6 != 0, by "." and the six zero-padded digits of k % 10^6 without their trailing zeros.
// On [0, 1] that is "0", "1" or "0." + one to six digits: at most 8 bytes, kept in one 64-bit integer, first byte lowest.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define PG_CSV_HD __host__ __device__ __forceinline__
#else
#define PG_CSV_HD inline
#endif

constexpr int PG_CSV_CELL_MAX = 8;     // bytes of a cell's text; its separator (',' or '\n') is a ninth
constexpr int PG_CSV_PREFIX_EXTRA = 24; // bytes of "chr,pos,allele," beside the chromosome's name: 20 digits, the letter, 3 commas

// Returns the length of the cell's text and leaves the text in *text; a value that is no frequency (outside [0, 1] and not NaN)
// sets *bad and prints as "0".
PG_CSV_HD int pg_csv_cell(double x, uint64_t *text, int *bad) {
    if (x != x) {
        *text = 0x4E614EULL; // "NaN"
        return 3;
    }
    uint32_t k = 0;
    if (x >= 0.0 && x <= 1.0) {
        const double t = x * 1e6;
        k = (uint32_t)t;                      // floor: t >= 0
        if (t - (double)k >= 0.5) ++k;        // the difference is exact, so this is round-half-away-from-zero
    } else
        *bad = 1;
    if (k == 0 || k == 1000000u) {
        *text = k ? 0x31ULL : 0x30ULL;
        return 1;
    }
    const uint32_t hi = k / 1000u, lo = k - hi * 1000u;
    const uint32_t d5 = hi / 100u, d4 = (hi / 10u) % 10u, d3 = hi % 10u;
    const uint32_t d2 = lo / 100u, d1 = (lo / 10u) % 10u, d0 = lo % 10u;
    const int tz = d0 ? 0 : d1 ? 1 : d2 ? 2 : d3 ? 3 : d4 ? 4 : 5; // k != 0: some digit is not zero
    const uint32_t w0 = 0x30302E30u + (d5 << 16) + (d4 << 24); // "0." and the two leading digits
    const uint32_t w1 = 0x30303030u + d3 + (d2 << 8) + (d1 << 16) + (d0 << 24);
    *text = (uint64_t)w0 | ((uint64_t)w1 << 32);
    return 8 - tz;
}

// decimal digits of a position (1 .. 20)
PG_CSV_HD int pg_csv_pos_digits(uint64_t pos) {
    int nd = 1;
    uint64_t t = 10;
#pragma unroll
    for (int i = 1; i < 20; ++i) {
        nd += pos >= t ? 1 : 0;
        t *= 10; // (the last product, 10^20, wraps and is not used)
    }
    return nd;
}

// the letter of allele `al` (an index into "ATCGND")
PG_CSV_HD unsigned char pg_csv_allele(int al) { return (unsigned char)((0x444E47435441ULL >> (8 * (al & 7))) & 0xff); }
