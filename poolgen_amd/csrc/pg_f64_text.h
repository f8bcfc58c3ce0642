// pg_f64_text.h -- the text of a double as the reference prints it, shared by the device result writer (pg_resultfmt.hip) and
// its host twin (pg_hostresultfmt.cpp): the same source on both sides, plain C++, no inline assembly, no array, no scratch.
//
// display(x) is Rust's `{}` of an f64:
//   NaN -> "NaN", infinities -> "inf" / "-inf", zero -> "0" / "-0"; any other value -> the SHORTEST decimal digit string (1 to
//   17 digits) that reads back as the same double, the closest such string, the even one on a tie, written in fixed notation:
//   no exponent, no trailing zeros behind the point, "0." and leading zeros for |x| < 1, padded with zeros for large exponents.
// roundup_own(x, nd) is parse_f64_roundup_and_own (base/helpers.rs:103-117): s = display(x); fewer than nd characters -> s;
//   otherwise display(round_half_away_from_zero(x * 10^nd) / 10^nd).  The product and the quotient are two separately rounded
//   binary64 operations (there is nothing here a compiler could contract; the build uses -ffp-contract=off all the same), 10^nd
//   is exact for nd <= 22.
//
// THE HOST WRITER'S DIFFERENCE.  The CLI's host writer prints through std::to_chars(x, chars_format::fixed) (rust_display,
// host/host_util.cpp).  That is display() for every |x| < 2^53 -- every fixture, every realistic statistic.  From about 2^54 on
// to_chars prints the EXACT integer (1e23 -> "99999999999999991611392") where Rust prints the shortest digits padded with zeros
// ("100000000000000000000000").  This header follows Rust, the reference: above 2^53 it is the correct one of the two.
//
// The shortest digits come from Schubfach (R. Giulietti, "The Schubfach way to render doubles", 2020): with c * 2^q the value,
// k = floor(log10(2^q)) and g ~ 10^-k * 2^-r (128 bits, pg_f64_pow10.h), the value and its two rounding boundaries are scaled
// by one 64 x 128-bit product each, rounded to odd, and the shortest digit string inside the interval is read off the quotient
// by 4, 40 and 10.  Two 64 x 64 -> 128-bit products per scaling, three scalings per value.
//
// Longest text: a value has at most 17 digits and its last digit stands no lower than 10^-324 (the spacing of the denormals is
// 4.9e-324), so "-0." + 307 zeros + 17 digits = 327 bytes (-2.2250738585072014e-308) is the maximum: PG_F64_TEXT_MAX_LEN.
//
// Two halves, because a row formatter needs the length of every cell before it may write one: pg_f64_parts(x) (what is to be
// printed: kind, sign, digits, digit count, exponent), then pg_f64_len(parts) and pg_f64_put(dst, parts).  Digits go from a
// 64-bit integer straight to their bytes by divisions by constants.
#pragma once
#include <cstdint>
#include "pg_f64_pow10.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h> // (the host twin's translation unit includes nothing of HIP itself: it also builds with a plain C++ compiler)
#define PG_F64_HD __host__ __device__ __forceinline__
#else
#define PG_F64_HD inline
#endif

constexpr int PG_F64_TEXT_MAX_LEN = 327; // bytes of the longest display(x)
constexpr int PG_F64_MAX_ROUND_DIGITS = 22; // 10^22 is the largest power of ten a double holds exactly

struct pg_f64_u128 {
    uint64_t hi, lo;
};

// the table: read-only data on either side
static const pg_f64_u128 pg_f64_pow10_host[PG_F64_POW10_MAX - PG_F64_POW10_MIN + 1] = {PG_F64_POW10_VALUES};
#if defined(__HIPCC__)
static __device__ const pg_f64_u128 pg_f64_pow10_device[PG_F64_POW10_MAX - PG_F64_POW10_MIN + 1] = {PG_F64_POW10_VALUES};
#endif

// g(k), PG_F64_POW10_MIN <= k <= PG_F64_POW10_MAX
PG_F64_HD pg_f64_u128 pg_f64_pow10(int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return pg_f64_pow10_device[k - PG_F64_POW10_MIN];
#else
    return pg_f64_pow10_host[k - PG_F64_POW10_MIN];
#endif
}

PG_F64_HD uint64_t pg_f64_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}

PG_F64_HD double pg_f64_from_bits(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}

// floor(g * cp / 2^128), with the lowest bit set when anything below it was lost ("round to odd"); g >= 2^127, cp < 2^64
PG_F64_HD uint64_t pg_f64_round_to_odd(pg_f64_u128 g, uint64_t cp) {
    const unsigned __int128 x = (unsigned __int128)g.lo * cp;
    const unsigned __int128 y = (unsigned __int128)g.hi * cp + (uint64_t)(x >> 64); // (2^64 - 1)^2 + 2^64 - 1 < 2^128
    const uint64_t y0 = (uint64_t)y, y1 = (uint64_t)(y >> 64);
    return y1 | (uint64_t)(y0 > 1);
}

// The shortest digits of the finite, non-zero double with fraction field `frac` and exponent field `bexp`: value = *digits * 10^*exp10.
// *digits has at most 17 decimal digits and may end in zeros (pg_f64_parts removes them).
PG_F64_HD void pg_f64_shortest(uint64_t frac, int bexp, uint64_t *digits, int *exp10) {
    const uint64_t c = bexp != 0 ? (1ull << 52) | frac : frac;
    const int q = bexp != 0 ? bexp - 1075 : -1074;
    const bool even = (c & 1) == 0;                    // the interval's ends belong to it when the significand is even
    const bool lower_closer = frac == 0 && bexp > 1;   // a power of two: the neighbour below is half as far
    const uint64_t cbl = 4 * c - 2 + (lower_closer ? 1 : 0), cb = 4 * c, cbr = 4 * c + 2;
    // k = floor(log10(2^q)), or floor(log10(3/4 * 2^q)) at a power of two; |q| <= 1074 (arithmetic shifts of negative values)
    const int k = lower_closer ? (q * 1262611 - 524031) >> 22 : (q * 1262611) >> 22;
    const int h = q + ((-k * 1741647) >> 19) + 1;      // q + floor(log2(10^-k)) + 1, 1 <= h <= 4
    const pg_f64_u128 g = pg_f64_pow10(-k);            // -292 <= -k <= 324
    const uint64_t vbl = pg_f64_round_to_odd(g, cbl << h), vb = pg_f64_round_to_odd(g, cb << h), vbr = pg_f64_round_to_odd(g, cbr << h);
    const uint64_t lower = vbl + (even ? 0 : 1), upper = vbr - (even ? 0 : 1);
    const uint64_t s = vb / 4; // 4 s <= vb < 4 (s + 1)
    if (s >= 10) {             // one digit fewer?
        const uint64_t sp = s / 10;
        const bool up_inside = lower <= 40 * sp, wp_inside = 40 * sp + 40 <= upper;
        if (up_inside != wp_inside) {
            *digits = sp + (wp_inside ? 1 : 0);
            *exp10 = k + 1;
            return;
        }
    }
    const bool u_inside = lower <= 4 * s, w_inside = 4 * s + 4 <= upper;
    *exp10 = k;
    if (u_inside != w_inside) {
        *digits = s + (w_inside ? 1 : 0);
        return;
    }
    const uint64_t mid = 4 * s + 2; // both or neither inside: the closer one, the even one on a tie
    const bool round_up = vb > mid || (vb == mid && (s & 1) != 0);
    *digits = s + (round_up ? 1 : 0);
}

// decimal digits of v (1 .. 20)
PG_F64_HD int pg_f64_digits64(uint64_t v) {
    int nd = 1;
    uint64_t t = 10;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (int i = 1; i < 20; ++i) {
        nd += v >= t ? 1 : 0;
        t *= 10; // (the last product, 10^20, wraps and is not used)
    }
    return nd;
}

// The nd digits of v (nd >= pg_f64_digits64(v): zeros in front otherwise), last digit first, eight at a time from 32-bit pieces.
// Digit i goes to dst[i], or to dst[i + 1] from digit `gap` on: the place of a decimal point.  gap >= nd: no gap.
PG_F64_HD void pg_f64_put_u64(unsigned char *dst, uint64_t v, int nd, int gap) {
    int i = nd - 1;
    for (;;) {
        const uint64_t hi = v / 100000000ull;
        uint32_t lo = (uint32_t)(v - hi * 100000000ull);
        for (int j = 0; j < 8 && i >= 0; ++j, --i) {
            const uint32_t w = lo / 10u;
            dst[i + (i >= gap ? 1 : 0)] = (unsigned char)('0' + (lo - w * 10u));
            lo = w;
        }
        if (i < 0) return;
        v = hi;
    }
}

enum { PG_F64_FINITE = 0, PG_F64_ZERO = 1, PG_F64_INF = 2, PG_F64_NAN = 3 };

struct pg_f64_parts_t { // what display(x) prints
    uint64_t digits;    // PG_F64_FINITE: the digits, no trailing zero
    int32_t exp10;      //                value = digits * 10^exp10
    int16_t nd;         //                decimal digits of `digits` (1 .. 17)
    int8_t kind;
    int8_t neg;
};

PG_F64_HD pg_f64_parts_t pg_f64_parts(double x) {
    const uint64_t u = pg_f64_bits(x);
    const uint64_t frac = u & ((1ull << 52) - 1);
    const int bexp = (int)((u >> 52) & 0x7ff);
    pg_f64_parts_t p;
    p.digits = 0; p.exp10 = 0; p.nd = 0;
    p.neg = (int8_t)(u >> 63);
    if (bexp == 0x7ff) {
        p.kind = frac ? PG_F64_NAN : PG_F64_INF;
        return p;
    }
    if (bexp == 0 && frac == 0) {
        p.kind = PG_F64_ZERO;
        return p;
    }
    p.kind = PG_F64_FINITE;
    uint64_t d;
    int e;
    pg_f64_shortest(frac, bexp, &d, &e);
    for (int i = 0; i < 2; ++i) // up to 16 trailing zeros
        if (d % 100000000ull == 0) { d /= 100000000ull; e += 8; }
    if (d % 10000u == 0) { d /= 10000u; e += 4; }
    if (d % 100u == 0) { d /= 100u; e += 2; }
    if (d % 10u == 0) { d /= 10u; e += 1; }
    p.digits = d;
    p.exp10 = e;
    p.nd = (int16_t)pg_f64_digits64(d);
    return p;
}

// bytes of the text (1 .. PG_F64_TEXT_MAX_LEN)
PG_F64_HD int pg_f64_len(const pg_f64_parts_t &p) {
    if (p.kind == PG_F64_NAN) return 3;
    if (p.kind == PG_F64_INF) return 3 + p.neg;
    if (p.kind == PG_F64_ZERO) return 1 + p.neg;
    const int nd = p.nd, e = p.exp10;
    if (e >= 0) return p.neg + nd + e;       // an integer: the digits, e zeros
    if (nd + e > 0) return p.neg + nd + 1;   // the point inside the digits
    return p.neg + 2 - e;                    // "0.", -(nd + e) zeros, the digits
}

// the text to dst[0 .. pg_f64_len(p)); returns its length
PG_F64_HD int pg_f64_put(unsigned char *dst, const pg_f64_parts_t &p) {
    if (p.kind == PG_F64_NAN) {
        dst[0] = 'N'; dst[1] = 'a'; dst[2] = 'N';
        return 3;
    }
    int o = 0;
    if (p.neg) dst[o++] = '-';
    if (p.kind == PG_F64_INF) {
        dst[o] = 'i'; dst[o + 1] = 'n'; dst[o + 2] = 'f';
        return o + 3;
    }
    if (p.kind == PG_F64_ZERO) {
        dst[o] = '0';
        return o + 1;
    }
    const int nd = p.nd, e = p.exp10;
    if (e >= 0) {
        pg_f64_put_u64(dst + o, p.digits, nd, nd);
        for (int i = 0; i < e; ++i) dst[o + nd + i] = '0';
        return o + nd + e;
    }
    if (nd + e > 0) { // the first nd + e digits, the point, the last -e digits
        pg_f64_put_u64(dst + o, p.digits, nd, nd + e);
        dst[o + nd + e] = '.';
        return o + nd + 1;
    }
    const int z = -(nd + e);
    dst[o] = '0'; dst[o + 1] = '.';
    for (int i = 0; i < z; ++i) dst[o + 2 + i] = '0';
    pg_f64_put_u64(dst + o + 2 + z, p.digits, nd, nd);
    return o + 2 + z + nd;
}

// 10^nd, 0 <= nd <= 22: every partial product is a power of ten a double holds exactly
PG_F64_HD double pg_f64_pow10_exact(int nd) {
    double f = 1.0;
    for (int i = 0; i < nd; ++i) f *= 10.0;
    return f;
}

// f64::round: to the nearest integer, half away from zero; the sign of a zero result is x's
PG_F64_HD double pg_f64_round_half_away(double v) {
    const uint64_t u = pg_f64_bits(v);
    const double a = pg_f64_from_bits(u & ~(1ull << 63));
    if (!(a < 4503599627370496.0)) return v; // 2^52 and above, infinities, NaN: already integral (or not a number)
    double t = (double)(int64_t)a;           // floor: a >= 0
    if (a - t >= 0.5) t += 1.0;              // the difference is exact
    return pg_f64_from_bits(pg_f64_bits(t) | (u & (1ull << 63)));
}

// sensible_round (base/helpers.rs:103-108): a rounded multiply, the rounding, a rounded divide
PG_F64_HD double pg_f64_sensible_round(double x, int nd) {
    const double f = pg_f64_pow10_exact(nd);
    const double v = x * f;
    return pg_f64_round_half_away(v) / f;
}

// what a cell prints: display(x) for nd < 0, roundup_own(x, nd) otherwise
PG_F64_HD pg_f64_parts_t pg_f64_cell(double x, int nd) {
    pg_f64_parts_t p;
    double v = x;
#if defined(__HIPCC__)
#pragma nounroll // one copy of the conversion per cell in a kernel's code, not two
#endif
    for (int pass = 0;; ++pass) {
        p = pg_f64_parts(v);
        if (pass == 1 || nd < 0 || pg_f64_len(p) < nd) break;
        v = pg_f64_sensible_round(x, nd);
    }
    return p;
}
