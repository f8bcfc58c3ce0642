// pg_vcf_line.h -- what one line of a VCF means to vcf2sync (base/vcf.rs), shared by the device parser (pg_vcf.hip) and its
// host twin (pg_host_vcf_parse, pg_hostvcf.cpp): the u64 reader, the allele-to-column mapping, the pieces of a sample field and
// the filter arithmetic.  The rules are DESIGN.md section 3.4h; the reason codes are pg_vcf_reason (include/poolgen_hip.h).
// A line that is wrong in several ways reports the SMALLEST of its codes, so that lanes which look at different samples of
// one line agree with a host loop that meets them one after the other.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/poolgen_hip.h"

#if defined(__HIPCC__)
#define PG_VCF_HD __host__ __device__ __forceinline__
#else
#define PG_VCF_HD inline
#endif

constexpr int PG_VCF_MAX_POOLS = 2048;   // pool sizes a call takes (the device keeps a line's field starts in LDS)
constexpr int PG_VCF_MIN_LINE = 20;      // per_chunk formats &line[0..20] into its message before it parses: shorter lines panic
constexpr int PG_VCF_FIXED_FIELDS = 9;   // CHROM POS ID REF ALT QUAL FILTER INFO FORMAT

PG_VCF_HD int pg_vcf_min_code(int a, int b) { return a == 0 ? b : (b == 0 ? a : (a < b ? a : b)); }

// str::parse::<u64>: an optional '+', then digits only, at least one, no overflow
PG_VCF_HD bool pg_vcf_u64(const unsigned char *p, int64_t len, uint64_t *out) {
    int64_t i = (len > 0 && p[0] == '+') ? 1 : 0;
    if (i >= len) return false;
    uint64_t v = 0;
    for (; i < len; ++i) {
        const unsigned d = (unsigned)p[i] - (unsigned)'0';
        if (d > 9u) return false;
        if (v > 1844674407370955161ULL || (v == 1844674407370955161ULL && d > 5u)) return false; // 10 v + d > 2^64 - 1
        v = v * 10u + d;
    }
    *out = v;
    return true;
}

// str::parse::<char> or 'D': one character stays itself, anything else (the empty string too) is the indel class
PG_VCF_HD unsigned char pg_vcf_allele(const unsigned char *p, int64_t len) { return len == 1 ? p[0] : (unsigned char)'D'; }

PG_VCF_HD bool pg_vcf_has_high_byte(const unsigned char *p, int64_t len) {
    unsigned char any = 0;
    for (int64_t i = 0; i < len; ++i) any |= p[i];
    return (any & 0x80) != 0;
}

// For each of A, T, C, G, D, N the index into [REF] + ALTs of the first allele equal to it (vcf_to_sync's inner loop with its
// break), or -1.  Members, not an array: the device keeps them in registers.
struct PgVcfMap {
    int a, t, c, g, d, n;
};

PG_VCF_HD void pg_vcf_map_add(PgVcfMap &m, unsigned char ch, int k) {
    if (ch == 'A' && m.a < 0) m.a = k;
    if (ch == 'T' && m.t < 0) m.t = k;
    if (ch == 'C' && m.c < 0) m.c = k;
    if (ch == 'G' && m.g < 0) m.g = k;
    if (ch == 'D' && m.d < 0) m.d = k;
    if (ch == 'N' && m.n < 0) m.n = k;
}

// REF and the comma-separated ALT (an empty ALT is one empty allele, as str::split gives it); returns the reference character
PG_VCF_HD unsigned char pg_vcf_alleles(const unsigned char *ref, int64_t ref_len, const unsigned char *alt, int64_t alt_len, PgVcfMap *map) {
    PgVcfMap m{-1, -1, -1, -1, -1, -1};
    const unsigned char rc = pg_vcf_allele(ref, ref_len);
    pg_vcf_map_add(m, rc, 0);
    int k = 1;
    int64_t s = 0;
    for (int64_t i = 0; i <= alt_len; ++i)
        if (i == alt_len || alt[i] == ',') {
            pg_vcf_map_add(m, pg_vcf_allele(alt + s, i - s), k);
            ++k;
            s = i + 1;
        }
    *map = m;
    return rc;
}

PG_VCF_HD bool pg_vcf_map_out_of(const PgVcfMap &m, int cols) {
    return m.a >= cols || m.t >= cols || m.c >= cols || m.g >= cols || m.d >= cols || m.n >= cols;
}

// FORMAT split on ':': the number of pieces equal to "AD"; *idx = the index of the last one
PG_VCF_HD int pg_vcf_ad_key(const unsigned char *p, int64_t len, int *idx) {
    int found = 0, k = 0;
    int64_t s = 0;
    for (int64_t i = 0; i <= len; ++i)
        if (i == len || p[i] == ':') {
            if (i - s == 2 && p[s] == 'A' && p[s + 1] == 'D') { ++found; *idx = k; }
            ++k;
            s = i + 1;
        }
    return found;
}

// The AD piece of a sample field: piece `ad_idx` of the split on ':'.  false = the field has too few pieces.
PG_VCF_HD bool pg_vcf_ad_piece(const unsigned char *p, int64_t len, int ad_idx, int64_t *lo, int64_t *hi) {
    int64_t i = 0;
    for (int k = 0; k < ad_idx; ++k) {
        while (i < len && p[i] != ':') ++i;
        if (i >= len) return false;
        ++i;
    }
    int64_t j = i;
    while (j < len && p[j] != ':') ++j;
    *lo = i;
    *hi = j;
    return true;
}

// the number of comma-separated values of a sample's AD (-1: too few pieces): of pool 0 it is to_counts' column count m
PG_VCF_HD int pg_vcf_ad_count(const unsigned char *p, int64_t len, int ad_idx) {
    int64_t lo, hi;
    if (!pg_vcf_ad_piece(p, len, ad_idx, &lo, &hi)) return -1;
    int c = 1;
    for (int64_t i = lo; i < hi; ++i) c += p[i] == ',' ? 1 : 0;
    return c;
}

struct PgVcfSample {
    uint64_t depth;   // the sum of all AD values: what the coverage rule compares
    uint64_t row_sum; // the sum of the first `cols` values: to_frequencies' denominator
    uint32_t v1;      // column 1: the only column the frequency rule comes to depend on
    uint32_t a, t, c, g, d, n; // vcf_to_sync's six, 0 where the letter is no allele of the line
    int count;        // values in the AD list
    int err;          // 0, or the smallest pg_vcf_reason met
};

PG_VCF_HD void pg_vcf_sample(const unsigned char *p, int64_t len, int ad_idx, int cols, const PgVcfMap &map, PgVcfSample *out) {
    PgVcfSample s{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int64_t lo, hi;
    if (!pg_vcf_ad_piece(p, len, ad_idx, &lo, &hi)) {
        s.err = PG_VCF_E_SUBFIELDS;
        *out = s;
        return;
    }
    int k = 0;
    int64_t b = lo;
    for (int64_t i = lo; i <= hi; ++i)
        if (i == hi || p[i] == ',') {
            uint64_t v = 0;
            if (!pg_vcf_u64(p + b, i - b, &v)) {
                s.err = pg_vcf_min_code(s.err, PG_VCF_E_AD_VALUE);
                v = 0;
            } else if (v > 0xffffffffULL) {
                s.err = pg_vcf_min_code(s.err, PG_VCF_E_COUNT32);
                v = 0;
            }
            s.depth += v;
            if (k < cols) s.row_sum += v;
            const uint32_t w = (uint32_t)v;
            if (k == 1) s.v1 = w;
            if (k == map.a) s.a = w;
            if (k == map.t) s.t = w;
            if (k == map.c) s.c = w;
            if (k == map.g) s.g = w;
            if (k == map.d) s.d = w;
            if (k == map.n) s.n = w;
            ++k;
            b = i + 1;
        }
    s.count = k;
    *out = s;
}

// ---- the filter (VcfLine::filter, vcf.rs:117-178) ---------------------------------------------------------------------------
// ceil(min_coverage_breadth x pools) as Rust's `as u32` casts it: NaN and negatives to 0, large values to u32::MAX
PG_VCF_HD uint32_t pg_vcf_breadth_threshold(double breadth, int n_sizes) {
    const double t = ceil(breadth * (double)n_sizes);
    if (!(t > 0.0)) return 0u;
    if (t >= 4294967295.0) return 0xffffffffu;
    return (uint32_t)t;
}

// The coverage loop breaks when the covered pools EQUAL the threshold and the line stays when they equal it afterwards.  For a
// threshold above 0 that is "at least that many pools are covered"; for 0 the loop can only break after pool 0, on a pool 0
// that is NOT covered, and a covered pool 0 never lets the count return to 0.  Without pools the count is 0.
PG_VCF_HD bool pg_vcf_breadth_pass(uint32_t threshold, int64_t covered, bool pool0_covered, int pools) {
    if (threshold == 0u) return pools == 0 || !pool0_covered;
    return covered >= (int64_t)threshold;
}

// one pool's share of q: f[i][1] * pool_sizes[i] / sum(pool_sizes), three roundings, no contraction
PG_VCF_HD double pg_vcf_q_term(uint32_t v1, uint64_t row_sum, double pool_size, double sizes_sum) {
    const double f = (double)v1 / (double)row_sum;
    const double w = f * pool_size;
    return w / sizes_sum;
}

PG_VCF_HD bool pg_vcf_maf_pass(double q, double maf) { return !((q < maf) | (q > (1.00 - maf))); }

// ---- the line ---------------------------------------------------------------------------------------------------------------
// What the fixed fields give: everything of a line but its samples.
struct PgVcfHead {
    uint64_t pos;
    PgVcfMap map;
    int ad_idx;
    int err; // 0, or the smallest of POS, HIGH_BYTE, AD_KEY
    bool ad_ok; // exactly one AD key: the samples can be read
    unsigned char ref;
};

// f1, f3, f4, f8: [start, end) of POS, REF, ALT and FORMAT inside `line`
PG_VCF_HD void pg_vcf_head(const unsigned char *line, int64_t p0, int64_t p1, int64_t r0, int64_t r1, int64_t a0, int64_t a1, int64_t f0,
                           int64_t f1, PgVcfHead *out) {
    PgVcfHead h;
    h.err = 0;
    h.pos = 0;
    h.ad_idx = 0;
    if (!pg_vcf_u64(line + p0, p1 - p0, &h.pos)) h.err = PG_VCF_E_POS;
    if (pg_vcf_has_high_byte(line + r0, r1 - r0) || pg_vcf_has_high_byte(line + a0, a1 - a0)) h.err = pg_vcf_min_code(h.err, PG_VCF_E_HIGH_BYTE);
    h.ref = pg_vcf_alleles(line + r0, r1 - r0, line + a0, a1 - a0, &h.map);
    h.ad_ok = pg_vcf_ad_key(line + f0, f1 - f0, &h.ad_idx) == 1;
    if (!h.ad_ok) h.err = pg_vcf_min_code(h.err, PG_VCF_E_AD_KEY);
    *out = h;
}

// the key both sides minimise: the first bad line in file order, and of that line the smallest reason
PG_VCF_HD uint64_t pg_vcf_err_key(int64_t line_off, int code) { return ((uint64_t)line_off << 8) | (uint64_t)(code & 0xff); }
constexpr uint64_t PG_VCF_NO_ERR = ~0ULL;
