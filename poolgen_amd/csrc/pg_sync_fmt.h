// pg_sync_fmt.h -- the text of a sync line's numbers and the length of a line, shared by the device formatter (pg_syncfmt.hip)
// and its host twin (pg_host_sync_format_rows, pg_hostsyncfmt.cpp).  A line is what append_sync_line (host/pileup.h) writes
// for pileup_to_sync (pileup.rs:348-371) and vcf_to_sync (vcf.rs:212-229):
//   <chromosome> '\t' <pos> '\t' <ref>, per pool '\t' and its six counts joined by ':', '\n'.
// A number is plain decimal: no sign, no leading zeros, "0" for zero; a count (uint32) has 1 to 10 digits, a position (uint64)
// 1 to 20.  Nothing here keeps digits in an array: a number is written from its last digit to its first straight to where it
// goes, so the device form needs no scratch.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h> // (the host twin's translation unit includes nothing of HIP itself: it also builds with a plain C++ compiler)
#define PG_SYNCFMT_HD __host__ __device__ __forceinline__
#define PG_SYNCFMT_UNROLL _Pragma("unroll")
#else
#define PG_SYNCFMT_HD inline
#define PG_SYNCFMT_UNROLL
#endif

constexpr int PG_SYNCFMT_MAX_POOLS = 4096;    // the sync parser's limit
constexpr int PG_SYNCFMT_POOL_MAX = 66;       // bytes of a pool's text: '\t', six counts of ten digits, five ':'
constexpr int PG_SYNCFMT_MAX_ROW = 1 << 22;   // bytes of one line (a longer one is refused): 256 of them still sum in an int32

// decimal digits of a count (1 .. 10)
PG_SYNCFMT_HD int pg_syncfmt_digits32(uint32_t v) {
    return 1 + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) +
           (v >= 100000000u) + (v >= 1000000000u);
}

// decimal digits of a position (1 .. 20)
PG_SYNCFMT_HD int pg_syncfmt_digits64(uint64_t v) {
    if (v <= 0xffffffffull) return pg_syncfmt_digits32((uint32_t)v);
    int nd = 10; // v >= 2^32 > 10^9
    uint64_t t = 10000000000ull;
    PG_SYNCFMT_UNROLL
    for (int i = 10; i < 20; ++i) {
        nd += v >= t ? 1 : 0;
        t *= 10; // (the last product, 10^20, wraps and is not used)
    }
    return nd;
}

// the nd = pg_syncfmt_digits32(v) digits of v to dst[0 .. nd)
PG_SYNCFMT_HD void pg_syncfmt_put32(unsigned char *dst, uint32_t v, int nd) {
    for (int i = nd - 1; i >= 0; --i) {
        const uint32_t w = v / 10u;
        dst[i] = (unsigned char)('0' + (v - w * 10u));
        v = w;
    }
}

// the nd = pg_syncfmt_digits64(v) digits of v to dst[0 .. nd)
PG_SYNCFMT_HD void pg_syncfmt_put64(unsigned char *dst, uint64_t v, int nd) {
    int i = nd - 1;
    for (; v > 0xffffffffull; --i) {
        const uint64_t w = v / 10u;
        dst[i] = (unsigned char)('0' + (uint32_t)(v - w * 10u));
        v = w;
    }
    pg_syncfmt_put32(dst, (uint32_t)v, i + 1);
}

// bytes of a pool's text: '\t' + six numbers + five ':' (7 .. PG_SYNCFMT_POOL_MAX)
PG_SYNCFMT_HD int pg_syncfmt_pool_len(const uint32_t *c) {
    return 6 + pg_syncfmt_digits32(c[0]) + pg_syncfmt_digits32(c[1]) + pg_syncfmt_digits32(c[2]) + pg_syncfmt_digits32(c[3]) +
           pg_syncfmt_digits32(c[4]) + pg_syncfmt_digits32(c[5]);
}

// a pool's text to dst; returns its length (pg_syncfmt_pool_len)
PG_SYNCFMT_HD int pg_syncfmt_put_pool(unsigned char *dst, const uint32_t *c) {
    int o = 0;
    PG_SYNCFMT_UNROLL
    for (int j = 0; j < 6; ++j) {
        const uint32_t v = c[j];
        const int nd = pg_syncfmt_digits32(v);
        dst[o] = j == 0 ? '\t' : ':';
        pg_syncfmt_put32(dst + o + 1, v, nd);
        o += nd + 1;
    }
    return o;
}

// May the row's chromosome name be read?  (It lies in slab[line_off .. line_off + chrom_len).)
PG_SYNCFMT_HD bool pg_syncfmt_name_ok(int64_t line_off, int32_t chrom_len, int64_t slab_bytes) {
    return line_off >= 0 && chrom_len >= 0 && line_off <= slab_bytes - (int64_t)chrom_len;
}

// bytes of the line in front of its pools: the name, '\t', the position, '\t', the reference byte
PG_SYNCFMT_HD int64_t pg_syncfmt_prefix_len(int32_t chrom_len, uint64_t pos) { return (int64_t)chrom_len + pg_syncfmt_digits64(pos) + 3; }

// "\t<pos>\t<ref>" to dst (behind the name); returns its length
PG_SYNCFMT_HD int pg_syncfmt_put_pos_ref(unsigned char *dst, uint64_t pos, unsigned char ref) {
    const int nd = pg_syncfmt_digits64(pos);
    dst[0] = '\t';
    pg_syncfmt_put64(dst + 1, pos, nd);
    dst[nd + 1] = '\t';
    dst[nd + 2] = ref;
    return nd + 3;
}

// bytes of a line: its prefix, the text of its pools (the sum of pg_syncfmt_pool_len), '\n'
PG_SYNCFMT_HD int64_t pg_syncfmt_row_len(int32_t chrom_len, uint64_t pos, int64_t pools_len) {
    return pg_syncfmt_prefix_len(chrom_len, pos) + pools_len + 1;
}
