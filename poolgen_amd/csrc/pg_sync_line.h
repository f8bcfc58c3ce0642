// pg_sync_line.h -- what one line of a sync file means (base/sync.rs String::lparse, as the CLI's parse_sync_buffer restates
// it), shared by the device parser (pg_sync.hip) and its host twin (pg_host_sync_parse, pg_hostsync.cpp): the number reader,
// the position field, a pool's field and the order of the line's checks.  The rules are DESIGN.md section 3.4i; the reason
// codes are pg_sync_reason (include/poolgen_hip.h).  A line that is wrong in several ways reports the SMALLEST of its codes,
// so that lanes which look at different pools of one line agree with a host loop that meets them one after the other.
#pragma once
#include <cstdint>
#include "../../include/poolgen_hip.h"

#if defined(__HIPCC__)
#define PG_SYNC_HD __host__ __device__ __forceinline__
#else
#define PG_SYNC_HD inline
#endif

constexpr int PG_SYNC_MAX_POOLS = 4096; // the operators' own limit
constexpr int PG_SYNC_TAB_BITS = 13;    // the first data line's (offset << 13 | tabs): tabs capped at PG_SYNC_TAB_CAP
constexpr int PG_SYNC_TAB_CAP = 8191;

PG_SYNC_HD int pg_sync_min_code(int a, int b) { return a == 0 ? b : (b == 0 ? a : (a < b ? a : b)); }

// A number from p[i]: an optional '+', then decimal digits up to the first other byte.  Returns where it stopped; *ok = one
// to nineteen digits were read (nineteen digits fit a u64; with more the value is not used).
PG_SYNC_HD int64_t pg_sync_number(const unsigned char *p, int64_t i, int64_t len, uint64_t *v, bool *ok) {
    if (i < len && p[i] == '+') ++i;
    const int64_t b = i;
    uint64_t x = 0;
    while (i < len) {
        const unsigned d = (unsigned)p[i] - (unsigned)'0';
        if (d > 9u) break;
        x = x * 10u + d;
        ++i;
    }
    *v = x;
    *ok = i != b && i - b <= 19;
    return i;
}

// the position: the whole second field is one number
PG_SYNC_HD bool pg_sync_pos(const unsigned char *p, int64_t len, uint64_t *pos) {
    bool ok;
    const int64_t i = pg_sync_number(p, 0, len, pos, &ok);
    return ok && i == len;
}

// What the fields in front of the pools decide.  tabs: the tabs of the line; pos_ok: pg_sync_pos of the second field (asked
// for only with two tabs or more).  0 = the line is skipped, 1 = its pools are read, else minus a pg_sync_reason.
PG_SYNC_HD int pg_sync_head(int64_t tabs, bool pos_ok) {
    if (tabs < 2) return -PG_SYNC_E_FIELDS;
    if (!pos_ok) return 0;
    if (tabs < 3) return -PG_SYNC_E_FIELDS;
    return 1;
}

// One pool: numbers separated by ':', six or more, nothing else.  Members, not an array: the device keeps them in registers.
struct PgSyncPool {
    uint32_t c0, c1, c2, c3, c4, c5;
    int err; // 0, or the smallest pg_sync_reason met
};

PG_SYNC_HD void pg_sync_pool(const unsigned char *p, int64_t len, PgSyncPool *out) {
    PgSyncPool s{0, 0, 0, 0, 0, 0, 0};
    int k = 0;
    int64_t i = 0;
    for (;;) {
        uint64_t v;
        bool ok;
        i = pg_sync_number(p, i, len, &v, &ok);
        if (!ok) {
            s.err = PG_SYNC_E_COUNT;
            break;
        }
        if (k < 6) {
            if (v > 0xffffffffULL) s.err = pg_sync_min_code(s.err, PG_SYNC_E_COUNT32);
            const uint32_t w = (uint32_t)v;
            if (k == 0) s.c0 = w;
            if (k == 1) s.c1 = w;
            if (k == 2) s.c2 = w;
            if (k == 3) s.c3 = w;
            if (k == 4) s.c4 = w;
            if (k == 5) s.c5 = w;
        }
        ++k;
        if (i >= len) break;
        if (p[i] != ':') {
            s.err = PG_SYNC_E_COUNT;
            break;
        }
        ++i;
    }
    if (k < 6) s.err = PG_SYNC_E_COUNT;
    *out = s;
}

// The first line of a slab that does not start with '#': `tabs` of it (capped at PG_SYNC_TAB_CAP) fix the pool count.
// Returns 0 or the pg_sync_reason of that line; *n = its pools (0 where it has none).
PG_SYNC_HD int pg_sync_first_line(int tabs, int expect_n, int *n) {
    *n = tabs >= 3 ? tabs - 2 : 0;
    if (tabs < 3) return PG_SYNC_E_FIELDS;
    if (tabs - 2 > PG_SYNC_MAX_POOLS || (expect_n > 0 && tabs - 2 != expect_n)) return PG_SYNC_E_POOLS;
    return 0;
}

// the key both sides minimise: the first bad line in file order, and of that line the smallest reason
PG_SYNC_HD uint64_t pg_sync_err_key(int64_t line_off, int code) { return ((uint64_t)line_off << 8) | (uint64_t)(code & 0xff); }
constexpr uint64_t PG_SYNC_NO_ERR = ~0ULL;
