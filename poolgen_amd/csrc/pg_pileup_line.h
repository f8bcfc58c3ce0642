// pg_pileup_line.h -- what one line of samtools mpileup text means to pileup2sync (base/pileup.rs: String::lparse :11-168,
// PileupLine::filter :240-334, to_counts :172-215, as the CLI's PileupConverter::decode restates them), shared by the device
// parser (pg_pileup.hip) and its host twin (pg_host_pileup_parse, pg_hostpileup.cpp): the number reader, the walk over one
// pool's read string and quality string, and the filter arithmetic.  The rules are DESIGN.md section 3.4j; the reason codes
// are pg_pileup_reason (include/poolgen_hip.h).  A pool reports the FIRST defect its own walk meets, a line the SMALLEST code
// among its header's and its pools', so that lanes which look at different pools of one line agree with a host loop that
// meets them one after the other.
#pragma once
#include <cmath>
#include <cstdint>
#include "../../include/poolgen_hip.h"

#if defined(__HIPCC__)
#define PG_PL_HD __host__ __device__ __forceinline__
#else
#define PG_PL_HD inline
#endif

constexpr int PG_PILEUP_MAX_POOLS = 4096; // pool sizes a call takes (the device keeps a line's field starts in LDS)

// The per-byte decisions, made once per call on the host (pg_pileup_tables) and read by both sides.
//   cls[b]   what read code b counts as: 0..5 = the column A,T,C,G,D,N; PG_PL_N = the allele byte 'N' itself (column N, or
//            gone under remove_ns); PG_PL_REF = '.' and ',': the reference allele as the line writes it
//   qcls[q]  0 = the quality stays; PG_PL_Q_LOW = 10^(-(q-33)/10) > max_base_error_rate, the read becomes 'N';
//            PG_PL_Q_OUT = below 33, the line is dropped
constexpr unsigned char PG_PL_N = 6, PG_PL_REF = 7, PG_PL_Q_LOW = 1, PG_PL_Q_OUT = 2;
struct PgPileupTables {
    unsigned char cls[256];
    unsigned char qcls[256];
};

// allele byte -> column of to_counts (:191-198); with keep_lowercase_reference through the remap of filter (:280-299) first,
// which sees the allele bytes lparse made: 'D' (what lparse made of '*') is then N, '*' (a reference allele) is D
PG_PL_HD unsigned char pg_pileup_allele_class(unsigned char a, bool keep_lc) {
    if (a == 78) return PG_PL_N; // before the remap: what remove_ns removes
    if (keep_lc) {
        if (a == 'A' || a == 'a') return 0;
        if (a == 'T' || a == 't') return 1;
        if (a == 'C' || a == 'c') return 2;
        if (a == 'G' || a == 'g') return 3;
        if (a == '*') return 4;
        return 5;
    }
    if (a == 65) return 0;
    if (a == 84) return 1;
    if (a == 67) return 2;
    if (a == 71) return 3;
    if (a == 68) return 4;
    return 5;
}

// host only: std::pow decides once for the 256 quality bytes
inline void pg_pileup_tables(bool keep_lc, double max_base_error_rate, PgPileupTables *t) {
    for (int b = 0; b < 256; ++b) {
        unsigned char a = 78; // lparse :111-127
        if (b == 'A' || b == 'a') a = 65;
        if (b == 'T' || b == 't') a = 84;
        if (b == 'C' || b == 'c') a = 67;
        if (b == 'G' || b == 'g') a = 71;
        if (b == '*') a = 68;
        t->cls[b] = (b == '.' || b == ',') ? PG_PL_REF : pg_pileup_allele_class(a, keep_lc);
        t->qcls[b] = b < 33 ? PG_PL_Q_OUT : (std::pow(10.0, -((double)b - 33.0) / 10.0) > max_base_error_rate ? PG_PL_Q_LOW : 0);
    }
}

PG_PL_HD int pg_pileup_min_code(int a, int b) { return a == 0 ? b : (b == 0 ? a : (a < b ? a : b)); }

// an optional '+' and 1-19 decimal digits
PG_PL_HD bool pg_pileup_u64(const unsigned char *p, int64_t len, uint64_t *out) {
    if (len > 0 && p[0] == '+') { ++p; --len; }
    if (len < 1 || len > 19) return false;
    uint64_t v = 0;
    for (int64_t i = 0; i < len; ++i) {
        const unsigned d = (unsigned)p[i] - (unsigned)'0';
        if (d > 9u) return false;
        v = v * 10u + d;
    }
    *out = v;
    return true;
}

// the first three fields: [p0, p1) the position, [r0, r1) the reference allele
PG_PL_HD int pg_pileup_head(const unsigned char *line, int64_t p0, int64_t p1, int64_t r0, int64_t r1, uint64_t *pos, unsigned char *ref) {
    int err = 0;
    *pos = 0;
    *ref = 0;
    if (!pg_pileup_u64(line + p0, p1 - p0, pos)) err = PG_PILEUP_E_POS;
    if (r1 - r0 != 1 || line[r0] >= 0x80) err = pg_pileup_min_code(err, PG_PILEUP_E_REF);
    else *ref = line[r0];
    return err;
}

struct PgPileupPool {
    uint32_t a, t, c, g, d, n; // to_counts' six, after the quality rule and the N removal
    int err;                   // 0, or the first pg_pileup_reason the pool's walk met
    int phred;                 // a quality below 33 among the paired ones: the line is dropped
};

// One pool.  Its fields inside `line`: [cb, ce) the coverage; [rb, re) the read string and [qb, qe) the quality string where
// have_r / have_q say that the line holds them.  refcls = pg_pileup_allele_class(reference allele).  Every loop moves `c`
// forward and stops at `re`; every byte read lies in [cb, max(ce, re, qe)).
PG_PL_HD void pg_pileup_pool(const unsigned char *line, int64_t cb, int64_t ce, bool have_r, int64_t rb, int64_t re, bool have_q, int64_t qb,
                             int64_t qe, unsigned char refcls, bool remove_ns, const unsigned char *cls, const unsigned char *qcls,
                             PgPileupPool *out) {
    PgPileupPool P{0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t cov = 0;
    if (!pg_pileup_u64(line + cb, ce - cb, &cov)) P.err = PG_PILEUP_E_COV;
    else if (!have_r || !have_q) P.err = PG_PILEUP_E_RAGGED;
    else if (cov > 0) { // (a pool nobody read is not looked at any further)
        const uint64_t nq = (uint64_t)(qe - qb);
        uint64_t j = 0; // reads so far: read j pairs with quality byte j
        int64_t c = rb;
        while (c < re) {
            const unsigned char ch = line[c++];
            if (ch == '+' || ch == '-') {
                if (c >= re) break; // the field ends on the marker
                unsigned d = (unsigned)line[c] - (unsigned)'0';
                if (d > 9u) { P.err = PG_PILEUP_E_INDEL; break; }
                uint64_t len = d;
                ++c;
                while (c < re && len == 0) { // "+0": the reference keeps waiting for a first non-zero digit
                    d = (unsigned)line[c] - (unsigned)'0';
                    if (d > 9u) { P.err = PG_PILEUP_E_INDEL; break; }
                    len = d;
                    ++c;
                }
                if (P.err || len == 0) break; // (len == 0: the field ended inside the zeros)
                while (c < re && (unsigned)line[c] - (unsigned)'0' <= 9u) { len = len * 10u + ((unsigned)line[c] - (unsigned)'0'); ++c; }
                // the first non-digit ends the number AND is the first of the `len` bytes to drop
                const uint64_t room = (uint64_t)(re - c);
                c += (int64_t)(len < room ? len : room);
                continue;
            }
            if (ch == '^') { if (c < re) ++c; continue; } // the mapping quality behind a read start, whatever byte it is
            if (ch == '$') continue;
            if (j < nq) {
                const unsigned char qc = qcls[line[qb + (int64_t)j]];
                if (qc == PG_PL_Q_OUT) P.phred = 1;
                unsigned char k = cls[ch];
                if (k == PG_PL_REF) k = refcls;
                if (qc == PG_PL_Q_LOW) k = PG_PL_N;
                if (k == PG_PL_N) k = remove_ns ? (unsigned char)255 : (unsigned char)5;
                P.a += k == 0 ? 1u : 0u;
                P.t += k == 1 ? 1u : 0u;
                P.c += k == 2 ? 1u : 0u;
                P.g += k == 3 ? 1u : 0u;
                P.d += k == 4 ? 1u : 0u;
                P.n += k == 5 ? 1u : 0u;
            }
            ++j;
        }
        if (!P.err && (j != cov || nq != cov)) P.err = PG_PILEUP_E_MISMATCH;
    }
    *out = P;
}

// The pools from byte `p` of the line on (p at a pool's coverage field), one after the other, for their defects alone:
// what a line with more pools than pool sizes still has to pass before it is dropped.  Returns the smallest code.
PG_PL_HD int pg_pileup_tail(const unsigned char *line, int64_t p, int64_t len, unsigned char refcls, bool remove_ns, const unsigned char *cls,
                            const unsigned char *qcls) {
    int err = 0;
    while (p <= len) { // every round moves p behind at least one field
        int64_t ce = p;
        while (ce < len && line[ce] != '\t') ++ce;
        const bool have_r = ce < len;
        int64_t re = have_r ? ce + 1 : len;
        while (re < len && line[re] != '\t') ++re;
        const bool have_q = have_r && re < len;
        int64_t qe = have_q ? re + 1 : len;
        while (qe < len && line[qe] != '\t') ++qe;
        PgPileupPool P;
        pg_pileup_pool(line, p, ce, have_r, ce + 1, re, have_q, re + 1, qe, refcls, remove_ns, cls, qcls, &P);
        err = pg_pileup_min_code(err, P.err);
        if (!have_q) break;
        p = qe + 1;
    }
    return err;
}

// ---- the filter (PileupLine::filter) ------------------------------------------------------------------------------------------
// ceil(min_coverage_breadth x pools) as Rust's `as u32` casts it: NaN and negatives to 0, large values to u32::MAX
PG_PL_HD uint32_t pg_pileup_breadth_threshold(double breadth, int n_sizes) {
    const double t = ceil(breadth * (double)n_sizes);
    if (!(t > 0.0)) return 0u;
    if (t >= 4294967295.0) return 0xffffffffu;
    return (uint32_t)t;
}

PG_PL_HD uint32_t pg_pileup_depth(const PgPileupPool &P) { return P.a + P.t + P.c + P.g + P.d + P.n; } // below 2^31: a line is

// one pool's share of q for column 1 (T): frequency, then the product, two roundings, no contraction; 0 / 0 is NaN
PG_PL_HD double pg_pileup_q_term(uint32_t count, uint32_t depth, double pool_size) {
    const double f = (double)count / (double)depth;
    return f * pool_size;
}

// The loop of :311-331 starts at column j = 1 with m = 6 columns; a column that fails shrinks m and is tested AGAIN, a column
// that passes moves j on.  q of a column does not change between its tests, so a failing column 1 takes m down to 1 (dropped)
// and a passing column 1 leaves m >= 2 whatever the later columns do (m only shrinks while j < m): the first column decides.
PG_PL_HD bool pg_pileup_maf_pass(double q1, double maf) { return !((q1 < maf) | (q1 > (1.00 - maf))); }

// the key both sides minimise: the first bad line in file order, and of that line the smallest reason
PG_PL_HD uint64_t pg_pileup_err_key(int64_t line_off, int code) { return ((uint64_t)line_off << 8) | (uint64_t)(code & 0xff); }
constexpr uint64_t PG_PILEUP_NO_ERR = ~0ULL;
