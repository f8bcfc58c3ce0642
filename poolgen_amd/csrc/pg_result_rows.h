// pg_result_rows.h -- the rows of the result writer, shared by the device formatter (pg_resultfmt.hip) and its host twin
// (pg_hostresultfmt.cpp): what a UNIT of text is made of and how it is written, once, for both sides.
//
// A unit is the piece of text one lane (or one turn of a host loop) writes, and the pieces follow each other in unit order:
//   PgF64Units      one value and its '\n'                                    (pg_f64_text_dev / pg_host_f64_text)
//   PgResultUnits   one locus with all its rows: slots, then traits           (pg_result_rows_dev / pg_host_result_rows)
//   PgKinshipUnits  one row  label_i,Pheno_j,D(beta),D(pval)                  (pg_kinship_rows_dev / pg_host_kinship_rows)
//   PgGudmcUnits    one row of gudmc's file, 15 fields                        (pg_gudmc_rows_dev / pg_host_gudmc_rows)
// Every kind has  bool ok(u)  (may the unit's labels be read and printed?) and  template <class Sink> void write(u, sink).
// A unit is written into a SINK: PgLenSink only adds the lengths up (the measure half), PgPutSink stores the bytes (the emit
// half).  The number cells are pg_f64_text.h's: D(x) = display, R(x, nd) = roundup_own.
#pragma once
#include "pg_f64_text.h"

constexpr int PG_RESULT_UNIT_MAX = 1 << 22; // bytes of one unit's text (a longer one is refused): 256 of them still sum in an int32
constexpr int PG_RESULT_SLOTS = 5;          // PG_MAX_OUT of the public header

struct PgLenSink {
    int64_t n;
    PG_F64_HD void ch(unsigned char) { n += 1; }
    PG_F64_HD void bytes(const unsigned char *, int len) { n += len; }
    PG_F64_HD void u64(uint64_t v) { n += pg_f64_digits64(v); }
    PG_F64_HD void f64(const pg_f64_parts_t &p) { n += pg_f64_len(p); }
};

struct PgPutSink {
    unsigned char *p;
    PG_F64_HD void ch(unsigned char c) { *p++ = c; }
    PG_F64_HD void bytes(const unsigned char *s, int len) {
        for (int i = 0; i < len; ++i) p[i] = s[i];
        p += len;
    }
    PG_F64_HD void u64(uint64_t v) {
        const int nd = pg_f64_digits64(v);
        pg_f64_put_u64(p, v, nd, nd);
        p += nd;
    }
    PG_F64_HD void f64(const pg_f64_parts_t &x) { p += pg_f64_put(p, x); }
};

// the letter of allele `al` (an index into "ATCGND")
PG_F64_HD unsigned char pg_result_allele(int al) { return (unsigned char)((0x444E47435441ULL >> (8 * (al & 7))) & 0xff); }

template <class Sink>
PG_F64_HD void pg_result_pheno(Sink &s, int j) { // "Pheno_<j>"
    s.ch('P'); s.ch('h'); s.ch('e'); s.ch('n'); s.ch('o'); s.ch('_');
    s.u64((uint64_t)j);
}

// the name table: n_chrom names in one byte string, n_chrom + 1 offsets
struct PgNames {
    const unsigned char *text;
    const int32_t *off;
    int n_chrom;
    PG_F64_HD bool ok(int cid) const { return cid >= 0 && cid < n_chrom && off[cid] >= 0 && off[cid + 1] >= off[cid]; }
    template <class Sink>
    PG_F64_HD void write(int cid, Sink &s) const {
        const int a = off[cid];
        s.bytes(text + a, off[cid + 1] - a);
    }
};

struct PgF64Units {
    const double *x;
    int nd;
    PG_F64_HD bool ok(int64_t) const { return true; }
    template <class Sink>
    PG_F64_HD void write(int64_t u, Sink &s) const {
        s.f64(pg_f64_cell(x[u], nd));
        s.ch('\n');
    }
};

enum { PG_ROWS_FISHER = 0, PG_ROWS_CHISQ = 1, PG_ROWS_GWALPHA = 2, PG_ROWS_PEARSON = 3, PG_ROWS_OLS_ITER = 4 }; // enum pg_result_op

struct PgResultUnits {
    int op;
    int64_t L;
    int k;
    const int32_t *n_out, *ids; // ids, freq: element (slot r, locus l) at r * L + l; stat, pval: at (r * L + l) * k + trait
    const double *freq, *stat, *pval;
    const int32_t *chrom;
    const uint64_t *pos;
    PgNames names;

    PG_F64_HD int slots(int64_t l) const {
        const int n = n_out[l];
        return n <= 0 ? 0 : n < PG_RESULT_SLOTS ? n : PG_RESULT_SLOTS;
    }
    PG_F64_HD bool ok(int64_t l) const {
        const int n = slots(l);
        if (n == 0) return true; // nothing of a dropped locus is read
        if (!names.ok(chrom[l])) return false;
        for (int r = 0; r < n; ++r) {
            const int al = ids[r * L + l];
            if (al < 0 || al >= 6) return false;
        }
        return true;
    }
    template <class Sink>
    PG_F64_HD void label(int64_t l, Sink &s) const { // "chr,pos,"
        names.write(chrom[l], s);
        s.ch(',');
        s.u64(pos[l]);
        s.ch(',');
    }
    template <class Sink>
    PG_F64_HD void write(int64_t l, Sink &s) const {
        const int n = slots(l);
        if (n == 0) return;
        if (op == PG_ROWS_FISHER || op == PG_ROWS_CHISQ) { // one row: the letters of all slots, stat[l], pval[l]
            label(l, s);
            for (int r = 0; r < n; ++r) s.ch(pg_result_allele(ids[r * L + l]));
            s.ch(',');
            s.f64(pg_f64_cell(stat[l], op == PG_ROWS_CHISQ ? 6 : -1));
            s.ch(',');
            s.f64(pg_f64_parts(pval[l]));
            s.ch('\n');
            return;
        }
        for (int r = 0; r < n; ++r) {
            const int64_t e = r * L + l;
            const unsigned char letter = pg_result_allele(ids[e]);
            const double f = freq[e];
            if (op == PG_ROWS_GWALPHA) {
                label(l, s);
                s.ch(letter); s.ch(',');
                s.f64(pg_f64_cell(f, 6));
                s.ch(',');
                pg_result_pheno(s, 0);
                s.ch(',');
                s.f64(pg_f64_cell(stat[e], 6));
                s.ch(','); s.ch('U'); s.ch('n'); s.ch('k'); s.ch('n'); s.ch('o'); s.ch('w'); s.ch('n'); s.ch('\n');
                continue;
            }
            const bool ols = op == PG_ROWS_OLS_ITER;
            const pg_f64_parts_t fp = pg_f64_cell(f, ols ? 8 : -1); // the same cell in the rows of every trait
            for (int j = 0; j < k; ++j) {
                label(l, s);
                s.ch(letter); s.ch(',');
                s.f64(fp);
                s.ch(',');
                pg_result_pheno(s, j);
                s.ch(',');
                s.f64(pg_f64_cell(stat[e * k + j], 6));
                s.ch(',');
                s.f64(pg_f64_cell(pval[e * k + j], ols ? 12 : -1));
                s.ch('\n');
            }
        }
    }
};

// gudmc's rows from pg_gudmc_dev's outputs as they lie (pitch w).  The rows of the file run pair by pair, pair i = a * n + b
// with the rows of population b, so global row r lies where the prefix sums of rows[i % n] place it: first[b] = the rows of the
// populations in front of b, first[n] = R those of all, and r = a * R + first[b] + j is row j of pair (a, b).
struct PgGudmcUnits {
    int n;
    int64_t w;
    const int64_t *first; // n + 1
    const double *d_mean, *d_sd, *f_mean, *f_sd;
    const int64_t *r_win;
    const double *r_d, *r_width, *r_wdev, *r_wp, *r_delta, *r_fp;
    const int32_t *win_chr;
    const uint64_t *win_ini, *win_fin;
    PgNames pools, chroms;

    PG_F64_HD void place(int64_t r, int *a, int *b, int64_t *e) const {
        const int64_t R = first[n], qa = r / R, rem = r - qa * R;
        int lo = 0, hi = n - 1; // the last population with first[b] <= rem: one without rows is passed over
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (first[mid] <= rem) lo = mid;
            else hi = mid - 1;
        }
        *a = (int)qa;
        *b = lo;
        *e = (qa * n + lo) * w + (rem - first[lo]);
    }
    PG_F64_HD bool ok(int64_t r) const {
        int a, b;
        int64_t e;
        place(r, &a, &b, &e);
        const int64_t win = r_win[e];
        return pools.ok(a) && pools.ok(b) && win >= 0 && win < w && chroms.ok(win_chr[win]);
    }
    template <class Sink>
    PG_F64_HD void write(int64_t r, Sink &s) const {
        int a, b;
        int64_t e;
        place(r, &a, &b, &e);
        const int64_t i = (int64_t)a * n + b, win = r_win[e];
        pools.write(a, s); s.ch(',');
        pools.write(b, s); s.ch(',');
        chroms.write(win_chr[win], s); s.ch(',');
        s.u64(win_ini[win]); s.ch(',');
        s.u64(win_fin[win]); s.ch(',');
        s.f64(pg_f64_cell(d_mean[b], 7)); s.ch(',');
        s.f64(pg_f64_cell(f_mean[i], 7)); s.ch(',');
        s.f64(pg_f64_cell(d_sd[b], 7)); s.ch(',');
        s.f64(pg_f64_cell(f_sd[i], 7)); s.ch(',');
        s.f64(pg_f64_parts(r_d[e])); s.ch(',');
        s.f64(pg_f64_parts(r_width[e])); s.ch(',');
        s.f64(pg_f64_parts(r_wdev[e])); s.ch(',');
        s.f64(pg_f64_cell(r_wp[e], 7)); s.ch(',');
        s.f64(pg_f64_cell(r_delta[e], 7)); s.ch(',');
        s.f64(pg_f64_cell(r_fp[e], 7)); s.ch('\n');
    }
};

struct PgKinshipUnits {
    int64_t p;
    int k;
    const double *beta, *pval;
    const int32_t *col_chrom;
    const uint64_t *col_pos;
    const int32_t *col_allele;
    PgNames names;

    PG_F64_HD bool ok(int64_t r) const {
        const int64_t i = r % p;
        if (i == 0) return true;
        const int al = col_allele[i - 1];
        return names.ok(col_chrom[i - 1]) && al >= 0 && al < 6;
    }
    template <class Sink>
    PG_F64_HD void write(int64_t r, Sink &s) const {
        const int64_t j = r / p, i = r - j * p; // trait-major
        if (i == 0) {                           // "intercept,0,intercept"
            for (int t = 0; t < 2; ++t) {
                s.ch('i'); s.ch('n'); s.ch('t'); s.ch('e'); s.ch('r'); s.ch('c'); s.ch('e'); s.ch('p'); s.ch('t');
                if (t == 0) { s.ch(','); s.ch('0'); s.ch(','); }
            }
        } else { // the label of column i - 1: the reference's shift (ols.rs:421-425)
            names.write(col_chrom[i - 1], s);
            s.ch(',');
            s.u64(col_pos[i - 1]);
            s.ch(',');
            s.ch(pg_result_allele(col_allele[i - 1]));
        }
        s.ch(',');
        pg_result_pheno(s, (int)j);
        s.ch(',');
        s.f64(pg_f64_parts(beta[i * k + j]));
        s.ch(',');
        s.f64(pg_f64_parts(pval[i * k + j]));
        s.ch('\n');
    }
};
