// pg_hostresultfmt.cpp -- pg_host_f64_text, pg_host_result_rows, pg_host_kinship_rows: the host twins of the device result
// writer (pg_resultfmt.hip).  Plain C++ on n_threads threads, no GPU, no context; they need nothing but the public header and
// the shared rules of pg_result_rows.h / pg_f64_text.h, so this file also builds on its own with a plain C++ compiler (the
// sanitizer build of tests/test_resultfmt_host.py).  Same steps as the device forms: measure every unit (and refuse a label out
// of range, a unit that is too long), sum, then emit into the caller's buffer.
#include "../../include/poolgen_hip.h"
#include "pg_result_rows.h"
#include <algorithm>
#include <thread>
#include <vector>

static_assert(PG_F64_TEXT_MAX_LEN == PG_F64_TEXT_MAX && PG_RESULT_SLOTS == PG_MAX_OUT, "the public header's constants");
static_assert(PG_ROWS_FISHER == (int)PG_RESULT_FISHER && PG_ROWS_CHISQ == (int)PG_RESULT_CHISQ && PG_ROWS_GWALPHA == (int)PG_RESULT_GWALPHA &&
                  PG_ROWS_PEARSON == (int)PG_RESULT_PEARSON && PG_ROWS_OLS_ITER == (int)PG_RESULT_OLS_ITER, "enum pg_result_op");

namespace {

// units [u0, u0 + count) of U into text; the conventions of the public header
template <class Units>
int rf_host_run(const Units &U, int64_t u0, int64_t count, char *text, int64_t cap, int64_t *bytes, int n_threads) {
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, count));
    const int64_t each = (count + parts - 1) / parts;
    std::vector<int64_t> size(parts, 0);
    auto on_parts = [&](auto fn) { // fn(part, first unit, end unit) on a thread per part
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t) th.emplace_back([&, t] { fn(t, std::min(count, t * each), std::min(count, (t + 1) * each)); });
        fn(0, (int64_t)0, std::min(count, each));
        for (auto &x : th) x.join();
    };
    on_parts([&](int t, int64_t lo, int64_t hi) { // measure
        int64_t sum = 0;
        for (int64_t i = lo; i < hi; ++i) {
            if (!U.ok(u0 + i)) { sum = -1; break; }
            PgLenSink s{0};
            U.write(u0 + i, s);
            if (s.n > PG_RESULT_UNIT_MAX) { sum = -1; break; }
            sum += s.n;
        }
        size[t] = sum;
    });
    int64_t total = 0;
    for (int t = 0; t < parts; ++t) {
        if (size[t] < 0) return PG_ERR_INVALID; // (a unit that cannot be formatted: no size either)
        total += size[t];
    }
    *bytes = total;
    if (total > cap) return PG_ERR_INVALID;
    std::vector<int64_t> at(parts, 0);
    for (int t = 1; t < parts; ++t) at[t] = at[t - 1] + size[t - 1];
    on_parts([&](int t, int64_t lo, int64_t hi) { // emit
        PgPutSink s{reinterpret_cast<unsigned char *>(text) + at[t]};
        for (int64_t i = lo; i < hi; ++i) U.write(u0 + i, s);
    });
    return PG_OK;
}

bool rf_host_shape_ok(int64_t count, char *text, int64_t cap) { return count >= 0 && count <= ((int64_t)1 << 31) && cap >= 0 && (cap == 0 || text); }

} // namespace

extern "C" int pg_host_f64_text(const double *x, int64_t count, int n_digits, char *text, int64_t cap, int64_t *bytes, int n_threads) {
    if (!bytes) return PG_ERR_INVALID;
    *bytes = 0;
    if (!rf_host_shape_ok(count, text, cap) || n_digits > PG_F64_MAX_ROUND_DIGITS) return PG_ERR_INVALID;
    if (count == 0) return PG_OK;
    if (!x) return PG_ERR_INVALID;
    return rf_host_run(PgF64Units{x, n_digits < 0 ? -1 : n_digits}, 0, count, text, cap, bytes, n_threads);
}

extern "C" int pg_host_result_rows(int op, int64_t L, int k, const int32_t *n_out, const int32_t *allele_ids, const double *mean_freq,
                                   const double *stat, const double *pval, const int32_t *locus_chrom, const uint64_t *locus_pos,
                                   const char *chrom_text, const int32_t *chrom_off, int n_chrom, char *text, int64_t cap, int64_t *bytes,
                                   int n_threads) {
    if (!bytes) return PG_ERR_INVALID;
    *bytes = 0;
    if (op < PG_RESULT_FISHER || op > PG_RESULT_OLS_ITER || !rf_host_shape_ok(L, text, cap) || n_chrom < 0) return PG_ERR_INVALID;
    const bool per_locus = op == PG_RESULT_FISHER || op == PG_RESULT_CHISQ;
    if (per_locus || op == PG_RESULT_GWALPHA) k = 1;
    if (k < 1 || k > PG_RESULT_MAX_TRAITS) return PG_ERR_INVALID;
    if (L == 0) return PG_OK;
    if (!n_out || !allele_ids || !stat || !locus_chrom || !locus_pos || !chrom_off || (!chrom_text && n_chrom > 0) || (!per_locus && !mean_freq) ||
        (op != PG_RESULT_GWALPHA && !pval))
        return PG_ERR_INVALID;
    const PgResultUnits U{op, L, k, n_out, allele_ids, mean_freq, stat, pval, locus_chrom, locus_pos,
                          PgNames{reinterpret_cast<const unsigned char *>(chrom_text), chrom_off, n_chrom}};
    return rf_host_run(U, 0, L, text, cap, bytes, n_threads);
}

extern "C" int pg_host_gudmc_rows(int n, int64_t w, int64_t row0, int64_t rows, const int64_t *pop_rows, const double *d_mean, const double *d_sd,
                                  const double *fst_mean, const double *fst_sd, const int64_t *row_window, const double *row_d,
                                  const double *row_width, const double *row_width_from_r, const double *row_width_p,
                                  const double *row_fst_delta, const double *row_fst_p, const int32_t *win_chr, const uint64_t *win_ini,
                                  const uint64_t *win_fin, const char *pool_text, const int32_t *pool_off, const char *chrom_text,
                                  const int32_t *chrom_off, int n_chrom, char *text, int64_t cap, int64_t *bytes, int n_threads) {
    if (!bytes) return PG_ERR_INVALID;
    *bytes = 0;
    if (n < 1 || w < 1 || row0 < 0 || !rf_host_shape_ok(rows, text, cap) || n_chrom < 0 || !pop_rows) return PG_ERR_INVALID;
    std::vector<int64_t> first((size_t)n + 1, 0);
    for (int b = 0; b < n; ++b) {
        if (pop_rows[b] < 0 || pop_rows[b] > w) return PG_ERR_INVALID;
        first[b + 1] = first[b] + pop_rows[b];
    }
    if (first[n] > INT64_MAX / n || row0 > first[n] * n - rows) return PG_ERR_INVALID;
    if (rows == 0) return PG_OK;
    if (!d_mean || !d_sd || !fst_mean || !fst_sd || !row_window || !row_d || !row_width || !row_width_from_r || !row_width_p || !row_fst_delta ||
        !row_fst_p || !win_chr || !win_ini || !win_fin || !pool_off || !chrom_off || (!chrom_text && n_chrom > 0))
        return PG_ERR_INVALID;
    const PgGudmcUnits U{n, w, first.data(), d_mean, d_sd, fst_mean, fst_sd, row_window, row_d, row_width, row_width_from_r, row_width_p,
                         row_fst_delta, row_fst_p, win_chr, win_ini, win_fin,
                         PgNames{reinterpret_cast<const unsigned char *>(pool_text), pool_off, n},
                         PgNames{reinterpret_cast<const unsigned char *>(chrom_text), chrom_off, n_chrom}};
    return rf_host_run(U, row0, rows, text, cap, bytes, n_threads);
}

extern "C" int pg_host_kinship_rows(int64_t p, int k, int64_t row0, int64_t rows, const double *beta, const double *pval,
                                    const int32_t *col_chrom, const uint64_t *col_pos, const int32_t *col_allele, const char *chrom_text,
                                    const int32_t *chrom_off, int n_chrom, char *text, int64_t cap, int64_t *bytes, int n_threads) {
    if (!bytes) return PG_ERR_INVALID;
    *bytes = 0;
    if (p < 1 || k < 1 || k > PG_RESULT_MAX_TRAITS || row0 < 0 || !rf_host_shape_ok(rows, text, cap) || n_chrom < 0) return PG_ERR_INVALID;
    if (p > INT64_MAX / k || row0 > p * k - rows) return PG_ERR_INVALID;
    if (rows == 0) return PG_OK;
    if (!beta || !pval || (p > 1 && (!col_chrom || !col_pos || !col_allele || !chrom_off || (!chrom_text && n_chrom > 0)))) return PG_ERR_INVALID;
    const PgKinshipUnits U{p, k, beta, pval, col_chrom, col_pos, col_allele,
                           PgNames{reinterpret_cast<const unsigned char *>(chrom_text), chrom_off, n_chrom}};
    return rf_host_run(U, row0, rows, text, cap, bytes, n_threads);
}
