// pg_hosttablefmt.cpp -- pg_host_f64_table: the host twin of the device table formatter (pg_tablefmt.hip).  Plain C++ on
// n_threads threads, no GPU, no context; it needs nothing but the public header and the shared rules of pg_table_cells.h /
// pg_f64_text.h, so this file also builds on its own with a plain C++ compiler.  Same steps as the device form: measure every
// element (and refuse a bad label), sum, then emit into the caller's buffer; the threads share the rows.
#include "../../include/poolgen_hip.h"
#include "pg_table_cells.h"
#include <algorithm>
#include <thread>
#include <vector>

extern "C" int pg_host_f64_table(const double *x, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride, int64_t row0, int64_t n_rows,
                                 int n_digits, int first_col_digits, const char *label_text, const int64_t *label_off, char *text, int64_t cap,
                                 int64_t *bytes, int n_threads) {
    if (!bytes) return PG_ERR_INVALID;
    *bytes = 0;
    if (rows < 0 || cols < 1 || row_stride < 0 || col_stride < 0 || cap < 0 || row0 < 0 || n_rows < 0 || row0 > rows || n_rows > rows - row0) return PG_ERR_INVALID;
    if (n_digits > PG_F64_MAX_ROUND_DIGITS || first_col_digits > PG_F64_MAX_ROUND_DIGITS || (cap > 0 && !text)) return PG_ERR_INVALID;
    if (n_rows > (((int64_t)1 << 39) - 1) / cols) return PG_ERR_INVALID;
    if (n_rows == 0) return PG_OK;
    if (!x || (label_off && !label_text)) return PG_ERR_INVALID;
    const PgTable T{x, cols, row_stride, col_stride, n_digits < 0 ? -1 : n_digits, first_col_digits < 0 ? -1 : first_col_digits,
                    reinterpret_cast<const unsigned char *>(label_text), label_off};
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, n_rows));
    const int64_t each = (n_rows + parts - 1) / parts;
    std::vector<int64_t> size(parts, 0);
    auto on_parts = [&](auto fn) { // fn(part, first row, end row) on a thread per part
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t) th.emplace_back([&, t] { fn(t, row0 + std::min(n_rows, t * each), row0 + std::min(n_rows, (t + 1) * each)); });
        fn(0, row0, row0 + std::min(n_rows, each));
        for (auto &h : th) h.join();
    };
    on_parts([&](int t, int64_t lo, int64_t hi) { // measure
        PgLenSink s{0};
        for (int64_t r = lo; r < hi; ++r) {
            if (T.label_len(r) < 0) { s.n = -1; break; }
            for (int64_t c = 0; c < cols; ++c) T.write(r, c, s);
        }
        size[t] = s.n;
    });
    int64_t total = 0;
    for (int t = 0; t < parts; ++t) {
        if (size[t] < 0) return PG_ERR_INVALID; // (a bad label: no size either)
        total += size[t];
    }
    *bytes = total;
    if (total > cap) return PG_ERR_INVALID;
    std::vector<int64_t> at(parts, 0);
    for (int t = 1; t < parts; ++t) at[t] = at[t - 1] + size[t - 1];
    on_parts([&](int t, int64_t lo, int64_t hi) { // emit
        PgPutSink s{reinterpret_cast<unsigned char *>(text) + at[t]};
        for (int64_t r = lo; r < hi; ++r)
            for (int64_t c = 0; c < cols; ++c) T.write(r, c, s);
    });
    return PG_OK;
}
