// pg_hostsyncfmt.cpp -- pg_host_sync_format_rows: the host twin of pg_sync_format_rows_dev (pg_syncfmt.hip).  Plain C++ on
// n_threads threads, no GPU, no context; it needs nothing but the public header and the shared rules of pg_sync_fmt.h, so it
// also builds on its own (the sanitizer build of tests/test_syncfmt_host.py).  Same steps as the device form: measure every
// row (and refuse a name outside the slab, a line that is too long), sum, then emit into the caller's buffer.
#include "../../include/poolgen_hip.h"
#include "pg_sync_fmt.h"
#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct SfHostRows {
    const char *slab;
    int64_t slab_bytes;
    const uint32_t *counts;
    const uint64_t *pos;
    const uint8_t *ref;
    const int64_t *line_off;
    const int32_t *chrom_len;
    int n;
};

// the length of row r; with dst, its text too.  -1: the name lies outside the slab, or the line is too long
int64_t sf_host_row(const SfHostRows &a, int64_t r, unsigned char *dst) {
    const uint32_t *row = a.counts + r * a.n * 6;
    const int32_t clen = a.chrom_len[r];
    if (!dst) {
        if (!pg_syncfmt_name_ok(a.line_off[r], clen, a.slab_bytes)) return -1;
        int64_t pools = 0;
        for (int j = 0; j < a.n; ++j) pools += pg_syncfmt_pool_len(row + j * 6);
        const int64_t len = pg_syncfmt_row_len(clen, a.pos[r], pools);
        return len > PG_SYNCFMT_MAX_ROW ? -1 : len;
    }
    if (clen > 0) std::memcpy(dst, a.slab + a.line_off[r], (size_t)clen);
    int64_t o = clen;
    o += pg_syncfmt_put_pos_ref(dst + o, a.pos[r], a.ref[r]);
    for (int j = 0; j < a.n; ++j) o += pg_syncfmt_put_pool(dst + o, row + j * 6);
    dst[o] = '\n';
    return o + 1;
}

} // namespace

extern "C" int pg_host_sync_format_rows(const char *slab, int64_t slab_bytes, const uint32_t *counts, const uint64_t *pos,
                                        const uint8_t *ref, const int64_t *line_off, const int32_t *chrom_len, int n_pools,
                                        int64_t rows, char *text, int64_t cap, int64_t *bytes, int n_threads) {
    if (!bytes) return PG_ERR_INVALID;
    *bytes = 0;
    if (n_pools < 1 || n_pools > PG_SYNCFMT_MAX_POOLS) return PG_ERR_INVALID;
    if (slab_bytes < 0 || rows < 0 || rows > ((int64_t)1 << 31) || cap < 0 || (cap > 0 && !text)) return PG_ERR_INVALID;
    if (rows == 0) return PG_OK;
    if ((!slab && slab_bytes != 0) || !counts || !pos || !ref || !line_off || !chrom_len) return PG_ERR_INVALID;
    const SfHostRows a{slab, slab_bytes, counts, pos, ref, line_off, chrom_len, n_pools};
    const int parts = (int)std::max<int64_t>(1, std::min<int64_t>(n_threads, rows));
    const int64_t each = (rows + parts - 1) / parts;
    std::vector<int64_t> size(parts, 0);
    auto on_parts = [&](auto fn) { // fn(part, first row, end row) on a thread per part
        std::vector<std::thread> th;
        for (int t = 1; t < parts; ++t) th.emplace_back([&, t] { fn(t, std::min(rows, t * each), std::min(rows, (t + 1) * each)); });
        fn(0, (int64_t)0, std::min(rows, each));
        for (auto &x : th) x.join();
    };
    on_parts([&](int t, int64_t lo, int64_t hi) { // measure
        int64_t sum = 0;
        for (int64_t r = lo; r < hi && sum >= 0; ++r) {
            const int64_t len = sf_host_row(a, r, nullptr);
            sum = len < 0 ? len : sum + len;
        }
        size[t] = sum;
    });
    int64_t total = 0;
    for (int t = 0; t < parts; ++t) {
        if (size[t] < 0) return PG_ERR_INVALID; // (a row that cannot be formatted: no size either)
        total += size[t];
    }
    *bytes = total;
    if (total > cap) return PG_ERR_INVALID;
    std::vector<int64_t> at(parts, 0);
    for (int t = 1; t < parts; ++t) at[t] = at[t - 1] + size[t - 1];
    on_parts([&](int t, int64_t lo, int64_t hi) { // emit
        unsigned char *dst = reinterpret_cast<unsigned char *>(text) + at[t];
        for (int64_t r = lo; r < hi; ++r) dst += sf_host_row(a, r, dst);
    });
    return PG_OK;
}
