// pg_resultfmt.hip -- the result writer: the CSV rows of the GWAS analyses (format_locus_rows and write_kinship_csv of the CLI)
// and the number text they are made of (pg_f64_text.h), formatted on the device.
//
// What is written is a sequence of UNITS (pg_result_rows.h): one value, one locus with all its rows, or one kinship row.  The
// structure is pg_syncfmt.hip's, three steps on the context's stream:
//   measure  k_rf_measure<Units>: the byte length of every unit (int32), a flag for a label out of range and for a unit that is
//            too long;
//   scan     PgLengthScan (pg_text_steps.h): k_scan_lengths (exclusive scan of PG_COUNT_ROWS = 256 lengths per workgroup, the longest
//            unit) + k_scan_blocks (64-bit exclusive scan of the workgroups' sums, PG_SCAN_WIDTH = 1024 per round): a unit's offset is
//            scan_off(u);
//   emit     k_rf_emit<Units, RF_STAGED>: a workgroup takes `upb` consecutive units -- one contiguous byte range of the output --
//            formats them into an LDS tile laid out like the 16-byte words of the output, then copies the tile out (tile_flush): whole
//            words by 16-byte stores (a lane a word, consecutive lanes consecutive words), the ragged head and tail by byte stores.  Two
//            workgroups meet inside a word only with byte stores; nothing is read back; nothing at or past the total is written.
//            k_rf_emit<Units, RF_DIRECT>: a unit longer than the tile goes to the output by byte stores.
// ONE LANE FORMATS ONE UNIT.  The work differs from the other formatters': a unit has two to four number cells, not hundreds, and
// a cell costs a few hundred integer instructions (three 64 x 128-bit products, the interval tests, the digit divisions), not a
// few.  There are millions of units and no dependence between them, so a lane per unit keeps all 64 lanes of a wave on the same
// instruction stream with no shuffle and no idle lane while units last; lanes diverge only where cells differ in kind (a second
// conversion for a rounded cell, a short cell against a long one).  The alternative, a lane per cell with the row's offsets from
// a scan over 4-lane groups, would shorten a lane's serial chain to one conversion but leave the label lane and the number lanes
// on different paths in every group (a quarter to a half of the lanes idle during the conversions) and add the shuffles; it
// pays only when units are too few to fill the machine, which the analyses' outputs are not.
// A conversion keeps its state in registers (pg_f64_parts_t: digits, exponent, count); digits go straight to their bytes: no
// array, no scratch.  The 128-bit powers of ten (pg_f64_pow10.h, 9872 bytes) are read-only device data.
#include "pg_common.h"
#include "pg_text_steps.h"
#include "pg_result_rows.h"
#include <algorithm>

static_assert(PG_F64_TEXT_MAX_LEN == PG_F64_TEXT_MAX && PG_RESULT_SLOTS == PG_MAX_OUT, "the public header's constants");
static_assert(PG_ROWS_FISHER == (int)PG_RESULT_FISHER && PG_ROWS_CHISQ == (int)PG_RESULT_CHISQ && PG_ROWS_GWALPHA == (int)PG_RESULT_GWALPHA &&
                  PG_ROWS_PEARSON == (int)PG_RESULT_PEARSON && PG_ROWS_OLS_ITER == (int)PG_RESULT_OLS_ITER, "enum pg_result_op");

namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_TILE = 16384; // bytes of text a workgroup stages (plus up to 15 in front of them: the word it starts in)
constexpr int RF_BAD_LABEL = 1, RF_BAD_LONG = 2;

// ---- measure -----------------------------------------------------------------------------------------------------------
template <class Units>
__global__ __launch_bounds__(RF_THREADS) void k_rf_measure(const Units U, int64_t u0, int64_t count, int32_t *__restrict__ unitlen,
                                                           PgScanCtl *__restrict__ ctl) {
    const int64_t u = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
    if (u >= count) return;
    int bad = 0;
    int64_t len = 0;
    if (!U.ok(u0 + u)) bad = RF_BAD_LABEL;
    else {
        PgLenSink s{0};
        U.write(u0 + u, s);
        len = s.n;
        if (len > PG_RESULT_UNIT_MAX) { bad = RF_BAD_LONG; len = 0; }
    }
    unitlen[u] = (int32_t)len;
    if (bad) atomicOr(&ctl->bad, bad);
}

// ---- emit --------------------------------------------------------------------------------------------------------------
enum { RF_STAGED = 0, RF_DIRECT = 1 }; // how k_rf_emit takes its units (the dispatch rule: rf_run)

// Launched with blockDim.x = a multiple of 64, at most RF_THREADS: as many lanes as a workgroup has units (RF_STAGED).
template <class Units, int MODE>
__global__ __launch_bounds__(RF_THREADS) void k_rf_emit(const Units U, int64_t u0, int64_t count, int upb, const int32_t *__restrict__ local,
                                                        const int64_t *__restrict__ blockoff, const PgScanCtl *__restrict__ ctl,
                                                        unsigned char *__restrict__ text) {
    const int tid = threadIdx.x, nthreads = blockDim.x;
    if (MODE == RF_DIRECT) { // a lane per unit, straight to the output
        const int64_t u = (int64_t)blockIdx.x * nthreads + tid;
        if (u < count) {
            PgPutSink s{text + scan_off(local, blockoff, ctl, u, count)};
            U.write(u0 + u, s);
        }
        return;
    }
    __shared__ __attribute__((aligned(16))) unsigned char tile[RF_TILE + 16];
    const int64_t u_lo = (int64_t)blockIdx.x * upb, u_hi = u_lo + upb < count ? u_lo + upb : count;
    const int64_t B = scan_off(local, blockoff, ctl, u_lo, count), E = scan_off(local, blockoff, ctl, u_hi, count);
    const int head = (int)((reinterpret_cast<uintptr_t>(text) + (uint64_t)B) & 15); // tile[head + i] is byte B + i of the output
    for (int64_t u = u_lo + tid; u < u_hi; u += nthreads) {
        PgPutSink s{tile + head + (int)(scan_off(local, blockoff, ctl, u, count) - B)};
        U.write(u0 + u, s);
    }
    __syncthreads();
    const int nbytes = (int)(E - B);                                  // <= RF_TILE: upb units of at most the longest unit's length
    tile_flush(tile, head, text + B, nbytes, tid, nthreads);
}

// units [u0, u0 + count) of U into text_dev; count >= 1 and the arguments checked
template <class Units>
int rf_run(pg_ctx *ctx, const char *who, const Units &U, int64_t u0, int64_t count, char *text_dev, int64_t cap, int64_t *bytes) {
    PG_HIP(ctx, hipSetDevice(ctx->device));
    PgLengthScan S;
    int rc = S.prepare(ctx, count);
    if (rc) return rc;
    const int64_t measure_blocks = (count + RF_THREADS - 1) / RF_THREADS;
    pg_prof_begin(ctx, PG_K_RESULTFMT);
    hipLaunchKernelGGL(k_rf_measure<Units>, dim3((unsigned)measure_blocks), dim3(RF_THREADS), 0, ctx->stream, U, u0, count, S.local, S.ctl);
    S.scan(ctx);
    pg_prof_end(ctx);
    PgScanCtl res{};
    rc = S.read(ctx, &res);
    if (rc) return rc;
    PG_CHECK(ctx, !(res.bad & RF_BAD_LABEL), "%s: a label is out of range (chromosome id, name offsets or allele id)", who);
    PG_CHECK(ctx, !(res.bad & RF_BAD_LONG), "%s: the text of one unit is longer than %d bytes", who, PG_RESULT_UNIT_MAX);
    *bytes = res.total;
    PG_CHECK(ctx, res.total <= cap, "%s: the text needs %lld bytes, the buffer holds %lld", who, (long long)res.total, (long long)cap);
    if (res.total == 0) return PG_OK; // (every locus dropped)
    unsigned char *text = reinterpret_cast<unsigned char *>(text_dev);
    pg_prof_begin(ctx, PG_K_RESULTFMT | PG_PROF_CONT);
    if (res.max > RF_TILE) { // the direct path: a unit does not fit the tile
        const int64_t blocks = (count + RF_THREADS - 1) / RF_THREADS;
        hipLaunchKernelGGL((k_rf_emit<Units, RF_DIRECT>), dim3((unsigned)blocks), dim3(RF_THREADS), 0, ctx->stream, U, u0, count, 0, S.local, S.boff, S.ctl, text);
    } else {
        const int upb = RF_TILE / std::max(1, res.max); // units per workgroup: upb units of at most the longest unit's length fit the tile
        const int threads = std::min(RF_THREADS, (upb + 63) & ~63);
        const int64_t blocks = (count + upb - 1) / upb;
        hipLaunchKernelGGL((k_rf_emit<Units, RF_STAGED>), dim3((unsigned)blocks), dim3(threads), 0, ctx->stream, U, u0, count, upb, S.local, S.boff, S.ctl, text);
    }
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}

} // namespace

extern "C" int pg_f64_text_dev(pg_ctx *ctx, const double *x_dev, int64_t count, int n_digits, char *text_dev, int64_t cap, int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "f64_text: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, count >= 0 && count <= ((int64_t)1 << 31) && cap >= 0, "f64_text: bad shape count=%lld cap=%lld", (long long)count, (long long)cap);
    PG_CHECK(ctx, n_digits <= PG_F64_MAX_ROUND_DIGITS, "f64_text: n_digits=%d (at most %d; negative prints the value as it is)", n_digits,
             PG_F64_MAX_ROUND_DIGITS);
    PG_CHECK(ctx, cap == 0 || text_dev, "f64_text: null text buffer");
    if (count == 0) return PG_OK;
    PG_CHECK(ctx, x_dev != nullptr, "f64_text: null pointer");
    return rf_run(ctx, "f64_text", PgF64Units{x_dev, n_digits < 0 ? -1 : n_digits}, 0, count, text_dev, cap, bytes);
}

extern "C" int pg_result_rows_dev(pg_ctx *ctx, int op, int64_t L, int k, const int32_t *n_out_dev, const int32_t *allele_ids_dev,
                                  const double *mean_freq_dev, const double *stat_dev, const double *pval_dev, const int32_t *locus_chrom_dev,
                                  const uint64_t *locus_pos_dev, const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom,
                                  char *text_dev, int64_t cap, int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "result_rows: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, op >= PG_RESULT_FISHER && op <= PG_RESULT_OLS_ITER, "result_rows: op=%d is no pg_result_op", op);
    PG_CHECK(ctx, L >= 0 && L <= ((int64_t)1 << 31) && cap >= 0 && n_chrom >= 0, "result_rows: bad shape L=%lld cap=%lld n_chrom=%d", (long long)L,
             (long long)cap, n_chrom);
    const bool per_locus = op == PG_RESULT_FISHER || op == PG_RESULT_CHISQ;
    if (per_locus || op == PG_RESULT_GWALPHA) k = 1;
    PG_CHECK(ctx, k >= 1 && k <= PG_RESULT_MAX_TRAITS, "result_rows: k=%d traits (1 to %d are formatted)", k, PG_RESULT_MAX_TRAITS);
    PG_CHECK(ctx, cap == 0 || text_dev, "result_rows: null text buffer");
    if (L == 0) return PG_OK;
    PG_CHECK(ctx, n_out_dev && allele_ids_dev && stat_dev && locus_chrom_dev && locus_pos_dev && chrom_off_dev && (chrom_text_dev || n_chrom == 0) &&
                      (per_locus || mean_freq_dev) && (op == PG_RESULT_GWALPHA || pval_dev),
             "result_rows: null pointer");
    const PgResultUnits U{op, L, k, n_out_dev, allele_ids_dev, mean_freq_dev, stat_dev, pval_dev, locus_chrom_dev, locus_pos_dev,
                          PgNames{reinterpret_cast<const unsigned char *>(chrom_text_dev), chrom_off_dev, n_chrom}};
    return rf_run(ctx, "result_rows", U, 0, L, text_dev, cap, bytes);
}

extern "C" int pg_gudmc_rows_dev(pg_ctx *ctx, int n, int64_t w, int64_t row0, int64_t rows, const int64_t *rows_dev, const double *d_mean_dev,
                                 const double *d_sd_dev, const double *fst_mean_dev, const double *fst_sd_dev, const int64_t *row_window_dev,
                                 const double *row_d_dev, const double *row_width_dev, const double *row_width_from_r_dev,
                                 const double *row_width_p_dev, const double *row_fst_delta_dev, const double *row_fst_p_dev,
                                 const int32_t *win_chr_dev, const uint64_t *win_ini_dev, const uint64_t *win_fin_dev,
                                 const char *pool_text_dev, const int32_t *pool_off_dev, const char *chrom_text_dev,
                                 const int32_t *chrom_off_dev, int n_chrom, char *text_dev, int64_t cap, int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "gudmc_rows: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, n >= 1 && w >= 1 && row0 >= 0 && rows >= 0 && rows <= ((int64_t)1 << 31) && cap >= 0 && n_chrom >= 0,
             "gudmc_rows: bad shape n=%d w=%lld row0=%lld rows=%lld cap=%lld n_chrom=%d", n, (long long)w, (long long)row0, (long long)rows,
             (long long)cap, n_chrom);
    PG_CHECK(ctx, cap == 0 || text_dev, "gudmc_rows: null text buffer");
    PG_CHECK(ctx, rows_dev != nullptr, "gudmc_rows: null pointer");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int64_t> first((size_t)n + 1, 0); // the populations' rows come down, for the prefix sum
    PG_HIP(ctx, hipMemcpyAsync(first.data() + 1, rows_dev, sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < n; ++b) {
        PG_CHECK(ctx, first[b + 1] >= 0 && first[b + 1] <= w, "gudmc_rows: population %d has %lld rows of %lld windows", b, (long long)first[b + 1],
                 (long long)w);
        first[b + 1] += first[b];
    }
    PG_CHECK(ctx, first[n] <= INT64_MAX / n && row0 <= first[n] * n - rows, "gudmc_rows: rows [%lld, %lld) of %lld", (long long)row0,
             (long long)(row0 + rows), (long long)(first[n] <= INT64_MAX / n ? first[n] * n : -1));
    if (rows == 0) return PG_OK;
    PG_CHECK(ctx, d_mean_dev && d_sd_dev && fst_mean_dev && fst_sd_dev && row_window_dev && row_d_dev && row_width_dev && row_width_from_r_dev &&
                      row_width_p_dev && row_fst_delta_dev && row_fst_p_dev && win_chr_dev && win_ini_dev && win_fin_dev &&
                      pool_off_dev && chrom_off_dev && (chrom_text_dev || n_chrom == 0),
             "gudmc_rows: null pointer");
    DevBuf<int64_t> first_dev;
    int rc = first_dev.alloc(ctx, sizeof(int64_t) * first.size(), "gudmc_rows");
    if (rc) return rc;
    PG_HIP(ctx, hipMemcpyAsync(first_dev.get(), first.data(), sizeof(int64_t) * first.size(), hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (`first` has been read)
    const PgGudmcUnits U{n, w, first_dev.get(), d_mean_dev, d_sd_dev, fst_mean_dev, fst_sd_dev, row_window_dev, row_d_dev, row_width_dev,
                         row_width_from_r_dev, row_width_p_dev, row_fst_delta_dev, row_fst_p_dev, win_chr_dev, win_ini_dev, win_fin_dev,
                         PgNames{reinterpret_cast<const unsigned char *>(pool_text_dev), pool_off_dev, n},
                         PgNames{reinterpret_cast<const unsigned char *>(chrom_text_dev), chrom_off_dev, n_chrom}};
    rc = rf_run(ctx, "gudmc_rows", U, row0, rows, text_dev, cap, bytes);
    if (rc == PG_OK) PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // first_dev goes with this call
    return rc;
}

extern "C" int pg_kinship_rows_dev(pg_ctx *ctx, int64_t p, int k, int64_t row0, int64_t rows, const double *beta_dev, const double *pval_dev,
                                   const int32_t *col_chrom_dev, const uint64_t *col_pos_dev, const int32_t *col_allele_dev,
                                   const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom, char *text_dev, int64_t cap,
                                   int64_t *bytes) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, bytes != nullptr, "kinship_rows: null pointer");
    *bytes = 0;
    PG_CHECK(ctx, p >= 1 && k >= 1 && k <= PG_RESULT_MAX_TRAITS && row0 >= 0 && rows >= 0 && rows <= ((int64_t)1 << 31) && cap >= 0 && n_chrom >= 0,
             "kinship_rows: bad shape p=%lld k=%d row0=%lld rows=%lld cap=%lld n_chrom=%d", (long long)p, k, (long long)row0, (long long)rows,
             (long long)cap, n_chrom);
    PG_CHECK(ctx, p <= INT64_MAX / k && row0 <= p * k - rows, "kinship_rows: rows [%lld, %lld) of %lld x %d", (long long)row0,
             (long long)(row0 + rows), (long long)p, k);
    PG_CHECK(ctx, cap == 0 || text_dev, "kinship_rows: null text buffer");
    if (rows == 0) return PG_OK;
    PG_CHECK(ctx, beta_dev && pval_dev && (p == 1 || (col_chrom_dev && col_pos_dev && col_allele_dev && chrom_off_dev && (chrom_text_dev || n_chrom == 0))),
             "kinship_rows: null pointer");
    const PgKinshipUnits U{p, k, beta_dev, pval_dev, col_chrom_dev, col_pos_dev, col_allele_dev,
                           PgNames{reinterpret_cast<const unsigned char *>(chrom_text_dev), chrom_off_dev, n_chrom}};
    return rf_run(ctx, "kinship_rows", U, row0, rows, text_dev, cap, bytes);
}
