// pg_gudmc.hip -- the stage popgen::gudmc (popgen/gudmc.rs:64-462) puts on top of the per-window Tajima's D (pg_tajima_d_dev) and
// the per-window pairwise Fst (pg_fst_dev): three families of Nelder-Mead normal fits (ml_normal_1d, :39-60) -- D per population,
// Fst per population pair, trough / peak width per population pair -- and one row per (pair, row of population b) with the width
// of the run the row belongs to, its deviation from the recombination width and two one-tailed p-values.
//
//   k_nf_moments  thread = column of a row-major table: count, mean and sum (x - mean)^2 of its non-NaN entries, rows in order
//                 (coalesced across the columns); with ROUND8 every entry is first rounded as tajima_d prints it (tajima_d.rs:164)
//   k_nf_fit      thread = fit.  The reference's cost is a left-to-right sum of -ln_pdf over the column (:15-29), O(rows) per
//                 evaluation; it depends on the data through (count, mean, sum (x - mean)^2) alone:
//                     cost(mu, sigma) = count (LN_SQRT_2PI + ln sigma) + (sum (x - mean)^2 + count (mean - mu)^2) / (2 sigma^2)
//                 so an evaluation is O(1).  The lanes of a wave walk one state machine whose every turn holds ONE cost, whatever
//                 step each fit is in (as k_gw_fit does); a lane whose fit has ended takes the next column from a device-wide
//                 cursor.  About one fit in six runs to the 10 000-iteration cap (the cost's last-bit noise keeps the sd of the
//                 three costs above EPSILON) against a median of ~130: without the cursor a wave would idle 63 lanes behind one.
//                 A fit's arithmetic depends on its three moments alone, so its result does not depend on the batch.
//   k_gd_scan     thread = population: the reference's sequential scan (:168-208) over the population's non-NaN windows --
//                 NaN windows are compacted away and row j takes the label of window j of the UNFILTERED list (a defect of the
//                 reference that is kept) -- significance |d - mean| >= sigma_threshold, widths as integers
//   k_gd_rows     thread = (pair, row): Fst of the row's window, delta, the two p-values, the width's deviation
// The solver is argmin 0.8's Nelder-Mead as pg_mle.hip, pg_gwalpha.hip and the oracle word it, from
// prepare_solver_neldermead(2, 1) (helpers.rs:132-146), on (mu, x) with sigma = EPSILON + (1e24 - EPSILON) / (1 + e^-x).
#include "pg_common.h"
#include "pg_stats_device.h"
#include <cmath>
#include <vector>

namespace {

constexpr int NF_D = 2, NF_V = 3;
constexpr int NF_MAXIT = 10000;                          // .configure(|state| state.max_iters(10_000)), gudmc.rs:42
constexpr double NF_UPPER = 1e24;                        // PARAMETER_UPPER_LIMIT, gudmc.rs:13
constexpr double NF_LN_SQRT_2PI = 0.91893853320467274178032973640561763986139747363778341281715154; // statrs consts::LN_SQRT_2PI
constexpr double NF_SQRT_2 = 1.4142135623730951;        // f64::consts::SQRT_2

enum { NF_FETCH = 0, NF_INIT, NF_REFLECT, NF_EXPAND, NF_CONTRACT, NF_SHRINK, NF_DONE };

// tajima_d writes D with parse_f64_roundup_and_own(x, 8) and gudmc parses the file: round half away from zero at 8 decimals;
// inf and NaN pass through
__device__ __forceinline__ double nf_round8(double x) { return round(x * 1e8) / 1e8; }

// mom: [count: cols][mean: cols][ss: cols]; bad is set where a column holds +-inf (the reference's cost is NaN, Normal::new panics)
template <bool ROUND8>
__global__ __launch_bounds__(256) void k_nf_moments(const double *__restrict__ T, int64_t rows, int64_t cols, int64_t ld,
                                                    double *__restrict__ mom, int64_t *__restrict__ count_out,
                                                    int *__restrict__ bad) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    int64_t cnt = 0;
    double s = 0.0;
    bool inf = false;
    for (int64_t r = 0; r < rows; ++r) {
        double x = T[r * ld + c];
        if (ROUND8) x = nf_round8(x);
        if (x != x) continue;
        inf = inf || isinf(x);
        s = s + x;
        ++cnt;
    }
    const double mean = s / (double)cnt;
    double ss = 0.0;
    for (int64_t r = 0; r < rows; ++r) {
        double x = T[r * ld + c];
        if (ROUND8) x = nf_round8(x);
        if (x != x) continue;
        ss = ss + (x - mean) * (x - mean);
    }
    mom[c] = (double)cnt;
    mom[cols + c] = mean;
    mom[2 * cols + c] = ss;
    if (count_out) count_out[c] = cnt;
    if (inf) atomicOr(bad, 1);
}

// bound_parameters_with_logit(x, EPSILON, 1e24) (helpers.rs:120-130, gudmc.rs:12-13)
__device__ __forceinline__ double nf_sigma(double x) { return PG_EPS + ((NF_UPPER - PG_EPS) / (1.00 + exp(-x))); }

__device__ __forceinline__ double nf_cost(double cnt, double mean, double ss, double mu, double x) {
    if (cnt == 0.0) return 0.0; // the fold over an empty column
    const double s = nf_sigma(x);
    const double dm = mean - mu;
    return cnt * (NF_LN_SQRT_2PI + log(s)) + (0.5 * (ss + cnt * (dm * dm))) / (s * s);
}

__global__ __launch_bounds__(64) void k_nf_fit(const double *__restrict__ mom, int64_t cols, unsigned long long *cursor,
                                               double *__restrict__ mu_out, double *__restrict__ sd_out,
                                               int32_t *__restrict__ iters_out) {
    int phase = NF_FETCH, it = 0, k = 0;
    int64_t col = 0;
    double sx[NF_V][NF_D] = {{1.0, 1.0}, {1.0, 1.0}, {1.0, 1.0}}, cost[NF_V] = {0.0, 0.0, 0.0}, xt[NF_D] = {1.0, 1.0};
    double cr = 0.0, cnt = 0.0, mean = 0.0, ss = 0.0;

    auto vertex = [&](int kk, double (&o)[NF_D]) { // sx[kk] without indexing the register file at run time
#pragma unroll
        for (int d = 0; d < NF_D; ++d) {
            double v = sx[0][d];
#pragma unroll
            for (int i = 1; i < NF_V; ++i) v = (kk == i) ? sx[i][d] : v;
            o[d] = v;
        }
    };
    auto centroid = [&](double (&x0)[NF_D], double (&xr)[NF_D]) { // of all vertices but the worst, and the worst one's reflection
#pragma unroll
        for (int d = 0; d < NF_D; ++d) {
            double c = sx[0][d];
#pragma unroll
            for (int i = 1; i < NF_V - 1; ++i) c += sx[i][d];
            x0[d] = c * (1.0 / ((double)NF_V - 1.0));
            xr[d] = x0[d] + (x0[d] - sx[NF_V - 1][d]);
        }
    };
    auto sort = [&]() { // stable insertion sort by cost (vertices move with their costs)
#pragma unroll
        for (int a = 1; a < NF_V; ++a) {
#pragma unroll
            for (int b = a; b >= 1; --b) {
                const bool sw = cost[b - 1] > cost[b];
                const double c0s = cost[b - 1], c1s = cost[b];
                cost[b - 1] = sw ? c1s : c0s;
                cost[b] = sw ? c0s : c1s;
#pragma unroll
                for (int d = 0; d < NF_D; ++d) {
                    const double v0 = sx[b - 1][d], v1 = sx[b][d];
                    sx[b - 1][d] = sw ? v1 : v0;
                    sx[b][d] = sw ? v0 : v1;
                }
            }
        }
    };
    auto finish = [&]() {
        mu_out[col] = sx[0][0];
        sd_out[col] = nf_sigma(sx[0][1]);
        if (iters_out) iters_out[col] = it;
        phase = NF_FETCH;
    };
    // the head of the solver's loop: stop (sd of the costs below EPSILON, or the cap), or reflect the worst vertex
    auto check = [&]() {
        double m = 0.0, sd = 0.0;
#pragma unroll
        for (int i = 0; i < NF_V; ++i) m += cost[i];
        m /= (double)NF_V;
#pragma unroll
        for (int i = 0; i < NF_V; ++i) sd += (cost[i] - m) * (cost[i] - m);
        sd = sqrt(sd / ((double)NF_V - 1.0));
        if (it >= NF_MAXIT || sd < PG_EPS) { finish(); return; }
        double x0[NF_D];
        centroid(x0, xt);
        phase = NF_REFLECT;
    };
    auto stepped = [&]() { sort(); ++it; check(); };

    for (;;) {
        if (phase == NF_FETCH) {
            const long long idx = (long long)atomicAdd(cursor, 1ull);
            if (idx >= (long long)cols) phase = NF_DONE;
            else {
                col = idx;
                cnt = mom[col]; mean = mom[cols + col]; ss = mom[2 * cols + col];
#pragma unroll
                for (int i = 0; i < NF_V; ++i)
#pragma unroll
                    for (int d = 0; d < NF_D; ++d) sx[i][d] = (i == d) ? 1.5 : 1.0; // prepare_solver_neldermead(2, 1)
                k = 0;
                it = 0;
                vertex(0, xt);
                phase = NF_INIT;
            }
        }
        if (__all(phase == NF_DONE)) break;
        // ---- one cost per turn, whatever the step --------------------------------------------------------------------------
        const double c = phase == NF_DONE ? 0.0 : nf_cost(cnt, mean, ss, xt[0], xt[1]);
        switch (phase) {
        case NF_INIT:
        case NF_SHRINK:
#pragma unroll
            for (int i = 0; i < NF_V; ++i) cost[i] = (k == i) ? c : cost[i];
            ++k;
            if (k < NF_V) vertex(k, xt);
            else if (phase == NF_INIT) { sort(); check(); }
            else stepped();
            break;
        case NF_REFLECT:
            cr = c;
            if (cr < cost[NF_V - 2] && cr >= cost[0]) { // reflection (xt is the reflected point)
#pragma unroll
                for (int d = 0; d < NF_D; ++d) sx[NF_V - 1][d] = xt[d];
                cost[NF_V - 1] = cr;
                stepped();
            } else if (cr < cost[0]) { // try the expansion
                double x0[NF_D], xr[NF_D];
                centroid(x0, xr);
#pragma unroll
                for (int d = 0; d < NF_D; ++d) xt[d] = x0[d] + (xr[d] - x0[d]) * 2.0;
                phase = NF_EXPAND;
            } else { // try the contraction
                double x0[NF_D], xr[NF_D];
                centroid(x0, xr);
#pragma unroll
                for (int d = 0; d < NF_D; ++d) xt[d] = x0[d] + (sx[NF_V - 1][d] - x0[d]) * 0.5;
                phase = NF_CONTRACT;
            }
            break;
        case NF_EXPAND: {
            const bool e = c < cr;
            double x0[NF_D], xr[NF_D];
            centroid(x0, xr);
#pragma unroll
            for (int d = 0; d < NF_D; ++d) sx[NF_V - 1][d] = e ? xt[d] : xr[d];
            cost[NF_V - 1] = e ? c : cr;
            stepped();
        } break;
        case NF_CONTRACT:
            if (c < cost[NF_V - 1]) {
#pragma unroll
                for (int d = 0; d < NF_D; ++d) sx[NF_V - 1][d] = xt[d];
                cost[NF_V - 1] = c;
                stepped();
            } else { // shrink towards the best vertex: two more costs
#pragma unroll
                for (int i = 1; i < NF_V; ++i)
#pragma unroll
                    for (int d = 0; d < NF_D; ++d) sx[i][d] = sx[0][d] + (sx[i][d] - sx[0][d]) * 0.5;
                k = 1;
                vertex(1, xt);
                phase = NF_SHRINK;
            }
            break;
        default: break;
        }
    }
}

// Per population b: d = the rounded D of its non-NaN windows, in order; row j carries the label of window j (gudmc.rs:168-176).
// dc, wd: w x n, row j of population b at j * n + b, NaN from rows[b] on (so that the width table's moments skip them).
__global__ __launch_bounds__(64) void k_gd_scan(const double *__restrict__ D, int64_t w, int n, const double *__restrict__ d_mean,
                                                const int32_t *__restrict__ chr, const uint64_t *__restrict__ ini,
                                                const uint64_t *__restrict__ fin, double thr, int64_t *__restrict__ rows,
                                                double *__restrict__ dc, double *__restrict__ wd, int *__restrict__ bad) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    const double mean = d_mean[b];
    int64_t j = 0;
    uint64_t prev = 0;
    for (int64_t win = 0; win < w; ++win) {
        const double x = nf_round8(D[win * n + b]);
        if (x != x) continue;
        uint64_t width = 0;
        if (fabs(x - mean) >= thr) { // not scaled by the fitted sd (:180)
            if (fin[j] < ini[j]) atomicOr(bad, 1); // the reference's u64 pos_fin - pos_ini overflows
            width = fin[j] - ini[j];
            if (j > 0 && chr[j] == chr[j - 1] && ini[j] <= fin[j - 1]) width += prev;
        }
        dc[j * n + b] = x;
        wd[j * n + b] = (double)width;
        prev = width;
        ++j;
    }
    rows[b] = j;
    for (int64_t r = j; r < w; ++r) { dc[r * n + b] = NAN; wd[r * n + b] = NAN; }
}

__global__ __launch_bounds__(256) void k_gd_pairs(const double *__restrict__ wm, const double *__restrict__ ws, int n,
                                                  double *__restrict__ width_mean, double *__restrict__ width_sd) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)n * n) return;
    const int b = (int)(i % n); // the pair's rows are population b's: one fit per population serves its n pairs
    width_mean[i] = wm[b];
    width_sd[i] = ws[b];
}

// statrs Normal::cdf, and the tail the reference takes (gudmc.rs:353-357, :370-374)
__device__ __forceinline__ double gd_one_tail(double x, double mean, double sd) {
    const double cdf = 0.5 * erfc((mean - x) / (sd * NF_SQRT_2));
    return x < mean ? cdf : 1.0 - cdf;
}

constexpr int GT = 16; // a block covers GT pairs x GT rows: the Fst tile is read along the pairs and used along the rows

__global__ __launch_bounds__(GT * GT) void k_gd_rows(const double *__restrict__ F, int64_t w, int n, const int64_t *__restrict__ rows,
                                                     const double *__restrict__ dc, const double *__restrict__ wd,
                                                     const double *__restrict__ fst_mean, const double *__restrict__ fst_sd,
                                                     const double *__restrict__ wm, const double *__restrict__ ws, double rec_width,
                                                     int64_t *__restrict__ o_win, double *__restrict__ o_d, double *__restrict__ o_width,
                                                     double *__restrict__ o_wdev, double *__restrict__ o_wp, double *__restrict__ o_delta,
                                                     double *__restrict__ o_fp) {
    __shared__ double tile[GT][GT + 1];
    const int64_t nn = (int64_t)n * n;
    const int64_t i0 = (int64_t)blockIdx.x * GT, j0 = (int64_t)blockIdx.y * GT;
    {
        const int jj = threadIdx.x / GT, ii = threadIdx.x % GT;
        const int64_t i = i0 + ii, j = j0 + jj;
        tile[jj][ii] = (i < nn && j < w) ? F[j * nn + i] : 0.0;
    }
    __syncthreads();
    const int ii = threadIdx.x / GT, jj = threadIdx.x % GT;
    const int64_t i = i0 + ii, j = j0 + jj;
    if (i >= nn || j >= w) return;
    const int b = (int)(i % n);
    if (j >= rows[b]) return;
    const double f = tile[jj][ii], fm = fst_mean[i], width = wd[j * n + b];
    const size_t o = (size_t)i * (size_t)w + (size_t)j;
    if (o_win) o_win[o] = j; // the Fst window with the row's label: both lists come from one define_sliding_windows
    if (o_d) o_d[o] = dc[j * n + b];
    if (o_width) o_width[o] = width;
    if (o_wdev) o_wdev[o] = width - rec_width;
    if (o_wp) o_wp[o] = gd_one_tail(width, wm[b], ws[b]);
    if (o_delta) o_delta[o] = f - fm;
    if (o_fp) o_fp[o] = gd_one_tail(f, fm, fst_sd[i]);
}

// moments -> (refusal) -> fits of the `cols` columns of a device table
int nf_run(pg_ctx *ctx, const char *who, const double *T, int64_t rows, int64_t cols, int64_t ld, bool round8, double *mu,
           double *sd, int64_t *count, int32_t *iters) {
    DevBuf<double> mom;
    DevBuf<unsigned long long> ctl; // [cursor][bad]
    int rc;
    if ((rc = mom.alloc(ctx, sizeof(double) * 3 * (size_t)cols, who))) return rc;
    if ((rc = ctl.alloc(ctx, 16, who))) return rc;
    PG_HIP(ctx, hipMemsetAsync(ctl.get(), 0, 16, ctx->stream));
    int *bad = reinterpret_cast<int *>(ctl.get() + 1);
    const dim3 grid((unsigned)((cols + 255) / 256));
    if (round8) hipLaunchKernelGGL(k_nf_moments<true>, grid, dim3(256), 0, ctx->stream, T, rows, cols, ld, mom.get(), count, bad);
    else hipLaunchKernelGGL(k_nf_moments<false>, grid, dim3(256), 0, ctx->stream, T, rows, cols, ld, mom.get(), count, bad);
    PG_HIP(ctx, hipGetLastError());
    int hbad = 0;
    PG_HIP(ctx, hipMemcpyAsync(&hbad, bad, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (hbad) // maximum_likelihood_normal's cost is NaN from the first evaluation on and Normal::new panics (gudmc.rs:22-25)
        return pg_fail(ctx, PG_ERR_INVALID, "%s: a column holds an infinite value; the normal fit has no defined cost there", who);
    // one lane per fit while the device has lanes to spare (the longest fit then sets the time); beyond that the cursor hands
    // the columns out, and the lanes of a wave stay busy behind a fit that runs to the cap
    const int64_t want = (cols + 63) / 64, cap = (int64_t)ctx->cus * 16;
    hipLaunchKernelGGL(k_nf_fit, dim3((unsigned)(want < cap ? want : cap)), dim3(64), 0, ctx->stream, (const double *)mom.get(), cols,
                       ctl.get(), mu, sd, iters);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // mom and ctl leave scope
    return PG_OK;
}

} // namespace

extern "C" int pg_normal_fit_dev(pg_ctx *ctx, const double *table_dev, int64_t rows, int64_t cols, int64_t ld, double *mu_dev,
                                 double *sd_dev, int64_t *count_dev, int32_t *iters_dev) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, rows >= 0 && cols >= 1 && ld >= cols && mu_dev && sd_dev && (rows == 0 || table_dev), "normal_fit: bad arguments");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    return nf_run(ctx, "normal_fit", table_dev, rows, cols, ld, false, mu_dev, sd_dev, count_dev, iters_dev);
}

extern "C" int pg_gudmc_dev(pg_ctx *ctx, const double *d_win_dev, const double *fst_win_dev, int64_t w, int n, const int32_t *win_chr,
                            const uint64_t *win_ini, const uint64_t *win_fin, double sigma_threshold,
                            double recombination_rate_cM_per_Mb, int64_t *rows_dev, double *d_mean_dev, double *d_sd_dev,
                            double *fst_mean_dev, double *fst_sd_dev, double *width_mean_dev, double *width_sd_dev,
                            int64_t *row_window_dev, double *row_d_dev, double *row_width_dev, double *row_width_dev_from_r_dev,
                            double *row_width_p_dev, double *row_fst_delta_dev, double *row_fst_p_dev) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, n >= 1 && w >= 1, "gudmc: %d pools and %lld windows; at least one of each is needed", n, (long long)w);
    PG_CHECK(ctx, n <= 46340, "gudmc: %d pools; the pairs are indexed with 32 bits", n);
    PG_CHECK(ctx, d_win_dev && fst_win_dev && win_chr && win_ini && win_fin && rows_dev && d_mean_dev && d_sd_dev && fst_mean_dev &&
                      fst_sd_dev && width_mean_dev && width_sd_dev, "gudmc: null argument");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const int64_t nn = (int64_t)n * n;
    const size_t wn = (size_t)w * n;
    int rc;
    if ((rc = nf_run(ctx, "gudmc (Tajima's D)", d_win_dev, w, n, n, true, d_mean_dev, d_sd_dev, nullptr, nullptr))) return rc;
    if ((rc = nf_run(ctx, "gudmc (Fst)", fst_win_dev, w, nn, nn, false, fst_mean_dev, fst_sd_dev, nullptr, nullptr))) return rc;
    DevBuf<double> tab, wfit; // [d compacted | widths], w x n each; [mean | sd] of the width fits, n each
    DevBuf<char> lab;         // [ini: w u64][fin: w u64][chr: w i32]
    DevBuf<int> bad;
    if ((rc = tab.alloc(ctx, sizeof(double) * 2 * wn, "gudmc"))) return rc;
    if ((rc = wfit.alloc(ctx, sizeof(double) * 2 * (size_t)n, "gudmc"))) return rc;
    if ((rc = lab.alloc(ctx, (size_t)w * 20, "gudmc"))) return rc;
    if ((rc = bad.alloc(ctx, sizeof(int), "gudmc"))) return rc;
    PG_HIP(ctx, hipMemsetAsync(bad.get(), 0, sizeof(int), ctx->stream));
    uint64_t *ini = reinterpret_cast<uint64_t *>(lab.get()), *fin = ini + w;
    int32_t *chr = reinterpret_cast<int32_t *>(fin + w);
    PG_HIP(ctx, hipMemcpyAsync(ini, win_ini, sizeof(uint64_t) * w, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(fin, win_fin, sizeof(uint64_t) * w, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(chr, win_chr, sizeof(int32_t) * w, hipMemcpyHostToDevice, ctx->stream));
    double *dc = tab.get(), *wd = dc + wn, *wm = wfit.get(), *ws = wm + n;
    hipLaunchKernelGGL(k_gd_scan, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, ctx->stream, d_win_dev, w, n, (const double *)d_mean_dev,
                       (const int32_t *)chr, (const uint64_t *)ini, (const uint64_t *)fin, sigma_threshold, rows_dev, dc, wd, bad.get());
    PG_HIP(ctx, hipGetLastError());
    int hbad = 0;
    PG_HIP(ctx, hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the caller's label arrays may be pageable, too)
    if (hbad) return pg_fail(ctx, PG_ERR_INVALID, "gudmc: a significant row carries the label of a window that ends before it starts");
    if ((rc = nf_run(ctx, "gudmc (widths)", wd, w, n, n, false, wm, ws, nullptr, nullptr))) return rc;
    hipLaunchKernelGGL(k_gd_pairs, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, ctx->stream, (const double *)wm, (const double *)ws,
                       n, width_mean_dev, width_sd_dev);
    const double rec_width = (recombination_rate_cM_per_Mb / 100.0) * 1.0e6; // gudmc.rs:293
    const int64_t gy = (w + GT - 1) / GT;
    PG_CHECK(ctx, gy <= 65535, "gudmc: %lld windows; the row kernel's grid holds 65535 tiles of %d", (long long)w, GT);
    hipLaunchKernelGGL(k_gd_rows, dim3((unsigned)((nn + GT - 1) / GT), (unsigned)gy), dim3(GT * GT), 0, ctx->stream, fst_win_dev, w, n,
                       (const int64_t *)rows_dev, (const double *)dc, (const double *)wd, (const double *)fst_mean_dev,
                       (const double *)fst_sd_dev, (const double *)wm, (const double *)ws, rec_width, row_window_dev, row_d_dev,
                       row_width_dev, row_width_dev_from_r_dev, row_width_p_dev, row_fst_delta_dev, row_fst_p_dev);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // tab, wfit and lab leave scope
    return PG_OK;
}
