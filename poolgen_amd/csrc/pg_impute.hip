// pg_impute.hip -- the reference's imputation (src/imputation/: filtering_missing.rs, mean_imputation.rs,
// adaptive_ld_knn_imputation.rs) on the loader's resident matrix G (p x ld, a row per allele column) and the coverages
// beside it (cov, laid out like G: every row of a locus holds the pools' depths).  locus_col[l] .. locus_col[l + 1] are
// the rows of locus l (count_loci, sync.rs:73-97, minus the intercept).
//
//   k_missing_by_depth   thread = (locus, pool): cov < min_depth -> cov = NaN and, except in the LAST locus (the
//                        reference's idx_fin = loci_idx[l - 1], filtering_missing.rs:30-34), the locus' frequencies
//   k_nan_per_pool / k_nan_per_locus   the NaN counts the keep rule of filter_out_top_missing_* sorts by
//   k_compact            thread = (kept row, kept pool): G, cov and the column labels of the kept pools and loci
//   k_mean_tiles         block = a tile of whole loci staged in LDS (one read of G): thread r folds row r in pool order
//                        (mean_axis_ignore_nan), a thread per locus sums the means in ndarray's order and rescales, then every
//                        thread fills the NaN cells of the tile; k_mean (wave = locus) takes the loci too wide for a tile
//   k_mark_cov           wave = locus: NaN coverages become +inf where the locus has a coverage at all
//   adaptive LD-kNN in two stages:
//   k_aldknn_links       block = (window, column with missing data): pairwise-complete Pearson correlation of the column
//                        with every column of the window from the read-only input, thread = one partner column, then the
//                        stable top-K selection (descending, NaN as +inf) by K rounds of a block-wide arg-max
//   k_aldknn_walk        block = window: walks the columns in order over the window's own copy in global scratch -- distance
//                        columns of the pools missing at j (thread = pair of pools), the pools one after another (rank sort
//                        by (distance, index), then the k-neighbour fold and the per-locus renormalisation by thread 0)
//   k_aldknn_writeback   every column is copied from the LAST window that holds it
// Every value that feeds a comparison or is written is formed by the reference's sequence of IEEE operations (sequential
// folds, ndarray's 8-lane sum, multiply then add: the library is built with -ffp-contract=off).
#include "pg_common.h"
#include <algorithm>
#include <cmath>
#include <numeric>
#include <vector>

namespace {

constexpr double IMP_EPS = 2.220446049250313e-16; // f64::EPSILON

// ndarray's unrolled_fold fed one element at a time: element q of `len` goes to partial sum q % 8 while q < len - len % 8;
// the partial sums are combined as (p0 + p4) + (p1 + p5) + (p2 + p6) + (p3 + p7) and the tail is added left to right.
struct Sum8 {
    double p0 = 0, p1 = 0, p2 = 0, p3 = 0, p4 = 0, p5 = 0, p6 = 0, p7 = 0, acc = 0;
    int q = 0, len8 = 0;
    bool folded = false;
    __device__ explicit Sum8(int len) : len8(len & ~7) {}
    __device__ void fold() {
        acc = acc + (p0 + p4); acc = acc + (p1 + p5); acc = acc + (p2 + p6); acc = acc + (p3 + p7);
        folded = true;
    }
    __device__ void add(double v) {
        if (q < len8) {
            const int u = q & 7; // select chain: the partial sums stay in registers
            p0 = u == 0 ? p0 + v : p0; p1 = u == 1 ? p1 + v : p1; p2 = u == 2 ? p2 + v : p2; p3 = u == 3 ? p3 + v : p3;
            p4 = u == 4 ? p4 + v : p4; p5 = u == 5 ? p5 + v : p5; p6 = u == 6 ? p6 + v : p6; p7 = u == 7 ? p7 + v : p7;
        } else {
            if (!folded) fold();
            acc = acc + v;
        }
        ++q;
    }
    __device__ double result() {
        if (!folded) fold();
        return acc;
    }
};

// pearsons_correlation(x, y, "sensible_corr").0 (gwas/correlation_test.rs:7-71) over n pools
__device__ double imp_pearson(const double *__restrict__ x, const double *__restrict__ y, int n) {
    double sx = 0.0, sy = 0.0;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const double a = x[i], b = y[i];
        if (!isnan(a) && !isnan(b)) { sx = sx + a; sy = sy + b; ++m; }
    }
    const double mux = sx / (double)m, muy = sy / (double)m;
    Sum8 num(m), sxx(m), syy(m);
    for (int i = 0; i < n; ++i) {
        const double a = x[i], b = y[i];
        if (!isnan(a) && !isnan(b)) {
            const double dx = a - mux, dy = b - muy;
            num.add(dx * dy); sxx.add(dx * dx); syy.add(dy * dy);
        }
    }
    const double r = num.result() / (sqrt(sxx.result()) * sqrt(syy.result()));
    if (isnan(r)) return NAN;
    const double q = (1.0 - r * r) / ((double)n - 2.0);
    if (q <= 0.0) return r;
    return round(r * 1e7) / 1e7; // sensible_round(r, 7)
}

__global__ __launch_bounds__(256) void k_missing_by_depth(double *__restrict__ G, double *__restrict__ cov,
                                                          const int64_t *__restrict__ locus_col, int64_t L, int n, int64_t ld,
                                                          double min_depth) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t l = gid / n;
    if (l >= L) return;
    const int i = (int)(gid - l * n);
    const int64_t c0 = locus_col[l], c1 = locus_col[l + 1];
    if (!(cov[c0 * ld + i] < min_depth)) return;
    for (int64_t c = c0; c < c1; ++c) cov[c * ld + i] = NAN;
    if (l < L - 1)
        for (int64_t c = c0; c < c1; ++c) G[c * ld + i] = NAN;
}

// block (64, 4): x strides the pools, y the rows of this block's 256-row chunk; integer atomics, so the counts are exact
__global__ __launch_bounds__(256) void k_nan_per_pool(const double *__restrict__ G, int64_t p, int n, int64_t ld,
                                                      unsigned long long *__restrict__ pool_nan) {
    const int64_t r0 = (int64_t)blockIdx.x * 256, r1 = r0 + 256 < p ? r0 + 256 : p;
    for (int i = threadIdx.x; i < n; i += 64) {
        unsigned long long cnt = 0;
        for (int64_t r = r0 + threadIdx.y; r < r1; r += 4) cnt += isnan(G[r * ld + i]) ? 1 : 0;
        if (cnt) atomicAdd(&pool_nan[i], cnt);
    }
}

__global__ __launch_bounds__(256) void k_nan_per_locus(const double *__restrict__ cov, const int64_t *__restrict__ locus_col,
                                                       int64_t L, int n, int64_t ld, int64_t *__restrict__ locus_nan) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const double *row = cov + locus_col[l] * ld;
    int64_t cnt = 0;
    for (int i = 0; i < n; ++i) cnt += isnan(row[i]) ? 1 : 0;
    locus_nan[l] = cnt;
}

__global__ __launch_bounds__(256) void k_compact(const double *__restrict__ G, const double *__restrict__ cov, int64_t ld,
                                                 const int64_t *__restrict__ col_locus, const int32_t *__restrict__ col_allele,
                                                 const int64_t *__restrict__ row_src, int64_t p_out,
                                                 const int32_t *__restrict__ pool_src, int n_out, int64_t ld_out,
                                                 double *__restrict__ G_out, double *__restrict__ cov_out,
                                                 int64_t *__restrict__ col_locus_out, int32_t *__restrict__ col_allele_out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t r = gid / ld_out;
    if (r >= p_out) return;
    const int i = (int)(gid - r * ld_out);
    const int64_t src = row_src[r];
    const bool pool = i < n_out; // the padding of a row (ld_out > n_out) is zero
    G_out[gid] = pool ? G[src * ld + pool_src[i]] : 0.0;
    if (cov_out) cov_out[gid] = pool ? cov[src * ld + pool_src[i]] : 0.0;
    if (i == 0) {
        if (col_locus_out) col_locus_out[r] = col_locus[src];
        if (col_allele_out) col_allele_out[r] = col_allele[src];
    }
}

// mean_imputation (mean_imputation.rs:6-41) for the loci that fit no tile of k_mean_tiles (`list`, L of them).  wave = locus;
// `means` (dynamic LDS) holds max_alleles doubles per wave.
__global__ __launch_bounds__(256) void k_mean(double *__restrict__ G, const int64_t *__restrict__ locus_col,
                                              const int64_t *__restrict__ list, int64_t L, int n, int64_t ld, int max_alleles) {
    extern __shared__ double imp_lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t idx = (int64_t)blockIdx.x * 4 + wave;
    if (idx >= L) return; // (no block-wide barrier below)
    const int64_t l = list[idx];
    double *means = imp_lds + (size_t)wave * max_alleles;
    const int64_t c0 = locus_col[l];
    const int A = (int)(locus_col[l + 1] - c0);
    for (int a = lane; a < A; a += 64) { // mean_axis_ignore_nan (helpers.rs:267-291): the fold runs in pool order
        const double *row = G + (c0 + a) * ld;
        double s = 0.0, cnt = 0.0;
        for (int i = 0; i < n; ++i) {
            const double x = row[i];
            if (!isnan(x)) { s = s + x; cnt += 1.0; }
        }
        means[a] = s / cnt;
    }
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    double tot = 0.0;
    if (lane == 0) { // mean_freqs.sum(): ndarray's order
        Sum8 t(A);
        for (int a = 0; a < A; ++a) t.add(means[a]);
        tot = t.result();
    }
    tot = __shfl(tot, 0);
    for (int a = 0; a < A; ++a) {
        const double m = tot != 1.0 ? means[a] / tot : means[a];
        double *row = G + (c0 + a) * ld;
        for (int i = lane; i < n; i += 64)
            if (isnan(row[i])) row[i] = m;
    }
}

// mean_imputation (mean_imputation.rs:6-41), one read of G: block = a tile of whole loci (tile_locus[2 b] .. tile_locus[2 b + 1], at
// most `rows_max` rows), staged in LDS with an odd pitch.  Thread r folds row r in pool order (mean_axis_ignore_nan,
// helpers.rs:267-291), a thread per locus sums its means in ndarray's order and rescales them, then every thread writes the
// means into the NaN cells it finds in the tile.  Dynamic LDS: rows_max * pitch + rows_max doubles.
__global__ __launch_bounds__(256) void k_mean_tiles(double *__restrict__ G, const int64_t *__restrict__ locus_col,
                                                    const int64_t *__restrict__ tile_locus, int n, int64_t ld, int rows_max, int pitch) {
    extern __shared__ double imp_lds[];
    double *tile = imp_lds, *means = imp_lds + (size_t)rows_max * pitch;
    const int tid = threadIdx.x;
    const int64_t l0 = tile_locus[2 * (size_t)blockIdx.x], l1 = tile_locus[2 * (size_t)blockIdx.x + 1];
    const int64_t r0 = locus_col[l0];
    const int rows = (int)(locus_col[l1] - r0);
    for (int e = tid; e < rows * n; e += 256) {
        const int r = e / n, i = e - r * n;
        tile[r * pitch + i] = G[(r0 + r) * ld + i];
    }
    __syncthreads();
    if (tid < rows) {
        const double *row = tile + tid * pitch;
        double s = 0.0, cnt = 0.0;
        for (int i = 0; i < n; ++i) {
            const double x = row[i];
            if (!isnan(x)) { s = s + x; cnt += 1.0; }
        }
        means[tid] = s / cnt;
    }
    __syncthreads();
    for (int64_t l = l0 + tid; l < l1; l += 256) { // mean_freqs.sum() and the rescaling: a locus' means belong to one thread
        const int a0 = (int)(locus_col[l] - r0), A = (int)(locus_col[l + 1] - locus_col[l]);
        Sum8 t(A);
        for (int a = 0; a < A; ++a) t.add(means[a0 + a]);
        const double tot = t.result();
        if (tot != 1.0)
            for (int a = 0; a < A; ++a) means[a0 + a] = means[a0 + a] / tot;
    }
    __syncthreads();
    for (int e = tid; e < rows * n; e += 256) {
        const int r = e / n, i = e - r * n;
        if (isnan(tile[r * pitch + i])) G[(r0 + r) * ld + i] = means[r];
    }
}

__global__ __launch_bounds__(256) void k_mark_cov(double *__restrict__ cov, const int64_t *__restrict__ locus_col, int64_t L,
                                                  int n, int64_t ld) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t l = (int64_t)blockIdx.x * 4 + wave;
    if (l >= L) return;
    const int64_t c0 = locus_col[l], c1 = locus_col[l + 1];
    int some = 0;
    for (int i = lane; i < n; i += 64) some |= !isnan(cov[c0 * ld + i]) ? 1 : 0;
    if (!__any(some)) return;
    for (int64_t c = c0; c < c1; ++c)
        for (int i = lane; i < n; i += 64)
            if (isnan(cov[c * ld + i])) cov[c * ld + i] = INFINITY;
}

// ---- adaptive LD-kNN -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_col_info(const double *__restrict__ G, const int64_t *__restrict__ locus_col, int64_t L,
                                                  int n, int64_t ld, uint8_t *__restrict__ has_nan,
                                                  int64_t *__restrict__ col_start, int64_t *__restrict__ col_end) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int64_t c0 = locus_col[l], c1 = locus_col[l + 1];
    for (int64_t c = c0; c < c1; ++c) {
        int any = 0;
        for (int i = 0; i < n; ++i) any |= isnan(G[c * ld + i]) ? 1 : 0;
        has_nan[c] = (uint8_t)any;
        col_start[c] = c0;
        col_end[c] = c1;
    }
}

struct ImpItems {           // one entry per (window, column with missing data), ordered by window, then column
    const int64_t *col;     // the column (a row of G)
    const int64_t *ini;     // first column of its window
    const int32_t *pw;      // columns of its window
    const int64_t *key_off; // where its pw sort keys start
};

constexpr int LINK_THREADS = 128;

__global__ __launch_bounds__(LINK_THREADS) void k_aldknn_links(const double *__restrict__ G, int n, int64_t ld, ImpItems it,
                                                               double *__restrict__ keys, int k_links,
                                                               int32_t *__restrict__ links) {
    __shared__ double s_key[LINK_THREADS];
    __shared__ int s_col[LINK_THREADS];
    const int64_t item = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t ini = it.ini[item], jg = it.col[item];
    const int pw = it.pw[item];
    const int j = (int)(jg - ini);
    double *key = keys + it.key_off[item];
    for (int c = tid; c < pw; c += LINK_THREADS) { // corr[(j0, j1)] with j0 <= j1, mirrored (:218-232)
        const int lo = c < j ? c : j, hi = c < j ? j : c;
        const double r = imp_pearson(G + (ini + lo) * ld, G + (ini + hi) * ld, n);
        key[c] = isnan(r) ? INFINITY : r; // NaN sorts as +inf (:25-32)
    }
    __syncthreads();
    // stable descending sort, first K: round t takes the best (key, then lower index) that comes after the last pick
    const int K = pw < k_links ? pw : k_links;
    double last_key = 0.0;
    int last_col = -1;
    for (int t = 0; t < K; ++t) {
        double bk = 0.0;
        int bc = INT32_MAX;
        for (int c = tid; c < pw; c += LINK_THREADS) {
            const double k = key[c];
            const bool after = t == 0 || k < last_key || (k == last_key && c > last_col);
            if (after && (bc == INT32_MAX || k > bk || (k == bk && c < bc))) { bk = k; bc = c; }
        }
        s_key[tid] = bk; s_col[tid] = bc;
        __syncthreads();
        for (int w = LINK_THREADS / 2; w > 0; w >>= 1) {
            if (tid < w) {
                const double ok = s_key[tid + w];
                const int oc = s_col[tid + w];
                if (oc != INT32_MAX && (s_col[tid] == INT32_MAX || ok > s_key[tid] || (ok == s_key[tid] && oc < s_col[tid]))) {
                    s_key[tid] = ok; s_col[tid] = oc;
                }
            }
            __syncthreads();
        }
        last_key = s_key[0]; last_col = s_col[0];
        if (tid == 0) links[item * k_links + t] = last_col;
        __syncthreads();
    }
}

struct ImpWindows {          // one entry per window of the batch that has columns to impute
    const int64_t *ini;      // first column
    const int32_t *pw;       // columns
    const int64_t *w_off;    // first row of its copy in the scratch
    const int64_t *item0;    // its items: item0 .. item1 of the batch
    const int64_t *item1;
    const int64_t *id;       // its index in the caller's window list
};

__global__ __launch_bounds__(256) void k_aldknn_copy(const double *__restrict__ G, int64_t ld, ImpWindows win,
                                                     double *__restrict__ W) {
    const int64_t a = blockIdx.x;
    const int64_t count = (int64_t)win.pw[a] * ld;
    const double *src = G + win.ini[a] * ld;
    double *dst = W + win.w_off[a] * ld;
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.y * 256) dst[e] = src[e];
}

__global__ __launch_bounds__(256) void k_aldknn_writeback(const double *__restrict__ W, int n, int64_t ld, ImpWindows win,
                                                          const int64_t *__restrict__ last_window, double *__restrict__ G_out) {
    const int64_t a = blockIdx.x;
    const int64_t count = (int64_t)win.pw[a] * ld, ini = win.ini[a], id = win.id[a];
    const double *src = W + win.w_off[a] * ld;
    for (int64_t e = (int64_t)blockIdx.y * 256 + threadIdx.x; e < count; e += (int64_t)gridDim.y * 256) {
        const int64_t row = e / ld;
        if ((int)(e - row * ld) < n && last_window[ini + row] == id) G_out[(ini + row) * ld + (e - row * ld)] = src[e];
    }
}

// correct_allele_frequencies_per_locus (:136-171) for pool i after column j (local) of the window copy Ww was imputed
__device__ void imp_renormalise(double *__restrict__ Ww, int64_t ld, int i, int j, int64_t ini, const int64_t *__restrict__ col_start,
                                const int64_t *__restrict__ col_end) {
    if (j <= 0 || col_end[ini + j] != ini + j + 1) return; // only at the last allele of a locus, never at the window's first column
    const int j_ini = (int)(col_start[ini + j] - ini);
    double s = 0.0;
    for (int jj = j_ini; jj <= j; ++jj) {
        const double x = Ww[(int64_t)jj * ld + i];
        if (!isnan(x)) s = s + x;
    }
    s = s + IMP_EPS;
    if (s != 1.0)
        for (int jj = j_ini; jj <= j; ++jj) Ww[(int64_t)jj * ld + i] = Ww[(int64_t)jj * ld + i] / s;
}

__device__ __forceinline__ double imp_sort_key(double d) { return isnan(d) ? INFINITY : d; }

// dynamic LDS: n ints (the pools missing at j) + n ints (the pools sorted by distance)
__global__ __launch_bounds__(256) void k_aldknn_walk(double *__restrict__ W, int n, int64_t ld, ImpWindows win, ImpItems it,
                                                     const int32_t *__restrict__ links, int k_links, int k_neighbours,
                                                     const int64_t *__restrict__ col_start, const int64_t *__restrict__ col_end,
                                                     double *__restrict__ dist) {
    extern __shared__ int imp_ilds[];
    int *miss = imp_ilds, *order = imp_ilds + n;
    __shared__ int s_nm, s_present, s_any;
    const int64_t a = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t ini = win.ini[a];
    const int pw = win.pw[a];
    double *Ww = W + win.w_off[a] * ld;
    double *D = dist + (size_t)a * n * n; // D[t * n + q]: distance of pool q to the t-th pool missing at j
    const int K = pw < k_links ? pw : k_links;
    for (int64_t item = win.item0[a]; item < win.item1[a]; ++item) {
        const int j = (int)(it.col[item] - ini);
        double *Wj = Ww + (int64_t)j * ld;
        const int32_t *lk = links + item * k_links;
        if (tid == 0) {
            int nm = 0;
            for (int i = 0; i < n; ++i)
                if (isnan(Wj[i])) miss[nm++] = i;
            s_nm = nm; s_present = n - nm; s_any = 0;
        }
        __syncthreads();
        const int nm = s_nm, present = s_present;
        // all_missing (:40-70): no pair of pools, a pool with itself included, shares a linked column
        for (int e = tid; e < K * n; e += 256) {
            const int t = e / n;
            if (!isnan(Ww[(int64_t)lk[t] * ld + (e - t * n)])) s_any = 1;
        }
        __syncthreads();
        if (!s_any) { // every pool gets the count of present values over n (mean_value_imputation, :76-82), one more each time
            for (int t = tid; t < nm; t += 256) {
                Wj[miss[t]] = (double)(present + t) / (double)n;
                imp_renormalise(Ww, ld, miss[t], j, ini, col_start, col_end);
            }
            __syncthreads();
            continue;
        }
        for (int e = tid; e < nm * n; e += 256) { // the distance columns, from W as it is before this column's pools are filled
            const int t = e / n, q = e - t * n, i = miss[t];
            const int i0 = q < i ? q : i, i1 = q < i ? i : q;
            int m = 0;
            for (int c = 0; c < K; ++c) {
                const double *row = Ww + (int64_t)lk[c] * ld;
                m += (!isnan(row[i0]) && !isnan(row[i1])) ? 1 : 0;
            }
            double d = NAN;
            if (m > 0) {
                Sum8 s(m);
                for (int c = 0; c < K; ++c) {
                    const double *row = Ww + (int64_t)lk[c] * ld;
                    const double x = row[i0], y = row[i1];
                    if (!isnan(x) && !isnan(y)) { const double df = x - y; s.add(df * df); }
                }
                d = sqrt(s.result());
            }
            D[e] = d;
        }
        __syncthreads();
        for (int t = 0; t < nm; ++t) { // the pools in order: a value imputed earlier in this column counts as present
            const double *Dc = D + (size_t)t * n;
            for (int q = tid; q < n; q += 256) { // stable ascending sort by distance, NaN as +inf: rank by (key, index)
                const double kq = imp_sort_key(Dc[q]);
                int r = 0;
                for (int o = 0; o < n; ++o) {
                    const double ko = imp_sort_key(Dc[o]);
                    r += (ko < kq || (ko == kq && o < q)) ? 1 : 0;
                }
                order[r] = q;
            }
            __syncthreads();
            if (tid == 0) { // find_k_nearest_neighbours (:84-134) and the weighted mean (:269-302)
                const int i = miss[t];
                int first_nan = n;
                for (int r = 0; r < n; ++r)
                    if (isnan(Wj[order[r]])) { first_nan = r; break; }
                int k = k_neighbours, m = k_neighbours; // m: length of freqs_k_neighbours, which lags k by one
                while (k < n) {
                    if (first_nan < m) break;
                    m = k;
                    k += 1;
                }
                int cnt = 0;
                double dist_sum = 0.0;
                for (int r = 0; r < m; ++r) {
                    const double v = Wj[order[r]], d = Dc[order[r]];
                    if (!isnan(v) && !isnan(d)) { dist_sum = dist_sum + d; ++cnt; }
                }
                double val;
                if (cnt == 0) {
                    double c = 0.0;
                    for (int q = 0; q < n; ++q)
                        if (!isnan(Wj[q])) c = c + 1.0;
                    val = c / (double)n;
                } else {
                    dist_sum = dist_sum + IMP_EPS;
                    double ws = 0.0;
                    for (int r = 0; r < m; ++r) {
                        const double v = Wj[order[r]], d = Dc[order[r]];
                        if (!isnan(v) && !isnan(d)) ws = ws + (1.0 - (d / dist_sum) + IMP_EPS);
                    }
                    Sum8 s(cnt);
                    for (int r = 0; r < m; ++r) {
                        const double v = Wj[order[r]], d = Dc[order[r]];
                        if (!isnan(v) && !isnan(d)) s.add(v * ((1.0 - (d / dist_sum) + IMP_EPS) / ws));
                    }
                    val = s.result();
                }
                Wj[i] = val;
                imp_renormalise(Ww, ld, i, j, ini, col_start, col_end);
            }
            __syncthreads();
        }
    }
}

int check_matrix(pg_ctx *ctx, const void *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L, const char *who) {
    PG_CHECK(ctx, G_dev && locus_col, "%s: null argument", who);
    PG_CHECK(ctx, p >= 1 && n >= 1 && ld >= n && L >= 1 && L <= p, "%s: bad shape (p=%lld n=%d ld=%lld L=%lld)", who, (long long)p, n,
             (long long)ld, (long long)L);
    PG_CHECK(ctx, locus_col[0] == 0 && locus_col[L] == p, "%s: locus_col must run from 0 to p", who);
    for (int64_t l = 0; l < L; ++l) PG_CHECK(ctx, locus_col[l] < locus_col[l + 1], "%s: locus_col must increase (locus %lld)", who, (long long)l);
    return PG_OK;
}

template <typename T>
int upload(pg_ctx *ctx, DevBuf<T> &buf, const T *host, size_t count, const char *who) {
    const int rc = buf.alloc(ctx, sizeof(T) * std::max<size_t>(count, 1), who);
    if (rc) return rc;
    if (count) PG_HIP(ctx, hipMemcpyAsync(buf.get(), host, sizeof(T) * count, hipMemcpyHostToDevice, ctx->stream));
    return PG_OK;
}

inline unsigned blocks_of(size_t items, unsigned per_block) { return (unsigned)((items + per_block - 1) / per_block); }

} // namespace

extern "C" int pg_set_missing_by_depth_dev(pg_ctx *ctx, double *G_dev, double *cov_dev, int64_t p, int n, int64_t ld,
                                           const int64_t *locus_col, int64_t L, double min_depth) {
    if (!ctx) return PG_ERR_INVALID;
    int rc = check_matrix(ctx, G_dev, p, n, ld, locus_col, L, "set_missing_by_depth");
    if (rc) return rc;
    PG_CHECK(ctx, cov_dev, "set_missing_by_depth: null argument");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    pg_spec_written(ctx, G_dev, sizeof(double) * (size_t)p * ld);
    pg_spec_written(ctx, cov_dev, sizeof(double) * (size_t)p * ld);
    DevBuf<int64_t> lc;
    if ((rc = upload(ctx, lc, locus_col, (size_t)L + 1, "set_missing_by_depth"))) return rc;
    pg_prof_begin(ctx, PG_K_IMPUTE);
    hipLaunchKernelGGL(k_missing_by_depth, dim3(blocks_of((size_t)L * n, 256)), dim3(256), 0, ctx->stream, G_dev, cov_dev, lc.get(), L, n, ld,
                       min_depth);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // lc goes with this call
    return PG_OK;
}

extern "C" int pg_missingness_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                                  const int64_t *locus_col, int64_t L, int64_t *pool_nan, int64_t *locus_nan) {
    if (!ctx) return PG_ERR_INVALID;
    int rc = check_matrix(ctx, G_dev, p, n, ld, locus_col, L, "missingness");
    if (rc) return rc;
    PG_CHECK(ctx, !locus_nan || cov_dev, "missingness: the loci are counted on the coverages");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<int64_t> lc, out;
    if ((rc = upload(ctx, lc, locus_col, (size_t)L + 1, "missingness"))) return rc;
    if ((rc = out.alloc(ctx, sizeof(int64_t) * ((size_t)n + L), "missingness"))) return rc;
    PG_HIP(ctx, hipMemsetAsync(out.get(), 0, sizeof(int64_t) * ((size_t)n + L), ctx->stream));
    pg_prof_begin(ctx, PG_K_IMPUTE);
    if (pool_nan)
        hipLaunchKernelGGL(k_nan_per_pool, dim3(blocks_of((size_t)p, 256)), dim3(64, 4), 0, ctx->stream, G_dev, p, n, ld,
                           reinterpret_cast<unsigned long long *>(out.get()));
    if (locus_nan)
        hipLaunchKernelGGL(k_nan_per_locus, dim3(blocks_of((size_t)L, 256)), dim3(256), 0, ctx->stream, cov_dev, lc.get(), L, n, ld, out.get() + n);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    if (pool_nan) PG_HIP(ctx, hipMemcpyAsync(pool_nan, out.get(), sizeof(int64_t) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (locus_nan) PG_HIP(ctx, hipMemcpyAsync(locus_nan, out.get() + n, sizeof(int64_t) * L, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

// The keep rule of filter_out_top_missing_pools / _loci (filtering_missing.rs:63-86, :146-170) from the NaN counts: the
// missingness count / denominator orders like the count, so the stable sort runs on the counts.
extern "C" int64_t pg_host_top_missing_keep(const int64_t *nan_count, int64_t count, double frac, int64_t *keep) {
    if (!nan_count || !keep || count < 1 || !(frac >= 0.0)) return PG_ERR_INVALID;
    double n_missing = 0.0;
    for (int64_t i = 0; i < count; ++i)
        if (nan_count[i] > 0) n_missing = n_missing + 1.0;
    const double drop = std::ceil(n_missing * frac);
    if (!(drop < (double)count)) return 0; // "No pools / loci left after filtering"
    const int64_t left = count - (int64_t)drop;
    std::vector<int64_t> idx((size_t)count);
    std::iota(idx.begin(), idx.end(), (int64_t)0);
    std::stable_sort(idx.begin(), idx.end(), [&](int64_t x, int64_t y) { return nan_count[x] < nan_count[y]; });
    std::sort(idx.begin(), idx.begin() + left);
    std::copy(idx.begin(), idx.begin() + left, keep);
    return left;
}

extern "C" int pg_impute_compact_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                                     const int64_t *col_locus_dev, const int32_t *col_allele_dev, const int64_t *locus_col, int64_t L,
                                     const int64_t *keep_pools, int n_keep, const int64_t *keep_loci, int64_t L_keep, double *G_out_dev,
                                     double *cov_out_dev, int64_t ld_out, int64_t *col_locus_out_dev, int32_t *col_allele_out_dev,
                                     int64_t *locus_col_out) {
    if (!ctx) return PG_ERR_INVALID;
    int rc = check_matrix(ctx, G_dev, p, n, ld, locus_col, L, "impute_compact");
    if (rc) return rc;
    PG_CHECK(ctx, keep_pools && keep_loci && G_out_dev && locus_col_out, "impute_compact: null argument");
    PG_CHECK(ctx, n_keep >= 1 && n_keep <= n && L_keep >= 1 && L_keep <= L && ld_out >= n_keep, "impute_compact: bad shape of the kept part");
    PG_CHECK(ctx, (cov_dev != nullptr) == (cov_out_dev != nullptr) && (!col_locus_out_dev || col_locus_dev) && (!col_allele_out_dev || col_allele_dev),
             "impute_compact: an output without its input");
    std::vector<int32_t> pools((size_t)n_keep);
    for (int i = 0; i < n_keep; ++i) {
        PG_CHECK(ctx, keep_pools[i] >= 0 && keep_pools[i] < n && (i == 0 || keep_pools[i] > keep_pools[i - 1]), "impute_compact: keep_pools must increase inside 0 .. n");
        pools[i] = (int32_t)keep_pools[i];
    }
    std::vector<int64_t> rows;
    locus_col_out[0] = 0;
    for (int64_t k = 0; k < L_keep; ++k) {
        const int64_t l = keep_loci[k];
        PG_CHECK(ctx, l >= 0 && l < L && (k == 0 || l > keep_loci[k - 1]), "impute_compact: keep_loci must increase inside 0 .. L");
        for (int64_t c = locus_col[l]; c < locus_col[l + 1]; ++c) rows.push_back(c);
        locus_col_out[k + 1] = (int64_t)rows.size();
    }
    PG_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<int64_t> rows_dev;
    DevBuf<int32_t> pools_dev;
    if ((rc = upload(ctx, rows_dev, rows.data(), rows.size(), "impute_compact"))) return rc;
    if ((rc = upload(ctx, pools_dev, pools.data(), pools.size(), "impute_compact"))) return rc;
    const int64_t p_out = (int64_t)rows.size();
    pg_spec_written(ctx, G_out_dev, sizeof(double) * (size_t)p_out * ld_out);
    pg_spec_written(ctx, cov_out_dev, sizeof(double) * (size_t)p_out * ld_out);
    pg_prof_begin(ctx, PG_K_IMPUTE);
    hipLaunchKernelGGL(k_compact, dim3(blocks_of((size_t)p_out * ld_out, 256)), dim3(256), 0, ctx->stream, G_dev, cov_dev, ld, col_locus_dev,
                       col_allele_dev, rows_dev.get(), p_out, pools_dev.get(), n_keep, ld_out, G_out_dev, cov_out_dev, col_locus_out_dev,
                       col_allele_out_dev);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

extern "C" int pg_impute_mean_dev(pg_ctx *ctx, double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L) {
    if (!ctx) return PG_ERR_INVALID;
    int rc = check_matrix(ctx, G_dev, p, n, ld, locus_col, L, "impute_mean");
    if (rc) return rc;
    // tiles of whole loci, at most rows_max rows each, as many as 60 KB of LDS hold (32 at the most); a locus wider than that goes
    // to the wave-per-locus kernel
    const int pitch = n | 1;
    const int rows_max = (int)std::min<size_t>(32, (60 * 1024) / (sizeof(double) * ((size_t)pitch + 1)));
    std::vector<int64_t> tiles, wide;
    int64_t max_alleles = 1;
    for (int64_t l = 0, open = -1; l <= L; ++l) { // open: first locus of the tile being filled
        const int64_t A = l < L ? locus_col[l + 1] - locus_col[l] : 0;
        const bool is_wide = l < L && A > rows_max;
        if (open >= 0 && (l == L || is_wide || locus_col[l + 1] - locus_col[open] > rows_max)) {
            tiles.push_back(open); tiles.push_back(l);
            open = -1;
        }
        if (l == L) break;
        if (is_wide) { wide.push_back(l); max_alleles = std::max(max_alleles, A); }
        else if (open < 0) open = l;
    }
    PG_CHECK(ctx, max_alleles <= 1024, "impute_mean: a locus with %lld allele columns (at most 1024)", (long long)max_alleles);
    PG_HIP(ctx, hipSetDevice(ctx->device));
    pg_spec_written(ctx, G_dev, sizeof(double) * (size_t)p * ld);
    DevBuf<int64_t> lc, list, wide_dev;
    if ((rc = upload(ctx, lc, locus_col, (size_t)L + 1, "impute_mean"))) return rc;
    pg_prof_begin(ctx, PG_K_IMPUTE);
    if (!tiles.empty()) {
        if ((rc = upload(ctx, list, tiles.data(), tiles.size(), "impute_mean"))) return rc;
        hipLaunchKernelGGL(k_mean_tiles, dim3((unsigned)(tiles.size() / 2)), dim3(256), sizeof(double) * ((size_t)rows_max * pitch + rows_max), ctx->stream,
                           G_dev, lc.get(), list.get(), n, ld, rows_max, pitch);
    }
    if (!wide.empty()) {
        if ((rc = upload(ctx, wide_dev, wide.data(), wide.size(), "impute_mean"))) return rc;
        hipLaunchKernelGGL(k_mean, dim3(blocks_of(wide.size(), 4)), dim3(256), sizeof(double) * 4 * (size_t)max_alleles, ctx->stream, G_dev, lc.get(),
                           wide_dev.get(), (int64_t)wide.size(), n, ld, (int)max_alleles);
    }
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

extern "C" int pg_impute_mark_cov_dev(pg_ctx *ctx, double *cov_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L) {
    if (!ctx) return PG_ERR_INVALID;
    int rc = check_matrix(ctx, cov_dev, p, n, ld, locus_col, L, "impute_mark_cov");
    if (rc) return rc;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<int64_t> lc;
    if ((rc = upload(ctx, lc, locus_col, (size_t)L + 1, "impute_mark_cov"))) return rc;
    pg_prof_begin(ctx, PG_K_IMPUTE);
    hipLaunchKernelGGL(k_mark_cov, dim3(blocks_of((size_t)L, 4)), dim3(256), 0, ctx->stream, cov_dev, lc.get(), L, n, ld);
    pg_prof_end(ctx);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

extern "C" int pg_impute_aldknn_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L,
                                    const int64_t *win_head, const int64_t *win_tail, int64_t n_windows, int64_t n_loci_to_estimate_distance,
                                    int64_t k_neighbours, int64_t scratch_bytes, double *G_out_dev) {
    const char *who = "impute_aldknn";
    if (!ctx) return PG_ERR_INVALID;
    int rc = check_matrix(ctx, G_dev, p, n, ld, locus_col, L, who);
    if (rc) return rc;
    PG_CHECK(ctx, G_out_dev && G_out_dev != G_dev, "%s: the result needs a buffer of its own (every window reads the input)", who);
    PG_CHECK(ctx, n_windows >= 0 && (n_windows == 0 || (win_head && win_tail)), "%s: null argument", who);
    PG_CHECK(ctx, n_loci_to_estimate_distance >= 1 && n_loci_to_estimate_distance <= 65536, "%s: n_loci_to_estimate_distance must be 1 .. 65536", who);
    PG_CHECK(ctx, k_neighbours >= 1, "%s: k_neighbours must be at least 1", who);
    PG_CHECK(ctx, k_neighbours <= n, "%s: k_neighbours (%lld) exceeds the number of pools (%d)", who, (long long)k_neighbours, n); // select(0..k) panics
    PG_CHECK(ctx, n <= 4096, "%s: at most 4096 pools", who);
    for (int64_t a = 0; a < n_windows; ++a) {
        PG_CHECK(ctx, win_head[a] >= 0 && win_head[a] <= win_tail[a] && win_tail[a] < L, "%s: window %lld out of range", who, (long long)a);
        PG_CHECK(ctx, locus_col[win_tail[a] + 1] - locus_col[win_head[a]] < (1ll << 30), "%s: window %lld is too wide", who, (long long)a);
    }
    const int k_links = (int)n_loci_to_estimate_distance;
    const size_t budget = scratch_bytes > 0 ? (size_t)scratch_bytes : (size_t)1 << 30;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    pg_spec_written(ctx, G_out_dev, sizeof(double) * (size_t)p * ld);
    PG_HIP(ctx, hipMemcpyAsync(G_out_dev, G_dev, sizeof(double) * (size_t)p * ld, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_windows == 0) return PG_OK;

    DevBuf<int64_t> lc, col_start, col_end, last_dev;
    DevBuf<uint8_t> has_nan_dev;
    if ((rc = upload(ctx, lc, locus_col, (size_t)L + 1, who))) return rc;
    if ((rc = col_start.alloc(ctx, sizeof(int64_t) * p, who)) || (rc = col_end.alloc(ctx, sizeof(int64_t) * p, who)) ||
        (rc = has_nan_dev.alloc(ctx, (size_t)p, who)))
        return rc;
    hipLaunchKernelGGL(k_col_info, dim3(blocks_of((size_t)L, 256)), dim3(256), 0, ctx->stream, G_dev, lc.get(), L, n, ld, has_nan_dev.get(),
                       col_start.get(), col_end.get());
    PG_HIP(ctx, hipGetLastError());
    std::vector<uint8_t> has_nan((size_t)p);
    PG_HIP(ctx, hipMemcpyAsync(has_nan.data(), has_nan_dev.get(), (size_t)p, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));

    // the last window that holds a column wins the write-back (the copies are written in window order, :330-341)
    std::vector<int64_t> last_window((size_t)p, -1);
    for (int64_t a = 0; a < n_windows; ++a)
        for (int64_t c = locus_col[win_head[a]]; c < locus_col[win_tail[a] + 1]; ++c) last_window[(size_t)c] = a;
    if ((rc = upload(ctx, last_dev, last_window.data(), (size_t)p, who))) return rc;

    // windows with work, in batches under the scratch budget: per window its copy and n x n distances, per item pw keys and K links
    struct Batch { std::vector<int64_t> ini, w_off, item0, item1, id, it_col, it_ini, it_key; std::vector<int32_t> pw, it_pw; int64_t rows = 0, keys = 0; size_t bytes = 0; };
    std::vector<Batch> batches;
    for (int64_t a = 0; a < n_windows; ++a) {
        const int64_t ini = locus_col[win_head[a]], fin = locus_col[win_tail[a] + 1], pw = fin - ini;
        int64_t items = 0;
        for (int64_t c = ini; c < fin; ++c) items += has_nan[(size_t)c];
        if (items == 0) continue; // its copy would equal the input
        const size_t need = sizeof(double) * ((size_t)pw * ld + (size_t)n * n + (size_t)items * pw) + sizeof(int32_t) * (size_t)items * k_links;
        if (batches.empty() || (batches.back().bytes + need > budget && !batches.back().ini.empty())) batches.emplace_back();
        Batch &b = batches.back();
        b.ini.push_back(ini); b.pw.push_back((int32_t)pw); b.w_off.push_back(b.rows); b.id.push_back(a);
        b.item0.push_back((int64_t)b.it_col.size());
        for (int64_t c = ini; c < fin; ++c)
            if (has_nan[(size_t)c]) {
                b.it_col.push_back(c); b.it_ini.push_back(ini); b.it_pw.push_back((int32_t)pw); b.it_key.push_back(b.keys);
                b.keys += pw;
            }
        b.item1.push_back((int64_t)b.it_col.size());
        b.rows += pw;
        b.bytes += need;
    }
    if (batches.empty()) return PG_OK;
    size_t max_rows = 0, max_keys = 0, max_items = 0, max_win = 0;
    for (const Batch &b : batches) {
        max_rows = std::max(max_rows, (size_t)b.rows); max_keys = std::max(max_keys, (size_t)b.keys);
        max_items = std::max(max_items, b.it_col.size()); max_win = std::max(max_win, b.ini.size());
    }
    DevBuf<double> W, keys, dist;
    DevBuf<int32_t> links, i32;
    DevBuf<int64_t> i64;
    if ((rc = W.alloc(ctx, sizeof(double) * max_rows * ld, who)) || (rc = keys.alloc(ctx, sizeof(double) * max_keys, who)) ||
        (rc = dist.alloc(ctx, sizeof(double) * max_win * n * n, who)) || (rc = links.alloc(ctx, sizeof(int32_t) * max_items * k_links, who)) ||
        (rc = i64.alloc(ctx, sizeof(int64_t) * (5 * max_win + 3 * max_items), who)) || (rc = i32.alloc(ctx, sizeof(int32_t) * (max_win + max_items), who)))
        return rc;
    for (const Batch &b : batches) {
        const size_t nw = b.ini.size(), ni = b.it_col.size();
        int64_t *d64 = i64.get();
        int32_t *d32 = i32.get();
        const std::vector<int64_t> *h64[8] = {&b.ini, &b.w_off, &b.item0, &b.item1, &b.id, &b.it_col, &b.it_ini, &b.it_key};
        const int64_t *p64[8];
        for (int v = 0; v < 8; ++v) {
            p64[v] = d64;
            PG_HIP(ctx, hipMemcpyAsync(d64, h64[v]->data(), sizeof(int64_t) * h64[v]->size(), hipMemcpyHostToDevice, ctx->stream));
            d64 += h64[v]->size();
        }
        PG_HIP(ctx, hipMemcpyAsync(d32, b.pw.data(), sizeof(int32_t) * nw, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(ctx, hipMemcpyAsync(d32 + nw, b.it_pw.data(), sizeof(int32_t) * ni, hipMemcpyHostToDevice, ctx->stream));
        const ImpWindows win{p64[0], d32, p64[1], p64[2], p64[3], p64[4]};
        const ImpItems items{p64[5], p64[6], d32 + nw, p64[7]};
        int32_t pw_max = 0;
        for (int32_t x : b.pw) pw_max = std::max(pw_max, x);
        const unsigned slices = (unsigned)std::min<size_t>(64, ((size_t)pw_max * ld + 2047) / 2048);
        hipLaunchKernelGGL(k_aldknn_copy, dim3((unsigned)nw, slices), dim3(256), 0, ctx->stream, G_dev, ld, win, W.get());
        pg_prof_begin(ctx, PG_K_IMPUTE_LINKS);
        hipLaunchKernelGGL(k_aldknn_links, dim3((unsigned)ni), dim3(LINK_THREADS), 0, ctx->stream, G_dev, n, ld, items, keys.get(), k_links, links.get());
        pg_prof_end(ctx);
        pg_prof_begin(ctx, PG_K_IMPUTE_WALK);
        hipLaunchKernelGGL(k_aldknn_walk, dim3((unsigned)nw), dim3(256), sizeof(int) * 2 * (size_t)n, ctx->stream, W.get(), n, ld, win, items,
                           links.get(), k_links, (int)k_neighbours, col_start.get(), col_end.get(), dist.get());
        pg_prof_end(ctx);
        hipLaunchKernelGGL(k_aldknn_writeback, dim3((unsigned)nw, slices), dim3(256), 0, ctx->stream, W.get(), n, ld, win, last_dev.get(), G_out_dev);
        PG_HIP(ctx, hipGetLastError());
        PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the batch's host arrays and the shared scratch are reused
    }
    return PG_OK;
}
