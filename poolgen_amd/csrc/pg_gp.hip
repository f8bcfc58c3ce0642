// pg_gp.hip -- genomic prediction: gp::ols (gp/ols.rs:8-101) and the penalised models over it, the ridge-like lambda
// path with k-fold cross-validation (gp/penalise.rs:133-159, :248-669).
//
// Reference flow (alpha = 0, iterative = false): for r repetitions x nfolds folds: b = gp::ols on the
// training pools; for every lambda of the path: b_lambda = expand_and_contract(b, b, alpha, lambda)
// (:248-357) and error_index on the validation pools (:359-426); per repetition the lambda with the
// smallest mean error over folds; the mode over repetitions; finally expand_and_contract of the
// all-rows fit.  The reference draws folds from an unseeded thread_rng (:452-453); here the fold of
// every training row in every repetition is an explicit argument, so results are reproducible.
//
// penalised_path: X X^T on the host, the work buffers, one of two cross-validations, then select_and_apply.
// cv_fused (a wide design): every pool is validated by ONE fold of a repetition, so per repetition
//   1. FoldSolver (host thread)   pinv(X X^T[train, train]) y of every fold, scattered over the pools (solve_scatter)
//   2. pg_gp_beta_cols            every fold's slopes as columns G Z: one streaming pass over G per repetition, or
//                                 (batched) 16 columns per pass whatever repetition they belong to
//   3. ridge_path_params_cols     per column the max of the penalty norm, then for all L lambdas at once the four
//                                 redistribution masses of expand_and_contract (one pass over the columns)
//   4. PredictPipeline            k_gp_predict_folds (+ reduce): yhat[pool][lambda] from the coefficients of the fold that
//                                 holds the pool out, contracted on the fly: the second streaming pass over G, kept
//                                 out while the host scores the pass before it (error_index, n_val x L numbers)
// cv_per_fold (a tall design, too many columns, POOLGEN_RIDGE_PER_FOLD=1) per (repetition, fold): pg_gp_ols_dev, then per trait
// ridge_path_params (the same masses), k_gp_blambda (B[l][i] = expand_and_contract(b)[l] for lambda_i) and k_gp_predict (+ reduce).
// All L lambdas share the two passes over G; the reference does 1 + L passes per fold.
#include "pg_common.h"
#include <algorithm>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

namespace {

constexpr int GP_LMAX = 16; // lambdas per path (the reference uses 11: 0, 0.1, ..., 1)

struct PathParams {
    double alpha;
    double nmax;                  // max penalty norm (proxy = b itself, :262-283)
    double lambda[GP_LMAX];
    double sub_scale[GP_LMAX];    // subtracted_penalised / subtracted_depenalised (0 if nothing to expand)
    double add_scale[GP_LMAX];    // added_penalised / added_depenalised
    int L;
};

// The coefficients whose norms pick the penalised set (:262-283): the fit itself, or, for the *_with_iterative_proxy_norms
// models, the per-locus GWAS-like estimates of pg_gp_proxy_dev ((1+p) x k, row 0 unused).  b == nullptr: the fit itself.
struct Proxy {
    const double *b;
    int k, j;
};

__device__ __forceinline__ double gp_norm(double b, double alpha) { // :259-261
    return ((1.00 - alpha) * (b * b) / 1.00) + (alpha * fabs(b));
}

// max over the slopes (rows 1..p of column j) of the penalty norm; partial maxima per block
__global__ void k_gp_norm_max(const double *__restrict__ beta, int64_t p, int k, int j, int row0, double alpha,
                              double *__restrict__ part) {
    double m = 0.0;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < p; l += (int64_t)gridDim.x * blockDim.x)
        m = fmax(m, gp_norm(beta[(l + row0) * k + j], alpha));
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    __shared__ double sm[16];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, sm[w]);
        part[blockIdx.x] = m;
    }
}

// all columns of a column-major matrix in one launch: blockIdx.y = column (its own values, or the proxy's column c % kx)
__global__ void k_gp_norm_max_cols(const double *__restrict__ cols, int64_t p, Proxy X, int kx, double alpha, const int *__restrict__ skip,
                                   double *__restrict__ part, int64_t part_stride) {
    const int c = blockIdx.y;
    if (skip[c]) return;
    const double *src = X.b ? X.b : cols + (size_t)c * p;
    const int k = X.b ? X.k : 1, j = X.b ? c % kx : 0, row0 = X.b ? 1 : 0;
    double m = 0.0;
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < p; l += (int64_t)gridDim.x * blockDim.x)
        m = fmax(m, gp_norm(src[(l + row0) * k + j], alpha));
    for (int off = 32; off >= 1; off >>= 1) m = fmax(m, __shfl_xor(m, off));
    __shared__ double sm[16];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = fmax(m, sm[w]);
        part[(size_t)c * part_stride + blockIdx.x] = m;
    }
}

// For every lambda_i: subtracted/added masses of the penalised set and the norm masses of the
// de-penalised set, split by the sign of b (:296-326).  part: [block][4][GP_LMAX].
// LP = the path length rounded up to even (a compile-time constant: the pass is bound by these 4 x LP conditional sums per element,
// 16 instead of 12 of them cost a third more)
template <int LP>
__device__ __forceinline__ void gp_path_sums_body(const double *__restrict__ beta, int64_t p, int k, int j, int row0,
                                                  const PathParams &P, Proxy X, double *__restrict__ part) {
    double sp[GP_LMAX], ap[GP_LMAX], sd[GP_LMAX], ad[GP_LMAX];
#pragma unroll
    for (int i = 0; i < GP_LMAX; ++i) { sp[i] = 0.0; ap[i] = 0.0; sd[i] = 0.0; ad[i] = 0.0; }
    for (int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; l < p; l += (int64_t)gridDim.x * blockDim.x) {
        const double b = beta[(l + row0) * k + j];
        const double nrm = gp_norm(b, P.alpha);
        const double nrx = X.b ? gp_norm(X.b[(l + 1) * X.k + X.j], P.alpha) : nrm;
        const double sc = nrx / P.nmax; // normed_proxy / normed_proxy_max (:282), a true division: max/max == 1
        const bool pos = b >= 0.0;
        const double pen_pos = pos ? (((b - nrm) < 0.0) ? b : nrm) : 0.0;       // :298-305
        const double pen_neg = pos ? 0.0 : (((b + nrm) > 0.0) ? fabs(b) : nrm); // :306-313
#pragma unroll
        for (int i = 0; i < LP; ++i) { // entries beyond P.L (lambda = 0) are never read: no guard, no branches
            const bool pen = sc < P.lambda[i];
            sp[i] += pen ? pen_pos : 0.0;
            ap[i] += pen ? pen_neg : 0.0;
            sd[i] += (!pen && pos) ? nrm : 0.0;
            ad[i] += (!pen && !pos) ? nrm : 0.0;
        }
    }
    __shared__ double sm[4][4 * GP_LMAX];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < GP_LMAX; ++i) {
        double a = sp[i], b2 = ap[i], c = sd[i], d = ad[i];
        for (int off = 32; off >= 1; off >>= 1) {
            a += __shfl_xor(a, off); b2 += __shfl_xor(b2, off); c += __shfl_xor(c, off); d += __shfl_xor(d, off);
        }
        if (lane == 0) { sm[wave][i] = a; sm[wave][GP_LMAX + i] = b2; sm[wave][2 * GP_LMAX + i] = c; sm[wave][3 * GP_LMAX + i] = d; }
    }
    __syncthreads();
    if (threadIdx.x < 4 * GP_LMAX) {
        double s = 0.0;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += sm[w][threadIdx.x];
        part[(size_t)blockIdx.x * 4 * GP_LMAX + threadIdx.x] = s;
    }
}
template <int LP>
__global__ __launch_bounds__(256) void k_gp_path_sums(const double *__restrict__ beta, int64_t p, int k, int j, int row0, PathParams P,
                                                      Proxy X, double *__restrict__ part) {
    gp_path_sums_body<LP>(beta, p, k, j, row0, P, X, part);
}
// all columns of a column-major matrix in one launch: blockIdx.y = column, its norm maximum from nmax[] (device)
template <int LP>
__global__ __launch_bounds__(256) void k_gp_path_sums_cols(const double *__restrict__ cols, int64_t p, PathParams P, Proxy X, int kx,
                                                           const double *__restrict__ nmax, const int *__restrict__ skip,
                                                           double *__restrict__ part) {
    const int c = blockIdx.y;
    if (skip[c]) return;
    P.nmax = nmax[c];
    X.j = c % kx;
    gp_path_sums_body<LP>(cols + (size_t)c * p, p, 1, 0, 0, P, X, part + (size_t)c * gridDim.x * 4 * GP_LMAX);
}

// expand_and_contract of one coefficient for lambda_i (:296-352), given the global masses
__device__ __forceinline__ double gp_contract(double b, double bx, const PathParams &P, int i) {
    const double nrm = gp_norm(b, P.alpha);
    const double sc = gp_norm(bx, P.alpha) / P.nmax;
    if (sc < P.lambda[i]) { // penalised: contract by its own norm, not across zero
        if (b >= 0.0) return ((b - nrm) < 0.0) ? 0.0 : b - nrm;
        return ((b + nrm) > 0.0) ? 0.0 : b + nrm;
    }
    // de-penalised: receives its share of the contracted mass of its sign
    if (b >= 0.0) return b + P.sub_scale[i] * nrm;
    return b - P.add_scale[i] * nrm;
}

// B[l][i] for all lambdas (row stride GP_LMAX)
__global__ void k_gp_blambda(const double *__restrict__ beta, int64_t p, int k, int j, PathParams P, Proxy X,
                             double *__restrict__ B) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= p) return;
    const double b = beta[(l + 1) * k + j];
    const double bx = X.b ? X.b[(l + 1) * X.k + X.j] : b;
#pragma unroll
    for (int i = 0; i < GP_LMAX; ++i) B[l * GP_LMAX + i] = (i < P.L) ? gp_contract(b, bx, P, i) : 0.0;
}

// the all-rows fit's slopes, formed as columns of a batched coefficient pass (column-major), into the model's [1 + p] x k layout
__global__ void k_gp_cols_to_rows(const double *__restrict__ cols, int64_t p, int k, double *__restrict__ rows) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= p) return;
    for (int j = 0; j < k; ++j) rows[l * k + j] = cols[(size_t)j * p + l];
}

// single-lambda variant writing the penalised column back (final model, :653-662)
__global__ void k_gp_apply(double *__restrict__ beta, int64_t p, int k, int j, PathParams P, Proxy X, int i) {
    const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= p) return;
    const double b = beta[(l + 1) * k + j];
    beta[(l + 1) * k + j] = gp_contract(b, X.b ? X.b[(l + 1) * X.k + X.j] : b, P, i);
}

// yhat partials: thread = pool, block = slab of loci; B rows are wave-uniform (scalar loads)
__global__ __launch_bounds__(256) void k_gp_predict(const double *__restrict__ G, const double *__restrict__ B,
                                                    int64_t p, int n, int64_t ld, int64_t loci_per_block,
                                                    double *__restrict__ part) {
    const int pool = blockIdx.y * 256 + threadIdx.x;
    const int64_t l0 = (int64_t)blockIdx.x * loci_per_block;
    const int64_t l1 = min(p, l0 + loci_per_block);
    double acc[GP_LMAX];
#pragma unroll
    for (int i = 0; i < GP_LMAX; ++i) acc[i] = 0.0;
    const bool on = pool < n;
    const double *gp = G + (on ? pool : 0);
    int64_t l = l0;
    for (; l + 4 <= l1; l += 4) {
        double g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) g[u] = gp[(l + u) * ld];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double *bl = B + (l + u) * GP_LMAX;
#pragma unroll
            for (int i = 0; i < GP_LMAX; ++i) acc[i] = fma(g[u], bl[i], acc[i]);
        }
    }
    for (; l < l1; ++l) {
        const double g = gp[l * ld];
        const double *bl = B + l * GP_LMAX;
#pragma unroll
        for (int i = 0; i < GP_LMAX; ++i) acc[i] = fma(g, bl[i], acc[i]);
    }
    if (on) {
        double *o = part + ((size_t)blockIdx.x * n + pool) * GP_LMAX;
#pragma unroll
        for (int i = 0; i < GP_LMAX; ++i) o[i] = acc[i];
    }
}

// All folds of a repetition at once: bf (p x C) holds the slopes of every fold's training fit (column of pool i
// for this trait = colof[i], the fold that VALIDATES pool i -- every pool is validated by exactly one fold, so one
// pass over G serves all of them).  The contracted coefficient is formed on the fly from the fold's masses
// (the very arithmetic of gp_contract); partials and their reduction are laid out as in k_gp_predict.
struct FoldMasses { double nmax, sub_scale[GP_LMAX], add_scale[GP_LMAX]; };
// The contracted coefficient depends on (locus, fold, lambda) only, not on the pool: a block first forms them for a
// chunk of loci in LDS (chunk x folds x lambdas), then every thread (= pool) accumulates yhat from ITS fold's entries:
// per (locus, pool) one load of G, L LDS operands and L FMAs instead of the whole expand_and_contract arithmetic.
// LP = the path length rounded up to even, a compile-time constant: entries beyond L carry lambda = 0 and zero masses
// (harmless finite numbers nobody reads), so neither loop needs a guard -- guarded, every FMA became a branch with its
// own LDS round trip.
// Bound: the LDS return path -- L / 2 16-byte operand reads per (locus, pool): 96 bytes per element at 12 lambdas, 1.39 ms
// of LDS time per 2 M loci x 500 pools against 1.46 ms measured (0.685 of the HBM peak).  A matrix-core form (pools
// regrouped by fold into 16-pool tiles, two LDS reads per 4 loci x 16 pools x 16 lambdas) was built twice, parity green,
// and is slower: 0.55 with two 8-wave workgroups per CU and one chunk of rows ahead, 0.46 with one 16-wave workgroup and
// two chunks ahead -- the serial phases of a chunk (stage write, table, barrier, products) outlast its memory time
// (tools/experiments/).
template <int LP, bool GROUPED, bool ODD = false>
__global__ __launch_bounds__(512) void k_gp_predict_folds(const double *__restrict__ G, const double *__restrict__ bf,
                                                          int C, const int32_t *__restrict__ colof,
                                                          const FoldMasses *__restrict__ FM, PathParams P0, Proxy X,
                                                          int64_t p, int n, int64_t ld, int64_t loci_per_block,
                                                          int chunk, double *__restrict__ part, int groups) {
    extern __shared__ __attribute__((aligned(16))) double Bs[]; // [chunk][F][LS]
    constexpr int LS = LP + 2; // fold stride: 8 * LS bytes put the folds' 16-byte reads of one lambda pair on distinct banks
    // ODD: the path has LP - 1 values (the reference's 11): the last one is read alone (8 bytes) and the padding entry neither formed
    // nor read nor multiplied -- 88 instead of 96 bytes of LDS operands per (locus, pool) of a pass the LDS return path bounds
    constexpr int LN = ODD ? LP - 1 : LP;
    const int k = X.k, j = X.j;
    const int F = C / k;
    // 256 or 512 threads: one block spans up to 512 pools.  With fewer pools than that the block splits into `groups` of
    // blockDim / groups threads: group g takes the loci g, g + groups, ... of every chunk (a row of 100 pools would leave three
    // fifths of a 256-thread block without a pool, and the pass with a third of its loads in flight) and leaves its own partial.
    // (GROUPED is a template parameter: the run-time strides cost the plain form 50 registers and half its occupancy)
    const int gsz = GROUPED ? blockDim.x / groups : blockDim.x, grp = GROUPED ? threadIdx.x / gsz : 0;
    const int pool = GROUPED ? (int)threadIdx.x - grp * gsz : (int)(blockIdx.y * blockDim.x + threadIdx.x);
    const int64_t l0 = (int64_t)blockIdx.x * loci_per_block;
    const int64_t l1 = min(p, l0 + loci_per_block);
    double acc[LP];
#pragma unroll
    for (int i = 0; i < LP; ++i) acc[i] = 0.0;
    const bool inr = pool < n;
    const int c = inr ? colof[pool] : -1;
    const bool on = c >= 0;
    const int f = on ? c / k : 0;
    const double *gp = G + (inr ? pool : 0);
    // The table's inputs must not cost a memory round trip per chunk between the two barriers: the folds' masses sit in
    // LDS for the whole launch, and the first PF_NI items of a thread (all of them at the shipped shapes) get the next
    // chunk's coefficients while this chunk is accumulated.
    constexpr int PF_NI = 2, FMW = 2 * GP_LMAX + 1;
    double *masses = Bs + (size_t)chunk * F * LS; // [F][FMW]: { nmax, sub_scale[], add_scale[] } of this trait's columns
    for (int i = threadIdx.x; i < F * FMW; i += blockDim.x) {
        const int ff = i / FMW, w = i - ff * FMW;
        const FoldMasses *src = FM + (ff * k + j);
        masses[i] = w == 0 ? src->nmax : (w <= GP_LMAX ? src->sub_scale[w - 1] : src->add_scale[w - 1 - GP_LMAX]);
    }
    double bn[PF_NI], xn[PF_NI];
    auto fetch = [&](int64_t lc2) {
        const int m2 = (int)min((int64_t)chunk, l1 - lc2);
#pragma unroll
        for (int q = 0; q < PF_NI; ++q) {
            const int item = threadIdx.x + q * blockDim.x;
            bn[q] = 0.0; xn[q] = 0.0;
            if (item < m2 * F) {
                const int ff = item / m2, ll = item - ff * m2; // bf is column-major: consecutive threads, consecutive loci
                bn[q] = bf[(size_t)(ff * k + j) * p + lc2 + ll];
                if (X.b) xn[q] = X.b[(lc2 + ll + 1) * X.k + X.j];
            }
        }
    };
    if (l0 < l1) fetch(l0);
    for (int64_t lc = l0; lc < l1; lc += chunk) {
        const int m = (int)min((int64_t)chunk, l1 - lc);
        __syncthreads();
        auto table_row = [&](int item, double b, double bx) {
            const int ff = item / m, ll = item - ff * m;
            const double *fm = masses + ff * FMW;
            const double nrm = gp_norm(b, P0.alpha);
            const double sc = (X.b ? gp_norm(bx, P0.alpha) : nrm) / fm[0];
            const bool pos = b >= 0.0;
            const double pen = pos ? (((b - nrm) < 0.0) ? 0.0 : b - nrm) : (((b + nrm) > 0.0) ? 0.0 : b + nrm);
            double *o = Bs + (size_t)(ll * F + ff) * LS;
#pragma unroll
            for (int i = 0; i < LN; ++i) {
                const double dep = pos ? b + fm[1 + i] * nrm : b - fm[1 + GP_LMAX + i] * nrm;
                o[i] = (sc < P0.lambda[i]) ? pen : dep;
            }
        };
#pragma unroll
        for (int q = 0; q < PF_NI; ++q) {
            const int item = threadIdx.x + q * blockDim.x;
            if (item < m * F) table_row(item, bn[q], xn[q]);
        }
        for (int item = threadIdx.x + PF_NI * blockDim.x; item < m * F; item += blockDim.x) {
            const int ff = item / m, ll = item - ff * m;
            const int64_t l = lc + ll;
            table_row(item, bf[(size_t)(ff * k + j) * p + l], X.b ? X.b[(l + 1) * X.k + X.j] : 0.0);
        }
        __syncthreads();
        if (lc + chunk < l1) fetch(lc + chunk);
        if (on) {
            const double *bs = Bs + (size_t)f * LS;
            constexpr int U = 8; // loads of G in flight per thread
            // this group's loci of the chunk: grp, grp + groups, ...  (mg of them; ll counts them)
            // (uniform trip count: the loci every group has; the m % groups left-over loci go to the first groups below)
            const int mg = GROUPED ? m / groups : m;
            // GROUPED: uniform row base + one 32-bit per-thread offset (a per-thread 64-bit base costs the loop 50 registers)
            const double *gq = GROUPED ? G + lc * ld : gp + lc * ld;
            const uint32_t voff = GROUPED ? (uint32_t)(((int64_t)grp * ld + (inr ? pool : 0)) * 8) : 0u;
            const int64_t gstep = GROUPED ? (int64_t)groups * ld : ld;
            auto gload = [&](int i) -> double {
                return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(gq + i * gstep) + voff);
            };
            const double *bq = bs + (size_t)grp * F * LS;
            const int bstep = GROUPED ? groups * F * LS : F * LS;
            int ll = 0;
            for (; ll + U <= mg; ll += U) {
                double g[U];
#pragma unroll
                for (int u = 0; u < U; ++u) g[u] = gload(ll + u);
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const double *q = bq + (ll + u) * bstep;
#pragma unroll
                    for (int i = 0; i + 2 <= LN; i += 2) {
                        const double2 b2 = *reinterpret_cast<const double2 *>(q + i);
                        acc[i] = fma(g[u], b2.x, acc[i]);
                        acc[i + 1] = fma(g[u], b2.y, acc[i + 1]);
                    }
                    if constexpr (ODD) acc[LN - 1] = fma(g[u], q[LN - 1], acc[LN - 1]);
                }
            }
            for (; ll < mg; ++ll) {
                const double g = gload(ll);
                const double *q = bq + ll * bstep;
#pragma unroll
                for (int i = 0; i + 2 <= LN; i += 2) {
                    const double2 b2 = *reinterpret_cast<const double2 *>(q + i);
                    acc[i] = fma(g, b2.x, acc[i]);
                    acc[i + 1] = fma(g, b2.y, acc[i + 1]);
                }
                if constexpr (ODD) acc[LN - 1] = fma(g, q[LN - 1], acc[LN - 1]);
            }
            if (GROUPED && grp + groups * mg < m) { // one of the m % groups left-over loci
                const double g = gload(mg);
                const double *q = bq + mg * bstep;
#pragma unroll
                for (int i = 0; i + 2 <= LN; i += 2) {
                    const double2 b2 = *reinterpret_cast<const double2 *>(q + i);
                    acc[i] = fma(g, b2.x, acc[i]);
                    acc[i + 1] = fma(g, b2.y, acc[i + 1]);
                }
                if constexpr (ODD) acc[LN - 1] = fma(g, q[LN - 1], acc[LN - 1]);
            }
        }
    }
    if (inr) {
        double *o = part + (((size_t)blockIdx.x * (GROUPED ? groups : 1) + grp) * n + pool) * GP_LMAX;
#pragma unroll
        for (int i = 0; i < GP_LMAX; ++i) o[i] = i < LP ? acc[i] : 0.0;
    }
}

// 64 outputs x 8 groups of slabs per workgroup; the groups' sums are combined in group order (same result every run)
__global__ __launch_bounds__(512) void k_gp_predict_reduce(const double *__restrict__ part, int nblocks, int n,
                                                           double *__restrict__ out) {
    __shared__ double sm[8][64];
    const int o = threadIdx.x & 63, g = threadIdx.x >> 6;
    const int idx = blockIdx.x * 64 + o; // pool * GP_LMAX + i
    double s = 0.0;
    if (idx < n * GP_LMAX)
        for (int b = g; b < nblocks; b += 8) s += part[(size_t)b * n * GP_LMAX + idx];
    sm[g][o] = s;
    __syncthreads();
    if (g == 0 && idx < n * GP_LMAX) {
        double t = sm[0][o];
        for (int q = 1; q < 8; ++q) t += sm[q][o];
        out[idx] = t;
    }
}

// yhat partials for a plain coefficient matrix: thread = pool, block = slab of loci, up to 8 traits
__global__ __launch_bounds__(256) void k_gp_predict_beta(const double *__restrict__ G, const double *__restrict__ beta,
                                                         int k, int64_t p, int n, int64_t ld, int64_t loci_per_block,
                                                         double *__restrict__ part) {
    const int pool = blockIdx.y * 256 + threadIdx.x;
    const int64_t l0 = (int64_t)blockIdx.x * loci_per_block;
    const int64_t l1 = min(p, l0 + loci_per_block);
    double acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0;
    const bool on = pool < n;
    const double *gp = G + (on ? pool : 0);
    for (int64_t l = l0; l < l1; ++l) {
        const double g = gp[l * ld];
        const double *bl = beta + (l + 1) * k; // row 0 of beta is the intercept
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (j < k) acc[j] = fma(g, bl[j], acc[j]);
    }
    if (on) {
        double *o = part + ((size_t)blockIdx.x * n + pool) * 8;
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = acc[j];
    }
}
__global__ void k_gp_predict_beta_reduce(const double *__restrict__ part, int nblocks, int n, double *__restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x; // pool * 8 + j
    if (idx >= n * 8) return;
    double s = 0.0;
    for (int b = 0; b < nblocks; ++b) s += part[(size_t)b * n * 8 + idx];
    out[idx] = s;
}

// pearsons_correlation (gwas/correlation_test.rs:7-71) on two complete vectors, as error_index calls it
double host_pearson_r(const std::vector<double> &x, const std::vector<double> &y) {
    const int n = (int)x.size();
    double mx = 0, my = 0;
    for (int i = 0; i < n; ++i) { mx += x[i]; my += y[i]; }
    mx /= n; my /= n;
    double sxy = 0, sxx = 0, syy = 0;
    for (int i = 0; i < n; ++i) { const double dx = x[i] - mx, dy = y[i] - my; sxy += dx * dy; sxx += dx * dx; syy += dy * dy; }
    const double r = sxy / (std::sqrt(sxx) * std::sqrt(syy));
    if (std::isnan(r)) return NAN;
    const double sden = (1.0 - r * r) / ((double)n - 2.0);
    if (sden <= 0.0) return r;
    return std::round(r * 1e7) / 1e7; // sensible_round(r, 7)
}

// ---- host side: the steps every route shares --------------------------------------------------------------------

// What a call of the path is given (the entry points fill it in the order of their own arguments), and the grid.
struct GpCall {
    const double *G; int64_t p; int n; int64_t ld;   // device: p loci x n pools, row pitch ld
    const double *Y; int k;                          // host: n x k
    const int64_t *rows; int n_rows;                 // the outer training pools
    const int32_t *fold_of; int n_reps, n_folds;     // fold of rows[i] in repetition r: fold_of[r * n_rows + i]
    double alpha;                                    // < 0: the 2-D grid alpha x lambda (:479-498)
    const double *proxy;                             // device (1 + p) x k of pg_gp_proxy_dev, or null (see Proxy)
    std::vector<double> path;                        // the lambda values (:470-476); the grid's alpha values are the same
    int L() const { return (int)path.size(); }
    int A() const { return alpha >= 0.0 ? 1 : L(); }
    int C() const { return n_folds * k; }            // fold x trait coefficient columns of one repetition
    double alpha_at(int a) const { return alpha >= 0.0 ? alpha : path[a]; }
    // error indices (rep, fold, alpha, lambda, trait) as the reference's `performances` (:509)
    size_t perf_at(int rep, int fold, int a, int li, int j) const { return ((((size_t)rep * n_folds + fold) * A() + a) * L() + li) * k + j; }
};

// POOLGEN_GP_TIMING=1: host-side phase times of a call on stderr.  A phase is what runs in the scope of a Phase on its field.
struct PhaseTimes {
    using Clock = std::chrono::steady_clock;
    const bool report = pg_switch(PG_SW_GP_TIMING) != nullptr;
    const Clock::time_point entry = Clock::now();
    double before = 0, solve = 0, beta = 0, params = 0, predict = 0, alloc = 0, release = 0; // seconds
    static double since(Clock::time_point t) { return std::chrono::duration<double>(Clock::now() - t).count(); }
    void report_phases() const {
        if (report)
            std::fprintf(stderr, "gp path: before the repetitions %.1f ms; fold solves %.1f ms, coefficient passes %.1f ms, masses %.1f ms, prediction + scores %.1f ms; the columns' memory: allocation %.1f ms, release %.1f ms; since entry %.1f ms\n",
                         1e3 * before, 1e3 * solve, 1e3 * beta, 1e3 * params, 1e3 * predict, 1e3 * alloc, 1e3 * release, 1e3 * since(entry));
    }
    void report_call() const { if (report) std::fprintf(stderr, "gp path: whole call %.1f ms\n", 1e3 * since(entry)); }
};
struct Phase {
    double &acc;
    PhaseTimes::Clock::time_point t0 = PhaseTimes::Clock::now();
    ~Phase() { acc += PhaseTimes::since(t0); }
};

// f(std::integral_constant<int, LP>{}) for LP = the even path length (upwards: downwards, the same kernels come out in the opposite order)
template <int LP = 2, typename F>
void with_path_len(int L, F f) {
    if (((L + 1) & ~1) == LP) f(std::integral_constant<int, LP>{});
    else if constexpr (LP < GP_LMAX) with_path_len<LP + 2>(L, f);
}

// the slabs of loci of a prediction pass: `nblk` blocks of `lpb` loci each
struct Slabs { int nblk; int64_t lpb; };
Slabs predict_slabs(const pg_ctx *ctx, int64_t p) {
    const int want = std::max(1, std::min<int>(ctx->cus * 4, (int)((p + 255) / 256)));
    const int64_t lpb = (p + want - 1) / want;
    return Slabs{(int)((p + lpb - 1) / lpb), lpb};
}

struct RidgeWork {
    DevBuf<double> raw;
    Slabs S{0, 0};
    double *part = nullptr;   // block partials (max / path sums / predictions)
    double *B = nullptr;      // p x GP_LMAX
    double *yhat = nullptr;   // n x GP_LMAX
    int alloc(pg_ctx *ctx, const GpCall &in) {
        S = predict_slabs(ctx, in.p);
        const size_t C = in.C();
        const size_t part_doubles = std::max<size_t>((C + 1) * 1024 * 4 * GP_LMAX + C * 4 * GP_LMAX,
                                                     (size_t)S.nblk * in.n * GP_LMAX * 4); // (x 4: the prediction pass' locus groups at n <= 256)
        if (int rc = raw.alloc(ctx, sizeof(double) * (part_doubles + (size_t)in.p * GP_LMAX + (size_t)in.n * GP_LMAX), "gp_ridge")) return rc;
        part = raw.get();
        B = part + part_doubles;
        yhat = B + (size_t)in.p * GP_LMAX;
        return PG_OK;
    }
};

// gp::ols, wide branch (gp/ols.rs:47-72), as far as the host takes it: the fit on the pools `rows` is b = X^T z with
// z = pinv(A) Y[rows] scattered over the pools and zero elsewhere, A the principal sub-block `rows` of the full-data X X^T
// (n x n, host).  Fills the columns col0 .. col0 + k - 1 of Z (n rows of `stride`, zero on entry) and adds the intercepts (the
// column sums: X's first column is all ones) to b0[0 .. k), in row order.  Non-zero when the pinv fails; nothing is written then.
int solve_scatter(const double *xxt, int n, const double *Y, int k, const int64_t *rows, int r, double *Z, int stride, int col0,
                  double *b0) {
    std::vector<double> A((size_t)r * r), Ysub((size_t)r * k), V((size_t)r * k);
    for (int a = 0; a < r; ++a) {
        for (int b = 0; b < r; ++b) A[(size_t)a * r + b] = xxt[(size_t)rows[a] * n + rows[b]];
        for (int j = 0; j < k; ++j) Ysub[(size_t)a * k + j] = Y[(size_t)rows[a] * k + j];
    }
    if (pg_pinv_solve_sym(A.data(), r, Ysub.data(), k, V.data()) != 0) return 1;
    for (int a = 0; a < r; ++a)
        for (int j = 0; j < k; ++j) {
            Z[(size_t)rows[a] * stride + col0 + j] = V[(size_t)a * k + j];
            b0[j] += V[(size_t)a * k + j];
        }
    return 0;
}

PathParams path_params(double alpha, const std::vector<double> &path) { // nmax and the masses still to come
    PathParams P;
    std::memset(&P, 0, sizeof P);
    P.alpha = alpha;
    P.L = (int)path.size();
    for (int i = 0; i < P.L; ++i) P.lambda[i] = path[i];
    return P;
}

// from the four sums of one lambda (subtracted / added of the penalised set, norms of the de-penalised set by sign) to its two quotients
void close_masses(double sp, double ap, double sd, double ad, double &sub_scale, double &add_scale) {
    // "absence of available slots" (:329-335)
    if ((sp > 0.0) & (sd == 0.0)) { ap -= sp; sp = 0.0; }
    else if ((ap > 0.0) & (ad == 0.0)) { sp -= ap; ap = 0.0; }
    // b += subtracted_penalised * (normed / subtracted_depenalised)  (:345-351); 0/0 never reaches a
    // coefficient because an empty de-penalised side has no coefficients to expand
    sub_scale = (sd != 0.0) ? sp / sd : 0.0;
    add_scale = (ad != 0.0) ? ap / ad : 0.0;
}

// norm maximum, path sums and masses for trait j of `beta_dev` ((1 + p) x k); the blocks' partials are combined on the host, in block order
int ridge_path_params(pg_ctx *ctx, const double *beta_dev, int64_t p, int k, int j, double alpha,
                      const std::vector<double> &path, RidgeWork &W, PathParams &P, int row0 = 1, Proxy X = Proxy{nullptr, 0, 0}) {
    const int nb = 1024;
    std::vector<double> h((size_t)nb * 4 * GP_LMAX);
    if (X.b) hipLaunchKernelGGL(k_gp_norm_max, dim3(nb), dim3(256), 0, ctx->stream, X.b, p, X.k, X.j, 1, alpha, W.part);
    else hipLaunchKernelGGL(k_gp_norm_max, dim3(nb), dim3(256), 0, ctx->stream, beta_dev, p, k, j, row0, alpha, W.part);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(h.data(), W.part, sizeof(double) * nb, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    P = path_params(alpha, path);
    for (int b = 0; b < nb; ++b) P.nmax = std::max(P.nmax, h[b]);
    with_path_len(P.L, [&](auto lp) {
        hipLaunchKernelGGL(k_gp_path_sums<decltype(lp)::value>, dim3(nb), dim3(256), 0, ctx->stream, beta_dev, p, k, j, row0, P, X, W.part);
    });
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(h.data(), W.part, sizeof(double) * nb * 4 * GP_LMAX, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < P.L; ++i) {
        double sp = 0, ap = 0, sd = 0, ad = 0;
        for (int b = 0; b < nb; ++b) {
            const double *q = &h[(size_t)b * 4 * GP_LMAX];
            sp += q[i]; ap += q[GP_LMAX + i]; sd += q[2 * GP_LMAX + i]; ad += q[3 * GP_LMAX + i];
        }
        close_masses(sp, ap, sd, ad, P.sub_scale[i], P.add_scale[i]);
    }
    return PG_OK;
}


// per column: out[c][q] = max or sum over the blocks' partials, in block order (what the host loop of ridge_path_params does)
// one wave per output: lane t takes blocks t, t + 64, ...; the 64 lane sums are combined by a fixed butterfly
__global__ __launch_bounds__(256) void k_gp_reduce_parts(const double *__restrict__ part, int ncols, int nb, int64_t col_stride,
                                                         int elem_stride, int use, int is_max, double *__restrict__ out) {
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6); // c * use + q
    const int lane = threadIdx.x & 63;
    if (idx >= ncols * use) return;
    const int c = idx / use, q = idx - c * use;
    const double *src = part + (size_t)c * col_stride + q;
    double r = 0.0;
    for (int b = lane; b < nb; b += 64) r = is_max ? fmax(r, src[(size_t)b * elem_stride]) : r + src[(size_t)b * elem_stride];
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(r, off);
        r = is_max ? fmax(r, o) : r + o;
    }
    if (lane == 0) out[idx] = r;
}

// ridge_path_params for all columns of `cols_dev` (COLUMN-major, ncols x p: every column is one contiguous stream) at once: the columns' launches queue up behind
// each other and the host synchronises twice instead of 2 * ncols times.  skip[c] != 0: column not in use.
// The blocks' partials are combined on the device (k_gp_reduce_parts): not the order of ridge_path_params, so the two are not interchangeable bit for bit.
int ridge_path_params_cols(pg_ctx *ctx, const double *cols_dev, int64_t p, int ncols, int k, double alpha,
                           const std::vector<double> &path, RidgeWork &W, const double *proxy_dev, const std::vector<int> &skip,
                           std::vector<FoldMasses> &out) {
    // blocks per column: enough to fill the chip on a long column, few on a short one (every block's 64 partial sums are
    // cleared, written and reduced again: at p = 2e5 that overhead was most of the mass step)
    const int nb = (int)std::min<int64_t>(1024, std::max<int64_t>(32, p / 2048));
    const int width = 4 * GP_LMAX;
    double *red = W.part + (size_t)ncols * nb * width; // room reserved by RidgeWork::alloc (sized for nb = 1024)
    std::vector<double> h((size_t)ncols * width);
    out.assign(ncols, FoldMasses{}); // (entries beyond the path stay zero)
    PG_HIP(ctx, hipMemsetAsync(W.part, 0, sizeof(double) * (size_t)ncols * nb * width, ctx->stream)); // skipped columns reduce to 0
    // the maxima stay on the device for the path sums (and travel to the host with them, further down)
    double *nmax_dev = red + (size_t)ncols * width;
    int *skip_dev = reinterpret_cast<int *>(nmax_dev + ncols);
    PG_HIP(ctx, hipMemcpyAsync(skip_dev, skip.data(), sizeof(int) * ncols, hipMemcpyHostToDevice, ctx->stream));
    const Proxy X{proxy_dev, k, 0};
    hipLaunchKernelGGL(k_gp_norm_max_cols, dim3(nb, ncols), dim3(256), 0, ctx->stream, cols_dev, p, X, k, alpha, skip_dev,
                       W.part, (int64_t)nb * width); // every column in one launch (was one launch per column: 200 per config-4 run)
    hipLaunchKernelGGL(k_gp_reduce_parts, dim3((ncols + 3) / 4), dim3(256), 0, ctx->stream, W.part, ncols, nb, (int64_t)nb * width, 1,
                       1, 1, red);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipMemcpyAsync(nmax_dev, red, sizeof(double) * ncols, hipMemcpyDeviceToDevice, ctx->stream));
    const PathParams Pc = path_params(alpha, path);
    with_path_len(Pc.L, [&](auto lp) {
        hipLaunchKernelGGL(k_gp_path_sums_cols<decltype(lp)::value>, dim3(nb, ncols), dim3(256), 0, ctx->stream, cols_dev, p, Pc, X, k,
                           nmax_dev, skip_dev, W.part);
    });
    hipLaunchKernelGGL(k_gp_reduce_parts, dim3((ncols * width + 3) / 4), dim3(256), 0, ctx->stream, W.part, ncols, nb,
                       (int64_t)nb * width, width, width, 0, red);
    PG_HIP(ctx, hipGetLastError());
    std::vector<double> hmax(ncols);
    PG_HIP(ctx, hipMemcpyAsync(h.data(), red, sizeof(double) * ncols * width, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(hmax.data(), nmax_dev, sizeof(double) * ncols, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // `skip` (the caller's) has been consumed as well
    for (int c = 0; c < ncols; ++c) {
        FoldMasses &M = out[c];
        M.nmax = skip[c] ? 1.0 : hmax[c];
        const double *q = &h[(size_t)c * width];
        for (int i = 0; i < Pc.L && !skip[c]; ++i) close_masses(q[i], q[GP_LMAX + i], q[2 * GP_LMAX + i], q[3 * GP_LMAX + i], M.sub_scale[i], M.add_scale[i]);
    }
    return PG_OK;
}

// error_index (:359-426) of trait j on the validation pools `iva`, for every lambda, from the slopes' part of the
// predictions yh (n x GP_LMAX) and the intercept b0j
void score(const GpCall &in, std::vector<double> &perf, const std::vector<double> &yh, int rep, int fold, int a, int j, double b0j,
           const std::vector<int64_t> &iva) {
    const int nv = (int)iva.size(), k = in.k;
    std::vector<double> yt(nv), yp(nv);
    double mn = 0, mx = 0;
    for (int i = 0; i < nv; ++i) {
        yt[i] = in.Y[(size_t)iva[i] * k + j];
        if (i == 0 || yt[i] < mn) mn = yt[i];
        if (i == 0 || yt[i] > mx) mx = yt[i];
    }
    for (int li = 0; li < in.L(); ++li) {
        for (int i = 0; i < nv; ++i) yp[i] = b0j + yh[(size_t)iva[i] * GP_LMAX + li];
        const double cor = host_pearson_r(yt, yp);
        double mae = 0, mse = 0;
        for (int i = 0; i < nv; ++i) { const double d = yt[i] - yp[i]; mae += std::fabs(d); mse += d * d; }
        mae /= (mx - mn);
        mse /= ((mx - mn) * (mx - mn));
        const double rmse = std::sqrt(mse) / (mx - mn);
        perf[in.perf_at(rep, fold, a, li, j)] = ((1.0 - std::fabs(cor)) + mae + mse + rmse) / 4.0;
    }
}

// ---- the fused cross-validation -------------------------------------------------------------------------------

// the host's part of the fits of one repetition (or, with no folds and k columns, of the all-rows fit)
struct RepSolve {
    std::vector<std::vector<int64_t>> tr, va; // per fold: training and validation pools
    std::vector<double> Z, b0c;               // n x columns: pinv(X X^T) y scattered over the pools; the columns' intercepts
    bool bad = false;                         // a pinv failed
    bool live(int f) const { return !va[f].empty() && !tr[f].empty(); } // an empty fold leaves NaN, as an empty slice would
    void split(const GpCall &in, int rep) {   // tr, va of repetition `rep`, pools in row order
        tr.assign(in.n_folds, {}); va.assign(in.n_folds, {});
        for (int i = 0; i < in.n_rows; ++i) {
            const int f = in.fold_of[(size_t)rep * in.n_rows + i];
            for (int g = 0; g < in.n_folds; ++g) (g == f ? va[g] : tr[g]).push_back(in.rows[i]);
        }
    }
};

// The folds' host solves need nothing from the GPU but X X^T: a background thread works through the repetitions (one
// worker thread per fold inside), then the all-rows fit, ahead of the device passes.  The destructor joins it.
class FoldSolver {
    const GpCall &in_;
    const double *xxt_;
    std::vector<RepSolve> fits_; // [n_reps] is the all-rows fit (gp/ols.rs:47-72 on `rows`)
    std::mutex m_;
    std::condition_variable cv_;
    int done_ = 0;               // fits_[0 .. done_) are final
    std::thread th_;

    void solve_rep(RepSolve &R, int rep) const {
        const int n_folds = in_.n_folds, k = in_.k, C = in_.C();
        R.split(in_, rep);
        R.Z.assign((size_t)in_.n * C, 0.0); R.b0c.assign(C, 0.0);
        std::vector<int> badf(n_folds, 0);
        std::vector<std::thread> th;
        for (int f = 0; f < n_folds; ++f)
            if (R.live(f))
                th.emplace_back([&, f] {
                    badf[f] = solve_scatter(xxt_, in_.n, in_.Y, k, R.tr[f].data(), (int)R.tr[f].size(), R.Z.data(), C, f * k, &R.b0c[f * k]);
                });
        for (auto &x : th) x.join();
        for (int f = 0; f < n_folds; ++f) R.bad = R.bad || badf[f];
    }

public:
    FoldSolver(const GpCall &in, const double *xxt, bool with_all_rows) : in_(in), xxt_(xxt), fits_(in.n_reps + 1) {
        th_ = std::thread([this, with_all_rows] {
            for (int r = 0; r <= in_.n_reps; ++r) {
                RepSolve &R = fits_[r];
                if (r < in_.n_reps) solve_rep(R, r);
                else if (with_all_rows) {
                    R.Z.assign((size_t)in_.n * in_.k, 0.0); R.b0c.assign(in_.k, 0.0);
                    R.bad = solve_scatter(xxt_, in_.n, in_.Y, in_.k, in_.rows, in_.n_rows, R.Z.data(), in_.k, 0, R.b0c.data()) != 0;
                }
                { std::lock_guard<std::mutex> g(m_); ++done_; }
                cv_.notify_all();
            }
        });
    }
    ~FoldSolver() { th_.join(); }
    const RepSolve *wait(int r) { // repetition r, or at n_reps the all-rows fit; null when one of its pinvs failed
        std::unique_lock<std::mutex> g(m_);
        cv_.wait(g, [&] { return done_ > r; });
        return fits_[r].bad ? nullptr : &fits_[r];
    }
};

// One prediction pass is kept OUT while the host goes on (the next repetition's coefficient passes, the next masses, the
// scores of the pass before): its predictions land in yh_in_[turn], the small host arrays its copies read stay alive in
// turn.  The destructor waits for whatever is still out: no return leaves a copy in flight into or out of this staging.
class PredictPipeline {
    pg_ctx *ctx_;
    const GpCall &in_;
    RidgeWork &W_;
    FoldMasses *fm_dev_;        // C
    int32_t *colof_dev_;        // n
    std::vector<double> &perf_;
    std::vector<double> yh_in_[2];
    std::vector<int32_t> colof_h_[2];
    std::vector<FoldMasses> fm_h_[2];
    int fm_turn_ = 0;
    struct Pending { const RepSolve *R; int rep, a, j, turn; } pend_{nullptr, 0, 0, 0, 0}; // R == null: nothing out
    bool busy_ = false;         // something has been queued since the last synchronisation this object has seen
    PathParams P0_;             // alpha and the path of the launches that follow (set_masses)

    void score_pass(const Pending &q) {
        for (int f = 0; f < in_.n_folds; ++f)
            if (q.R->live(f)) score(in_, perf_, yh_in_[q.turn], q.rep, f, q.a, q.j, q.R->b0c[f * in_.k + q.j], q.R->va[f]);
    }

public:
    PredictPipeline(pg_ctx *ctx, const GpCall &in, RidgeWork &W, FoldMasses *fm_dev, int32_t *colof_dev, std::vector<double> &perf)
        : ctx_(ctx), in_(in), W_(W), fm_dev_(fm_dev), colof_dev_(colof_dev), perf_(perf) {}
    ~PredictPipeline() { if (busy_) (void)hipStreamSynchronize(ctx_->stream); }

    // the redistribution masses of every (fold, trait) column of repetition R (bfr: its C columns) for the launches that follow.
    // Their own launches queue up behind the prediction pass that is still out, so the latency of this chain of small kernels
    // and of its synchronisation is the device's busy time
    int set_masses(const RepSolve &R, const double *bfr, double alpha) {
        const int C = in_.C(), k = in_.k;
        std::vector<FoldMasses> &fm = fm_h_[fm_turn_ ^= 1];
        std::vector<int> skip(C, 0);
        for (int c = 0; c < C; ++c) skip[c] = !R.live(c / k);
        if (int rc = ridge_path_params_cols(ctx_, bfr, in_.p, C, k, alpha, in_.path, W_, in_.proxy, skip, fm)) return rc;
        P0_ = path_params(alpha, in_.path); // alpha, lambda[], L are the same for every column; the masses travel in fm
        busy_ = true;
        if (hipMemcpyAsync(fm_dev_, fm.data(), sizeof(FoldMasses) * C, hipMemcpyHostToDevice, ctx_->stream) != hipSuccess)
            return pg_fail(ctx_, PG_ERR_HIP, "gp_ridge: H2D failed");
        return PG_OK;
    }

    // the pass of trait j (repetition `rep` and alpha index a, as set_masses was last given); scores the pass before it meanwhile
    int launch(const RepSolve &R, const double *bfr, int rep, int a, int j) {
        const int n = in_.n, n_folds = in_.n_folds, k = in_.k, C = in_.C();
        // (the masses' synchronisation has seen the pass that was out: its predictions are on the host)
        const Pending prev = pend_;
        const int turn = prev.R ? (prev.turn ^ 1) : 0;
        std::vector<int32_t> &colof = colof_h_[turn];
        colof.assign(n, -1);
        yh_in_[turn].resize((size_t)n * GP_LMAX);
        for (int f = 0; f < n_folds; ++f)
            if (R.live(f))
                for (int64_t pool : R.va[f]) colof[pool] = f * k + j;
        if (prev.R && hipStreamSynchronize(ctx_->stream) != hipSuccess) // (a no-op after the masses' own; the k > 1 traits of one alpha need it)
            return pg_fail(ctx_, PG_ERR_HIP, "gp_ridge: prediction pass failed");
        busy_ = true;
        if (hipMemcpyAsync(colof_dev_, colof.data(), sizeof(int32_t) * n, hipMemcpyHostToDevice, ctx_->stream) != hipSuccess)
            return pg_fail(ctx_, PG_ERR_HIP, "gp_ridge: H2D failed");
        const int LPr = (P0_.L + 1) & ~1;
        const size_t masses_b = sizeof(double) * n_folds * (2 * GP_LMAX + 1);
        const int chunk = std::max(4, std::min(64, (int)((49152 - masses_b) / (sizeof(double) * n_folds * (LPr + 2)))));
        const int bthreads = n > 128 ? 512 : 256; // the coefficient stage is shared by all waves of a block
        const int groups = n <= 256 ? bthreads / (((n + 63) / 64) * 64) : 1; // locus groups inside a block (n <= 256: 2 .. 4)
        const dim3 grid(W_.S.nblk, groups > 1 ? 1 : (n + bthreads - 1) / bthreads);
        const size_t lds = sizeof(double) * chunk * n_folds * (LPr + 2) + masses_b;
        const Proxy X{in_.proxy, k, j};
        pg_prof_begin(ctx_, PG_K_GP_PREDICT);
        with_path_len(P0_.L, [&](auto lp) {
            constexpr int LP = decltype(lp)::value;
            auto go = [&](auto kern, int g) {
                hipLaunchKernelGGL(kern, grid, dim3(bthreads), lds, ctx_->stream, in_.G, bfr, C, colof_dev_, fm_dev_, P0_, X, in_.p, n, in_.ld,
                                   W_.S.lpb, chunk, W_.part, g);
            };
            if (P0_.L & 1) groups > 1 ? go(k_gp_predict_folds<LP, true, true>, groups) : go(k_gp_predict_folds<LP, false, true>, 1);
            else groups > 1 ? go(k_gp_predict_folds<LP, true, false>, groups) : go(k_gp_predict_folds<LP, false, false>, 1);
        });
        pg_prof_end(ctx_);
        hipLaunchKernelGGL(k_gp_predict_reduce, dim3((n * GP_LMAX + 63) / 64), dim3(512), 0, ctx_->stream, W_.part, W_.S.nblk * groups, n, W_.yhat);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(yh_in_[turn].data(), W_.yhat, sizeof(double) * n * GP_LMAX, hipMemcpyDeviceToHost, ctx_->stream) != hipSuccess)
            return pg_fail(ctx_, PG_ERR_HIP, "gp_ridge: prediction pass failed");
        pend_ = Pending{&R, rep, a, j, turn};
        // ... and while this pass runs, the host scores the one before it
        if (prev.R) score_pass(prev);
        return PG_OK;
    }

    int drain() { // waits for the last pass out and scores it
        if (!pend_.R) return PG_OK;
        if (hipStreamSynchronize(ctx_->stream) != hipSuccess) return pg_fail(ctx_, PG_ERR_HIP, "gp_ridge: prediction pass failed");
        busy_ = false;
        score_pass(pend_);
        pend_.R = nullptr;
        return PG_OK;
    }
};

constexpr int GP_CP = 16; // columns per batched coefficient pass: what the sweep kernel's products mode carries at 500 pools

// All folds of a repetition share two passes over G: one that forms the slopes of every fold's training fit (n_folds * k
// columns), one (per alpha and trait) that predicts every pool with the coefficients of the fold that holds it out.  Every
// fit comes from pinv(X X^T) (solve_scatter): the wide branch of gp/ols.rs:47.  Two ways to the slopes, the same bits:
//   batched   the slopes of ALL repetitions' folds (and of the all-rows fit) are columns G Z of the same matrix: formed GP_CP
//             at a time, whatever repetition they belong to, they take ceil((n_reps C + k) / GP_CP) passes over G instead of
//             n_reps + 1 (config 4: 101 columns, 7 passes instead of 11).  Needs the n_reps C + k columns resident (config 4:
//             4 GB of the 288).  Leaves the all-rows fit in beta_dev (*have_fit).
//   per rep   one pass per repetition: n_reps == 1, columns that do not fit, or POOLGEN_RIDGE_PER_REP=1.
int cv_fused(pg_ctx *ctx, const GpCall &in, const std::vector<double> &xxt, RidgeWork &W, PhaseTimes &T, std::vector<double> &perf,
             double *beta_dev, bool *have_fit) {
    const int64_t p = in.p;
    const int n = in.n, k = in.k, C = in.C(), n_reps = in.n_reps;
    const size_t ncols_all = (size_t)n_reps * C + k;
    bool batched = n_reps > 1 && !pg_switch(PG_SW_RIDGE_PER_REP);
    if (batched) {
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) != hipSuccess || sizeof(double) * (size_t)p * ncols_all > fr / 2) batched = false;
    }
    DevBuf<double> bf;          // the slopes, column-major: C x p, batched (n_reps C + k) x p
    DevBuf<FoldMasses> fm_dev;
    DevBuf<int32_t> colof_dev;
    {
        Phase t{T.alloc};
        int rc = bf.alloc(ctx, sizeof(double) * (size_t)p * (batched ? ncols_all : (size_t)C), "gp_ridge");
        if (!rc) rc = fm_dev.alloc(ctx, sizeof(FoldMasses) * C, "gp_ridge");
        if (!rc) rc = colof_dev.alloc(ctx, sizeof(int32_t) * n, "gp_ridge");
        if (rc) return rc;
    }
    FoldSolver solver(in, xxt.data(), batched);
    PredictPipeline pipe(ctx, in, W, fm_dev.get(), colof_dev.get(), perf);
    // batched: the columns [0, formed) of the global numbering (repetition-major, then the all-rows fit) are in bf; one pass
    // over G per GP_CP more of them
    size_t formed = 0;
    auto form_upto = [&](size_t want) -> int {
        while (formed < want) {
            // the first pass takes repetition 0 alone when that costs no extra pass: it then waits for ONE repetition's host
            // solves (5 ms at config 4) instead of two before the device has anything to do
            const bool short_first = formed == 0 && (size_t)C < (size_t)GP_CP &&
                                     1 + (ncols_all - C + GP_CP - 1) / GP_CP == (ncols_all + GP_CP - 1) / GP_CP;
            const size_t c1 = short_first ? (size_t)C : std::min(formed + (size_t)GP_CP, ncols_all);
            const int nc = (int)(c1 - formed);
            std::vector<double> Zb((size_t)n * nc, 0.0);
            for (size_t c = formed; c < c1; ++c) {
                Phase t{T.solve};
                const int r = (int)(c / C); // (n_reps: the all-rows fit)
                const RepSolve *R = solver.wait(r);
                if (!R) return pg_fail(ctx, PG_ERR_INVALID, "gp_ridge: pinv failed");
                const int stride = (int)R->b0c.size(), cc = (int)(c - (size_t)r * C);
                for (int i = 0; i < n; ++i) Zb[(size_t)i * nc + (c - formed)] = R->Z[(size_t)i * stride + cc];
            }
            Phase t{T.beta};
            if (int rc = pg_gp_beta_cols(ctx, in.G, p, n, in.ld, Zb.data(), nc, bf.get() + formed * (size_t)p, 1)) return rc;
            formed = c1;
        }
        return PG_OK;
    };
    for (int rep = 0; rep < n_reps; ++rep) {
        const RepSolve *R;
        { Phase t{T.solve}; R = solver.wait(rep); }
        if (!R) return pg_fail(ctx, PG_ERR_INVALID, "gp_ridge: pinv failed");
        const double *bfr = batched ? bf.get() + (size_t)rep * C * (size_t)p : bf.get(); // this repetition's C columns
        if (batched) {
            if (int rc = form_upto((size_t)(rep + 1) * C)) return rc;
        } else {
            Phase t{T.beta};
            if (int rc = pg_gp_beta_cols(ctx, in.G, p, n, in.ld, R->Z.data(), C, bf.get(), 1)) return rc; // :526 for every fold at once, column-major
        }
        for (int a = 0; a < in.A(); ++a) {
            { Phase t{T.params}; if (int rc = pipe.set_masses(*R, bfr, in.alpha_at(a))) return rc; }
            Phase t{T.predict};
            for (int j = 0; j < k; ++j)
                if (int rc = pipe.launch(*R, bfr, rep, a, j)) return rc;
        }
    }
    if (int rc = pipe.drain()) return rc;
    if (batched) { // whatever is left of the columns (the all-rows fit at least, unless it rode in a repetition's pass)
        if (int rc = form_upto(ncols_all)) return rc;
        if (hipMemcpyAsync(beta_dev, solver.wait(n_reps)->b0c.data(), sizeof(double) * k, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
            return pg_fail(ctx, PG_ERR_HIP, "gp_ridge: H2D failed");
        hipLaunchKernelGGL(k_gp_cols_to_rows, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, ctx->stream, bf.get() + (size_t)n_reps * C * (size_t)p, p, k, beta_dev + k);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) // (the intercepts are read by the copy)
            return pg_fail(ctx, PG_ERR_HIP, "gp_ridge: the all-rows fit failed");
        *have_fit = true;
    }
    Phase t{T.release}; // (here, not at scope end: the report times them)
    bf.reset(); fm_dev.reset(); colof_dev.reset();
    return PG_OK;
}

// ---- the per-fold cross-validation: per (repetition, fold) the fit of pg_gp_ols_dev, then per (alpha, trait) the masses, the
// contracted coefficients of all lambdas and one prediction pass.  What a tall design takes (n >= p + 1: gp::ols then uses
// pinv(X'X), which pg_gp_ols_dev follows and the fused passes do not), and more fold x trait columns than one pass carries.
int cv_per_fold(pg_ctx *ctx, const GpCall &in, const std::vector<double> &xxt, RidgeWork &W, std::vector<double> &perf, double *beta_dev) {
    const int64_t p = in.p;
    const int n = in.n, k = in.k;
    RepSolve R; // (its pools only)
    std::vector<double> b0(k), yh((size_t)n * GP_LMAX);
    for (int rep = 0; rep < in.n_reps; ++rep) {
        R.split(in, rep);
        for (int fold = 0; fold < in.n_folds; ++fold) {
            if (!R.live(fold)) continue;
            const std::vector<int64_t> &itr = R.tr[fold], &iva = R.va[fold];
            if (int rc = pg_gp_ols_dev(ctx, in.G, p, n, in.ld, in.Y, k, itr.data(), (int)itr.size(), xxt.data(), beta_dev)) return rc; // :526
            if (hipMemcpyAsync(b0.data(), beta_dev, sizeof(double) * k, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
                return pg_fail(ctx, PG_ERR_HIP, "gp_ridge: D2H failed");
            for (int a = 0; a < in.A(); ++a)
                for (int j = 0; j < k; ++j) {
                    PathParams P;
                    const Proxy X{in.proxy, k, j};
                    if (int rc = ridge_path_params(ctx, beta_dev, p, k, j, in.alpha_at(a), in.path, W, P, 1, X)) return rc;
                    hipLaunchKernelGGL(k_gp_blambda, dim3((unsigned)((p + 255) / 256)), dim3(256), 0, ctx->stream, beta_dev, p, k, j, P, X, W.B);
                    hipLaunchKernelGGL(k_gp_predict, dim3(W.S.nblk, (n + 255) / 256), dim3(256), 0, ctx->stream, in.G, W.B, p, n, in.ld, W.S.lpb, W.part);
                    hipLaunchKernelGGL(k_gp_predict_reduce, dim3((n * GP_LMAX + 63) / 64), dim3(512), 0, ctx->stream, W.part, W.S.nblk, n, W.yhat);
                    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(yh.data(), W.yhat, sizeof(double) * n * GP_LMAX, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
                        hipStreamSynchronize(ctx->stream) != hipSuccess)
                        return pg_fail(ctx, PG_ERR_HIP, "gp_ridge: prediction pass failed");
                    score(in, perf, yh, rep, fold, a, j, b0[j], iva);
                }
        }
    }
    return PG_OK;
}

// Per trait the mode over repetitions of the per-repetition arg-min over the (alpha, lambda) grid (:573-627): alpha and
// lambda are counted separately, each against the path values.  Then expand_and_contract of the all-rows fit in beta_dev
// at the chosen pair (:653-662).
int select_and_apply(pg_ctx *ctx, const GpCall &in, const std::vector<double> &perf, RidgeWork &W, double *beta_dev, double *alphas_out,
                     double *lambdas_out) {
    const int L = in.L(), A = in.A(), k = in.k;
    for (int j = 0; j < k; ++j) {
        std::vector<int> acount(L, 0), lcount(L, 0);
        for (int rep = 0; rep < in.n_reps; ++rep) {
            std::vector<double> mean((size_t)A * L);
            for (int a = 0; a < A; ++a)
                for (int li = 0; li < L; ++li) {
                    double sum = 0.0;
                    for (int fold = 0; fold < in.n_folds; ++fold) sum += perf[in.perf_at(rep, fold, a, li, j)];
                    mean[(size_t)a * L + li] = sum / (double)in.n_folds;
                }
            double mnv = mean[0];
            for (double x : mean) if (x < mnv) mnv = x;
            for (size_t q = 0; q < mean.size(); ++q)
                if (mean[q] == mnv) {
                    const double aval = in.alpha_at((int)(q / L)), lval = in.path[q % L];
                    for (int c = 0; c < L; ++c) { acount[c] += (aval == in.path[c]); lcount[c] += (lval == in.path[c]); }
                    break;
                }
        }
        const int abest = (int)(std::max_element(acount.begin(), acount.end()) - acount.begin()); // (the first of equal counts)
        const int lbest = (int)(std::max_element(lcount.begin(), lcount.end()) - lcount.begin());
        // a single alpha off the path grid counts nowhere in the reference (:605-608), which then reports and applies
        // path[0]; such an alpha never reaches it from its own callers (0, 1, grid), here it is kept as given
        const double afinal = in.alpha >= 0.0 ? in.alpha : in.path[abest];
        if (alphas_out) alphas_out[j] = afinal;
        lambdas_out[j] = in.path[lbest];
        PathParams P;
        const Proxy X{in.proxy, k, j};
        if (int rc = ridge_path_params(ctx, beta_dev, in.p, k, j, afinal, in.path, W, P, 1, X)) return rc;
        hipLaunchKernelGGL(k_gp_apply, dim3((unsigned)((in.p + 255) / 256)), dim3(256), 0, ctx->stream, beta_dev, in.p, k, j, P, X, lbest);
        if (hipGetLastError() != hipSuccess) return pg_fail(ctx, PG_ERR_HIP, "gp_ridge: apply failed");
    }
    return PG_OK;
}

// The lambda path with k-fold cross-validation (:461-669) behind penalise_lasso_like / _ridge_like (alpha = 1 / 0, one
// path), penalise_glmnet (alpha < 0: the 2-D grid alpha x lambda over the same path values, :479-498) and the
// *_with_iterative_proxy_norms models (in.proxy != nullptr, :540-553, :655-657).
int penalised_path(pg_ctx *ctx, GpCall in, double lambda_step, double *beta_dev, double *alphas_out, double *lambdas_out,
                   double *perf_out, const double *xxt_host_or_null) {
    const int maxu = (int)std::llround(1.0 / lambda_step);
    PG_CHECK(ctx, maxu + 1 <= GP_LMAX, "gp_ridge: at most %d lambdas on the path", GP_LMAX);
    in.path.resize(maxu + 1);
    for (int i = 0; i <= maxu; ++i) in.path[i] = (double)i / (double)maxu; // :470-476
    PG_HIP(ctx, hipSetDevice(ctx->device));
    PhaseTimes T;
    // the full-data X X^T once; every training subset uses a principal sub-block
    std::vector<double> xxt;
    if (int rc = pg_gp_xxt_host(ctx, in.G, in.p, in.n, in.ld, xxt_host_or_null, "gp_ridge", xxt)) return rc;
    RidgeWork W;
    if (int rc = W.alloc(ctx, in)) return rc;
    for (int i = 0; i < in.n_reps * in.n_rows; ++i)
        if (in.fold_of[i] < 0 || in.fold_of[i] > in.n_folds /* == n_folds: the left-over group of k_split (:444-448), never validated */)
            return pg_fail(ctx, PG_ERR_INVALID, "gp_ridge: fold id out of range");
    std::vector<double> perf((size_t)in.n_reps * in.n_folds * in.A() * in.L() * in.k, NAN);
    const bool fused = in.C() <= PG_MAX_SWEEP_COLS && (int64_t)in.n < in.p + 1 && !pg_switch(PG_SW_RIDGE_PER_FOLD);
    T.before = PhaseTimes::since(T.entry); // X X^T, its copy to the host, the work buffers
    bool have_fit = false; // the all-rows fit is in beta_dev
    if (int rc = fused ? cv_fused(ctx, in, xxt, W, T, perf, beta_dev, &have_fit) : cv_per_fold(ctx, in, xxt, W, perf, beta_dev)) return rc;
    T.report_phases();
    if (!have_fit)
        if (int rc = pg_gp_ols_dev(ctx, in.G, in.p, in.n, in.ld, in.Y, in.k, in.rows, in.n_rows, xxt.data(), beta_dev)) return rc;
    if (int rc = select_and_apply(ctx, in, perf, W, beta_dev, alphas_out, lambdas_out)) return rc;
    if (perf_out) std::memcpy(perf_out, perf.data(), sizeof(double) * perf.size());
    (void)hipStreamSynchronize(ctx->stream);
    W.raw.reset(); // (inside the whole-call time)
    T.report_call();
    return PG_OK;
}

} // namespace

// (pg_common.h) the caller's copy when there is one, else the kinship pass into the context's n x n buffer and a copy from there
int pg_gp_xxt_host(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *given_or_null, const char *who,
                   std::vector<double> &xxt) {
    xxt.resize((size_t)n * n);
    if (given_or_null) {
        std::memcpy(xxt.data(), given_or_null, sizeof(double) * (size_t)n * n);
        return PG_OK;
    }
    int rc = ctx->S_dev.reserve(ctx, sizeof(double) * n * n, who);
    if (!rc) rc = pg_gp_xxt_dev(ctx, G_dev, p, n, ld, ctx->S_dev);
    if (rc) return rc;
    PG_HIP(ctx, hipMemcpyAsync(xxt.data(), ctx->S_dev, sizeof(double) * n * n, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

extern "C" int pg_gp_ols_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y,
                             int k, const int64_t *row_idx, int n_rows, const double *XXt_host_or_null,
                             double *beta_dev) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, G_dev && Y && row_idx && beta_dev && p > 0 && n >= 1 && k >= 1 && n_rows >= 1 && n_rows <= n,
             "gp_ols: bad arguments");
    PG_CHECK(ctx, ld >= n && (ld % 2) == 0, "gp_ols: ld must be even and >= n");
    if (k > 8) return pg_fail(ctx, PG_ERR_UNSUPPORTED, "gp_ols: at most 8 traits per call");
    for (int a = 0; a < n_rows; ++a) PG_CHECK(ctx, row_idx[a] >= 0 && row_idx[a] < n, "gp_ols: row index out of range");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    if ((int64_t)n >= p + 1) {
        // The tall branch (gp/ols.rs:72-99, taken when x.nrows() >= x.ncols(): at most n - 1 loci, i.e. the reference's own 5 x 3
        // test, never a pool-seq matrix): b = pinv(X'X over the training rows) X' y.  (1 + p)^2 <= n^2 numbers: the host's,
        // not a GPU problem.  pinv as in the wide branch (helpers.rs:463-482).
        const int P = (int)p + 1;
        std::vector<double> Gh((size_t)p * ld);
        PG_HIP(ctx, hipMemcpyAsync(Gh.data(), G_dev, sizeof(double) * (size_t)p * ld, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
        auto X = [&](int64_t i, int c) { return c == 0 ? 1.0 : Gh[(size_t)(c - 1) * ld + i]; };
        std::vector<double> xtx((size_t)P * P), pinv((size_t)P * P), T((size_t)P * n_rows), b((size_t)P * k);
        for (int a = 0; a < P; ++a)
            for (int c = 0; c < P; ++c) {
                double x = 0.0;
                for (int i = 0; i < n_rows; ++i) x += X(row_idx[i], a) * X(row_idx[i], c);
                xtx[(size_t)a * P + c] = x;
            }
        if (pg_pinv_sym(xtx.data(), P, pinv.data()) != 0) return pg_fail(ctx, PG_ERR_INVALID, "gp_ols: pinv failed");
        for (int a = 0; a < P; ++a) // (pinv X') y, in the reference's order of products
            for (int i = 0; i < n_rows; ++i) {
                double x = 0.0;
                for (int c = 0; c < P; ++c) x += pinv[(size_t)a * P + c] * X(row_idx[i], c);
                T[(size_t)a * n_rows + i] = x;
            }
        for (int a = 0; a < P; ++a)
            for (int j = 0; j < k; ++j) {
                double x = 0.0;
                for (int i = 0; i < n_rows; ++i) x += T[(size_t)a * n_rows + i] * Y[(size_t)row_idx[i] * k + j];
                b[(size_t)a * k + j] = x;
            }
        PG_HIP(ctx, hipMemcpyAsync(beta_dev, b.data(), sizeof(double) * (size_t)P * k, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // b is stack-owned
        return PG_OK;
    }
    // the wide branch (gp/ols.rs:47-72): b = X^T pinv(X X^T) y.  Every training subset's X X^T is a principal sub-block of the full-data one
    std::vector<double> xxt;
    if (int rc = pg_gp_xxt_host(ctx, G_dev, p, n, ld, XXt_host_or_null, "gp_ols", xxt)) return rc;
    std::vector<double> Z((size_t)n * k, 0.0), b0(k, 0.0);
    if (solve_scatter(xxt.data(), n, Y, k, row_idx, n_rows, Z.data(), k, 0, b0.data()) != 0) return pg_fail(ctx, PG_ERR_INVALID, "gp_ols: pinv failed");
    PG_HIP(ctx, hipMemcpyAsync(beta_dev, b0.data(), sizeof(double) * k, hipMemcpyHostToDevice, ctx->stream));
    return pg_gp_beta_cols(ctx, G_dev, p, n, ld, Z.data(), k, beta_dev + k); // rows 1..p: one streaming pass over G; synchronises (b0 is stack-owned)
}

extern "C" int pg_gp_ridge_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y,
                               int k, const int64_t *row_idx, int n_rows, const int32_t *fold_of, int n_reps,
                               int n_folds, double alpha, double lambda_step, double *beta_dev,
                               double *lambdas_out, double *perf_out) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, G_dev && Y && row_idx && fold_of && beta_dev && lambdas_out, "gp_ridge: null pointer");
    PG_CHECK(ctx, p > 0 && n >= 3 && k >= 1 && k <= 8 && n_rows >= 3 && n_rows <= n && n_reps >= 1 && n_folds >= 2,
             "gp_ridge: bad shape");
    PG_CHECK(ctx, alpha >= 0.0 && alpha <= 1.0 && lambda_step > 0.0 && lambda_step <= 1.0, "gp_ridge: bad alpha / lambda step");
    return penalised_path(ctx, GpCall{G_dev, p, n, ld, Y, k, row_idx, n_rows, fold_of, n_reps, n_folds, alpha, nullptr, {}}, lambda_step,
                          beta_dev, nullptr, lambdas_out, perf_out, nullptr);
}

extern "C" int pg_gp_penalised_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y,
                                   int k, const int64_t *row_idx, int n_rows, const int32_t *fold_of, int n_reps,
                                   int n_folds, double alpha, int iterative_proxy, double lambda_step, double *beta_dev,
                                   double *alphas_out, double *lambdas_out, double *perf_out, const double *XXt_host_or_null) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, G_dev && Y && row_idx && fold_of && beta_dev && lambdas_out, "gp_penalised: null pointer");
    PG_CHECK(ctx, p > 0 && n >= 3 && k >= 1 && k <= 8 && n_rows >= 3 && n_rows <= n && n_reps >= 1 && n_folds >= 2,
             "gp_penalised: bad shape");
    PG_CHECK(ctx, alpha <= 1.0 && lambda_step > 0.0 && lambda_step <= 1.0, "gp_penalised: bad alpha / lambda step");
    DevBuf<double> proxy;
    if (iterative_proxy) { // the same proxy serves every fold and the final fit (:543, :656: always on `row_idx`)
        PG_HIP(ctx, hipSetDevice(ctx->device));
        int rc = proxy.alloc(ctx, sizeof(double) * (size_t)(p + 1) * k, "gp_penalised");
        if (!rc) rc = pg_gp_proxy_dev(ctx, G_dev, p, n, ld, Y, k, row_idx, n_rows, XXt_host_or_null, proxy.get());
        if (rc) return rc;
    }
    return penalised_path(ctx, GpCall{G_dev, p, n, ld, Y, k, row_idx, n_rows, fold_of, n_reps, n_folds, alpha, proxy.get(), {}}, lambda_step,
                          beta_dev, alphas_out, lambdas_out, perf_out, XXt_host_or_null);
}

// yhat = X beta for every pool (the multiply_views_xx of gp/cv.rs:160-168, all rows at once)
extern "C" int pg_gp_predict_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *beta_dev,
                                 int k, double *yhat) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, G_dev && beta_dev && yhat && p > 0 && n >= 1 && k >= 1 && k <= 8, "gp_predict: bad arguments");
    PG_CHECK(ctx, ld >= n, "gp_predict: ld must be >= n");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const Slabs S = predict_slabs(ctx, p);
    const size_t need = sizeof(double) * ((size_t)S.nblk * n * 8 + (size_t)n * 8);
    int rc = pg_ws_reserve(ctx, need);
    if (rc) return rc;
    double *part = static_cast<double *>(ctx->ws.get());
    double *out = part + (size_t)S.nblk * n * 8;
    hipLaunchKernelGGL(k_gp_predict_beta, dim3(S.nblk, (n + 255) / 256), dim3(256), 0, ctx->stream, G_dev, beta_dev, k, p, n, ld, S.lpb, part);
    hipLaunchKernelGGL(k_gp_predict_beta_reduce, dim3((n * 8 + 255) / 256), dim3(256), 0, ctx->stream, part, S.nblk, n, out);
    PG_HIP(ctx, hipGetLastError());
    std::vector<double> h((size_t)n * 8), b0(k);
    PG_HIP(ctx, hipMemcpyAsync(h.data(), out, sizeof(double) * n * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(b0.data(), beta_dev, sizeof(double) * k, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < k; ++j) yhat[(size_t)i * k + j] = b0[j] + h[(size_t)i * 8 + j];
    return PG_OK;
}
