// pg_gwalpha.hip -- gwalpha == gwas::gwalpha_ls / gwalpha_ml (gwas/gwalpha.rs:281-380): per locus the loader's filter with the
// alleles ordered by decreasing frequency, the first one dropped (:176-196), and per kept allele (= row) a Nelder-Mead fit of two
// Beta distributions to the cumulative allele distribution over the phenotype-ranked pools (:227-279).
//
// One fit is up to 1000 simplex steps of one to six cost evaluations, each of ~2 n regularised incomplete Beta functions = continued
// fractions of fp64 divisions: the operator is bound by arithmetic, not by the 24 n bytes of counts a locus brings.
//
// Mapping: A SUB-GROUP OF 8 LANES PER FIT.  The lanes stride over the evaluation points of one cost; the six ln_gamma values behind
// the two prefactors are formed once per cost, one per lane; the simplex is held redundantly by every lane of the sub-group, and
// every lane closes the cost for itself from the terms in LDS, in the reference's order of summation: the SAME bits in every lane,
// so the lanes of a sub-group take every Nelder-Mead branch together.  The sub-groups of a wave walk one state machine whose every
// turn holds ONE cost evaluation, whatever step each fit is in (start vertex, reflection, expansion, contraction, shrink): fits do
// not wait for each other's branches, and a sub-group whose fit has ended takes the next row from a device-wide cursor while its
// neighbours go on.  A row's arithmetic depends on the row alone -- points are assigned to lanes by their index, the sums run in
// pool order -- so its result does not depend on where the row sits in the batch or in the launch.
//
// The solver is the one of pg_mle.hip and of the oracle (argmin 0.8's Nelder-Mead: alpha 1, gamma 2, rho 0.5, sigma 0.5, stable
// sort, stop when the sample standard deviation of the five costs is below f64::EPSILON or after 1000 iterations) from
// prepare_solver_neldermead(4, 1) (helpers.rs:132-146).
#include "pg_common.h"
#include "pg_stats_device.h"
#include <cmath>
#include <vector>

namespace {

constexpr int GW_D = 4, GW_V = 5;   // shapes of the two distributions; vertices
constexpr int GW_MAXIT = 1000;      // .configure(|state| state.max_iters(1_000)), gwalpha.rs:120
constexpr int GW_LDS_MAX = 160 * 1024;

typedef unsigned int gw_uint2 __attribute__((ext_vector_type(2)));

struct GwParams {
    int64_t L;
    int n;
    double sig, mn, mx;
};

enum { PH_FETCH = 0, PH_INIT, PH_REFLECT, PH_EXPAND, PH_CONTRACT, PH_SHRINK, PH_DONE };

// bound_parameters_with_logit(x, EPSILON, 10) (helpers.rs:120-130, gwalpha.rs:8-9)
__device__ __forceinline__ double gw_bound(double x) { return PG_EPS + ((10.00 - PG_EPS) / (1.00 + exp(-x))); }

__device__ __forceinline__ void gw_wave_sync() { // LDS written by some lanes of this wave, read by others
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The two heavy pieces of a cost are CALLED, not inlined: inlined into the state machine their constants and the continued fraction's
// state were kept live around the whole solver loop (256 VGPRs, or ~180 spilled at 128).
__device__ __noinline__ double gw_ln_gamma(double x) { return pg_ln_gamma(x); }
// Beta(a, b).cdf(x) with the prefactor's ln B(a, b) given (statrs Beta::cdf: 0 below the support, 1 from x = 1 on)
__device__ __noinline__ double gw_cdf(double a, double b, double x, double ln_beta) {
    if (x <= 0.0) return 0.0;
    if (x >= 1.0) return 1.0;
    return pg_beta_reg_ln(a, b, x, ln_beta);
}

// ndarray 0.15 `sum()` of a contiguous slice (numeric_util::unrolled_fold): eight partial sums, then the rest in order
__device__ __forceinline__ double gw_nd_sum(const double *x, int len) {
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int i = 0;
    while (len - i >= 8) {
#pragma unroll
        for (int j = 0; j < 8; ++j) p[j] = p[j] + x[i + j];
        i += 8;
    }
    double acc = 0.0;
    acc = acc + (p[0] + p[4]);
    acc = acc + (p[1] + p[5]);
    acc = acc + (p[2] + p[6]);
    acc = acc + (p[3] + p[7]);
    for (; i < len; ++i) acc = acc + x[i];
    return acc;
}

// rows of the batch: n_out and the allele of every row from the header word, and the list of (locus, row) the fit kernel walks
__global__ __launch_bounds__(256) void k_gw_rows(const int32_t *__restrict__ flags, int64_t L, int32_t *__restrict__ n_out,
                                                 int32_t *__restrict__ ids, int64_t *__restrict__ rows,
                                                 unsigned long long *__restrict__ count) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int hdr = flags[l];
    const int nk = (hdr >> PG_HDR_NK_SHIFT) & 7;
    // the filter keeps no locus with fewer than two alleles (sync.rs:284), so "keep the only allele" (gwalpha.rs:193) never applies
    const bool alive = (hdr & PG_HDR_ALIVE) != 0 && nk >= 2;
    const int nr = alive ? (nk - 1 < PG_MAX_OUT ? nk - 1 : PG_MAX_OUT) : 0;
    n_out[l] = nr;
    if (nr == 0) return;
    const int ord = hdr >> PG_HDR_ORD_SHIFT;
    const unsigned long long at = atomicAdd(count, (unsigned long long)nr);
    for (int r = 0; r < nr; ++r) {
        ids[(size_t)r * (size_t)L + (size_t)l] = (ord >> (3 * (r + 1))) & 7; // rank 0, the most frequent allele, is dropped
        rows[at + r] = l * 8 + r;
    }
}

// LDS of a sub-group: [pts: 2n][fv: 2n][tm: 2n][hd: 4].
//   ML  pts = percs_a[0 .. n-2], percs_b[0 .. n-2], percs_a[n-1], percs_b[n-1] (the last percentile of a distribution is 1 to a few
//       ulp: it takes the short way through the cdf and sits behind the interior points), fv = the cdf values of one cost
//   LS  pts = percs_a[1 .. n-1], percs_b[1 .. n-1]; the point of pool 0 is q' = 0, cdf 0: its two squares are constants (hd)
//   tm  = the terms of one cost (LS: squared residuals, ML: log10 of the cdf differences), summed in the reference's order
//   hd  = p_a, the LS term of pool 0 of distribution A, the mean frequency, the LS term of pool 0 of B
template <int SG, bool ML>
__global__ __launch_bounds__(64, 4) void k_gw_fit(const uint32_t *__restrict__ counts, const int32_t *__restrict__ flags,
                                               const int64_t *__restrict__ rows, const unsigned long long *__restrict__ count,
                                               unsigned long long *cursor, const double *__restrict__ bins,
                                               const double *__restrict__ qp, const GwParams P, double *__restrict__ mean_freq,
                                               double *__restrict__ alpha, double *__restrict__ shapes, double *__restrict__ cost_out,
                                               int32_t *__restrict__ iters) {
    extern __shared__ double gw_lds[];
    const int lane = threadIdx.x, sg = lane / SG, sl = lane % SG;
    const int n = P.n;
    double *const pts = gw_lds + (size_t)sg * (size_t)(6 * n + 4);
    double *const fv = pts + 2 * n;
    double *const tm = fv + 2 * n;
    double *const hd = tm + 2 * n;
    const long long nrows = (long long)*count;
    const int npts = ML ? 2 * n : 2 * (n - 1);

    int phase = PH_FETCH, it = 0, k = 0, r = 0;
    int64_t l = 0;
    double sx[GW_V][GW_D], cost[GW_V], xt[GW_D] = {1.0, 1.0, 1.0, 1.0};
    double cr = 0.0, p_a = 0.5, c0a = 0.0, c0b = 0.0;
#pragma unroll
    for (int i = 0; i < GW_V; ++i) {
        cost[i] = 0.0;
#pragma unroll
        for (int d = 0; d < GW_D; ++d) sx[i][d] = 1.0;
    }

    auto vertex = [&](int kk, double (&o)[GW_D]) { // sx[kk] without indexing the register file at run time
#pragma unroll
        for (int d = 0; d < GW_D; ++d) {
            double v = sx[0][d];
#pragma unroll
            for (int i = 1; i < GW_V; ++i) v = (kk == i) ? sx[i][d] : v;
            o[d] = v;
        }
    };
    // centroid of all vertices but the worst, and the worst one's reflection: formed again where a step needs them (the same bits
    // every time, the simplex does not move in between) rather than kept in registers across the costs
    auto centroid = [&](double (&x0)[GW_D], double (&xr)[GW_D]) {
#pragma unroll
        for (int d = 0; d < GW_D; ++d) {
            double c = sx[0][d];
#pragma unroll
            for (int i = 1; i < GW_V - 1; ++i) c += sx[i][d];
            x0[d] = c * (1.0 / ((double)GW_V - 1.0));
            xr[d] = x0[d] + (x0[d] - sx[GW_V - 1][d]);
        }
    };
    auto sort = [&]() { // stable insertion sort by cost, fully unrolled (vertices move with their costs)
#pragma unroll
        for (int a = 1; a < GW_V; ++a) {
#pragma unroll
            for (int b = a; b >= 1; --b) {
                const bool sw = cost[b - 1] > cost[b];
                const double c0s = cost[b - 1], c1s = cost[b];
                cost[b - 1] = sw ? c1s : c0s;
                cost[b] = sw ? c0s : c1s;
#pragma unroll
                for (int d = 0; d < GW_D; ++d) {
                    const double v0 = sx[b - 1][d], v1 = sx[b][d];
                    sx[b - 1][d] = sw ? v1 : v0;
                    sx[b][d] = sw ? v0 : v1;
                }
            }
        }
    };
    // the fit has ended: shapes, alpha (gwalpha.rs:314-316), and the sub-group is free for the next row
    auto finish = [&]() {
        double s[GW_D];
#pragma unroll
        for (int d = 0; d < GW_D; ++d) s[d] = gw_bound(sx[0][d]);
        const double a_mu = P.mn + (P.mx - P.mn) * (s[0] / (s[0] + s[1]));
        const double b_mu = P.mn + (P.mx - P.mn) * (s[2] / (s[2] + s[3]));
        const double al = (2.00 * sqrt(p_a * (1.0 - p_a))) * (a_mu - b_mu) / P.sig;
        if (sl == 0) {
            const size_t o = (size_t)r * (size_t)P.L + (size_t)l;
            alpha[o] = al;
            if (shapes) {
#pragma unroll
                for (int d = 0; d < GW_D; ++d) shapes[o * 4 + d] = s[d];
            }
            if (cost_out) cost_out[o] = cost[0];
            if (iters) iters[o] = it;
        }
        phase = PH_FETCH;
    };
    // the head of the solver's loop: stop (sd of the costs below EPSILON, or the cap), or reflect the worst vertex
    auto check = [&]() {
        double mean = 0.0, sd = 0.0;
#pragma unroll
        for (int i = 0; i < GW_V; ++i) mean += cost[i];
        mean /= (double)GW_V;
#pragma unroll
        for (int i = 0; i < GW_V; ++i) sd += (cost[i] - mean) * (cost[i] - mean);
        sd = sqrt(sd / ((double)GW_V - 1.0));
        if (it >= GW_MAXIT || sd < PG_EPS) { finish(); return; }
        double x0[GW_D];
        centroid(x0, xt);
        phase = PH_REFLECT;
    };
    auto stepped = [&]() { sort(); ++it; check(); };

    // the cost of `par` for the row this sub-group holds; every lane of the wave comes here together
    auto cost_of = [&](const double (&par)[GW_D], bool active) -> double {
        double s[GW_D];
#pragma unroll
        for (int d = 0; d < GW_D; ++d) s[d] = gw_bound(par[d]);
        // the six ln_gamma of the two prefactors, one per lane
        double lg = 0.0;
        if (sl < 6) {
            const double arg = sl == 0 ? s[0] + s[1] : sl == 1 ? s[0] : sl == 2 ? s[1] : sl == 3 ? s[2] + s[3] : sl == 4 ? s[2] : s[3];
            lg = gw_ln_gamma(arg);
        }
        const double lb_a = __shfl(lg, 0, SG) - __shfl(lg, 1, SG) - __shfl(lg, 2, SG);
        const double lb_b = __shfl(lg, 3, SG) - __shfl(lg, 4, SG) - __shfl(lg, 5, SG);
        // the cdf of every point: maximum_likelihood_beta at the percentiles (gwalpha.rs:58-60), least_squares_beta at q' (:34-37)
        for (int t = sl; t < npts; t += SG) {
            if (active) {
                const bool is_b = ML ? ((t >= n - 1 && t < 2 * (n - 1)) || t == 2 * n - 1) : t >= n - 1;
                const double x = ML ? pts[t] : qp[1 + t - (is_b ? n - 1 : 0)];
                const double F = gw_cdf(is_b ? s[2] : s[0], is_b ? s[3] : s[1], x, is_b ? lb_b : lb_a);
                if (ML) fv[t] = F;
                else {
                    const double e = pts[t] - F;
                    tm[t] = e * e;
                }
            }
        }
        gw_wave_sync();
        if (ML) { // the terms log10(max(cdf(percs[i]) - cdf(percs0[i]), EPSILON)), at dist * n + i (:61-70)
            for (int t = sl; t < npts; t += SG) {
                if (active) {
                    int dist, i;
                    if (t < 2 * (n - 1)) { dist = t >= n - 1 ? 1 : 0; i = t - dist * (n - 1); }
                    else { dist = t - 2 * (n - 1); i = n - 1; }
                    const double F0 = i == 0 ? 0.0 : fv[dist * (n - 1) + i - 1]; // percs0[i] = percs[i - 1], cdf(0) = 0
                    double df = fv[t] - F0;
                    df = df < PG_EPS ? PG_EPS : df;
                    tm[dist * n + i] = log10(df);
                }
            }
            gw_wave_sync();
        }
        // The sums in the reference's order -- pool after pool, the two distributions apart, then joined -- by every lane of the
        // sub-group for itself: the same bits in all of them, and the same order wherever the row sits.
        double sa = 0.0, sb = 0.0;
        if (active) {
            if (ML) {
                for (int i = 0; i < n; ++i) { sa = sa + tm[i]; sb = sb + tm[n + i]; }
            } else {
                sa = c0a; sb = c0b; // pool 0: q' = 0, cdf 0
                for (int i = 0; i < n - 1; ++i) { sa = sa + tm[i]; sb = sb + tm[n - 1 + i]; }
            }
        }
        gw_wave_sync(); // the next cost rewrites fv and tm
        return ML ? -sa - sb : sa + sb;
    };

    for (;;) {
        // ---- sub-groups without a row take the next one and lay its points out ------------------------------------------------
        const bool want = phase == PH_FETCH;
        long long idx = -1;
        if (want && sl == 0) idx = (long long)atomicAdd(cursor, 1ull);
        idx = __shfl(idx, 0, SG);
        if (want) {
            if (idx >= nrows) phase = PH_DONE;
            else {
                const int64_t code = rows[idx];
                l = code >> 3;
                r = (int)(code & 7);
                if (sl == 0) {
                    const int hdr = flags[l];
                    const int al = ((hdr >> PG_HDR_ORD_SHIFT) >> (3 * (r + 1))) & 7;
                    const uint32_t *row = counts + (size_t)l * (size_t)n * 6;
                    double pa = 0.0, fsum = 0.0;
                    for (int i = 0; i < n; ++i) { // to_frequencies over the surviving alleles (sync.rs:166-192), as the loader does
                        const gw_uint2 *cp = reinterpret_cast<const gw_uint2 *>(row + (size_t)i * 6);
                        const gw_uint2 a = cp[0], b = cp[1], d = cp[2];
                        const uint32_t c[6] = {a.x, a.y, b.x, b.y, d.x, d.y};
                        double rs = 0.0;
                        uint32_t cv = c[0];
#pragma unroll
                        for (int j = 0; j < 6; ++j) {
                            rs = (hdr & (2 << j)) ? rs + (double)c[j] : rs;
                            cv = (al == j) ? c[j] : cv;
                        }
                        const double f = (rs == 0.0) ? NAN : (double)cv / rs;
                        const double bi = bins[i];
                        fv[i] = f;
                        pa = pa + f * bi; // freqs_a.t().dot(bins) on a strided column: the plain loop (gwalpha.rs:245)
                        fsum = fsum + f;
                    }
                    for (int i = 0; i < n; ++i) { // bins_a, bins_b (:256-259)
                        const double f = fv[i], bi = bins[i];
                        pts[i] = f * bi / pa;
                        pts[n + i] = (1.0 - f) * bi / (1.0 - pa);
                    }
                    for (int i = 0; i < n; ++i) { // percs (:263-268)
                        fv[i] = i == 0 ? pts[0] : gw_nd_sum(pts, i + 1);
                        fv[n + i] = i == 0 ? pts[n] : gw_nd_sum(pts + n, i + 1);
                    }
                    if (ML) {
                        for (int i = 0; i < n - 1; ++i) { pts[i] = fv[i]; pts[n - 1 + i] = fv[n + i]; }
                        pts[2 * (n - 1)] = fv[n - 1];
                        pts[2 * n - 1] = fv[2 * n - 1];
                        hd[1] = 0.0; hd[3] = 0.0;
                    } else {
                        for (int i = 1; i < n; ++i) { pts[i - 1] = fv[i]; pts[n - 1 + i - 1] = fv[n + i]; }
                        hd[1] = fv[0] * fv[0]; hd[3] = fv[n] * fv[n];
                    }
                    hd[0] = pa;
                    hd[2] = fsum / (double)n;
                }
            }
        }
        gw_wave_sync();
        if (want && phase != PH_DONE) {
            p_a = hd[0];
            c0a = hd[1];
            c0b = hd[3];
            const size_t o = (size_t)r * (size_t)P.L + (size_t)l;
            if (sl == 0) mean_freq[o] = hd[2];
            if (!(p_a > 0.0 && p_a < 1.0)) { // no defined cost in the reference: NaN, and on to the next row
                if (sl == 0) {
                    alpha[o] = NAN;
                    if (shapes) { shapes[o * 4] = NAN; shapes[o * 4 + 1] = NAN; shapes[o * 4 + 2] = NAN; shapes[o * 4 + 3] = NAN; }
                    if (cost_out) cost_out[o] = NAN;
                    if (iters) iters[o] = 0;
                }
            } else { // prepare_solver_neldermead(4, 1): ones, 1.5 on the diagonal
#pragma unroll
                for (int i = 0; i < GW_V; ++i)
#pragma unroll
                    for (int d = 0; d < GW_D; ++d) sx[i][d] = (i == d) ? 1.5 : 1.0;
                k = 0;
                it = 0;
                vertex(0, xt);
                phase = PH_INIT;
            }
        }
        if (__all(phase == PH_DONE)) break;
        // ---- one cost per turn, whatever the step ---------------------------------------------------------------------------
        const bool active = phase != PH_DONE && phase != PH_FETCH;
        const double c = cost_of(xt, active);
        switch (phase) {
        case PH_INIT:
        case PH_SHRINK:
#pragma unroll
            for (int i = 0; i < GW_V; ++i) cost[i] = (k == i) ? c : cost[i];
            ++k;
            if (k < GW_V) vertex(k, xt);
            else if (phase == PH_INIT) { sort(); check(); }
            else stepped();
            break;
        case PH_REFLECT:
            cr = c;
            if (cr < cost[GW_V - 2] && cr >= cost[0]) { // reflection (xt is the reflected point)
#pragma unroll
                for (int d = 0; d < GW_D; ++d) sx[GW_V - 1][d] = xt[d];
                cost[GW_V - 1] = cr;
                stepped();
            } else if (cr < cost[0]) { // try the expansion
                double x0[GW_D], xr[GW_D];
                centroid(x0, xr);
#pragma unroll
                for (int d = 0; d < GW_D; ++d) xt[d] = x0[d] + (xr[d] - x0[d]) * 2.0;
                phase = PH_EXPAND;
            } else { // try the contraction
                double x0[GW_D], xr[GW_D];
                centroid(x0, xr);
#pragma unroll
                for (int d = 0; d < GW_D; ++d) xt[d] = x0[d] + (sx[GW_V - 1][d] - x0[d]) * 0.5;
                phase = PH_CONTRACT;
            }
            break;
        case PH_EXPAND: {
            const bool e = c < cr;
            double x0[GW_D], xr[GW_D];
            centroid(x0, xr);
#pragma unroll
            for (int d = 0; d < GW_D; ++d) sx[GW_V - 1][d] = e ? xt[d] : xr[d];
            cost[GW_V - 1] = e ? c : cr;
            stepped();
        } break;
        case PH_CONTRACT:
            if (c < cost[GW_V - 1]) {
#pragma unroll
                for (int d = 0; d < GW_D; ++d) sx[GW_V - 1][d] = xt[d];
                cost[GW_V - 1] = c;
                stepped();
            } else { // shrink towards the best vertex: four more costs
#pragma unroll
                for (int i = 1; i < GW_V; ++i)
#pragma unroll
                    for (int d = 0; d < GW_D; ++d) sx[i][d] = sx[0][d] + (sx[i][d] - sx[0][d]) * 0.5;
                k = 1;
                vertex(1, xt);
                phase = PH_SHRINK;
            }
            break;
        default: break;
        }
    }
}

__global__ __launch_bounds__(256) void k_beta_reg(const double *__restrict__ a, const double *__restrict__ b,
                                                  const double *__restrict__ x, int64_t count, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < count) out[i] = pg_beta_reg(a[i], b[i], x[i]);
}

inline size_t gw_up16(size_t x) { return (x + 15) & ~(size_t)15; }

// Lanes per fit.  Measured at 1 M loci (tools/bench_gwalpha.py, profiles/gwalpha_ops.jsonl): 8 lanes beat 16 at 5 pools (LS 685 vs
// 1129 ms, ML 1808 vs 2679 ms) and at 10 pools (919 vs 1142 ms, 2269 vs 2885 ms) -- what every lane of a sub-group repeats (the
// simplex, the sums) is repeated half as often -- with the same bits in every result; the 16-lane instance is not kept.
constexpr int GW_LANES = 8;

int gwalpha_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n, const double *bins, const double *q, double sig,
                double mn, double mx, const pg_filter *flt, int method, int32_t *n_out, int32_t *ids, double *mean_freq,
                double *alpha, double *shapes, double *cost, int32_t *iters) {
    PG_CHECK(ctx, bins && q && n_out && ids && mean_freq && alpha, "gwalpha: null pointer");
    PG_CHECK(ctx, n >= 3, "gwalpha: %d pools; the reference's phenotype matrix needs at least 3 (sig, MIN, MAX rows)", n);
    PG_CHECK(ctx, method == PG_GWALPHA_LS || method == PG_GWALPHA_ML, "gwalpha: method %d (PG_GWALPHA_LS or PG_GWALPHA_ML)", method);
    const int sgl = GW_LANES;
    const size_t lds = sizeof(double) * (size_t)(64 / sgl) * (size_t)(6 * n + 4);
    if (lds > (size_t)GW_LDS_MAX)
        return pg_fail(ctx, PG_ERR_UNSUPPORTED, "gwalpha: %d pools; the fit kernel keeps 6 n doubles per fit in LDS (n <= %d)", n,
                       (int)(GW_LDS_MAX / (8 * (64 / sgl)) - 4) / 6);
    // tail of the workspace: [count, cursor][bins: n][q': n][rows: PG_MAX_OUT * L]
    size_t off = 0;
    const size_t t_cnt = off; off = gw_up16(off + 16);
    const size_t t_bins = off; off = gw_up16(off + sizeof(double) * n);
    const size_t t_qp = off; off = gw_up16(off + sizeof(double) * n);
    const size_t t_rows = off; off = gw_up16(off + sizeof(int64_t) * (size_t)PG_MAX_OUT * (size_t)(L > 0 ? L : 0));
    const int32_t *flags = nullptr;
    int64_t listed = 0;
    char *tail = nullptr;
    // the pools' shares are the pool sizes the filter sees (main.rs:210, phen.rs:157)
    int rc = pg_filter_headers(ctx, "gwalpha", PG_K_GWALPHA, true, counts_dev, L, n, bins, flt, 1, off, &flags, &listed, &tail);
    if (rc) return rc;
    std::vector<double> hb(2 * (size_t)n);
    for (int i = 0; i < n; ++i) {
        hb[i] = bins[i];
        hb[n + i] = i == 0 ? 0.0 : (q[i] - mn) / (mx - mn); // q_prime, gwalpha.rs:248-251
    }
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(tail + t_cnt);
    double *bins_dev = reinterpret_cast<double *>(tail + t_bins), *qp_dev = reinterpret_cast<double *>(tail + t_qp);
    int64_t *rows = reinterpret_cast<int64_t *>(tail + t_rows);
    PG_HIP(ctx, hipMemsetAsync(cnt, 0, 16, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(bins_dev, hb.data(), sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(qp_dev, hb.data() + n, sizeof(double) * n, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // hb is pageable and leaves scope
    GwParams P;
    P.L = L; P.n = n; P.sig = sig; P.mn = mn; P.mx = mx;
    const int fits_per_wave = 64 / sgl;
    const int64_t want = ((int64_t)PG_MAX_OUT * L + fits_per_wave - 1) / fits_per_wave, cap = (int64_t)ctx->cus * 32;
    const dim3 grid((unsigned)(want < cap ? want : cap));
    const bool mlm = method == PG_GWALPHA_ML;
    auto launch = [&](auto kern) -> int {
        PG_HIP(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        pg_prof_begin(ctx, PG_K_GWALPHA | PG_PROF_CONT);
        hipLaunchKernelGGL(k_gw_rows, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, ctx->stream, flags, L, n_out, ids, rows, cnt);
        hipLaunchKernelGGL(kern, grid, dim3(64), lds, ctx->stream, counts_dev, flags, (const int64_t *)rows,
                           (const unsigned long long *)cnt, cnt + 1, (const double *)bins_dev, (const double *)qp_dev, P, mean_freq,
                           alpha, shapes, cost, iters);
        pg_prof_end(ctx);
        return PG_OK;
    };
    rc = mlm ? launch(k_gw_fit<GW_LANES, true>) : launch(k_gw_fit<GW_LANES, false>);
    if (rc) return rc;
    PG_HIP(ctx, hipGetLastError());
    ctx->lo_last_L = L; ctx->lo_last_listed = listed;
    return PG_OK;
}

} // namespace

extern "C" int pg_gwalpha_batch_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n, const double *bins, const double *q,
                                    double sig, double min, double max, const pg_filter *filter, int method, int32_t *n_out_dev,
                                    int32_t *allele_ids_dev, double *mean_freq_dev, double *alpha_dev, double *shapes_dev,
                                    double *cost_dev, int32_t *iters_dev) {
    if (!ctx) return PG_ERR_INVALID;
    return gwalpha_dev(ctx, counts_dev, L, n, bins, q, sig, min, max, filter, method, n_out_dev, allele_ids_dev, mean_freq_dev,
                       alpha_dev, shapes_dev, cost_dev, iters_dev);
}

extern "C" int pg_gwalpha_batch(pg_ctx *ctx, const uint32_t *counts, int64_t L, int n, const double *bins, const double *q, double sig,
                                double min, double max, const pg_filter *filter, int method, int32_t *n_out, int32_t *allele_ids,
                                double *mean_freq, double *alpha, double *shapes, double *cost, int32_t *iters) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, counts && n_out && allele_ids && mean_freq && alpha && L > 0 && n >= 3, "gwalpha: bad arguments");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    // one device block: [counts | alpha | mean_freq | shapes | cost | allele_ids | n_out | iters], every piece 16-byte aligned
    const size_t rowsz = (size_t)L * PG_MAX_OUT;
    const size_t cb = (size_t)L * n * 6 * sizeof(uint32_t);
    struct Out { void *host; size_t bytes; size_t off; } o[] = {
        {alpha, rowsz * 8, 0}, {mean_freq, rowsz * 8, 0}, {shapes, rowsz * 32, 0}, {cost, rowsz * 8, 0},
        {allele_ids, rowsz * 4, 0}, {n_out, (size_t)L * 4, 0}, {iters, rowsz * 4, 0}};
    size_t total = gw_up16(cb);
    for (Out &e : o) { e.off = total; total = gw_up16(total + e.bytes); }
    DevBuf<char> block;
    int rc = block.alloc(ctx, total, "gwalpha");
    if (rc) return rc;
    char *const d = block.get();
    if (hipMemcpyAsync(d, counts, cb, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = pg_fail(ctx, PG_ERR_HIP, "gwalpha: H2D failed");
    if (!rc)
        rc = gwalpha_dev(ctx, reinterpret_cast<const uint32_t *>(d), L, n, bins, q, sig, min, max, filter, method,
                         (int32_t *)(d + o[5].off), (int32_t *)(d + o[4].off), (double *)(d + o[1].off), (double *)(d + o[0].off),
                         shapes ? (double *)(d + o[2].off) : nullptr, cost ? (double *)(d + o[3].off) : nullptr,
                         iters ? (int32_t *)(d + o[6].off) : nullptr);
    if (!rc) {
        bool okc = true;
        for (const Out &e : o)
            if (e.host) okc = okc && hipMemcpyAsync(e.host, d + e.off, e.bytes, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess;
        if (!okc) rc = pg_fail(ctx, PG_ERR_HIP, "gwalpha: D2H failed");
    }
    (void)hipStreamSynchronize(ctx->stream); // on every path: the copies read and write the caller's host buffers
    return rc;
}

extern "C" int pg_beta_reg_dev(pg_ctx *ctx, const double *a_dev, const double *b_dev, const double *x_dev, int64_t count,
                               double *out_dev) {
    if (!ctx) return PG_ERR_INVALID;
    if (count == 0) return PG_OK;
    PG_CHECK(ctx, a_dev && b_dev && x_dev && out_dev && count > 0, "beta_reg: bad arguments");
    PG_HIP(ctx, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_beta_reg, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, ctx->stream, a_dev, b_dev, x_dev, count, out_dev);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}
