// pg_popgen.hip -- fst (popgen/fst.rs:10-115, :158-200) and theta_pi / heterozygosity (popgen/pi.rs:10-113) on the
// resident locus-major genotype matrix G (p x ld, one row per allele column) of the loader, with the coverages the
// loader writes beside it (row of a locus' first column = the pools' depths over the surviving alleles,
// sync.rs:1142-1152).  A "locus" is a run of columns with the same (chromosome, position) (count_loci, sync.rs:73-97):
// locus_col[l] .. locus_col[l+1] are its rows of G.
//
//   k_pop_locus      thread = (locus, pool): sum of squared frequencies over the locus' alleles, the n/(n-1) factor,
//                    q1 (fst.rs:69-75) and pi (pi.rs:51-54): two L x n arrays, 1/a of the size of G
//                    (optionally, in the same pass, the polymorphic flag of watterson_theta.rs:8-30: one byte)
//   k_poly_locus     thread = (locus, pool): the flag alone, for watterson_estimator, which needs no pi
//   k_diversity_windows  thread = (window, pool): one walk over the window's loci -> the pi sum (k_range_mean_1d's order
//                    and bits) and the count of flagged loci, then theta_W (watterson_theta.rs:175-182) and Tajima's D
//                    (tajima_d.rs:62-81) from per-pool constants the host computed
//   k_pop_check      thread = locus: the reference's guard that the frequencies of a locus sum to n (fst.rs:66), in
//                    ndarray's summation orders
//   k_range_mean_1d  thread = (window, pool): mean of pi over the window's loci, summed left to right as
//                    mean_axis does (pi.rs:84-95)
//   k_fst_ranges     block = (range of loci, 32 x 32 tile of pool pairs, upper triangle), thread = 4 x 4 pairs: per locus
//                    q2 = sum_a g_j g_k, the clamped ratio (fst.rs:76-91), summed left to right over the range;
//                    ranges are the windows (divide: per-window means, :178-199) or equal chunks of the genome
//                    (partial sums, then k_chunk_reduce -> the genome-wide mean, :145)
// All arithmetic is fp64 VALU; the matrix is read a few times (once per overlapping window + once for the genome-wide
// mean) through L2: these are elementwise n^2-per-locus reductions (2.0e4 pairs x ~30 flops per locus at n = 200), bound
// by the fp64 vector pipe, not by HBM and not GEMM-shaped (the ratio is taken per locus before averaging).
#include "pg_common.h"
#include <cmath>
#include <vector>

namespace {

constexpr double POP_EPS = 2.220446049250313e-16; // f64::EPSILON

// FLAG (polymorphic_loci_per_pool, watterson_theta.rs:20-27): 1 iff the fold (0.0, |max, x| if x > max { x } else { max })
// over the locus' frequencies ends below 1.0 -- a NaN never wins the comparison, so an all-NaN pool counts as polymorphic.
__device__ __forceinline__ double poly_fold(double m, double g) { return g > m ? g : m; }

template <bool WITH_Q1, bool WITH_FLAG>
__global__ __launch_bounds__(256) void k_pop_locus(const double *__restrict__ G, const double *__restrict__ cov,
                                                   const int64_t *__restrict__ locus_col, int64_t L, int n, int64_t ld,
                                                   double *__restrict__ Q1, double *__restrict__ PI,
                                                   uint8_t *__restrict__ FLAG) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t l = gid / n;
    if (l >= L) return;
    const int pool = (int)(gid - l * n);
    const int64_t c0 = locus_col[l], c1 = locus_col[l + 1];
    double s = 0.0, m = 0.0;
    for (int64_t c = c0; c < c1; ++c) {
        const double g = G[c * ld + pool];
        s = s + g * g;
        if (WITH_FLAG) m = poly_fold(m, g);
    }
    const double nj = cov[c0 * ld + pool];
    const double r = nj / (nj - 1.00 + POP_EPS);
    if (WITH_Q1) Q1[gid] = (s * r) + (1.00 - r);
    PI[gid] = fabs((s * r) - r);
    if (WITH_FLAG) FLAG[gid] = m < 1.0 ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_poly_locus(const double *__restrict__ G, const int64_t *__restrict__ locus_col,
                                                    int64_t L, int n, int64_t ld, uint8_t *__restrict__ FLAG) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t l = gid / n;
    if (l >= L) return;
    const int pool = (int)(gid - l * n);
    double m = 0.0;
    for (int64_t c = locus_col[l]; c < locus_col[l + 1]; ++c) m = poly_fold(m, G[c * ld + pool]);
    FLAG[gid] = m < 1.0 ? 1 : 0;
}

// |sum_i (sum_a g) - n| <= eps with ndarray's orders: the lane of < 8 alleles left to right, the n row sums by
// unrolled_fold (8 partial sums, then (p0+p4)+(p1+p5)+(p2+p6)+(p3+p7), then the tail left to right)
__global__ __launch_bounds__(256) void k_pop_check(const double *__restrict__ G, const int64_t *__restrict__ locus_col,
                                                   int64_t L, int n, int64_t ld, int *__restrict__ bad) {
    const int64_t l = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (l >= L) return;
    const int64_t c0 = locus_col[l], c1 = locus_col[l + 1];
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    auto rowsum = [&](int i) {
        double s = 0.0;
        if (c1 - c0 >= 8) { // more alleles than the format has; kept for the arithmetic's sake
            double q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            int64_t c = c0;
            for (; c1 - c >= 8; c += 8)
                for (int u = 0; u < 8; ++u) q[u] = q[u] + G[(c + u) * ld + i];
            s = s + (q[0] + q[4]); s = s + (q[1] + q[5]); s = s + (q[2] + q[6]); s = s + (q[3] + q[7]);
            for (; c < c1; ++c) s = s + G[c * ld + i];
            return s;
        }
        for (int64_t c = c0; c < c1; ++c) s = s + G[c * ld + i];
        return s;
    };
    int i = 0;
    for (; n - i >= 8; i += 8)
        for (int u = 0; u < 8; ++u) p[u] = p[u] + rowsum(i + u);
    double acc = 0.0;
    acc = acc + (p[0] + p[4]); acc = acc + (p[1] + p[5]); acc = acc + (p[2] + p[6]); acc = acc + (p[3] + p[7]);
    for (; i < n; ++i) acc = acc + rowsum(i);
    if (!(fabs(acc - (double)n) <= POP_EPS)) atomicOr(bad, 1);
}

__global__ __launch_bounds__(256) void k_range_mean_1d(const double *__restrict__ V, const int64_t *__restrict__ head,
                                                       const int64_t *__restrict__ tail, int64_t nw, int n,
                                                       double *__restrict__ out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t w = gid / n;
    if (w >= nw) return;
    const int pool = (int)(gid - w * n);
    double s = 0.0;
    for (int64_t l = head[w]; l <= tail[w]; ++l) s = s + V[l * n + pool];
    out[gid] = s / (double)(tail[w] + 1 - head[w]);
}

// Per (window, pool): S, theta_W and -- TAJIMA -- pi and D.  wcov == nullptr is the counted mode (S = the flagged loci of
// head..tail, cov = their number); otherwise the reference's count (watterson_theta.rs:107-137): the window's first flag plus
// cov - 1 times the flag of the locus whose index is the window's slot.  kc = a1[n], e1[n], e2[n] (tajima_d.rs:53-61).
// Every step is one IEEE operation in the reference's order; NaN fails each comparison and reaches the division.
template <bool TAJIMA>
__global__ __launch_bounds__(256) void k_diversity_windows(const double *__restrict__ PI, const uint8_t *__restrict__ FLAG,
                                                           const int64_t *__restrict__ head, const int64_t *__restrict__ tail,
                                                           const int64_t *__restrict__ wcov, const int64_t *__restrict__ wseed,
                                                           const int64_t *__restrict__ wslot, int64_t nw, int n,
                                                           const double *__restrict__ kc, int64_t *__restrict__ seg,
                                                           double *__restrict__ theta_out, double *__restrict__ pi_out,
                                                           double *__restrict__ d_out) {
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t w = gid / n;
    if (w >= nw) return;
    const int pool = (int)(gid - w * n);
    const int64_t l0 = head[w], l1 = tail[w];
    const bool counted = wcov == nullptr;
    int64_t S = 0, c = l1 + 1 - l0;
    double s = 0.0;
    if (TAJIMA || counted)
        for (int64_t l = l0; l <= l1; ++l) {
            if (TAJIMA) s = s + PI[l * n + pool];
            if (counted) S += FLAG[l * n + pool];
        }
    if (!counted) {
        c = wcov[w];
        S = (int64_t)FLAG[wseed[w] * n + pool] + (c - 1) * (int64_t)FLAG[wslot[w] * n + pool];
    }
    const double a1 = kc[pool];
    const double theta = ((double)S / (double)c) / a1; // :177-180
    if (seg) seg[gid] = S;
    theta_out[gid] = theta;
    if (TAJIMA) {
        const double pi = s / (double)(l1 + 1 - l0); // k_range_mean_1d
        const double e1 = kc[n + pool], e2 = kc[2 * n + pool];
        const double sw = theta <= POP_EPS ? 0.0 : theta / a1;
        const double vd = (e1 * sw) + ((e2 * sw) * (sw - 1.0));
        pi_out[gid] = pi;
        d_out[gid] = fabs(pi - theta) <= POP_EPS ? 0.0 : (vd <= POP_EPS ? 0.0 : (pi - theta) / sqrt(vd));
    }
}

// a / b as hipcc's own fp64 division computes it for normal-range operands, minus the scaling and fix-up steps those
// operands do not need (1 - q2 + eps lies in [eps, 1 + eps]; the quotient is 0, NaN or of ordinary size): v_rcp_f64, two
// Newton steps, then quotient, fused residual, fused correction.  Same helper and same argument as pg_locus_ops.hip; the
// per-window table is compared bit for bit with the oracle's `/` (tests/test_gpu_popgen.py).
__device__ __forceinline__ double pop_div(double a, double b) {
    const double r0 = __builtin_amdgcn_rcp(b);
    const double r1 = fma(fma(-b, r0, 1.0), r0, r0);
    const double r = fma(fma(-b, r1, 1.0), r1, r1);
    const double q0 = a * r;
    return fma(fma(-b, q0, a), r, q0);
}

constexpr int FT = 8;       // threads per tile edge (one wave per block)
constexpr int FR = 4;       // pools per thread along each edge: a block covers a (FT*FR)^2 = 32 x 32 tile of pairs
constexpr int FTILE = FT * FR;

// grid.x = range, grid.y = upper-triangular tile id; out[range][n][n] (both triangles written).  Every thread keeps a
// 4 x 4 block of pairs: 8 frequencies and 8 q1 per allele row serve 16 ratios, and the 16 independent divisions
// overlap each other's latency.  Per pair the operations and their order are those of the reference (fst.rs:69-91).
__global__ __launch_bounds__(FT * FT) void k_fst_ranges(const double *__restrict__ G, const double *__restrict__ Q1,
                                                        const int64_t *__restrict__ locus_col,
                                                        const int64_t *__restrict__ head, const int64_t *__restrict__ tail,
                                                        int n, int64_t ld, int ntile, int divide, double *__restrict__ out) {
    // tile id -> (tj, tk) with tj <= tk
    int t = blockIdx.y, tj = 0;
    while (t >= ntile - tj) { t -= ntile - tj; ++tj; }
    const int tk = tj + t;
    const int j0 = tj * FTILE + (threadIdx.x / FT) * FR, k0 = tk * FTILE + (threadIdx.x % FT) * FR;
    int jj[FR], kk[FR];
#pragma unroll
    for (int u = 0; u < FR; ++u) { jj[u] = min(j0 + u, n - 1); kk[u] = min(k0 + u, n - 1); }
    const int64_t w = blockIdx.x;
    const int64_t l0 = head[w], l1 = tail[w];
    double s[FR][FR];
#pragma unroll
    for (int u = 0; u < FR; ++u)
#pragma unroll
        for (int v = 0; v < FR; ++v) s[u][v] = 0.0;
    int64_t c0 = locus_col[l0];
    for (int64_t l = l0; l <= l1; ++l) {
        const int64_t c1 = locus_col[l + 1];
        double q2[FR][FR];
#pragma unroll
        for (int u = 0; u < FR; ++u)
#pragma unroll
            for (int v = 0; v < FR; ++v) q2[u][v] = 0.0;
        for (int64_t c = c0; c < c1; ++c) {
            const double *row = G + c * ld;
            double gj[FR], gk[FR];
#pragma unroll
            for (int u = 0; u < FR; ++u) { gj[u] = row[jj[u]]; gk[u] = row[kk[u]]; }
#pragma unroll
            for (int u = 0; u < FR; ++u)
#pragma unroll
                for (int v = 0; v < FR; ++v) q2[u][v] = q2[u][v] + (gj[u] * gk[v]);
        }
        const double *qrow = Q1 + l * n;
        double q1j[FR], q1k[FR];
#pragma unroll
        for (int u = 0; u < FR; ++u) { q1j[u] = qrow[jj[u]]; q1k[u] = qrow[kk[u]]; }
#pragma unroll
        for (int u = 0; u < FR; ++u)
#pragma unroll
            for (int v = 0; v < FR; ++v) {
                const double fu = pop_div(0.5 * (q1j[u] + q1k[v]) - q2[u][v], 1.00 - q2[u][v] + POP_EPS);
                s[u][v] = s[u][v] + (fu < 0.0 ? 0.0 : (fu > 1.0 ? 1.0 : fu)); // NaN passes through, as in the reference
            }
        c0 = c1;
    }
    const double den = (double)(l1 + 1 - l0);
    double *o = out + (size_t)w * n * n;
#pragma unroll
    for (int u = 0; u < FR; ++u)
#pragma unroll
        for (int v = 0; v < FR; ++v) {
            const int j = j0 + u, k = k0 + v;
            if (j < n && k < n && j <= k) {
                const double r = divide ? s[u][v] / den : s[u][v];
                o[(size_t)j * n + k] = r;
                o[(size_t)k * n + j] = r; // every term is symmetric in (j, k): x*y, q1_j + q1_k
            }
        }
}

__global__ __launch_bounds__(256) void k_chunk_reduce(const double *__restrict__ part, int64_t nchunks, int64_t nn,
                                                      double denom, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nn) return;
    double s = 0.0;
    for (int64_t c = 0; c < nchunks; ++c) s = s + part[c * nn + i];
    out[i] = s / denom;
}

// mean_axis(Axis(0)) of a windows x n table, the one statement of it: the windows added left to right, a lane a pool
__global__ __launch_bounds__(256) void k_window_mean(const double *__restrict__ vals, int64_t nw, int n, double *__restrict__ mean) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double s = 0.0;
    for (int64_t w = 0; w < nw; ++w) s = s + vals[(size_t)w * n + j];
    mean[j] = s / (double)nw;
}

// What every entry point is handed, as plain data: the loader's matrix with the first column of every locus (host; cov is
// null where no coverages are read), and the windows (host; cov, seed and slot are the reference's count of
// watterson_estimator and tajima_d, all three null in the counted mode and for pi and fst).
struct PopMatrix { const double *G, *cov; int64_t p; int n; int64_t ld; const int64_t *locus_col; int64_t L; };
struct PopWindows { const int64_t *head, *tail; int64_t nw; const int64_t *cov, *seed, *slot; };

int check_shape(pg_ctx *ctx, const PopMatrix &m, bool with_cov, const PopWindows &w, const char *who) {
    PG_CHECK(ctx, m.G && (m.cov || !with_cov) && m.locus_col && m.p > 0 && m.n >= 1 && m.ld >= m.n && m.L >= 1, "%s: bad arguments", who);
    PG_CHECK(ctx, m.locus_col[0] == 0 && m.locus_col[m.L] == m.p, "%s: locus_col must run from 0 to p", who);
    for (int64_t l = 0; l < m.L; ++l) PG_CHECK(ctx, m.locus_col[l] < m.locus_col[l + 1], "%s: empty locus %lld", who, (long long)l);
    PG_CHECK(ctx, w.nw >= 0 && (w.nw == 0 || (w.head && w.tail)), "%s: windows missing", who);
    for (int64_t i = 0; i < w.nw; ++i)
        PG_CHECK(ctx, w.head[i] >= 0 && w.head[i] <= w.tail[i] && w.tail[i] < m.L, "%s: window %lld out of range", who, (long long)i);
    return PG_OK;
}

// pool_sizes[j] as usize (watterson_theta.rs:179, tajima_d.rs:52): Rust's saturating truncation, NaN -> 0
uint64_t pool_size_as_usize(double x) {
    if (!(x >= 1.0)) return 0;
    return x >= 18446744073709551615.0 ? UINT64_MAX : (uint64_t)x;
}

// a1[n], e1[n], e2[n] of tajima_d.rs:53-61 (a1 alone is watterson_theta.rs:178-179), every operation and its order as
// written there.  powf is libm's pow: the exponent is read through a volatile so that the call is not folded into x * x.
void diversity_constants(const double *pool_sizes, int n, std::vector<double> &kc) {
    volatile double two_v = 2.0;
    const double two = two_v;
    kc.assign((size_t)3 * n, 0.0);
    for (int j = 0; j < n; ++j) {
        const uint64_t m = pool_size_as_usize(pool_sizes[j]);
        double a1 = 0.0, a2 = 0.0;
        for (uint64_t x = 1; x < m; ++x) a1 = a1 + (1.00 / (double)x);
        for (uint64_t x = 1; x < m; ++x) a2 = a2 + (1.00 / std::pow((double)x, two));
        const double nn = (double)m;
        const double b1 = (nn + 1.0) / (3.0 * (nn - 1.0));
        const double b2 = (2.0 * (std::pow(nn, two) + nn + 3.0)) / (9.0 * nn * (nn - 1.0));
        const double c1 = b1 - (1.0 / a1);
        const double c2 = b2 - ((nn + 2.0) / (a1 * nn)) + (a2 / std::pow(a1, two));
        kc[j] = a1;
        kc[(size_t)n + j] = c1 / a1;
        kc[(size_t)2 * n + j] = c2 / (std::pow(a1, two) + a2);
    }
}

constexpr double POOL_SIZE_MAX = 1e9; // the harmonic sums are loops over 1 .. pool size

// The statistics per (window, pool): watterson_estimator's theta_W, theta_pi's pi and tajima_d's D, which fills the other two
// tables on its way where asked to.  A statistic is named by the index of its table (windows x n) in WindowOut: win[stat] and
// mean (n: its mean across windows) are required, the other tables (tajima_d) and seg (watterson: S per window) optional.
enum Stat { THETA_W, THETA_PI, TAJIMA_D, N_STATS };
const char *const STAT_NAME[N_STATS] = {"watterson", "pi", "tajima_d"};
struct WindowOut { double *win[N_STATS]; int64_t *seg; double *mean; };

// the refusals, the same for both forms: `o` holds the caller's pointers, host or device
int stat_check(pg_ctx *ctx, Stat stat, const PopMatrix &m, const PopWindows &w, const double *pool_sizes, const WindowOut &o) {
    const char *who = STAT_NAME[stat];
    const int rc = check_shape(ctx, m, stat != THETA_W, w, who);
    if (rc) return rc;
    if (stat == THETA_PI) {
        PG_CHECK(ctx, w.nw >= 1 && o.win[THETA_PI] && o.mean, "pi: There were no windows defined."); // pi.rs:81
        return PG_OK;
    }
    PG_CHECK(ctx, w.nw >= 1, "%s: There were no windows defined.", who);
    PG_CHECK(ctx, pool_sizes && o.win[stat] && o.mean, "%s: null argument", who);
    const bool reference = w.cov || w.seed || w.slot;
    PG_CHECK(ctx, !reference || (w.cov && w.seed && w.slot), "%s: win_cov, win_seed and win_slot go together", who);
    for (int64_t i = 0; reference && i < w.nw; ++i)
        PG_CHECK(ctx, w.cov[i] >= 1 && w.seed[i] >= 0 && w.seed[i] < m.L && w.slot[i] >= 0 && w.slot[i] < m.L,
                 "%s: count of window %lld out of range", who, (long long)i);
    for (int j = 0; j < m.n; ++j)
        PG_CHECK(ctx, !(pool_sizes[j] > POOL_SIZE_MAX), "%s: pool size %d is beyond %.0f", who, j, POOL_SIZE_MAX);
    return PG_OK;
}

// watterson_estimator (tajima == false: no coverages, no pi) and tajima_d on one locus pass and one window pass, checked
// arguments, every pointer of `o` device memory: the kernels write into the caller's tables
int diversity_tables(pg_ctx *ctx, bool tajima, const PopMatrix &m, const PopWindows &w, const double *pool_sizes, const WindowOut &o) {
    const char *who = tajima ? "tajima_d" : "watterson";
    const int n = m.n;
    const int64_t L = m.L, nw = w.nw;
    std::vector<double> kc;
    diversity_constants(pool_sizes, n, kc);
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t ln = (size_t)L * n, wn = (size_t)nw * n;
    const bool reference = w.cov != nullptr;
    const int nwin = reference ? 5 : 2; // head | tail | cov | seed | slot
    // the window kernel writes theta always and pi for tajima_d: scratch for the one the caller did not ask for
    double *theta_dev = o.win[THETA_W], *pi_dev = o.win[THETA_PI];
    const bool own_theta = !theta_dev, own_pi = tajima && !pi_dev;
    DevBuf<int64_t> lc, win;
    DevBuf<double> pi, kcd, scratch;
    DevBuf<uint8_t> flag;
    int rc;
    if ((rc = lc.alloc(ctx, sizeof(int64_t) * (L + 1), who))) return rc;
    if ((rc = flag.alloc(ctx, ln, who))) return rc;
    if (tajima && (rc = pi.alloc(ctx, sizeof(double) * ln, who))) return rc;
    if ((rc = win.alloc(ctx, sizeof(int64_t) * nwin * nw, who))) return rc;
    if ((rc = kcd.alloc(ctx, sizeof(double) * 3 * n, who))) return rc;
    if ((rc = scratch.alloc(ctx, sizeof(double) * ((size_t)own_theta + (size_t)own_pi) * wn, who))) return rc;
    if (own_theta) theta_dev = scratch.get();
    if (own_pi) pi_dev = scratch.get() + (own_theta ? wn : 0);
    const int64_t *host_win[5] = {w.head, w.tail, w.cov, w.seed, w.slot};
    PG_HIP(ctx, hipMemcpyAsync(lc.get(), m.locus_col, sizeof(int64_t) * (L + 1), hipMemcpyHostToDevice, ctx->stream));
    for (int i = 0; i < nwin; ++i)
        PG_HIP(ctx, hipMemcpyAsync(win.get() + (size_t)i * nw, host_win[i], sizeof(int64_t) * nw, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(kcd.get(), kc.data(), sizeof(double) * 3 * n, hipMemcpyHostToDevice, ctx->stream));
    const int64_t *wh = win.get(), *wt = wh + nw;
    const int64_t *wc = reference ? wt + nw : nullptr, *wsd = reference ? wc + nw : nullptr, *wsl = reference ? wsd + nw : nullptr;
    const dim3 lgrid((unsigned)((ln + 255) / 256)), wgrid((unsigned)((wn + 255) / 256));
    if (tajima) {
        hipLaunchKernelGGL((k_pop_locus<false, true>), lgrid, dim3(256), 0, ctx->stream, m.G, m.cov, lc.get(), L, n, m.ld,
                           (double *)nullptr, pi.get(), flag.get());
        hipLaunchKernelGGL(k_diversity_windows<true>, wgrid, dim3(256), 0, ctx->stream, pi.get(), flag.get(), wh, wt, wc, wsd, wsl,
                           nw, n, kcd.get(), o.seg, theta_dev, pi_dev, o.win[TAJIMA_D]);
    } else {
        hipLaunchKernelGGL(k_poly_locus, lgrid, dim3(256), 0, ctx->stream, m.G, lc.get(), L, n, m.ld, flag.get());
        hipLaunchKernelGGL(k_diversity_windows<false>, wgrid, dim3(256), 0, ctx->stream, (const double *)nullptr, flag.get(), wh, wt,
                           wc, wsd, wsl, nw, n, kcd.get(), o.seg, theta_dev, (double *)nullptr, (double *)nullptr);
    }
    hipLaunchKernelGGL(k_window_mean, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, tajima ? o.win[TAJIMA_D] : theta_dev, nw, n,
                       o.mean); // watterson_theta.rs:213-215, tajima_d.rs:98
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the temporaries go with this call
    return PG_OK;
}

// checked arguments, outputs on the device
int pi_tables(pg_ctx *ctx, const PopMatrix &m, const PopWindows &w, double *win_dev, double *mean_dev) {
    const int n = m.n;
    const int64_t L = m.L, nw = w.nw;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<int64_t> lc, wh, wt;
    DevBuf<double> q1, pi;
    int rc;
    if ((rc = lc.alloc(ctx, sizeof(int64_t) * (L + 1), "pi"))) return rc;
    if ((rc = q1.alloc(ctx, sizeof(double) * (size_t)L * n, "pi"))) return rc;
    if ((rc = pi.alloc(ctx, sizeof(double) * (size_t)L * n, "pi"))) return rc;
    if ((rc = wh.alloc(ctx, sizeof(int64_t) * nw, "pi"))) return rc;
    if ((rc = wt.alloc(ctx, sizeof(int64_t) * nw, "pi"))) return rc;
    PG_HIP(ctx, hipMemcpyAsync(lc.get(), m.locus_col, sizeof(int64_t) * (L + 1), hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(wh.get(), w.head, sizeof(int64_t) * nw, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(wt.get(), w.tail, sizeof(int64_t) * nw, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL((k_pop_locus<true, false>), dim3((unsigned)(((size_t)L * n + 255) / 256)), dim3(256), 0, ctx->stream, m.G,
                       m.cov, lc.get(), L, n, m.ld, q1.get(), pi.get(), (uint8_t *)nullptr);
    hipLaunchKernelGGL(k_range_mean_1d, dim3((unsigned)(((size_t)nw * n + 255) / 256)), dim3(256), 0, ctx->stream,
                       pi.get(), wh.get(), wt.get(), nw, n, win_dev);
    hipLaunchKernelGGL(k_window_mean, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, win_dev, nw, n, mean_dev); // pi.rs:133
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the temporaries go with this call
    return PG_OK;
}

// a statistic's device function: checked arguments, every pointer of `o` device memory
int stat_tables(pg_ctx *ctx, Stat stat, const PopMatrix &m, const PopWindows &w, const double *pool_sizes, const WindowOut &o) {
    return stat == THETA_PI ? pi_tables(ctx, m, w, o.win[THETA_PI], o.mean) : diversity_tables(ctx, stat == TAJIMA_D, m, w, pool_sizes, o);
}

// The tables form: the refusals, then the device function on the caller's device memory.
int tables_form(pg_ctx *ctx, Stat stat, const PopMatrix &m, const PopWindows &w, const double *pool_sizes, const WindowOut &o) {
    if (!ctx) return PG_ERR_INVALID;
    const int rc = stat_check(ctx, stat, m, w, pool_sizes, o);
    return rc ? rc : stat_tables(ctx, stat, m, w, pool_sizes, o);
}

// The host form: the same into a block of this call's own, [mean: n | the tables asked for], then the copy down -- so the
// two forms cannot differ in a bit.
int host_form(pg_ctx *ctx, Stat stat, const PopMatrix &m, const PopWindows &w, const double *pool_sizes, const WindowOut &host) {
    if (!ctx) return PG_ERR_INVALID;
    int rc = stat_check(ctx, stat, m, w, pool_sizes, host);
    if (rc) return rc;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t wn = (size_t)w.nw * m.n;
    size_t asked = 0;
    for (const double *t : host.win) asked += t != nullptr;
    DevBuf<double> block;
    DevBuf<int64_t> seg;
    if ((rc = block.alloc(ctx, sizeof(double) * (m.n + asked * wn), STAT_NAME[stat]))) return rc;
    if (host.seg && (rc = seg.alloc(ctx, sizeof(int64_t) * wn, STAT_NAME[stat]))) return rc;
    WindowOut dev = {{nullptr, nullptr, nullptr}, seg.get(), block.get()};
    double *next = block.get() + m.n;
    for (int t = 0; t < N_STATS; ++t)
        if (host.win[t]) { dev.win[t] = next; next += wn; }
    if ((rc = stat_tables(ctx, stat, m, w, pool_sizes, dev))) return rc;
    for (int t = 0; t < N_STATS; ++t)
        if (host.win[t]) PG_HIP(ctx, hipMemcpyAsync(host.win[t], dev.win[t], sizeof(double) * wn, hipMemcpyDeviceToHost, ctx->stream));
    if (host.seg) PG_HIP(ctx, hipMemcpyAsync(host.seg, dev.seg, sizeof(int64_t) * wn, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(host.mean, dev.mean, sizeof(double) * m.n, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

// ---- fst, in two steps, so that the host form never holds more than a slab of the window table on the device ----

int fst_check(pg_ctx *ctx, const PopMatrix &m, const PopWindows &w, const double *fst_mean, const double *fst_win) {
    const int rc = check_shape(ctx, m, true, w, "fst");
    if (rc) return rc;
    PG_CHECK(ctx, fst_mean && (w.nw == 0 || fst_win), "fst: null output");
    return PG_OK;
}

// what the first step leaves on the device for the second: the loci's first columns, q1 per (locus, pool), the windows
struct FstPlan { DevBuf<int64_t> lc, wh, wt; DevBuf<double> q1; };

// k_fst_ranges over `ranges` ranges of loci (head, tail: device), n x n each, queued on the context's stream: their sums for step
// 1, or (divide) their means -- step 2, windows [w0, w0 + k) of the per-window table, is this on s.wh + w0 and s.wt + w0
int fst_ranges(pg_ctx *ctx, const PopMatrix &m, const FstPlan &s, const int64_t *head, const int64_t *tail, int64_t ranges, int divide,
               double *out_dev) {
    const int ntile = (m.n + FTILE - 1) / FTILE;
    const int ntri = ntile * (ntile + 1) / 2;
    hipLaunchKernelGGL(k_fst_ranges, dim3((unsigned)ranges, ntri), dim3(FT * FT), 0, ctx->stream, m.G, s.q1.get(), s.lc.get(), head, tail,
                       m.n, m.ld, ntile, divide, out_dev);
    PG_HIP(ctx, hipGetLastError());
    return PG_OK;
}

// Step 1 (checked arguments): the reference's guard, q1, the genome-wide mean into mean_dev (n x n), the windows sent up.
int fst_prepare(pg_ctx *ctx, const PopMatrix &m, const PopWindows &w, double *mean_dev, FstPlan &s) {
    const int n = m.n;
    const int64_t L = m.L;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n * n;
    // the genome-wide mean: equal chunks of loci -> partial sums -> one ordered reduction
    const int64_t chunk = std::max<int64_t>(64, (L + 2047) / 2048);
    const int64_t nchunks = (L + chunk - 1) / chunk;
    std::vector<int64_t> ch(2 * nchunks); // heads | tails
    for (int64_t c = 0; c < nchunks; ++c) { ch[c] = c * chunk; ch[nchunks + c] = std::min<int64_t>(L, (c + 1) * chunk) - 1; }
    DevBuf<int64_t> chunks;
    DevBuf<double> pi, part;
    DevBuf<int> bad;
    int rc;
    if ((rc = s.lc.alloc(ctx, sizeof(int64_t) * (L + 1), "fst"))) return rc;
    if ((rc = s.q1.alloc(ctx, sizeof(double) * (size_t)L * n, "fst"))) return rc;
    if ((rc = pi.alloc(ctx, sizeof(double) * (size_t)L * n, "fst"))) return rc;
    if ((rc = chunks.alloc(ctx, sizeof(int64_t) * 2 * nchunks, "fst"))) return rc;
    if ((rc = part.alloc(ctx, sizeof(double) * nchunks * nn, "fst"))) return rc;
    if ((rc = bad.alloc(ctx, sizeof(int), "fst"))) return rc;
    if ((rc = s.wh.alloc(ctx, sizeof(int64_t) * w.nw, "fst"))) return rc;
    if ((rc = s.wt.alloc(ctx, sizeof(int64_t) * w.nw, "fst"))) return rc;
    PG_HIP(ctx, hipMemsetAsync(bad.get(), 0, sizeof(int), ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(s.lc.get(), m.locus_col, sizeof(int64_t) * (L + 1), hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(ctx, hipMemcpyAsync(chunks.get(), ch.data(), sizeof(int64_t) * 2 * nchunks, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_pop_check, dim3((unsigned)((L + 255) / 256)), dim3(256), 0, ctx->stream, m.G, s.lc.get(), L, n, m.ld, bad.get());
    hipLaunchKernelGGL((k_pop_locus<true, false>), dim3((unsigned)(((size_t)L * n + 255) / 256)), dim3(256), 0, ctx->stream, m.G,
                       m.cov, s.lc.get(), L, n, m.ld, s.q1.get(), pi.get(), (uint8_t *)nullptr);
    int hbad = 0;
    PG_HIP(ctx, hipMemcpyAsync(&hbad, bad.get(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (hbad) // the reference's assert!((g.sum_axis(Axis(1)).sum() - n as f64).abs() <= f64::EPSILON) (fst.rs:66)
        return pg_fail(ctx, PG_ERR_INVALID, "fst: the allele frequencies of a locus do not sum up to one in every pool");
    if ((rc = fst_ranges(ctx, m, s, chunks.get(), chunks.get() + nchunks, nchunks, 0, part.get()))) return rc;
    hipLaunchKernelGGL(k_chunk_reduce, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, ctx->stream, part.get(), nchunks,
                       (int64_t)nn, (double)L, mean_dev);
    PG_HIP(ctx, hipGetLastError());
    if (w.nw > 0) {
        PG_HIP(ctx, hipMemcpyAsync(s.wh.get(), w.head, sizeof(int64_t) * w.nw, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(ctx, hipMemcpyAsync(s.wt.get(), w.tail, sizeof(int64_t) * w.nw, hipMemcpyHostToDevice, ctx->stream));
    }
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the temporaries go with this step
    return PG_OK;
}

// the windows of one launch, in both forms: the slab of the host form, 2^30 bytes of the table (it is n^2 doubles per window)
int64_t fst_slab(int n, int64_t nw) {
    return std::min<int64_t>(nw, std::max<int64_t>(1, (int64_t)(((size_t)1 << 30) / ((size_t)n * n * sizeof(double)))));
}

} // namespace

extern "C" int pg_pi_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                         const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                         int64_t n_windows, double *pi_win, double *pi_mean) {
    return host_form(ctx, THETA_PI, {G_dev, cov_dev, p, n, ld, locus_col, L}, {win_head, win_tail, n_windows, nullptr, nullptr, nullptr}, nullptr,
                     {{nullptr, pi_win, nullptr}, nullptr, pi_mean});
}

extern "C" int pg_pi_tables_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                                const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                                int64_t n_windows, double *pi_win_dev, double *pi_mean_dev) {
    return tables_form(ctx, THETA_PI, {G_dev, cov_dev, p, n, ld, locus_col, L}, {win_head, win_tail, n_windows, nullptr, nullptr, nullptr}, nullptr,
                       {{nullptr, pi_win_dev, nullptr}, nullptr, pi_mean_dev});
}

// the slabs of windows write straight into the caller's table
extern "C" int pg_fst_tables_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                                 const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                                 int64_t n_windows, double *fst_mean_dev, double *fst_win_dev) {
    if (!ctx) return PG_ERR_INVALID;
    const PopMatrix m = {G_dev, cov_dev, p, n, ld, locus_col, L};
    const PopWindows w = {win_head, win_tail, n_windows, nullptr, nullptr, nullptr};
    int rc = fst_check(ctx, m, w, fst_mean_dev, fst_win_dev);
    if (rc) return rc;
    FstPlan s;
    if ((rc = fst_prepare(ctx, m, w, fst_mean_dev, s))) return rc;
    const int64_t slab = fst_slab(n, n_windows);
    for (int64_t w0 = 0; w0 < n_windows; w0 += slab)
        if ((rc = fst_ranges(ctx, m, s, s.wh.get() + w0, s.wt.get() + w0, std::min<int64_t>(slab, n_windows - w0), 1, fst_win_dev + (size_t)w0 * n * n)))
            return rc;
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

// slab by slab through one slab of device memory
extern "C" int pg_fst_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                          const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                          int64_t n_windows, double *fst_mean, double *fst_win) {
    if (!ctx) return PG_ERR_INVALID;
    const PopMatrix m = {G_dev, cov_dev, p, n, ld, locus_col, L};
    const PopWindows w = {win_head, win_tail, n_windows, nullptr, nullptr, nullptr};
    int rc = fst_check(ctx, m, w, fst_mean, fst_win);
    if (rc) return rc;
    PG_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nn = (size_t)n * n;
    const int64_t slab = fst_slab(n, n_windows);
    FstPlan s;
    DevBuf<double> mean, out;
    if ((rc = mean.alloc(ctx, sizeof(double) * nn, "fst"))) return rc;
    if ((rc = out.alloc(ctx, sizeof(double) * slab * nn, "fst"))) return rc;
    if ((rc = fst_prepare(ctx, m, w, mean.get(), s))) return rc;
    PG_HIP(ctx, hipMemcpyAsync(fst_mean, mean.get(), sizeof(double) * nn, hipMemcpyDeviceToHost, ctx->stream));
    for (int64_t w0 = 0; w0 < n_windows; w0 += slab) {
        const int64_t nwb = std::min<int64_t>(slab, n_windows - w0);
        if ((rc = fst_ranges(ctx, m, s, s.wh.get() + w0, s.wt.get() + w0, nwb, 1, out.get()))) return rc;
        PG_HIP(ctx, hipMemcpyAsync(fst_win + (size_t)w0 * nn, out.get(), sizeof(double) * nwb * nn, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

// row w of the table = row slot[w] of the kept rows, NaN where slot[w] < 0
__global__ __launch_bounds__(256) void k_window_scatter(const double *__restrict__ kept, const int64_t *__restrict__ slot, int64_t w, int64_t cols,
                                                        double *__restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= w * cols) return;
    const int64_t r = i / cols, q = slot[r];
    table[i] = q >= 0 ? kept[q * cols + (i - r * cols)] : __builtin_nan("");
}

extern "C" int pg_window_scatter_dev(pg_ctx *ctx, const double *kept_dev, int64_t n_kept, const int64_t *keep, int64_t w, int64_t cols,
                                     double *table_dev) {
    if (!ctx) return PG_ERR_INVALID;
    PG_CHECK(ctx, n_kept >= 0 && w >= 1 && cols >= 1 && n_kept <= w && table_dev && (n_kept == 0 || (kept_dev && keep)) && w <= (((int64_t)1 << 39) - 1) / cols,
             "window_scatter: bad arguments");
    std::vector<int64_t> slot((size_t)w, -1);
    for (int64_t q = 0; q < n_kept; ++q) {
        PG_CHECK(ctx, keep[q] >= 0 && keep[q] < w && (q == 0 || keep[q] > keep[q - 1]), "window_scatter: kept window %lld out of order or range", (long long)q);
        slot[(size_t)keep[q]] = q;
    }
    PG_HIP(ctx, hipSetDevice(ctx->device));
    DevBuf<int64_t> slot_dev;
    int rc = slot_dev.alloc(ctx, sizeof(int64_t) * (size_t)w, "window_scatter");
    if (rc) return rc;
    PG_HIP(ctx, hipMemcpyAsync(slot_dev.get(), slot.data(), sizeof(int64_t) * (size_t)w, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_window_scatter, dim3((unsigned)((w * cols + 255) / 256)), dim3(256), 0, ctx->stream, kept_dev, slot_dev.get(), w, cols, table_dev);
    PG_HIP(ctx, hipGetLastError());
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the temporaries go with this call
    return PG_OK;
}

extern "C" int pg_watterson_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L,
                                const int64_t *win_head, const int64_t *win_tail, const int64_t *win_cov, const int64_t *win_seed,
                                const int64_t *win_slot, int64_t n_windows, const double *pool_sizes, double *theta_win,
                                double *theta_mean, int64_t *seg_win) {
    return host_form(ctx, THETA_W, {G_dev, nullptr, p, n, ld, locus_col, L}, {win_head, win_tail, n_windows, win_cov, win_seed, win_slot}, pool_sizes,
                     {{theta_win, nullptr, nullptr}, seg_win, theta_mean});
}

extern "C" int pg_watterson_tables_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L,
                                       const int64_t *win_head, const int64_t *win_tail, const int64_t *win_cov, const int64_t *win_seed,
                                       const int64_t *win_slot, int64_t n_windows, const double *pool_sizes, double *theta_win_dev,
                                       double *theta_mean_dev, int64_t *seg_win_dev) {
    return tables_form(ctx, THETA_W, {G_dev, nullptr, p, n, ld, locus_col, L}, {win_head, win_tail, n_windows, win_cov, win_seed, win_slot}, pool_sizes,
                       {{theta_win_dev, nullptr, nullptr}, seg_win_dev, theta_mean_dev});
}

extern "C" int pg_tajima_d_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                               const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                               const int64_t *win_cov, const int64_t *win_seed, const int64_t *win_slot, int64_t n_windows,
                               const double *pool_sizes, double *d_win, double *d_mean, double *theta_win, double *pi_win) {
    return host_form(ctx, TAJIMA_D, {G_dev, cov_dev, p, n, ld, locus_col, L}, {win_head, win_tail, n_windows, win_cov, win_seed, win_slot}, pool_sizes,
                     {{theta_win, pi_win, d_win}, nullptr, d_mean});
}

extern "C" int pg_tajima_d_tables_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                                      const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                                      const int64_t *win_cov, const int64_t *win_seed, const int64_t *win_slot, int64_t n_windows,
                                      const double *pool_sizes, double *d_win_dev, double *d_mean_dev, double *theta_win_dev,
                                      double *pi_win_dev) {
    return tables_form(ctx, TAJIMA_D, {G_dev, cov_dev, p, n, ld, locus_col, L}, {win_head, win_tail, n_windows, win_cov, win_seed, win_slot}, pool_sizes,
                       {{theta_win_dev, pi_win_dev, d_win_dev}, nullptr, d_mean_dev});
}
