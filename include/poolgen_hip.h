/*
 * poolgen_hip.h -- C ABI of libpoolgen_hip.so: the MI355X (gfx950) implementation of poolgen's
 * per-locus regression hot path.  This is the drop-in boundary: plain pointers and sizes, no
 * C++/torch types.  Each entry point cites the reference interface (file:line relative to the
 * poolgen source tree) it replaces; INTEGRATION.md shows the Rust `extern "C"` binding a
 * poolgen maintainer would add.
 *
 * Conventions
 *  - All floating point is fp64.  Integer/index outputs are bit-exact w.r.t. the reference.
 *  - Genotype matrices are LOCUS-MAJOR: G[l * ld + i] = allele frequency of pool i at column
 *    (locus/allele) l, ld >= n, ld even (16-byte aligned rows).  The reference stores
 *    `intercept_and_allele_frequencies` pool-major n x (1+p) (base/structs_and_traits.rs:144);
 *    the intercept column is implicit here.
 *  - Phenotypes Y are n x k row-major on the HOST (the reference's Array2<f64>, :145).
 *  - `*_dev` pointers are device (HBM) addresses on the context's GPU; everything else is host.
 *  - Return value: 0 on success, negative pg_status on failure; pg_last_error() gives text.
 *    A single bad locus never fails a batch: it is reported per locus (None -> n_alleles = 0,
 *    regression failure -> NaN) exactly like the reference operators (gwas/ols.rs:210-253,
 *    :358-369).
 *  - One in-flight call per pg_ctx; contexts are independent (one per GPU / per process rank).
 *  - There is NO CPU fallback: without a usable gfx950 device every compute call fails.
 */
#ifndef POOLGEN_HIP_H
#define POOLGEN_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pg_ctx pg_ctx;

enum pg_status {
    PG_OK = 0,
    PG_ERR_INVALID = -1,   /* bad shape / argument */
    PG_ERR_HIP = -2,       /* HIP runtime error (text in pg_last_error) */
    PG_ERR_NO_DEVICE = -3, /* no gfx950 device */
    PG_ERR_STATE = -4,     /* call order violated (e.g. sweep before covariates) */
    PG_ERR_UNSUPPORTED = -5
};

/* FilterStats subset used by the sync-derived operators (base/structs_and_traits.rs:68-78,
 * filled from the CLI flags at main.rs:202-211). */
typedef struct {
    int32_t remove_ns;            /* !--keep-ns */
    int32_t reserved;
    uint64_t min_coverage_depth;  /* --min-coverage-depth */
    double min_allele_frequency;  /* --min-allele-frequency */
    double max_missingness_rate;  /* --max-missingness-rate */
} pg_filter;

/* Per-locus output of the sync-derived batch operators (struct-of-arrays, slot-major, device or host; see below).
 * PG_MAX_OUT alleles (= rows = slots) per locus: 6 sync columns minus the one dropped. */
#define PG_MAX_OUT 5

/* ---------------------------------------------------------------------------------------
 * context
 * ------------------------------------------------------------------------------------- */
/* device: HIP ordinal.  stream: a hipStream_t owned by the caller (e.g. torch's current
 * stream); NULL = the device's default (null) stream.  All kernels and copies of this context
 * are enqueued on that stream, so they are ordered with the caller's own work on it. */
int pg_create(pg_ctx **out, int device, void *stream);
void pg_destroy(pg_ctx *ctx);
const char *pg_last_error(const pg_ctx *ctx);
const char *pg_version(void);
int pg_synchronize(pg_ctx *ctx);
/* Per-kernel HIP-event timing (used by bench.py for the roofline record). */
enum pg_kernel_id { PG_K_KINSHIP = 0, PG_K_KINSHIP_REDUCE = 1, PG_K_SWEEP = 2, PG_K_OLS_ITER = 3,
                    PG_K_PEARSON = 4, PG_K_CHISQ = 5, PG_K_GP_XXT = 6, PG_K_GP_BETA = 7,
                    PG_K_SWEEP_FINISH = 8, PG_K_ALLREDUCE = 9, PG_K_GP_PREDICT = 10, PG_K_FISHER = 11, PG_K_GWALPHA = 12, PG_K_CSV = 13,
                    PG_K_IMPUTE = 14, PG_K_IMPUTE_LINKS = 15, PG_K_IMPUTE_WALK = 16, PG_K_VCF = 17, PG_K_SYNC = 18, PG_K_PILEUP = 19, PG_K_SYNCFMT = 20,
                    PG_K_RESULTFMT = 21, PG_K_COUNT = 22 };
int pg_profile_enable(pg_ctx *ctx, int on);
int pg_profile_reset(pg_ctx *ctx);
/* Synchronises, then returns total milliseconds and launch count of one kernel id. */
int pg_profile_get(pg_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches);
/* Diagnostics of the last batch operator call (pg_ols_iter_batch[_dev], pg_pearson_batch[_dev], pg_chisq_batch[_dev],
 * pg_fisher_batch[_dev], pg_gwalpha_batch[_dev], pg_load_plan_dev) on this context: *loci = L of that call, *listed = the loci its streaming pass could not close in place
 * and handed to the second pass (three or more surviving alleles, or a speculated allele pair that did not hold; summed
 * over the launch groups of a multi-trait call).  Either pointer may be NULL. */
int pg_locus_op_stats(const pg_ctx *ctx, int64_t *loci, int64_t *listed);

/* ---------------------------------------------------------------------------------------
 * ols_iter_with_kinship   == gwas::ols_with_covariate (gwas/ols.rs:278-436, numeric core
 * :291-370; CLI main.rs:280-298).  Staged so that loci can be sharded over GPUs:
 *   1. pg_kinship_partial_dev : S_r = G_r^T-contraction over this rank's loci (unscaled)
 *   2. (multi-GPU) pg_allreduce_sum_dev : sum of S over the ranks (RCCL, see "Multi-GPU" below)
 *   3. pg_kinship_set        : K = S / p_total, eigen-decomposition, n_eigenvecs rule,
 *                               orthonormal basis of [1 | C], projected phenotypes
 *   4. pg_ols_sweep_dev      : per-column fit of y ~ [1 | C | g], last coefficient
 * pg_ols_kinship_dev runs 1,3,4 on one GPU.
 * ------------------------------------------------------------------------------------- */
/* Optional, before pg_kinship_partial_dev: announce the phenotypes (host, n x k row-major, no NaN,
 * k <= 4).  The kinship pass then also accumulates, from the SAME read of G, the three per-locus
 * sums an intercept-only fit needs.  If the n_eigenvecs rule later yields m = 0 (the outcome of the
 * default -x 0.75 on uncentred allele-frequency kinships, where lambda_1 carries ~98 % of the trace),
 * pg_ols_sweep_dev closes the fits from those sums instead of reading G a second time; for m > 0 the
 * sums are ignored and the regular sweep runs.  Results are the same either way (same formula,
 * different summation order).  pg_set_phenotypes(ctx, 0, NULL, 0) switches the behaviour off.
 * What the sums stand for, and for how long:
 *   - they belong to the pointer and shape (G_dev, p, n, ld) of the LAST kinship pass and to the phenotypes announced here;
 *   - the matrix must be unchanged from that pass until the sweep.  The library drops the sums when one of its own calls
 *     writes into that matrix (pg_load_emit_dev, pg_load_emit_cov_dev, pg_impute_mean_dev, pg_set_missing_by_depth_dev,
 *     pg_impute_compact_dev, pg_impute_aldknn_dev); it cannot see the caller's own writes, nor a matrix that was freed and
 *     another allocated at the same address;
 *   - ONE pg_ols_sweep_dev uses them: the next call of the sweep after the kinship pass leaves them invalid, whatever its
 *     arguments and also when it fails a check, and a second sweep reads G again.  The sweep that pg_gp_proxy_dev (and
 *     pg_gp_penalised_dev with iterative_proxy) runs inside counts as that call.
 *   - pg_ols_kinship_dev / pg_ols_kinship_sharded_dev announce their Y themselves, for the length of the call: the sums they
 *     make are invalid when the call returns, and the call opts nobody in -- a later pg_kinship_partial_dev fuses only if
 *     the caller announced phenotypes himself.  An announcement of the caller's stays in force across such a call when it
 *     was for the same phenotypes; when the call replaced it with other phenotypes it is over, and the two-pass path runs
 *     until the caller announces again. */
int pg_set_phenotypes(pg_ctx *ctx, int n, const double *Y, int k);
/* S_dev: n x n fp64, row-major, full symmetric sum_l g_l g_l^T over this call's p columns. */
int pg_kinship_partial_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld,
                           double *S_dev);
/* S_dev: the (all-reduced) sum.  force_m < 0 => m by the cumulative-variance rule
 * (ols.rs:297-311) on eigenvalues sorted descending (the reference's stated intent, :296);
 * force_m >= 0 overrides it.  Y (host, n x k row-major) must have no NaN (remove_missing is the
 * caller's job, ols.rs:287).  Outputs (host, optional): m_out, K_out n x n, evals_out n. */
int pg_kinship_set(pg_ctx *ctx, const double *S_dev, int64_t p_total, int n, const double *Y,
                   int k, double var_explained, int force_m, int *m_out, double *K_out,
                   double *evals_out);
/* Same as pg_kinship_set but with caller-provided covariates C (host, n x m row-major) instead
 * of kinship eigenvectors; m = 0 gives plain y ~ [1 | g]. */
int pg_covariates_set(pg_ctx *ctx, int n, const double *C, int m, const double *Y, int k);
/* beta/var/pval: p x k row-major on the device; NaN where the reference's fit fails. */
int pg_ols_sweep_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld,
                     double *beta_dev, double *var_dev, double *pval_dev);
/* All three stages in one call.  K_out (host, n x n) is optional, and leaving it NULL (with force_m < 0) permits the LAZY route:
 * the n_eigenvecs rule (gwas/ols.rs:297-311) yields m = 0 as soon as lambda_1 / trace(K) >= var_explained, and
 * lambda_1 >= 1'K1 / n = sum_l (sum_i g_li)^2 / (n p) for any K, so when that bound clears var_explained by 1e-9 (an uncentred
 * kinship of allele frequencies: always) the intercept-only sweep alone -- ONE pass over G, no kinship matrix -- gives the
 * analysis' beta / var / pval (bit-identical to pg_kinship_partial_dev + pg_kinship_set + pg_ols_sweep_dev without fused sums);
 * otherwise the full route runs.  POOLGEN_NO_LAZY_KINSHIP=1 disables it. */
int pg_ols_kinship_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld,
                       const double *Y, int k, double var_explained, int force_m, int *m_out,
                       double *K_out, double *beta_dev, double *var_dev, double *pval_dev);
/* Host-buffer form (PCIe inclusive; what main.rs:285-291 hands over): G, beta, var, pval on the host.  G crosses the
 * bus ONCE, in slabs (default 256 MB, POOLGEN_HOST_SLAB_MB) on a copy stream while the partial kinship of the slab
 * that has landed runs; the matrix stays resident in HBM; after the n x n step the sweep runs slab by slab and the
 * results of slab s return while slab s + 1 is swept.  A pinned caller buffer (hipHostMalloc / hipHostRegister) is
 * used as is; pageable pages are pinned in place by the runtime.  The link sets the pace: ~0.3 s for the 16 GB of
 * 200 pools x 10 M loci against 10 ms of kernels. */
int pg_ols_kinship(pg_ctx *ctx, const double *G, int64_t p, int n, int64_t ld, const double *Y,
                   int k, double var_explained, int force_m, int *m_out, double *K_out,
                   double *beta, double *var, double *pval);

/* mle_iter_with_kinship == gwas::mle_with_covariate (gwas/mle.rs:307-463): the same kinship preamble (:317-343), then per
 * (column, trait) a Nelder-Mead maximum-likelihood fit of y ~ [1 | C | g] on (logit-bounded sigma^2, b) (mle.rs:13-30, :84-115;
 * argmin 0.8, start simplex of base/helpers.rs:132-146, <= 1000 iterations), ve = sigma^2, v_b = ve [(X'X)^-1]_last,
 * t = b / v_b as written (:175), p = 2 (1 - T_{n-1}(|t|)).  PARITY UNPINNED: the reference has no test of this path and the
 * solver's source is not in its tree; the published algorithm is restated (here and, literally, in the oracle) and the two
 * agree at the solver's resolution (~1e-6), not at 1e-10.  Up to 8 kinship covariates (10 design columns: what the eigen rule can
 * hand the sweep as well), k <= 4 traits.  With 3 and more covariates the 1000-iteration cap ends the simplex before it has
 * converged, in the reference as here (tests/test_gpu_mle.py).
 * beta/var/pval: p x k on the device. */
int pg_mle_kinship_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y, int k,
                       double var_explained, int force_m, int *m_out, double *K_out, double *beta_dev, double *var_dev,
                       double *pval_dev);

/* ---------------------------------------------------------------------------------------
 * Multi-GPU: loci shard over the GPUs of a node in contiguous slabs, one pg_ctx (= one GPU, one host thread or
 * process) per rank.  The reference's parallel axis is the same one -- a worker per file chunk (base/sync.rs:913-939)
 * -- and the only quantity that needs every worker's loci is the kinship sum (gwas/ols.rs:291-295): ONE in-place
 * RCCL all-reduce(sum) of n x n doubles over xGMI (320 KB at n = 200: latency-bound).  Outputs stay sharded (rank
 * order = locus order).  ols_iter / pearson_corr / chisq_test need no exchange at all.
 *   bootstrap: one rank calls pg_comm_unique_id and hands the PG_COMM_ID_BYTES to the others by any means (threads
 *   of one process: shared memory; processes: a file, MPI, a torch.distributed store); then EVERY rank calls
 *   pg_comm_init_rank(ctx, id, nranks, rank) -- collective, like ncclCommInitRank.  RCCL itself is loaded on first use.
 * pg_allreduce_sum_dev is the identity on a context without communicator, so single-GPU callers may use the
 * sharded entry point unchanged.
 * ------------------------------------------------------------------------------------- */
#define PG_COMM_ID_BYTES 128
int pg_comm_unique_id(void *id_out);
int pg_comm_init_rank(pg_ctx *ctx, const void *id, int nranks, int rank);
int pg_comm_destroy(pg_ctx *ctx);
int pg_comm_size(const pg_ctx *ctx);
int pg_comm_rank(const pg_ctx *ctx);
int pg_comm_version(int *version_out); /* ncclGetVersion of the RCCL that was loaded */
/* In-place sum over the ranks, enqueued on the context's stream (ordered with the kernels around it). */
int pg_allreduce_sum_dev(pg_ctx *ctx, double *buf_dev, int64_t count);
/* One rank's share of ols_iter_with_kinship: partial kinship of its p_local columns -> all-reduce -> the n x n
 * step with p_total (every rank computes the same m, basis and projected phenotypes) -> sweep of its own slab.
 * beta/var/pval: p_local x k on this rank's device. */
int pg_ols_kinship_sharded_dev(pg_ctx *ctx, const double *G_dev, int64_t p_local, int64_t p_total, int n, int64_t ld,
                               const double *Y, int k, double var_explained, int force_m, int *m_out, double *K_out,
                               double *beta_dev, double *var_dev, double *pval_dev);

/* ---------------------------------------------------------------------------------------
 * Sync-derived per-locus operators.  The reference calls these once per text line through
 * ChunkyReadAnalyseWrite::read_analyse_write (base/structs_and_traits.rs:245-265,
 * base/sync.rs:864, :674); here one call handles a batch of L parsed loci.
 * counts: L x n x 6 uint32, locus-major, sync column order A,T,C,G,N,D (base/sync.rs:134); every count below 2^29
 *   (the streaming pass sums coverages as integers; a larger count fails the call with PG_ERR_INVALID).  The *_dev forms (and
 *   pg_load_plan_dev) require counts_dev to be 16-BYTE ALIGNED (PG_ERR_INVALID otherwise: the streaming pass reads 16-byte
 *   pieces; a hipMalloc'ed buffer always is, a view that starts at an odd locus of a batch with odd n is not -- copy it).
 *   Nothing behind the L * n * 24 bytes of the batch is ever interpreted, whatever it holds.
 *   Real counts carry reads of alleles the MAF filter drops, and the reference recomputes the frequencies on the FILTERED
 *   counts (gwas/ols.rs:210-230 -> base/sync.rs:166-192), so those reads change every denominator: the streaming pass closes
 *   such loci in place whenever exactly two alleles survive; pg_locus_op_stats says how many loci needed the second pass.
 * pool_sizes: host, n (normalised or not -- only ratios are used, sync.rs:266-268).
 * Outputs are struct-of-arrays, SLOT-MAJOR (a locus emits up to PG_MAX_OUT rows = slots):
 *   n_out[L]            int32  rows emitted per trait (0 = locus dropped = None)
 *   allele_ids[5*L]     int32  index into "ATCGND"; element (slot r, locus l) at r*L + l
 *   mean_freq[5*L]      double element (r, l) at r*L + l
 *   stat[5*L*k], pval[5*L*k] double  element (r, l, trait t) at (r*L + l)*k + t
 * Only the slots r < n_out[l] of a locus are specified (chisq_test: one row per locus whose allele list occupies the
 * allele_ids slots r < n_out[l]; its stat / pval are plain [L] arrays).  A biallelic locus emits one row and touches slot 0
 * only: the operators write 32 instead of 144 bytes per locus, and a caller that wants rows copies slot 0 and, where
 * n_out > 1, the further slots.
 * ------------------------------------------------------------------------------------- */
/* gwas::ols_iterate (gwas/ols.rs:201-276): stat = beta. */
int pg_ols_iter_batch_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n,
                          const double *pool_sizes, const pg_filter *filter, const double *Y, int k,
                          int32_t *n_out_dev, int32_t *allele_ids_dev, double *mean_freq_dev,
                          double *stat_dev, double *pval_dev);
/* gwas::correlation (gwas/correlation_test.rs:73-129): stat = Pearson r (rounded to 7 dp as the
 * reference's pearsons_correlation returns it, :70). */
int pg_pearson_batch_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n,
                         const double *pool_sizes, const pg_filter *filter, const double *Y, int k,
                         int32_t *n_out_dev, int32_t *allele_ids_dev, double *mean_freq_dev,
                         double *stat_dev, double *pval_dev);
/* tables::chisq (tables/chisq_test.rs:5-47): n_out = number of alleles kept (all are listed in
 * allele_ids), chi2[L], pval[L]. */
int pg_chisq_batch_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n,
                       const double *pool_sizes, const pg_filter *filter, int32_t *n_out_dev,
                       int32_t *allele_ids_dev, double *chi2_dev, double *pval_dev);
/* tables::fisher (tables/fisher_exact_test.rs:32-130): n_out = alleles kept (listed in allele_ids, slot-major),
 * p_observed[L], pval[L] = p_observed + p_extremes.  Slots / values of loci with n_out == 0 are unspecified.
 * The table is the FILTERED COUNTS (n pools x surviving alleles), scaled to at most 34 reads when it holds more
 * (coef = 34 / total, cell = floor(cell * coef), :50-58); p_observed = the hypergeometric ratio of that table, p_extremes =
 * the sum of the ratio over the n * p tables the reference rebuilds (:72-118; duplicates counted as often as they occur, so
 * pval may exceed 1).  A locus' result depends on its counts, the filter and n only -- not on the batch or the context. */
int pg_fisher_batch_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n, const double *pool_sizes,
                        const pg_filter *filter, int32_t *n_out_dev, int32_t *allele_ids_dev,
                        double *p_observed_dev, double *pval_dev);
/* The loader, FileSyncPhen::load + into_genotypes_and_phenotypes (base/sync.rs:972-1180), on counts that
 * are already in HBM: per locus LocusCounts::filter (:195-303) -> to_frequencies over the surviving
 * alleles (:166-192) -> with keep_p_minus_1 sort by decreasing frequency and drop the first allele
 * (:1033-1037).  One column of G per surviving allele, loci in the caller's order (`order_dev`: a
 * permutation of 0..L-1, e.g. the (chromosome, position) sort of :1092-1101; NULL = input order).
 * Two calls because the column count is a result:
 *   pg_load_plan_dev  runs the filter for every locus and returns the number of columns p;
 *   pg_load_emit_dev  (directly afterwards, same ctx) writes G (p x ld, locus-major, pools kept =
 *                     pool_map[i] >= 0 at row position pool_map[i]; NULL = all pools), and for every
 *                     column the locus it came from and its allele (index into "ATCGND").
 * The coverage matrix the reference also fills (:1157-1167) is not produced (nothing on this path
 * reads it). */
int pg_load_plan_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n, const double *pool_sizes,
                     const pg_filter *filter, int keep_p_minus_1, const int64_t *order_dev, int64_t *p_out);
int pg_load_emit_dev(pg_ctx *ctx, const int32_t *pool_map, int n_out, double *G_dev, int64_t ld,
                     int64_t *col_locus_dev, int32_t *col_allele_dev);
/* Counts stored as 16-bit integers (the host parser's compact form: half the bytes to pin and to copy) -> the 32-bit
 * L x n x 6 layout every operator reads.  Both buffers on the device, 16-byte aligned; n_values = L * n * 6. */
int pg_expand_counts_u16_dev(pg_ctx *ctx, const uint16_t *src_dev, int64_t n_values, uint32_t *dst_dev);
/* pg_load_emit_dev that also writes the coverages GenotypesAndPhenotypes carries (sync.rs:1129-1152): cov_dev is
 * p x ld like G; every column row of a locus holds, per pool, the depth summed over the locus' surviving alleles. */
int pg_load_emit_cov_dev(pg_ctx *ctx, const int32_t *pool_map, int n_out, double *G_dev, int64_t ld,
                         int64_t *col_locus_dev, int32_t *col_allele_dev, double *cov_dev);
/* Host-buffer forms of the batch operators (H2D/D2H inside). */
int pg_ols_iter_batch(pg_ctx *ctx, const uint32_t *counts, int64_t L, int n,
                      const double *pool_sizes, const pg_filter *filter, const double *Y, int k,
                      int32_t *n_out, int32_t *allele_ids, double *mean_freq, double *stat,
                      double *pval);
int pg_pearson_batch(pg_ctx *ctx, const uint32_t *counts, int64_t L, int n,
                     const double *pool_sizes, const pg_filter *filter, const double *Y, int k,
                     int32_t *n_out, int32_t *allele_ids, double *mean_freq, double *stat,
                     double *pval);
int pg_chisq_batch(pg_ctx *ctx, const uint32_t *counts, int64_t L, int n, const double *pool_sizes,
                   const pg_filter *filter, int32_t *n_out, int32_t *allele_ids, double *chi2,
                   double *pval);
int pg_fisher_batch(pg_ctx *ctx, const uint32_t *counts, int64_t L, int n, const double *pool_sizes,
                    const pg_filter *filter, int32_t *n_out, int32_t *allele_ids, double *p_observed,
                    double *pval);

/* gwas::gwalpha_ls / gwalpha_ml (gwas/gwalpha.rs:281-380; CLI main.rs:335-356): per locus filter -> to_frequencies ->
 * sort_by_allele_freq(decreasing) -> drop the first allele (:176-196); per kept allele (= row = slot) two Beta distributions are
 * fitted to the cumulative allele distribution over the phenotype-ranked pools (:227-279) by Nelder-Mead (argmin 0.8 as
 * pg_mle_kinship_dev words it, start simplex prepare_solver_neldermead(4, 1), <= 1000 iterations) on the four logit-bounded
 * shapes in [EPSILON, 10], cost = least squares (:11-41) or -log10 likelihood (:43-79), and
 *   alpha = 2 sqrt(p_a (1 - p_a)) (mu_A - mu_B) / sig,  mu = min + (max - min) s0 / (s0 + s1)      (:314-316).
 * bins (host, n): the pools' shares; they are also the pool sizes the filter sees (main.rs:210, phen.rs:157).  q (host, n):
 * column 1 of the reference's phenotype matrix AS HANDED OVER (the gwalpha_fmt parser has normalised it once already,
 * phen.rs:139-142); the operator applies q'_0 = 0, q'_i = (q_i - min) / (max - min) to it as written (:248-251).  n >= 3
 * (the reference's phenotype matrix does not match the counts below that and check() panics): PG_ERR_INVALID otherwise.
 * Outputs slot-major as above: n_out[L], allele_ids / mean_freq / alpha [5*L]; optional (NULL = not wanted) what makes a fit
 * checkable: shapes[(r*L + l)*4 + c] the fit's final bounded shapes (A: c = 0, 1; B: c = 2, 3), cost[r*L + l] its lowest cost,
 * iters[r*L + l] the iterations done (1000 = the cap ended it).
 * A row whose p_a = sum_i f_i bins_i is 0, 1 or NaN has no defined cost in the reference (bins_a or bins_b are 0/0; statrs
 * panics on the NaN percentile): alpha, shapes and cost are NaN and iters 0 there.  Such a row needs --min-allele-frequency 0
 * (an allele nobody carries survives) or a pool without reads under a filter that lets it pass (min_coverage_depth 0 and
 * max_missingness_rate > 0).
 * A row's result depends on its counts, the filter, bins, q, sig, min, max, method and n only -- not on the batch. */
enum { PG_GWALPHA_LS = 0, PG_GWALPHA_ML = 1 };
int pg_gwalpha_batch_dev(pg_ctx *ctx, const uint32_t *counts_dev, int64_t L, int n, const double *bins, const double *q,
                         double sig, double min, double max, const pg_filter *filter, int method, int32_t *n_out_dev,
                         int32_t *allele_ids_dev, double *mean_freq_dev, double *alpha_dev, double *shapes_dev,
                         double *cost_dev, int32_t *iters_dev);
int pg_gwalpha_batch(pg_ctx *ctx, const uint32_t *counts, int64_t L, int n, const double *bins, const double *q, double sig,
                     double min, double max, const pg_filter *filter, int method, int32_t *n_out, int32_t *allele_ids,
                     double *mean_freq, double *alpha, double *shapes, double *cost, int32_t *iters);
/* out[i] = Beta(a[i], b[i]).cdf(x[i]) as the fit evaluates it: 0 for x <= 0, 1 for x >= 1, else statrs' beta_reg (modified
 * Lentz continued fraction, <= 140 iterations, symmetry switch at (a + 1) / (a + b + 2)); NaN for a or b not > 0 or a NaN x. */
int pg_beta_reg_dev(pg_ctx *ctx, const double *a_dev, const double *b_dev, const double *x_dev, int64_t count, double *out_dev);

/* ---------------------------------------------------------------------------------------
 * Genomic prediction: gp::ols (gp/ols.rs:8-101) for the n < p case, b = X^T pinv(X X^T) y,
 * with X = [1 | G^T] (intercept implicit).  beta_dev: (1+p) x k row-major, row 0 = intercept.
 * row_idx: host, training rows (the reference's `row_idx: &Vec<usize>`).
 * pg_gp_xxt_dev exposes the full-data X X^T (n x n, incl. intercept) so that every training
 * subset's X X^T can be taken as a principal sub-block without another pass over G.
 * ------------------------------------------------------------------------------------- */
int pg_gp_xxt_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, double *XXt_dev);
int pg_gp_ols_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y,
                  int k, const int64_t *row_idx, int n_rows, const double *XXt_host_or_null,
                  double *beta_dev);

/* gp::penalise_ridge_like (gp/penalise.rs:133-159) = the lambda path with k-fold cross-validation
 * (:461-669) at alpha = 0, generalised to 0 <= alpha <= 1 (alpha = 1 is penalise_lasso_like, :101-130).
 * The reference draws its folds from an unseeded RNG (:452-453); here they are explicit:
 * fold_of[rep * n_rows + i] in 0..n_folds-1 is the fold of pool row_idx[i] in repetition rep; the value
 * n_folds marks the left-over group k_split makes (:444-448), which trains in every fold and is never validated.
 * lambda path = {0, step, 2 step, ..., 1} (step 0.1 in the reference).  Outputs: beta_dev (1+p) x k
 * (penalised coefficients of the all-rows fit, row 0 = intercept), lambdas_out[k] (host), optional
 * perf_out (host, n_reps x n_folds x L x k error indices, :359-426).
 * Device memory beside G: the slopes of every fold's fit of every repetition and of the all-rows fit stay resident while the
 * repetitions are scored -- (n_reps * n_folds * k + k) * p doubles (BASELINE configs[3]: 101 x 40 MB) -- so that they can be
 * formed 16 columns per pass over G whatever repetition they belong to; when that is more than half of the free device memory
 * (or with POOLGEN_RIDGE_PER_REP=1) one repetition's n_folds * k columns are resident at a time and every repetition costs a
 * pass of its own.  Same results, bit for bit.
 * Every fit on every path (folds, all-rows fit, per-fold and per-repetition fallbacks) takes gp::ols' branch from n and p as
 * pg_gp_ols_dev does: a tall design (n >= p + 1) is fitted by pinv(X'X) X'y, one fold at a time. */
int pg_gp_ridge_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y,
                    int k, const int64_t *row_idx, int n_rows, const int32_t *fold_of, int n_reps,
                    int n_folds, double alpha, double lambda_step, double *beta_dev,
                    double *lambdas_out, double *perf_out);
/* The whole family behind penalised_lambda_path_with_k_fold_cross_validation (gp/penalise.rs:461-669):
 *   alpha in [0, 1], iterative_proxy = 0 : pg_gp_ridge_dev (penalise_lasso_like alpha = 1, penalise_ridge_like alpha = 0);
 *   alpha < 0                            : penalise_glmnet (:168-195): the grid alpha x lambda over the same path values
 *                                          (:479-498), alpha and lambda chosen by separate mode counts (:605-627);
 *   iterative_proxy != 0                 : the *_with_iterative_proxy_norms models (:197-246): the penalised set is
 *                                          picked by the norms of pg_gp_proxy_dev's coefficients (fitted once on
 *                                          row_idx, :543, :656), the amounts by the fit's own norms (:262-283).
 * alphas_out[k] (host, optional), lambdas_out[k]; perf_out (optional) n_reps x n_folds x A x L x k, A = 1 or L.
 * The covariate state of ctx (pg_covariates_set / pg_kinship_set) is gone afterwards, with or without iterative_proxy:
 * pg_ols_sweep_dev fails with PG_ERR_STATE until it is set again (the same holds after pg_gp_ols_dev, pg_gp_ridge_dev and
 * pg_mle_kinship_dev, whose coefficient passes use the same device table).
 * XXt_host_or_null: the full-data X X^T of pg_gp_xxt_dev (host, n x n) when the caller already has it -- a harness that
 * fits many models on the same genotypes computes it once. */
int pg_gp_penalised_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y,
                        int k, const int64_t *row_idx, int n_rows, const int32_t *fold_of, int n_reps,
                        int n_folds, double alpha, int iterative_proxy, double lambda_step, double *beta_dev,
                        double *alphas_out, double *lambdas_out, double *perf_out, const double *XXt_host_or_null);
/* gp::ols_iterative_with_kinship_pca_covariate (gp/ols.rs:104-199): proxy_dev (1+p) x k on the device, row 0 = the
 * trait means over the training pools, row 1+l = the locus coefficient of y ~ [1 | PC1 | g_l] on the training pools
 * (PC1: leading eigenvector of the reference's centred X X^T of those pools, :115-141, with its two indexing quirks:
 * columns = intercept and all loci but the last; means over the first n_rows pools).  Overwrites ctx's covariates and leaves
 * none: pg_ols_sweep_dev fails with PG_ERR_STATE until pg_covariates_set / pg_kinship_set is called again. */
int pg_gp_proxy_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Y, int k,
                    const int64_t *row_idx, int n_rows, const double *XXt_host_or_null, double *proxy_dev);
/* yhat (n x k, host) = X beta for EVERY pool, X = [1 | G^T], beta (1+p) x k on the device: the prediction step of
 * the cross-validation harness (multiply_views_xx in gp/cv.rs:160-168); the caller reads the validation rows. */
int pg_gp_predict_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *beta_dev,
                      int k, double *yhat);

/* ---------------------------------------------------------------------------------------
 * popgen on the loader's matrix: fst (popgen/fst.rs:10-115, :158-200) and
 * theta_pi / `heterozygosity` (popgen/pi.rs:10-113).  G and cov as written by pg_load_emit_cov_dev
 * (all alleles kept); locus_col (host, L + 1 entries, 0 .. p): the first column of every locus =
 * count_loci (sync.rs:73-97) minus the intercept; windows = inclusive locus index ranges from
 * pg_host_sliding_windows = define_sliding_windows (base/helpers.rs:294-403; chromosomes as ids,
 * only equality is used; head/tail need room for L entries; returns the number of windows).
 *   pg_pi_dev : pi_win (host, n_windows x n) per-window means, pi_mean (host, n) their mean (:133).
 *   pg_fst_dev: fst_mean (host, n x n) mean over all loci (:145), fst_win (host, n_windows x n*n);
 *               fails with PG_ERR_INVALID where the reference's assert does (a locus whose
 *               frequencies do not sum to one in every pool, :66).
 * Each is its tables form (below) plus the copy to the host: pg_pi_dev into device memory of its own;
 * pg_fst_dev window slab by window slab, never more than 2^30 bytes of fst_win on the device.
 * ------------------------------------------------------------------------------------- */
int64_t pg_host_sliding_windows(const int32_t *chr_id, const uint64_t *pos, int64_t L, uint64_t window_size_bp,
                                uint64_t window_slide_size_bp, uint64_t min_loci_per_window, int64_t *head,
                                int64_t *tail);
int pg_pi_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
              const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
              int64_t n_windows, double *pi_win, double *pi_mean);
int pg_fst_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
               const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
               int64_t n_windows, double *fst_mean, double *fst_win);
/* The tables forms: the same arguments, but the outputs are DEVICE memory of the same shapes, so a table can go on to
 * pg_gudmc_dev or to pg_f64_table_dev without touching the host.  They are the one device path of these statistics: a host form
 * above runs the same refusals and the same kernels and copies the results down, so the two forms agree in every bit.  The means
 * across windows are summed on the device, left to right; pg_fst_tables_dev's slabs of windows write straight into fst_win_dev.
 * Every form has returned only when its work on the device is done.  (pg_watterson_tables_dev, pg_tajima_d_tables_dev: below.) */
int pg_pi_tables_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                     const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                     int64_t n_windows, double *pi_win_dev, double *pi_mean_dev);
int pg_fst_tables_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                      const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                      int64_t n_windows, double *fst_mean_dev, double *fst_win_dev);

/* ---------------------------------------------------------------------------------------
 * watterson_estimator (popgen/watterson_theta.rs:8-188) and tajima_d (popgen/tajima_d.rs:10-96) on
 * the same matrix and windows.  A (locus, pool) is polymorphic iff no frequency of the locus is
 * >= 1.0 in the pool (:8-30; NaN never wins the fold, so an all-NaN pool counts).  Per window and
 * pool, theta_W = (S / cov) / a1 with a1 = sum_{x = 1}^{(pool_size as usize) - 1} 1/x (:175-182);
 * D = (pi - theta_W) / sqrt(e1 s + e2 s (s - 1)), s = theta_W / a1, with the reference's guards
 * (tajima_d.rs:51-96); pi is pg_pi_dev's, from the same pass over G.
 * Two ways to count S:
 *   reference: what the reference's loop ends up with, S = poly(seed) + (cov - 1) * poly(slot) --
 *              it evaluates the flag at the window's index, not at the locus (:107-137);
 *   counted  : S = the polymorphic loci of head .. tail, cov = tail - head + 1.
 * pool_sizes are used as given (the reference's CLI hands in fractions that sum to one, so that
 * a1 = 0 and every value is inf or NaN, main.rs:463, phen.rs:83-84); sizes above 1e9 are refused.
 * A window with tail < head (the stale tail of a ditched slot; the reference panics) is refused
 * with PG_ERR_INVALID, as is n_windows < 1.
 * ------------------------------------------------------------------------------------- */
/* theta_watterson's own window loop (watterson_theta.rs:56-164): head/tail as pg_host_sliding_windows, plus per kept
 * window the loci counted (cov), the locus its count starts from (seed) and its index in the unfiltered window list
 * (slot): S = poly(seed) + (cov - 1) * poly(slot) is the reference's count (:107-137).  Arrays need room for L. */
int64_t pg_host_watterson_windows(const int32_t *chr_id, const uint64_t *pos, int64_t L, uint64_t window_size_bp,
                                  uint64_t window_slide_size_bp, uint64_t min_loci_per_window, int64_t *head,
                                  int64_t *tail, int64_t *cov, int64_t *seed, int64_t *slot);
/* win_cov, win_seed, win_slot all NULL = counted mode.  pool_sizes: host, n, used as given.
 * theta_win n_windows x n, theta_mean n, seg_win (optional) n_windows x n counts S.
 * The host form of pg_watterson_tables_dev: that into device memory of its own, then the copy down. */
int pg_watterson_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L,
                     const int64_t *win_head, const int64_t *win_tail, const int64_t *win_cov, const int64_t *win_seed,
                     const int64_t *win_slot, int64_t n_windows, const double *pool_sizes, double *theta_win,
                     double *theta_mean, int64_t *seg_win);
/* d_win n_windows x n, d_mean n; theta_win / pi_win optional outputs of the same pass.
 * The host form of pg_tajima_d_tables_dev, as above. */
int pg_tajima_d_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                    const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                    const int64_t *win_cov, const int64_t *win_seed, const int64_t *win_slot, int64_t n_windows,
                    const double *pool_sizes, double *d_win, double *d_mean, double *theta_win, double *pi_win);
/* The tables forms of the two (see pg_pi_tables_dev), which the host forms above copy from: outputs on the device, the
 * optional ones may be NULL as above. */
int pg_watterson_tables_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L,
                            const int64_t *win_head, const int64_t *win_tail, const int64_t *win_cov, const int64_t *win_seed,
                            const int64_t *win_slot, int64_t n_windows, const double *pool_sizes, double *theta_win_dev,
                            double *theta_mean_dev, int64_t *seg_win_dev);
int pg_tajima_d_tables_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                           const int64_t *locus_col, int64_t L, const int64_t *win_head, const int64_t *win_tail,
                           const int64_t *win_cov, const int64_t *win_seed, const int64_t *win_slot, int64_t n_windows,
                           const double *pool_sizes, double *d_win_dev, double *d_mean_dev, double *theta_win_dev,
                           double *pi_win_dev);

/* ---------------------------------------------------------------------------------------
 * gudmc (popgen/gudmc.rs:64-462): Tajima's D peaks and troughs against pairwise Fst.  The stage on top of
 * pg_tajima_d_dev and pg_fst_dev: Nelder-Mead normal fits (ml_normal_1d, :39-60; argmin 0.8 as pg_mle_kinship_dev
 * words it, start simplex prepare_solver_neldermead(2, 1), <= 10 000 iterations) on (mu, x),
 * sigma = EPSILON + (1e24 - EPSILON) / (1 + e^-x), cost = sum of -ln_pdf.  The cost is evaluated from the column's
 * (count, mean, sum (x - mean)^2), not as the reference's sum over the column: the simplex's path is chaotic under
 * last-bit changes of the cost, so mu and sigma agree with the reference at the solver's resolution (measured:
 * DESIGN.md section 3.4e), not bit for bit.
 * ------------------------------------------------------------------------------------- */
/* Per column of a row-major table on the device (rows x cols, pitch ld >= cols), over its non-NaN entries: the fitted
 * mu_dev[cols] and sd_dev[cols]; optional count_dev[cols] (non-NaN entries) and iters_dev[cols] (iterations done;
 * 10000 = the cap ended the fit).  A column without entries gives (1.5, sigma(1.0)) at 0 iterations, as the reference's
 * fold over an empty array does.  A +-inf entry has no defined cost (the reference panics): PG_ERR_INVALID.
 * A column's result depends on its entries alone -- not on cols, ld or the other columns. */
int pg_normal_fit_dev(pg_ctx *ctx, const double *table_dev, int64_t rows, int64_t cols, int64_t ld, double *mu_dev,
                      double *sd_dev, int64_t *count_dev, int32_t *iters_dev);
/* d_win_dev: w x n, D per window and population as pg_tajima_d_dev returns it (copied to the device); the entry rounds it
 * to 8 decimals, half away from zero, as the reference reads it back from tajima_d's file (tajima_d.rs:164).  fst_win_dev:
 * w x n*n as pg_fst_dev returns it, pair (a, b) in column a*n + b.  win_chr / win_ini / win_fin (host, w): the windows'
 * chromosome ids (only equality is used), first and last position.
 * Per population b, d = its non-NaN D in window order; ROW j of b takes the label of window j of the unfiltered list
 * (gudmc.rs:168-176: a NaN window in the middle shifts every later value to an earlier window; kept as the reference has
 * it), is significant iff |d_j - d_mean| >= sigma_threshold (not scaled by d_sd, :180), and has width 0, or
 * pos_fin - pos_ini plus the previous row's width when that row is on the same chromosome and reaches pos_ini (:180-208).
 * Outputs, all on the device:
 *   rows_dev[n] int64, d_mean_dev[n], d_sd_dev[n]                        per population
 *   fst_mean_dev, fst_sd_dev, width_mean_dev, width_sd_dev [n*n]        per pair (a, b); the width fit runs over b's rows
 *   row_* [n*n*w], pair-major with pitch w: element (pair i, row j) at i*w + j, specified for j < rows_dev[i % n] only:
 *     row_window (int64: the row's window = its Fst window), row_d, row_width (an integer, exact), row_width_from_r =
 *     width - (recombination_rate_cM_per_Mb / 100) * 1e6, row_width_p and row_fst_p (one-tailed: cdf below the mean, else
 *     1 - cdf, cdf = erfc((mean - x) / (sd sqrt 2)) / 2), row_fst_delta = fst - fst_mean.  Any row_* may be NULL.
 * Memory: the caller's seven row_* arrays are n*n*w * 8 bytes each (200 pools x 1 496 windows: 0.48 GB each, 3.4 GB in all);
 * the entry itself holds 2 w n + 3 n*n doubles beside them.
 * Errors: PG_ERR_INVALID for n < 1, w < 1, a +-inf among a population's D (or in Fst), and a significant row whose label has
 * pos_fin < pos_ini (the reference's unsigned subtraction overflows). */
int pg_gudmc_dev(pg_ctx *ctx, const double *d_win_dev, const double *fst_win_dev, int64_t w, int n, const int32_t *win_chr,
                 const uint64_t *win_ini, const uint64_t *win_fin, double sigma_threshold, double recombination_rate_cM_per_Mb,
                 int64_t *rows_dev, double *d_mean_dev, double *d_sd_dev, double *fst_mean_dev, double *fst_sd_dev,
                 double *width_mean_dev, double *width_sd_dev, int64_t *row_window_dev, double *row_d_dev,
                 double *row_width_dev, double *row_width_from_r_dev, double *row_width_p_dev, double *row_fst_delta_dev,
                 double *row_fst_p_dev);
/* The tables of the kept windows, as the tables entry points leave them on the device, into the tables of all w windows that
 * pg_gudmc_dev reads: row keep[q] of table_dev (w x cols) = row q of kept_dev (n_kept x cols), every other row NaN.  keep: host,
 * increasing, inside [0, w). */
int pg_window_scatter_dev(pg_ctx *ctx, const double *kept_dev, int64_t n_kept, const int64_t *keep, int64_t w, int64_t cols,
                          double *table_dev);

/* ---------------------------------------------------------------------------------------
 * sync2csv's writer (FileSyncPhen::write_csv, base/sync.rs:1182-1262): rows [row0, row0 + rows) of the loader's matrix as
 * the bytes of the allele-frequency CSV, one line per row: "chromosome,position,allele," + the n cells joined by ',' + '\n'
 * (no header line).  G, col_locus (int64) and col_allele (int32, index into "ATCGND") as pg_load_emit_dev writes them;
 * per locus its chromosome id (locus_chrom, int32) and position (locus_pos, uint64); the distinct chromosome names as one
 * byte string (chrom_text) with n_chrom + 1 int32 offsets (chrom_off).  A cell prints as parse_f64_roundup_and_own(x, 6)
 * (base/helpers.rs:103-117) does for a frequency: NaN -> "NaN"; else k = x * 1e6 rounded half away from zero, "0" for
 * k = 0, else the decimal of k / 10^6 and, when k % 10^6 != 0, "." and its six digits without trailing zeros.
 * *bytes is always set to the size the text needs; bytes > cap fails with PG_ERR_INVALID and writes nothing (cap = 0 is a
 * size query, text may then be NULL).  A cell outside [0, 1] that is not NaN fails the call with PG_ERR_INVALID (*bytes is
 * set as usual, the text is unspecified); so does a label out of range (the one case without a size: *bytes = 0).  Both
 * forms behave alike in all of this.  Nothing at or behind text[bytes] is written.
 * The device form formats on the GPU (three kernels on the context's stream; it synchronises once to read the size, and
 * the text is complete once the stream has passed the call); the host form is plain C++ on n_threads threads, no context.
 * ------------------------------------------------------------------------------------- */
int pg_csv_freq_rows_dev(pg_ctx *ctx, const double *G_dev, int64_t ld, int n, int64_t row0, int64_t rows,
                         const int64_t *col_locus_dev, const int32_t *col_allele_dev, const int32_t *locus_chrom_dev,
                         const uint64_t *locus_pos_dev, const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom,
                         char *text_dev, int64_t cap, int64_t *bytes);
int pg_host_csv_freq_rows(const double *G, int64_t ld, int n, int64_t row0, int64_t rows, const int64_t *col_locus,
                          const int32_t *col_allele, const int32_t *locus_chrom, const uint64_t *locus_pos,
                          const char *chrom_text, const int32_t *chrom_off, int n_chrom, char *text, int64_t cap,
                          int64_t *bytes, int n_threads);

/* ---------------------------------------------------------------------------------------
 * vcf2sync's reader (base/vcf.rs: lparse :12-68, filter :117-178, vcf_to_sync :182-230, per_chunk :268-300): a slab of VCF
 * text -- it starts at a line start, its last line may lack the newline -- to the allele counts of the loci the filter
 * keeps, in file order.  pool_sizes (host, n_sizes <= 2048 of them) and the three thresholds are FilterStats'.
 * Outputs, `kept` rows each:
 *   counts    uint32, kept x n_pools x 6, the six numbers of a pool in the order vcf_to_sync writes them (A:T:C:G:D:N; the
 *             sync reader reads the same positions back as A,T,C,G,N,D: quirk 13 of SURVEY.md)
 *   pos       uint64;  ref: the reference character ('D' for anything that is not one character)
 *   line_off  the byte offset of the line in the slab;  chrom_len: the length of its first field (the chromosome's name)
 * info->kept, data_lines (lines that do not start with '#'), n_pools (the sample fields of the data lines; 0 without data
 * lines), chrom_line_off (the last line that begins with "#CHROM", or -1).
 * Capacities: cap_loci rows of pos / ref / line_off / chrom_len, cap_counts elements of counts.  info->kept and n_pools are
 * always set; more rows or elements than the capacities hold fails with PG_ERR_INVALID and writes nothing (capacities of 0
 * are the size query, the output pointers may then be NULL).  Nothing at or behind the stated capacities is written.
 * Where the reference panics the call fails with PG_ERR_INVALID: info->err_line_off is the offset of the FIRST such line in
 * file order, info->err_reason the smallest pg_vcf_reason that holds of it (else -1 and 0); kept and n_pools are then 0.
 * Three reasons are deliberate deviations (the reference would go on): PG_VCF_E_COUNT32, PG_VCF_E_HIGH_BYTE, PG_VCF_E_POOLS.
 * The result does not depend on where a text is cut into slabs (the caller compares n_pools between slabs).
 * The device form parses on the GPU (index, parse, scan, emit on the context's stream; it synchronises to read the sizes,
 * and the rows are complete once the stream has passed the call); the host form is plain C++ on n_threads threads, no
 * context, and gives the same bytes.
 * ------------------------------------------------------------------------------------- */
enum pg_vcf_reason {
    PG_VCF_E_EMPTY = 1,      /* an empty line (per_chunk indexes its first byte) */
    PG_VCF_E_SHORT = 2,      /* a data line under 20 bytes (per_chunk slices &line[0..20] for its message before it parses) */
    PG_VCF_E_LONG = 3,       /* a line of 2^31 bytes or more (this library's limit) */
    PG_VCF_E_FIELDS = 4,     /* fewer than 9 tab-separated fields */
    PG_VCF_E_POS = 5,        /* POS is no u64 */
    PG_VCF_E_HIGH_BYTE = 6,  /* deviation: a byte >= 0x80 in REF or ALT (no UTF-8 decoding here) */
    PG_VCF_E_AD_KEY = 7,     /* FORMAT has no AD, or more than one */
    PG_VCF_E_POOLS = 8,      /* deviation: more samples than pool sizes, or not as many as the first data line has */
    PG_VCF_E_SUBFIELDS = 9,  /* a sample with too few ':' pieces to hold AD */
    PG_VCF_E_AD_VALUE = 10,  /* an AD value that is no u64 ("." among them) */
    PG_VCF_E_COUNT32 = 11,   /* deviation: an AD value above 2^32 - 1 (the counts are 32-bit) */
    PG_VCF_E_NO_SAMPLES = 12,/* no sample fields on a line that passes the breadth rule (to_counts indexes pool 0) */
    PG_VCF_E_AD_RAGGED = 13, /* a pool with fewer AD values than pool 0, on a line that passes the breadth rule */
    PG_VCF_E_ALLELE_OOB = 14 /* a kept line whose first A/T/C/G/D/N allele has no AD column in pool 0 */
};
typedef struct {
    int64_t kept;
    int64_t data_lines;
    int64_t chrom_line_off;
    int64_t err_line_off;
    int32_t n_pools;
    int32_t err_reason;
} pg_vcf_info;
int pg_vcf_parse_dev(pg_ctx *ctx, const char *text_dev, int64_t bytes, const double *pool_sizes, int n_sizes,
                     uint64_t min_coverage_depth, double min_coverage_breadth, double min_allele_frequency,
                     uint32_t *counts_dev, uint64_t *pos_dev, uint8_t *ref_dev, int64_t *line_off_dev, int32_t *chrom_len_dev,
                     int64_t cap_loci, int64_t cap_counts, pg_vcf_info *info);
int pg_host_vcf_parse(const char *text, int64_t bytes, const double *pool_sizes, int n_sizes, uint64_t min_coverage_depth,
                      double min_coverage_breadth, double min_allele_frequency, uint32_t *counts, uint64_t *pos, uint8_t *ref,
                      int64_t *line_off, int32_t *chrom_len, int64_t cap_loci, int64_t cap_counts, pg_vcf_info *info,
                      int n_threads);

/* ---------------------------------------------------------------------------------------
 * The sync reader (base/sync.rs: String::lparse :100-156, as the CLI's parse_sync_buffer restates it): a slab of sync text --
 * it starts at a line start, its last line may lack the newline, the pointer may have any alignment -- to the counts of its
 * loci, in file order.  expect_n: 0 = the pool count is that of the first data line of the slab, else the required count
 * (at most 4096; more is PG_ERR_INVALID before anything is launched).
 * The rules.  A line ends at '\n', one trailing '\r' is dropped.  A line starting with '#' is skipped.  A number is an
 * optional '+' and 1-19 decimal digits.  A line whose second field is no number is skipped, provided it has a second tab.
 * A pool is six or more numbers separated by ':'; the first six are stored (each at most 2^32 - 1), further ones are checked
 * and ignored.  The FIRST line of the slab that does not start with '#' fixes the pool count (its fields minus three) and
 * must have four fields or more and expect_n pools, even where its position is no number and the line is then skipped.
 * Outputs, `kept` rows each:
 *   counts    uint32, kept x n_pools x 6, the first six numbers of every pool at the positions they have in the text
 *   pos       uint64;  line_off: the byte offset of the line in the slab;  chrom_len: the length of its first field
 * info->kept, data_lines (lines that are not empty and do not start with '#'), n_pools (0 without such a line).
 * Capacities as for pg_vcf_parse_dev: cap_loci rows, cap_counts elements; 0 is the size query; too small a buffer fails with
 * PG_ERR_INVALID and writes nothing; nothing at or behind the stated capacities is written.
 * Where the CLI's host parser throws the call fails with PG_ERR_INVALID: info->err_line_off is the FIRST such line in file
 * order, info->err_reason the smallest pg_sync_reason that holds of it (of the pools only the first n_pools are looked at);
 * else -1 and 0.  kept and n_pools are then 0.
 * The device form works on the context's stream out of the context's workspace and synchronises only to read sizes; the rows
 * are complete once the stream has passed the call.  The host form is plain C++ on n_threads threads, needs no context, and
 * gives the same bytes.
 * ------------------------------------------------------------------------------------- */
enum pg_sync_reason {
    PG_SYNC_E_EMPTY = 1,   /* an empty line (or one that is only '\r') */
    PG_SYNC_E_FIELDS = 2,  /* fewer than four tab-separated fields */
    PG_SYNC_E_COUNT = 3,   /* a count that is no number, or a pool with fewer than six */
    PG_SYNC_E_COUNT32 = 4, /* one of a pool's first six counts is above 2^32 - 1 */
    PG_SYNC_E_POOLS = 5,   /* another number of pools than the first data line's or expect_n, or more than 4096 */
    PG_SYNC_E_LONG = 6     /* a line of 2^31 bytes or more (this library's limit) */
};
typedef struct {
    int64_t kept;
    int64_t data_lines;
    int64_t err_line_off;
    int32_t n_pools;
    int32_t err_reason;
} pg_sync_info;
int pg_sync_parse_dev(pg_ctx *ctx, const char *text_dev, int64_t bytes, int expect_n, uint32_t *counts_dev, uint64_t *pos_dev,
                      int64_t *line_off_dev, int32_t *chrom_len_dev, int64_t cap_loci, int64_t cap_counts, pg_sync_info *info);
int pg_host_sync_parse(const char *text, int64_t bytes, int expect_n, uint32_t *counts, uint64_t *pos, int64_t *line_off,
                       int32_t *chrom_len, int64_t cap_loci, int64_t cap_counts, pg_sync_info *info, int n_threads);

/* ---------------------------------------------------------------------------------------
 * pileup2sync's reader (base/pileup.rs: String::lparse :11-168, PileupLine::filter :240-334, to_counts :172-215, as the CLI's
 * PileupConverter::decode restates them): a slab of samtools mpileup text -- it starts at a line start, its last line may
 * lack the newline, the pointer may have any alignment -- to the allele counts of the loci the filter keeps, in file order.
 * pool_sizes (host, n_sizes of them; more than 4096 is PG_ERR_INVALID before anything is launched), remove_ns,
 * keep_lowercase_reference, max_base_error_rate and the three thresholds are FilterStats' fields.
 * The rules.  A line ends at '\n', one trailing '\r' is dropped; there are no comments, and an empty line has too few fields.
 * A number is an optional '+' and 1-19 decimal digits.  Pools are triples of fields (coverage, reads, qualities) behind the
 * third field; a line with another number of pools than n_sizes is checked in full and then dropped.  A pool of coverage 0 is
 * not looked at beyond its coverage.  In the read string '+' / '-' start a decimal length (leading zeros are skipped; the
 * first non-digit ends the number and is the first of the `length` bytes skipped, the skip stops at the field end), '^'
 * skips the byte behind it, '$' is dropped; '.' and ',' are the reference byte as the line writes it, every other byte goes
 * through lparse's table (anything unknown is N).  Read j pairs with quality byte j: a quality below 33 drops the line, a
 * quality whose error rate 10^(-(q-33)/10) exceeds max_base_error_rate makes the read an N, and Ns vanish under remove_ns.
 * Then the breadth rule on the sums that are left (ceil(min_coverage_breadth x n_sizes) pools of min_coverage_depth or more)
 * and the frequency rule on column T, q = the sum in pool order of the separately rounded (count / sum) x pool_size; a pool
 * with nothing left makes q NaN, which passes.
 * Outputs, `kept` rows each:
 *   counts    uint32, kept x n_sizes x 6 at the positions pileup_to_sync writes (A:T:C:G:D:N)
 *   pos       uint64;  ref: the reference byte
 *   line_off  the byte offset of the line in the slab;  chrom_len: the length of its first field (the chromosome's name)
 * info->kept, lines (all lines of the slab).  Capacities as for pg_vcf_parse_dev: cap_loci rows, cap_counts elements; 0 is the
 * size query; too small a buffer fails with PG_ERR_INVALID and writes nothing; nothing at or behind the capacities is written.
 * Where the reference panics the call fails with PG_ERR_INVALID: info->err_line_off is the FIRST such line in file order,
 * info->err_reason a pg_pileup_reason (else -1 and 0), kept is then 0.  A pool reports the first defect its walk meets (COV,
 * RAGGED, INDEL, MISMATCH in that order), the line the smallest code among its first three fields' and its pools'.
 * The result does not depend on where a text is cut into slabs at line starts.
 * The device form works on the context's stream out of the context's workspace (index, scan, parse, scan, emit) and
 * synchronises only to read sizes; the rows are complete once the stream has passed the call.  The host form is plain C++ on
 * n_threads threads, needs no context, and gives the same bytes and the same info.
 * ------------------------------------------------------------------------------------- */
enum pg_pileup_reason {
    PG_PILEUP_E_LONG = 1,    /* a line of 2^31 bytes or more (this library's limit) */
    PG_PILEUP_E_FIELDS = 2,  /* fewer than three tab-separated fields (an empty line too) */
    PG_PILEUP_E_POS = 3,     /* the position is no number */
    PG_PILEUP_E_REF = 4,     /* the reference allele is not one byte below 0x80 */
    PG_PILEUP_E_COV = 5,     /* a pool's coverage is no number */
    PG_PILEUP_E_RAGGED = 6,  /* a pool without its read or its quality field */
    PG_PILEUP_E_INDEL = 7,   /* coverage > 0: a non-digit where the length behind '+' / '-' must start */
    PG_PILEUP_E_MISMATCH = 8 /* coverage > 0: the reads or the quality bytes are not as many as the coverage says */
};
typedef struct {
    int64_t kept;
    int64_t lines;
    int64_t err_line_off;
    int32_t err_reason;
    int32_t reserved;
} pg_pileup_info;
int pg_pileup_parse_dev(pg_ctx *ctx, const char *text_dev, int64_t bytes, const double *pool_sizes, int n_sizes, int remove_ns,
                        int keep_lowercase_reference, double max_base_error_rate, uint64_t min_coverage_depth,
                        double min_coverage_breadth, double min_allele_frequency, uint32_t *counts_dev, uint64_t *pos_dev,
                        uint8_t *ref_dev, int64_t *line_off_dev, int32_t *chrom_len_dev, int64_t cap_loci, int64_t cap_counts,
                        pg_pileup_info *info);
int pg_host_pileup_parse(const char *text, int64_t bytes, const double *pool_sizes, int n_sizes, int remove_ns,
                         int keep_lowercase_reference, double max_base_error_rate, uint64_t min_coverage_depth,
                         double min_coverage_breadth, double min_allele_frequency, uint32_t *counts, uint64_t *pos, uint8_t *ref,
                         int64_t *line_off, int32_t *chrom_len, int64_t cap_loci, int64_t cap_counts, pg_pileup_info *info,
                         int n_threads);

/* ---------------------------------------------------------------------------------------
 * The sync writer of pileup2sync and vcf2sync (pileup_to_sync, base/pileup.rs:348-371; vcf_to_sync, base/vcf.rs:212-229): the
 * rows the three parsers above leave -- counts (rows x n_pools x 6), pos, ref, line_off, chrom_len -- plus the slab of text
 * their line offsets point into, as the bytes of their sync lines, in row order.  A line is
 *   slab[line_off .. line_off + chrom_len) '\t' pos '\t' ref, per pool '\t' and its six counts joined by ':', '\n'
 * with every number in plain decimal (no sign, no leading zeros, "0" for zero).  pg_sync_parse_dev writes no ref array: its
 * caller supplies one.  n_pools is 1 to 4096, the sync parser's limit; more is PG_ERR_INVALID before anything is launched.
 * *bytes is always set to the size the text needs; bytes > cap fails with PG_ERR_INVALID and writes nothing (cap = 0 is the
 * size query, text may then be NULL).  Nothing at or behind text[bytes] is written; text may have any alignment.  A row whose
 * line_off < 0, chrom_len < 0 or line_off + chrom_len > slab_bytes fails the call with PG_ERR_INVALID and *bytes = 0; so does
 * a row whose line would be longer than 2^22 bytes (this library's limit; 4096 pools of ten-digit counts are 270 KB).
 * rows = 0 is PG_OK with *bytes = 0.  Both forms behave alike in all of this.
 * The device form formats on the GPU (measure, scan, emit on the context's stream out of the context's workspace; it
 * synchronises once to read the size, and the text is complete once the stream has passed the call); the host form is plain
 * C++ on n_threads threads, no context, and gives the same bytes.
 * ------------------------------------------------------------------------------------- */
int pg_sync_format_rows_dev(pg_ctx *ctx, const char *slab_dev, int64_t slab_bytes, const uint32_t *counts_dev,
                            const uint64_t *pos_dev, const uint8_t *ref_dev, const int64_t *line_off_dev,
                            const int32_t *chrom_len_dev, int n_pools, int64_t rows, char *text_dev, int64_t cap, int64_t *bytes);
int pg_host_sync_format_rows(const char *slab, int64_t slab_bytes, const uint32_t *counts, const uint64_t *pos,
                             const uint8_t *ref, const int64_t *line_off, const int32_t *chrom_len, int n_pools, int64_t rows,
                             char *text, int64_t cap, int64_t *bytes, int n_threads);

/* ---------------------------------------------------------------------------------------
 * The result writer: the CSV rows of the GWAS analyses, formatted where the statistics are.
 *
 * The number text (pg_f64_text.h, one source for host and device).  display(x) is Rust's `{}` of an f64, which is what the
 * reference prints: "NaN", "inf", "-inf", "0", "-0", otherwise the SHORTEST decimal digit string (1 to 17 digits) that reads
 * back as the same double -- the closest such string, the even one on a tie -- in fixed notation: no exponent, no trailing
 * zeros behind the point, "0." and leading zeros below 1, padded with zeros for large exponents.  At most PG_F64_TEXT_MAX = 327
 * bytes ("-0." + 307 zeros + 17 digits).  roundup_own(x, nd) is parse_f64_roundup_and_own (base/helpers.rs:103-117): display(x)
 * when that has fewer than nd characters, else display(round_half_away_from_zero(x * 10^nd) / 10^nd), the product and the
 * quotient rounded separately.
 * THE HOST WRITER'S DIFFERENCE: the CLI's rust_display is std::to_chars(fixed), which equals display() for every |x| < 2^53
 * -- every fixture and every realistic statistic -- but prints the exact integer from about 2^54 on, where Rust (and this
 * formatter) print the shortest digits padded with zeros.  There this formatter is the one that matches the reference.
 *
 * Conventions of the three pairs below, those of pg_sync_format_rows_dev: *bytes is always set to the size the text needs;
 * bytes > cap fails with PG_ERR_INVALID and writes nothing (cap = 0 is the size query, text may then be NULL); nothing at or
 * behind text[bytes] is written; text may have any alignment; no rows is PG_OK with *bytes = 0; bad arguments, a label out of
 * range (a chromosome id outside [0, n_chrom), name offsets that decrease, an allele id outside [0, 6)) or a unit above the row
 * limit fail with PG_ERR_INVALID and *bytes = 0.  The row limit: the text of one unit -- one value, one locus with all its
 * rows, one kinship row -- is at most 2^22 bytes; at most 2^31 units per call; k is 1 to PG_RESULT_MAX_TRAITS.  Both forms
 * behave alike in all of this and give the same bytes.  The device form formats on the GPU (measure, 64-bit scan, emit on the
 * context's stream out of the context's workspace; it synchronises once to read the size, and the text is complete once the
 * stream has passed the call); the host form is plain C++ on n_threads threads and needs no context.
 * ------------------------------------------------------------------------------------- */
#define PG_F64_TEXT_MAX 327
#define PG_RESULT_MAX_TRAITS 4096
/* One line per value: display(x) for n_digits < 0, roundup_own(x, n_digits) for 0 <= n_digits <= 22 (more is PG_ERR_INVALID),
 * then '\n'. */
int pg_f64_text_dev(pg_ctx *ctx, const double *x_dev, int64_t count, int n_digits, char *text_dev, int64_t cap, int64_t *bytes);
int pg_host_f64_text(const double *x, int64_t count, int n_digits, char *text, int64_t cap, int64_t *bytes, int n_threads);
/* The rows of the per-locus operators (format_locus_rows of the CLI; fisher_exact_test.rs:119-129, chisq_test.rs:37-45,
 * gwalpha.rs:318-326, correlation_test.rs:117-124, ols.rs:263-271) from the slot-major outputs of the pg_*_batch_dev entry
 * points exactly as they leave them, labels as pg_csv_freq_rows_dev takes them (chromosome id and position per locus, the
 * names as one byte string with n_chrom + 1 int32 offsets).  Order: locus, then slot, then trait; a locus with n_out <= 0
 * emits nothing; n_out is clipped at PG_MAX_OUT.  D = display, R(x, n) = roundup_own, a letter indexes "ATCGND":
 *   PG_RESULT_FISHER   chr,pos,<letters of all slots>,D(stat[l]),D(pval[l])            one row per locus (k is ignored)
 *   PG_RESULT_CHISQ    chr,pos,<letters of all slots>,R(stat[l],6),D(pval[l])          one row per locus (k is ignored)
 *   PG_RESULT_GWALPHA  chr,pos,letter,R(freq,6),Pheno_0,R(stat,6),Unknown              per slot (k = 1; pval may be NULL)
 *   PG_RESULT_PEARSON  chr,pos,letter,D(freq),Pheno_j,R(stat,6),D(pval)                per slot and trait j
 *   PG_RESULT_OLS_ITER chr,pos,letter,R(freq,8),Pheno_j,R(stat,6),R(pval,12)           per slot and trait j
 * mean_freq may be NULL for the first two. */
enum pg_result_op { PG_RESULT_FISHER = 0, PG_RESULT_CHISQ = 1, PG_RESULT_GWALPHA = 2, PG_RESULT_PEARSON = 3, PG_RESULT_OLS_ITER = 4 };
int pg_result_rows_dev(pg_ctx *ctx, int op, int64_t L, int k, const int32_t *n_out_dev, const int32_t *allele_ids_dev,
                       const double *mean_freq_dev, const double *stat_dev, const double *pval_dev, const int32_t *locus_chrom_dev,
                       const uint64_t *locus_pos_dev, const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom,
                       char *text_dev, int64_t cap, int64_t *bytes);
int pg_host_result_rows(int op, int64_t L, int k, const int32_t *n_out, const int32_t *allele_ids, const double *mean_freq,
                        const double *stat, const double *pval, const int32_t *locus_chrom, const uint64_t *locus_pos,
                        const char *chrom_text, const int32_t *chrom_off, int n_chrom, char *text, int64_t cap, int64_t *bytes,
                        int n_threads);
/* Rows [row0, row0 + rows) of the k * p rows of the kinship analyses' CSV (write_kinship_csv of the CLI; ols.rs:409-433),
 * trait-major: row r = j * p + i is  label_i,Pheno_j,D(beta[i*k+j]),D(pval[i*k+j])  with the reference's label shift kept as
 * it is (ols.rs:421-425): coefficient 0 is "intercept,0,intercept", coefficient i >= 1 carries chromosome, position and allele
 * letter of column i - 1 (col_chrom int32, col_pos uint64, col_allele int32, p - 1 entries are read each); the last column's
 * label is never printed.  row0 < 0, rows < 0 or row0 + rows > k * p is PG_ERR_INVALID. */
int pg_kinship_rows_dev(pg_ctx *ctx, int64_t p, int k, int64_t row0, int64_t rows, const double *beta_dev, const double *pval_dev,
                        const int32_t *col_chrom_dev, const uint64_t *col_pos_dev, const int32_t *col_allele_dev,
                        const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom, char *text_dev, int64_t cap,
                        int64_t *bytes);
int pg_host_kinship_rows(int64_t p, int k, int64_t row0, int64_t rows, const double *beta, const double *pval,
                         const int32_t *col_chrom, const uint64_t *col_pos, const int32_t *col_allele, const char *chrom_text,
                         const int32_t *chrom_off, int n_chrom, char *text, int64_t cap, int64_t *bytes, int n_threads);

/* ---------------------------------------------------------------------------------------
 * The popgen writer: the tables of fst, heterozygosity, watterson_estimator and tajima_d and the rows of gudmc, formatted
 * where the values are.  Conventions of the result writer above, unchanged: *bytes is always set; cap = 0 is the size query;
 * bytes > cap is PG_ERR_INVALID and writes nothing; nothing at or behind text[bytes] is written; text may have any alignment;
 * no rows is PG_OK with *bytes = 0; bad arguments fail with PG_ERR_INVALID and *bytes = 0.  Host and device forms give the
 * same bytes.
 *
 * pg_f64_table: rows [row0, row0 + n_rows) of a rows x cols table, cell (r, c) = x[r * row_stride + c * col_stride] (so a
 * window-major table prints pool by pool with row_stride = 1: no transpose).  Row r is label_r (the bytes
 * label_text[label_off[r] .. label_off[r + 1]) as given, no separator added; label_off = NULL: no labels), the cells joined by
 * ',', then '\n'.  A cell is display(x) for n_digits < 0 and roundup_own(x, n_digits) for 0 .. 22; column 0 takes
 * first_col_digits instead.  The device form works cell by cell (pg_tablefmt.hip), so there is no limit on a row; a label is
 * at most 2^22 bytes; the total is 64-bit; at most 2^39 - 1 cells per call.  Label offsets that decrease (among the rows
 * formatted) and a row range outside [0, rows] are PG_ERR_INVALID.
 * ------------------------------------------------------------------------------------- */
int pg_f64_table_dev(pg_ctx *ctx, const double *x_dev, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride,
                     int64_t row0, int64_t n_rows, int n_digits, int first_col_digits, const char *label_text_dev,
                     const int64_t *label_off_dev, char *text_dev, int64_t cap, int64_t *bytes);
int pg_host_f64_table(const double *x, int64_t rows, int64_t cols, int64_t row_stride, int64_t col_stride, int64_t row0,
                      int64_t n_rows, int n_digits, int first_col_digits, const char *label_text, const int64_t *label_off,
                      char *text, int64_t cap, int64_t *bytes, int n_threads);
/* Rows [row0, row0 + rows) of gudmc's file (gudmc.rs:433-455) from pg_gudmc_dev's outputs as it leaves them (row_* with pitch
 * w) and the windows' chromosome id, first and last position (here on the device).  The file runs pair by pair, pair
 * i = a * n + b carrying the rows_dev[b] rows of population b; only rows_dev[n] is read back, for that prefix sum.  A row is
 *   pop_a,pop_b,chr,pos_ini,pos_fin,R(d_mean[b],7),R(fst_mean[i],7),R(d_sd[b],7),R(fst_sd[i],7),D(d),D(width),D(width_from_r),
 *   R(width_p,7),R(fst_delta,7),R(fst_p,7)
 * with the pool names and the chromosome names each as one byte string with int32 offsets (n + 1 and n_chrom + 1).  One lane
 * per row, at most 2^31 rows per call, a row at most 2^22 bytes.  A row range outside the file's rows, a population with more
 * than w rows, a row's window outside [0, w) and a window's chromosome id outside [0, n_chrom) are PG_ERR_INVALID. */
int pg_gudmc_rows_dev(pg_ctx *ctx, int n, int64_t w, int64_t row0, int64_t rows, const int64_t *rows_dev, const double *d_mean_dev,
                      const double *d_sd_dev, const double *fst_mean_dev, const double *fst_sd_dev, const int64_t *row_window_dev,
                      const double *row_d_dev, const double *row_width_dev, const double *row_width_from_r_dev,
                      const double *row_width_p_dev, const double *row_fst_delta_dev, const double *row_fst_p_dev,
                      const int32_t *win_chr_dev, const uint64_t *win_ini_dev, const uint64_t *win_fin_dev, const char *pool_text_dev,
                      const int32_t *pool_off_dev, const char *chrom_text_dev, const int32_t *chrom_off_dev, int n_chrom,
                      char *text_dev, int64_t cap, int64_t *bytes);
int pg_host_gudmc_rows(int n, int64_t w, int64_t row0, int64_t rows, const int64_t *pop_rows, const double *d_mean, const double *d_sd,
                       const double *fst_mean, const double *fst_sd, const int64_t *row_window, const double *row_d,
                       const double *row_width, const double *row_width_from_r, const double *row_width_p, const double *row_fst_delta,
                       const double *row_fst_p, const int32_t *win_chr, const uint64_t *win_ini, const uint64_t *win_fin,
                       const char *pool_text, const int32_t *pool_off, const char *chrom_text, const int32_t *chrom_off, int n_chrom,
                       char *text, int64_t cap, int64_t *bytes, int n_threads);

/* ---------------------------------------------------------------------------------------
 * impute (src/imputation/: filtering_missing.rs, mean_imputation.rs, adaptive_ld_knn_imputation.rs; CLI main.rs:125-142,
 * :367-396) on the loader's matrix: G and cov as pg_load_emit_cov_dev writes them (all alleles kept), locus_col (host, L + 1
 * entries, 0 .. p) as for the popgen tools.  The steps of impute_mean / impute_aLDkNN are separate entry points; every one
 * has returned only when its work on the device is done.  All results are bit for bit the reference's: sequential folds where
 * it folds, ndarray's 8-lane order where it calls sum().
 * ------------------------------------------------------------------------------------- */
/* set_missing_by_depth (filtering_missing.rs:15-44), in place: every (pool, locus) with cov < min_depth gets cov = NaN (in every
 * row of the locus) and NaN frequencies -- except in the LAST locus, whose frequencies stay as they are (the reference's
 * idx_fin = loci_idx[l - 1] is an empty range; its coverage still goes). */
int pg_set_missing_by_depth_dev(pg_ctx *ctx, double *G_dev, double *cov_dev, int64_t p, int n, int64_t ld,
                                const int64_t *locus_col, int64_t L, double min_depth);
/* The NaN counts the filters sort by (host outputs, either may be NULL): pool_nan[n] over the p rows of G
 * (filter_out_top_missing_pools, :53-61), locus_nan[L] over the pools of cov (filter_out_top_missing_loci, :136-144; cov_dev
 * may be NULL when locus_nan is).  missing_rate() (:7-13) is the sum of locus_nan over n * L. */
int pg_missingness_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                       const int64_t *locus_col, int64_t L, int64_t *pool_nan, int64_t *locus_nan);
/* The keep rule of both filters (:63-86, :146-170), no GPU: of `count` pools or loci, those with a NaN count > 0 number
 * n_missing; count - ceil(n_missing * frac) stay: the first of a STABLE ascending sort by NaN count, returned in ascending
 * index order in keep (room for count).  Returns how many stay; 0 is the reference's "No pools / loci left after filtering";
 * negative = bad argument. */
int64_t pg_host_top_missing_keep(const int64_t *nan_count, int64_t count, double frac, int64_t *keep);
/* G, cov and the column labels restricted to the kept pools (keep_pools: host, n_keep ascending indices) and loci (keep_loci:
 * host, L_keep ascending indices): G_out / cov_out are p_out x ld_out with the padding columns zeroed, p_out = the columns of
 * the kept loci = locus_col_out[L_keep] (host, L_keep + 1 entries, written by the call; the caller sizes the outputs from
 * locus_col).  cov_dev / cov_out_dev, col_locus_dev / col_locus_out_dev and col_allele_dev / col_allele_out_dev are optional
 * pairs.  Outputs must not overlap inputs. */
int pg_impute_compact_dev(pg_ctx *ctx, const double *G_dev, const double *cov_dev, int64_t p, int n, int64_t ld,
                          const int64_t *col_locus_dev, const int32_t *col_allele_dev, const int64_t *locus_col, int64_t L,
                          const int64_t *keep_pools, int n_keep, const int64_t *keep_loci, int64_t L_keep, double *G_out_dev,
                          double *cov_out_dev, int64_t ld_out, int64_t *col_locus_out_dev, int32_t *col_allele_out_dev,
                          int64_t *locus_col_out);
/* mean_imputation (mean_imputation.rs:6-41), in place: per locus the means of its allele columns over the non-NaN pools (fold
 * in pool order / count), divided by their sum when that is != 1.0, written into the NaN cells.  A locus missing in every
 * pool stays NaN. */
int pg_impute_mean_dev(pg_ctx *ctx, double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L);
/* adaptive_ld_knn_imputation (adaptive_ld_knn_imputation.rs:174-341) into G_out_dev (p x ld, must not be G_dev: every window
 * works on its own copy of the INPUT; the copies are written back in window order, so the last window that holds a column
 * wins, and loci in no window are copied through).  Windows as pg_host_sliding_windows gives them (n_windows = 0: a plain
 * copy).  Per window and column with missing data: Pearson correlations with every column of the window ("sensible_corr",
 * correlation_test.rs:7-71), the min(p_w, n_loci_to_estimate_distance) most correlated columns (stable, NaN first), Euclidean
 * pool distances over them on the window's current state, and per missing pool the adaptive k-nearest-neighbour weighted mean
 * with the reference's fall-backs (the count of present values over n) and its per-locus renormalisation, quirks included.
 * k_neighbours > n (the reference panics) fails with PG_ERR_INVALID.  scratch_bytes: device memory for the window copies,
 * sort keys and distance columns of one batch of windows (0 = 1 GiB; a window that needs more runs alone). */
int pg_impute_aldknn_dev(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L,
                         const int64_t *win_head, const int64_t *win_tail, int64_t n_windows, int64_t n_loci_to_estimate_distance,
                         int64_t k_neighbours, int64_t scratch_bytes, double *G_out_dev);
/* The mark both methods end with (mean_imputation.rs:42-59), in place: in every locus with at least one non-NaN coverage the
 * NaN coverages become +inf. */
int pg_impute_mark_cov_dev(pg_ctx *ctx, double *cov_dev, int64_t p, int n, int64_t ld, const int64_t *locus_col, int64_t L);

/* ---------------------------------------------------------------------------------------
 * Host-side pieces of the path (O(n^3), n = pools): exported so that they can be validated
 * without a GPU and reused by a host integration.
 * ------------------------------------------------------------------------------------- */
/* Symmetric eigen-decomposition standing in for `kinship.eig()` (gwas/ols.rs:296): eigenvalues
 * DESCENDING, eigenvectors in the columns of V (n x n row-major; V may be NULL). */
int pg_host_sym_eig(const double *A, int n, double *evals, double *V);
/* All eigenvalues (descending) and the m leading eigenvectors only (V: n x m row-major) -- what pg_kinship_set
 * needs for the covariates of gwas/ols.rs:312-315: values-only QL + inverse iteration + back-transformation,
 * verified against A, full decomposition as the fallback. */
int pg_host_sym_eig_top(const double *A, int n, int m, double *evals, double *V);
/* n_eigenvecs from the cumulative-variance rule, literal (gwas/ols.rs:297-311). */
int pg_host_n_eigenvecs(const double *evals, int n, double var_explained);
/* Moore-Penrose pseudo-inverse of a symmetric matrix with the reference tolerance
 * eps * len(s) * max(s) (base/helpers.rs:463-482). */
int pg_host_pinv_sym(const double *A, int n, double *out);
/* Two-sided Student-t p-value for integer df, evaluated by the same finite series the device
 * code uses (stands in for 2 * (1 - StudentsT::cdf(|t|)), gwas/ols.rs:153). */
double pg_host_t_two_sided_p(double t_abs, int df);

#ifdef __cplusplus
}
#endif
#endif
