// pg_common.h -- internal declarations shared by the libpoolgen_hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdarg>
#include <cstring>
#include <string>
#include <vector>
#include "../../include/poolgen_hip.h"

#define PG_MAX_SWEEP_COLS 34 // Q columns (m+1) + traits handled by one sweep launch

struct pg_event_pair { hipEvent_t a, b; int kid; };

int pg_fail(pg_ctx *ctx, int code, const char *fmt, ...);
// every allocation and release of the library (pg_context.hip); `pinned` = page-locked host memory
int pg_mem_alloc(pg_ctx *ctx, void **p, size_t bytes, bool pinned, const char *who);
void pg_mem_free(void *p, bool pinned);
// grow on demand: nothing if *cap >= bytes; else the context's stream is drained, the old block goes (pointer and capacity
// cleared first, so a failed allocation leaves a consistent state) and a block of `bytes` takes its place
int pg_mem_reserve(pg_ctx *ctx, void **p, size_t *cap, size_t bytes, bool pinned, const char *who);

// Move-only owner of one block of device (or pinned host) memory.  A per-call temporary takes alloc() and is released on
// every return, so PG_HIP / PG_CHECK may leave early behind it; a buffer the context keeps between calls takes reserve()
// and goes with the context.
template <typename T, bool Pinned = false>
class DevBuf {
    T *p_ = nullptr;
    size_t bytes_ = 0;

public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), bytes_(o.bytes_) { o.p_ = nullptr; o.bytes_ = 0; }
    DevBuf &operator=(DevBuf &&o) noexcept {
        if (this != &o) { reset(); p_ = o.p_; bytes_ = o.bytes_; o.p_ = nullptr; o.bytes_ = 0; }
        return *this;
    }
    ~DevBuf() { reset(); }
    // exactly `bytes`, replacing what was held; 0 bytes succeed and leave it null
    int alloc(pg_ctx *ctx, size_t bytes, const char *who) {
        reset();
        const int rc = pg_mem_alloc(ctx, reinterpret_cast<void **>(&p_), bytes, Pinned, who);
        if (rc == PG_OK) bytes_ = bytes;
        return rc;
    }
    int reserve(pg_ctx *ctx, size_t bytes, const char *who) {
        return pg_mem_reserve(ctx, reinterpret_cast<void **>(&p_), &bytes_, bytes, Pinned, who);
    }
    void reset() {
        if (p_) pg_mem_free(p_, Pinned);
        p_ = nullptr;
        bytes_ = 0;
    }
    T *get() const { return p_; }
    size_t bytes() const { return bytes_; } // the capacity: it changes exactly when reserve() replaced the block, whose contents are then gone
    operator T *() const { return p_; } // the context's buffers are read as the plain pointers they replace
};

struct pg_ctx {
    int device = -1;
    int cus = 256; // compute units of the device (cached at pg_create)
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;
    // profiling
    bool prof = false;
    std::vector<pg_event_pair> ev_pending;
    std::vector<pg_event_pair> ev_free;
    double prof_ms[PG_K_COUNT] = {0};
    int64_t prof_n[PG_K_COUNT] = {0};
    // generic device workspace (grown on demand, reused between calls)
    DevBuf<void> ws;
    // regression state set by pg_kinship_set / pg_covariates_set
    int st_n = 0, st_m = -1, st_k = 0, st_cols = 0;
    DevBuf<double> W_dev;     // n x st_cols row-major: [Q_0..Q_m | ytilde_0..ytilde_{k-1}]
    DevBuf<double> syy_dev;   // 64 trait slots + 2 (pg_syy_reserve)
    DevBuf<double> tcoef_dev; // t-distribution series coefficients for df = n - 1 (pg_tcoef_reserve)
    int tcoef_df = 0, tcoef_len = 0;
    DevBuf<double> S_dev;     // n x n kinship sum of the single-GPU convenience path
    // speculative intercept-only sums produced by the kinship pass (see pg_set_phenotypes)
    std::vector<double> ph_Y;    // n x k row-major copy of the phenotypes announced up front
    int ph_n = 0, ph_k = 0;
    bool ph_armed = false;       // the announcement is in force: the caller's own pg_set_phenotypes, or a composed call while it runs
    int64_t ph_serial = 0;       // counts the announcements that replaced ph_Y (a composed call sees whether it replaced the caller's)
    DevBuf<double> ph_ytil_dev; // k x 256 centred phenotypes, zero padded
    double ph_syy[4] = {0, 0, 0, 0};
    DevBuf<double> spec_dev;  // p x (2 + k): sum g', sum g'^2, sum g' ytil_t   (g' = g - g[0])
    const double *spec_G = nullptr;
    int64_t spec_p = 0, spec_ld = 0;
    int spec_n = 0, spec_k = 0;
    bool spec_valid = false;
    bool st_Y_matches_ph = false;
    // loader plan (pg_load_plan_dev -> pg_load_emit_dev); lives in ws, so any other ws user invalidates it
    bool load_valid = false;
    const uint32_t *load_counts = nullptr;
    const int64_t *load_order = nullptr;
    int64_t load_L = 0, load_total = 0, load_nunits = 0;
    int load_n = 0, load_kpm1 = 0;
    size_t load_off_flags = 0, load_off_local = 0, load_off_blockoff = 0, load_off_poolmap = 0;
    int64_t lo_last_L = 0, lo_last_listed = 0; // pg_locus_op_stats
    bool rows_call[2] = {true, true};   // ... and what the current call's launch groups run
    bool rows_next[2] = {true, true}; // ols_iter, chisq_test: the next batch runs the order-free kernel (the last one looked error-bearing, or none has run)
    DevBuf<double> lz_dev;    // per-wave (1'S1, trace S) partials of the lazy-kinship sweep
    bool lazy_taken = false;     // the last pg_ols_kinship_dev decided m = 0 without forming K
    std::vector<double> st_Y;    // phenotypes of the last m = 0 covariate state (lets an identical call skip the upload)
    // small pinned host staging
    DevBuf<void, true> pin;
    // RCCL communicator of the locus-sharded path (pg_comm.cpp); null = single GPU
    void *comm = nullptr;
    int comm_size = 1, comm_rank = 0;
};

// The fused sums describe the p x ld doubles at spec_G as the kinship pass read them: a library call that is about to write
// `bytes` at `dst` drops them when the two ranges overlap (a null dst or 0 bytes writes nothing).
inline void pg_spec_written(pg_ctx *ctx, const void *dst, size_t bytes) {
    if (!ctx->spec_valid || !dst || !bytes) return;
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst), b = reinterpret_cast<uintptr_t>(ctx->spec_G);
    const uintptr_t bl = (uintptr_t)ctx->spec_p * (uintptr_t)ctx->spec_ld * sizeof(double);
    if (a < b + bl && b < a + bytes) ctx->spec_valid = false;
}

#define PG_HIP(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return pg_fail(ctx, PG_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                               \
    } while (0)
#define PG_CHECK(ctx, cond, ...)                                   \
    do {                                                           \
        if (!(cond)) return pg_fail(ctx, PG_ERR_INVALID, __VA_ARGS__); \
    } while (0)

// The environment switches of the library: each forces a route that the default dispatch takes only at other shapes.  The table
// (name, what it forces, what it replaces) is in pg_context.hip; pg_switch returns the variable's value, or null when unset.
enum pg_switch_id {
    PG_SW_SWEEP_V1, PG_SW_SWEEP_V2, PG_SW_SWEEP_GRID_MULT, PG_SW_NO_LAZY_KINSHIP, PG_SW_HOST_SLAB_MB,
    PG_SW_GP_BETA_OLD, PG_SW_GP_BETA_VALU, PG_SW_GP_BETA_SCALAR, PG_SW_GP_TIMING, PG_SW_RIDGE_PER_REP, PG_SW_RIDGE_PER_FOLD,
    PG_SW_MLE_LDS, PG_SW_OLS_ITER_KERNEL, PG_SW_ROWS_DIRECT, PG_SW_LOCUS_GROUPED,
    PG_SW_COUNT
};
const char *pg_switch(pg_switch_id id);

// pg_set_phenotypes without the opt-in: the centred phenotypes on the device (ph_*), ph_armed untouched (pg_kinship.hip).  The
// composed calls announce through PhScope, so that their announcement ends with them: a caller who never called
// pg_set_phenotypes is not opted in afterwards, and one who did stays opted in only if his phenotypes were not replaced.
int pg_phenotypes_upload(pg_ctx *ctx, int n, const double *Y, int k);
struct PhScope {
    pg_ctx *ctx;
    bool armed;
    int64_t serial;
    explicit PhScope(pg_ctx *c) : ctx(c), armed(c->ph_armed), serial(c->ph_serial) {}
    int announce(int n, const double *Y, int k) {
        const int rc = pg_phenotypes_upload(ctx, n, Y, k);
        ctx->ph_armed = rc == PG_OK && ctx->ph_n > 0;
        return rc;
    }
    ~PhScope() {
        ctx->ph_armed = armed && ctx->ph_serial == serial;
        ctx->spec_valid = false; // the fused sums of a composed call are its own sweep's: gone on every return, a failed one included
    }
};

int pg_ws_reserve(pg_ctx *ctx, size_t bytes);
int pg_pin_reserve(pg_ctx *ctx, size_t bytes);
int pg_tcoef_reserve(pg_ctx *ctx, int df); // the t-distribution coefficients of `df` on the device (tcoef_dev, tcoef_df, tcoef_len)
inline int pg_syy_reserve(pg_ctx *ctx) { return ctx->syy_dev.reserve(ctx, sizeof(double) * 66, "syy"); }
constexpr int PG_PROF_CONT = 0x100; // pg_prof_begin(kid | PG_PROF_CONT): more device time of an operation already counted
void pg_prof_begin(pg_ctx *ctx, int kid);
void pg_prof_end(pg_ctx *ctx);

// host math (pg_hostmath.cpp)
// symmetric eigen-decomposition: eigenvalues descending, eigenvectors in columns of V (row-major)
int pg_sym_eig(const double *A, int n, double *evals, double *V, bool want_vectors);
int pg_sym_eig_top(const double *A, int n, int m, double *evals, double *V); // all values, the m leading vectors (n x m)
// thin Householder QR of Z (n x c row-major) -> Q (n x c row-major), returns numerical rank
int pg_thin_qr(const double *Z, int n, int c, double *Q);
// t-distribution finite-series coefficients (Abramowitz & Stegun 26.7.3/26.7.4)
std::vector<double> pg_tdist_coef(int df);
// symmetric pseudo-inverse with the reference's tolerance (helpers.rs:463-482)
int pg_pinv_sym(const double *A, int n, double *out);
// X X^T of the full data (n x n, intercept included) on the host: the caller's copy, or the kinship pass and a copy (pg_gp.hip)
int pg_gp_xxt_host(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *given_or_null, const char *who,
                   std::vector<double> &xxt);
int pg_gp_beta_cols(pg_ctx *ctx, const double *G_dev, int64_t p, int n, int64_t ld, const double *Z_host, int ncol,
                    double *out_dev, int colmajor = 0, double *ss_out_dev = nullptr); // out p x ncol, or ncol x p when colmajor; ss: g'g per row
int pg_pinv_solve_sym(const double *A, int n, const double *B, int k, double *X); // pinv(A) B, Cholesky when A is safely SPD

// The loader's filter pass for operators that live in other translation units (pg_locus_ops.hip): one header word per locus at
// (*flags)[l] -- bit 0 alive, bits 1..6 the surviving alleles, PG_HDR_NK_SHIFT.. +3 their number, from PG_HDR_ORD_SHIFT three bits
// per surviving allele in column order (sort_desc = 0) or by decreasing frequency (sort_desc = 1).  `tail_bytes` of the context's
// workspace behind the pass' own are the caller's, 16-byte aligned at *tail; *listed = loci the second pass took.
constexpr int PG_HDR_ALIVE = 1, PG_HDR_NK_SHIFT = 8, PG_HDR_ORD_SHIFT = 11;
int pg_filter_headers(pg_ctx *ctx, const char *who, int kid, bool args_ok, const uint32_t *counts_dev, int64_t L, int n,
                      const double *pool_sizes, const pg_filter *flt, int sort_desc, size_t tail_bytes, const int32_t **flags,
                      int64_t *listed, char **tail);

// launchers (defined in the .hip files)
int pg_launch_kinship(pg_ctx *ctx, const double *G, int64_t p, int n, int64_t ld, double *S,
                      bool add_intercept, int kid, bool allow_fuse = false);
int pg_launch_kinship_w8(pg_ctx *ctx, const double *G, int64_t p, int n, int64_t ld, double *S,
                         bool add_intercept, int kid, bool allow_fuse = false); // 8-wave workgroups (pg_kinship_w8.hip): <= 64 pools
