// pg_context.hip -- context lifetime, error reporting, workspace and HIP-event profiling.
#include "pg_common.h"
#include <cstdlib>

// ---- the environment switches --------------------------------------------------------------------------------------------
// Every variable the library reads, in the order of pg_switch_id, and the library's only getenv.  None of them changes what is
// computed: each sends a call down a route that the default dispatch takes at other shapes, so that the tests can run both
// routes on one input (INTEGRATION.md repeats this table).  A switch is read on every call, on purpose: the tests flip them
// between calls on one context that lives for the whole session, so nothing here is cached.
static const struct { const char *name, *forces, *replaces; } pg_switches[PG_SW_COUNT] = {
    {"POOLGEN_SWEEP_V1", "the regression sweep runs the lane-per-locus row kernel (k_ols_sweep_rows)",
     "the matrix-core sweep from 33 pools while its B table fits 160 KB; the super-row kernel below 12 columns"},
    {"POOLGEN_SWEEP_V2", "the regression sweep runs the lane-per-locus super-row kernel (k_ols_sweep)",
     "the matrix-core sweep; the row kernel from 12 columns on and up to 32 pools"},
    {"POOLGEN_SWEEP_GRID_MULT", "=N: N workgroups per CU in the sweep's grid (N = 1: every wave walks many tiles)",
     "what the occupancy allows (matrix-core sweep), 8 per CU (lane-per-locus sweeps)"},
    {"POOLGEN_NO_LAZY_KINSHIP", "pg_ols_kinship_dev forms K and runs the eigen rule even when the caller does not ask for K",
     "the one-pass lazy route (MODE 2 sweep) that decides m = 0 from 1'S1 and trace S"},
    {"POOLGEN_HOST_SLAB_MB", "=N: pg_ols_kinship (host matrix) uploads and sweeps in slabs of N MB", "256 MB slabs"},
    {"POOLGEN_GP_BETA_OLD", "pg_gp_beta_cols skips the matrix-core products kernel",
     "the matrix-core kernel from 33 pools while its B table fits 160 KB (even ld, aligned G)"},
    {"POOLGEN_GP_BETA_VALU", "... and skips k_gp_beta_mfma", "k_gp_beta_mfma for 5 .. 16 column-major columns"},
    {"POOLGEN_GP_BETA_SCALAR", "... and skips k_gp_beta_lds, which leaves the scalar-operand k_gp_beta",
     "k_gp_beta_lds when Z is past 12 KB (6 .. 24 columns)"},
    {"POOLGEN_GP_TIMING", "host-side phase times of a penalised_path call on stderr", "no report"},
    {"POOLGEN_RIDGE_PER_REP", "cross-validation runs one repetition per coefficient pass",
     "all repetitions batched into shared passes when n_reps > 1"},
    {"POOLGEN_RIDGE_PER_FOLD", "cross-validation fits every fold on its own",
     "the fused route when the fold x trait columns fit one sweep (<= 34) and n < p + 1"},
    {"POOLGEN_MLE_LDS", "the MLE runs its LDS kernel for small designs too", "the register kernel up to 4 design columns (m <= 2)"},
    {"POOLGEN_OLS_ITER_KERNEL", "=stream: ols_iter / chisq_test run the streaming kernel; any other value: the row kernel",
     "the choice by the last batch's error flags (rows_next), row kernel for 32 .. 448 pools"},
    {"POOLGEN_ROWS_DIRECT", "=0: chisq_test's row kernel stages its pools through the LDS buffer",
     "direct register loads (chisq_test only; ols_iter always stages)"},
    {"POOLGEN_LOCUS_GROUPED", "=0 / =1: the listed-locus operators run ungrouped / grouped by allele count",
     "grouped from LO_GROUP_FROM listed loci on"},
};

const char *pg_switch(pg_switch_id id) { return std::getenv(pg_switches[id].name); }

int pg_fail(pg_ctx *ctx, int code, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

static std::string g_create_error;

extern "C" const char *pg_version(void) { return "poolgen_hip 0.1.0 (gfx950)"; }

extern "C" const char *pg_last_error(const pg_ctx *ctx) {
    return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

extern "C" int pg_create(pg_ctx **out, int device, void *stream) {
    if (!out) return PG_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        g_create_error = std::string("no HIP device available: ") + hipGetErrorString(e) +
                         " -- libpoolgen_hip has no CPU fallback";
        return PG_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= count) {
        g_create_error = "device ordinal out of range";
        return PG_ERR_INVALID;
    }
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device);
    if (e != hipSuccess) {
        g_create_error = std::string("hipGetDeviceProperties: ") + hipGetErrorString(e);
        return PG_ERR_HIP;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName +
                         ", this library contains gfx950 code objects only";
        return PG_ERR_NO_DEVICE;
    }
    e = hipSetDevice(device);
    if (e != hipSuccess) {
        g_create_error = std::string("hipSetDevice: ") + hipGetErrorString(e);
        return PG_ERR_HIP;
    }
    pg_ctx *ctx = new pg_ctx();
    ctx->device = device;
    ctx->cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // NULL = the device's default (null) stream, which is what torch hands out as cuda_stream 0;
    // work is therefore always ordered with the caller's stream.
    ctx->stream = (hipStream_t)stream;
    ctx->own_stream = false;
    *out = ctx;
    return PG_OK;
}

extern "C" void pg_destroy(pg_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) (void)pg_comm_destroy(ctx);
    for (auto &p : ctx->ev_pending) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    for (auto &p : ctx->ev_free) { (void)hipEventDestroy(p.a); (void)hipEventDestroy(p.b); }
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx; // (every buffer of the context is a DevBuf member: released here)
}

extern "C" int pg_synchronize(pg_ctx *ctx) {
    if (!ctx) return PG_ERR_INVALID;
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_mem_alloc(pg_ctx *ctx, void **p, size_t bytes, bool pinned, const char *who) {
    *p = nullptr;
    if (bytes == 0) return PG_OK;
    const hipError_t e = pinned ? hipHostMalloc(p, bytes, hipHostMallocDefault) : hipMalloc(p, bytes);
    if (e == hipSuccess) return PG_OK;
    *p = nullptr;
    return pg_fail(ctx, PG_ERR_HIP, "%s: out of %s memory (%.1f MB: %s)", who, pinned ? "pinned host" : "device", bytes / 1e6,
                   hipGetErrorString(e));
}

void pg_mem_free(void *p, bool pinned) {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
}

int pg_mem_reserve(pg_ctx *ctx, void **p, size_t *cap, size_t bytes, bool pinned, const char *who) {
    if (bytes <= *cap) return PG_OK;
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (*p) PG_HIP(ctx, pinned ? hipHostFree(*p) : hipFree(*p));
    *p = nullptr;
    *cap = 0;
    const int rc = pg_mem_alloc(ctx, p, bytes, pinned, who);
    if (rc == PG_OK) *cap = bytes;
    return rc;
}

int pg_ws_reserve(pg_ctx *ctx, size_t bytes) {
    ctx->load_valid = false; // whoever asks for the workspace is about to overwrite it
    return ctx->ws.reserve(ctx, bytes, "workspace");
}

int pg_pin_reserve(pg_ctx *ctx, size_t bytes) { return ctx->pin.reserve(ctx, bytes, "staging"); }

int pg_tcoef_reserve(pg_ctx *ctx, int df) {
    if (ctx->tcoef_df == df && ctx->tcoef_dev) return PG_OK;
    const std::vector<double> tc = pg_tdist_coef(df);
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    int rc = ctx->tcoef_dev.alloc(ctx, sizeof(double) * (tc.size() + 1), "t coefficients");
    if (rc) return rc;
    if (!tc.empty())
        PG_HIP(ctx, hipMemcpyAsync(ctx->tcoef_dev, tc.data(), sizeof(double) * tc.size(), hipMemcpyHostToDevice, ctx->stream));
    ctx->tcoef_df = df;
    ctx->tcoef_len = (int)tc.size();
    PG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // tc is stack-owned
    return PG_OK;
}

// ---- profiling: one event pair per launch, on the launch stream, resolved at query time ----
void pg_prof_begin(pg_ctx *ctx, int kid) {
    if (!ctx->prof || kid < 0) return;
    pg_event_pair p;
    if (!ctx->ev_free.empty()) {
        p = ctx->ev_free.back();
        ctx->ev_free.pop_back();
    } else {
        if (hipEventCreate(&p.a) != hipSuccess) return;
        if (hipEventCreate(&p.b) != hipSuccess) { (void)hipEventDestroy(p.a); return; }
    }
    p.kid = kid;
    (void)hipEventRecord(p.a, ctx->stream);
    ctx->ev_pending.push_back(p);
}

void pg_prof_end(pg_ctx *ctx) {
    if (!ctx->prof || ctx->ev_pending.empty()) return;
    (void)hipEventRecord(ctx->ev_pending.back().b, ctx->stream);
}

static void prof_drain(pg_ctx *ctx) {
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &p : ctx->ev_pending) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, p.a, p.b) == hipSuccess) {
            ctx->prof_ms[p.kid & 0xff] += ms;
            if (!(p.kid & PG_PROF_CONT)) ctx->prof_n[p.kid & 0xff] += 1; // (a continuation bracket adds time to the launch its first bracket counted)
        }
        ctx->ev_free.push_back(p);
    }
    ctx->ev_pending.clear();
}

extern "C" int pg_profile_enable(pg_ctx *ctx, int on) {
    if (!ctx) return PG_ERR_INVALID;
    prof_drain(ctx);
    ctx->prof = on != 0;
    return PG_OK;
}

extern "C" int pg_profile_reset(pg_ctx *ctx) {
    if (!ctx) return PG_ERR_INVALID;
    prof_drain(ctx);
    for (int i = 0; i < PG_K_COUNT; ++i) { ctx->prof_ms[i] = 0; ctx->prof_n[i] = 0; }
    return PG_OK;
}

extern "C" int pg_profile_get(pg_ctx *ctx, int kernel_id, double *total_ms, int64_t *launches) {
    if (!ctx || kernel_id < 0 || kernel_id >= PG_K_COUNT) return PG_ERR_INVALID;
    prof_drain(ctx);
    if (total_ms) *total_ms = ctx->prof_ms[kernel_id];
    if (launches) *launches = ctx->prof_n[kernel_id];
    return PG_OK;
}
