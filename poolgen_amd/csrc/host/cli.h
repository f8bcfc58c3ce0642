// cli.h -- what the translation units of the `poolgen` command line share; all arithmetic on the loci is libpoolgen_hip.so's.
#pragma once
#include "cli_args.h"
#include "gpu_mem.h"
#include "host_util.h"
#include "rank_gate.h"
#include "result_writer.h"
#include <algorithm>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <mutex>
#include <thread>
#include <time.h>
#include <fcntl.h>
#include <unistd.h>

using namespace pgh; // (the CLI's own translation units only: what main.cpp did before it was split)

inline std::string basename_no_ext(const std::string &f) { // sync.rs:889-902
    const auto p = f.rfind('.');
    return p == std::string::npos ? std::string() : f.substr(0, p);
}

inline std::string unix_time_string() {
    const double t = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    return rust_display(t);
}

// OpenOptions::create_new: refuse to overwrite (sync.rs:906, :942-947; ols.rs:285, :402-407)
inline FILE *create_new(const std::string &path) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (fd < 0) throw std::runtime_error("Unable to create file: " + path + " (it must not exist)");
    return fdopen(fd, "w");
}

inline void probe_output(const std::string &path) { // the same refusal before any work is done, as in the reference (sync.rs:906, ols.rs:285)
    fclose(create_new(path));
    ::unlink(path.c_str());
}

struct Ctx {
    pg_ctx *c = nullptr;
    int device = 0;
    explicit Ctx(int dev = 0) : device(dev) {
        if (pg_create(&c, dev, nullptr) != PG_OK)
            throw std::runtime_error("GPU " + std::to_string(dev) + ": " + pg_last_error(nullptr));
    }
    Ctx(const Ctx &) = delete;
    Ctx &operator=(const Ctx &) = delete;
    ~Ctx() { pg_destroy(c); }
    void ok(int rc, const char *what) {
        if (rc != PG_OK) throw std::runtime_error(std::string(what) + ": " + pg_last_error(c));
    }
};

// pools with a missing phenotype are removed before the locus operators (remove_missing,
// sync.rs:508-549).  The reference forgets to shrink FilterStats.pool_sizes and panics in that
// case; here the pool sizes are subset consistently.
inline std::vector<int> complete_pools(const Phen &ph) {
    std::vector<int> idx;
    for (int i = 0; i < ph.n; ++i) {
        double s = 0.0;
        for (int j = 0; j < ph.k; ++j) s += ph.phen[(size_t)i * ph.k + j];
        if (!std::isnan(s)) idx.push_back(i);
    }
    return idx;
}

// Formats items [0, count) with `fn(i, text)` on `n_threads` workers and writes them in item order: the file is byte-identical to
// a sequential loop.  Every worker owns ONE contiguous range per round (a round = what fits PGH_WRITE_ROUND_MB of text, default
// 1024: the 20 M rows of a 10 M-site kinship run are one round), formats it into its own buffer and -- once the sizes of the
// buffers in front of it are known -- copies it into the file itself with pwrite at its own offset; the file is extended once per
// round (ftruncate) so that the workers' writes never fight over its length.  (Round 3 re-spawned the workers twice per 64 k rows
// and took 0.6 - 1.2 s for those 20 M rows.)
template <typename F>
static void write_rows_parallel(FILE *fo, int64_t count, int n_threads, F fn) {
    if (n_threads < 1) n_threads = 1;
    if (count <= 0) return;
    size_t round_mb = 1024;
    if (const char *e = std::getenv("PGH_WRITE_ROUND_MB")) round_mb = (size_t)std::max(1L, std::atol(e));
    const int64_t per_round = std::max<int64_t>(n_threads, (int64_t)((round_mb << 20) / 64)); // ~64 bytes of text per item
    std::fflush(fo);
    const int fd = fileno(fo);
    off_t off = ftello(fo);
    for (int64_t base = 0; base < count; base += per_round) {
        const int64_t end = std::min(count, base + per_round);
        const int parts = (int)std::min<int64_t>(n_threads, end - base);
        const int64_t each = (end - base + parts - 1) / parts;
        std::vector<std::string> text(parts);
        std::vector<size_t> size(parts, 0);
        std::vector<int> failed(parts, 0);
        std::mutex mu;
        std::condition_variable cv;
        int formatted = 0;
        off_t round_off = off, round_end = off;
        bool sized = false;
        std::vector<std::thread> th;
        for (int t = 0; t < parts; ++t)
            th.emplace_back([&, t] {
                const int64_t lo = base + t * each, hi = std::min(end, lo + each);
                std::string &out = text[t];
                out.reserve((size_t)std::max<int64_t>(0, hi - lo) * 64);
                for (int64_t i = lo; i < hi; ++i) fn(i, out);
                off_t at;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    size[t] = out.size();
                    if (++formatted == parts) { // the last one to finish knows every size: extend the file once, release everybody
                        for (int q = 0; q < parts; ++q) round_end += (off_t)size[q];
                        if (::ftruncate(fd, round_end) != 0) failed[t] = 1;
                        sized = true;
                        cv.notify_all();
                    } else cv.wait(lk, [&] { return sized; });
                    at = round_off;
                    for (int q = 0; q < t; ++q) at += (off_t)size[q];
                }
                const char *q = out.data();
                size_t left = out.size();
                while (left > 0) {
                    const ssize_t w = ::pwrite(fd, q, left, at);
                    if (w <= 0) { failed[t] = 1; return; }
                    q += w; at += w; left -= (size_t)w;
                }
                std::string().swap(out);
            });
        for (auto &x : th) x.join();
        for (int t = 0; t < parts; ++t)
            if (failed[t]) throw std::runtime_error("write failed (disk full?)");
        off = round_end;
    }
    fseeko(fo, off, SEEK_SET);
}

// PGH_TIMING=1: wall-clock of the CLI's phases on stderr
struct Lap {
    bool on = std::getenv("PGH_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void operator()(const char *what) {
        if (!on) return;
        const auto n = std::chrono::steady_clock::now();
        std::fprintf(stderr, "poolgen: %-24s %.3f s\n", what, std::chrono::duration<double>(n - t).count());
        t = n;
    }
};

// The results are on disk and the file name is printed: end the process here.  Releasing tens of GB of device and pinned
// memory buffer by buffer (destructors, device frees, the HIP runtime's shutdown) took 0.3 s of a 1.4 s run; the driver
// reclaims everything when the process ends.  PGH_CLEAN_EXIT=1 keeps the orderly teardown (leak checkers).
inline void stamp(const char *what) { // PGH_TIMING=1: the wall clock itself, so that a wrapper can see what lies outside the laps
    if (!std::getenv("PGH_TIMING")) return;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    std::fprintf(stderr, "poolgen: clock at %-15s %lld.%09ld\n", what, (long long)ts.tv_sec, ts.tv_nsec);
}
inline int done_ok() {
    stamp("exit");
    std::cout.flush();
    std::cerr.flush();
    std::fflush(nullptr);
    if (!std::getenv("PGH_CLEAN_EXIT")) ::_exit(0);
    return 0;
}
inline int done_ok(const std::string &out) { // the name of the file written is the program's answer (main.rs:507)
    std::cout << out << "\n";
    return done_ok();
}

// The counts of a parsed batch -> the 32-bit device buffer the operators read.  A 16-bit batch (every count fits: the
// usual case) crosses the bus at half the size and is widened on the device; `stage16` is a reusable device scratch.
struct CountsUpload {
    DeviceBuf<uint16_t> stage16;
    void operator()(Ctx &gpu, const SyncBatch &sb, uint32_t *counts_dev) {
        if (!sb.counts16) {
            hip_ok(hipMemcpyAsync(counts_dev, sb.counts, sb.counts_bytes(), hipMemcpyHostToDevice, nullptr), "H2D counts");
            return;
        }
        stage16.reserve(sb.counts_bytes(), "device memory for the compact counts");
        hip_ok(hipMemcpyAsync(stage16.get(), sb.counts16, sb.counts_bytes(), hipMemcpyHostToDevice, nullptr), "H2D counts");
        gpu.ok(pg_expand_counts_u16_dev(gpu.c, stage16.get(), (int64_t)sb.L * sb.n * 6, counts_dev), "expand counts");
    }
};

// ---- ranks: one GPU, one pg_ctx, one host thread (plus its share of the parser threads) each -------------------------
// The reference's parallel axis is a worker per contiguous byte range of the input (base/sync.rs:913-939); here a rank
// is such a worker with a GPU behind it.  Ranks are threads of this process; the kinship sums are all-reduced with RCCL
// inside libpoolgen_hip (pg_comm_init_rank / pg_allreduce_sum_dev).  PGH_COMM=host is a REHEARSAL mode for boxes with
// fewer GPUs than ranks (--gpu-ids 0,0: RCCL refuses two ranks on one device): the partial sums are then added on the
// host in rank order -- same control flow, same byte ranges, same files.
struct RankSetup {
    int n_ranks = 1;
    std::vector<int> devices;   // per rank
    std::vector<int> threads;   // parser / writer threads per rank
    bool rccl = false;          // --n-gpus given: a communicator is set up even for one rank
    bool host_comm = false;     // PGH_COMM=host
    unsigned char id[PG_COMM_ID_BYTES] = {0};
};

inline RankSetup rank_setup(const Args &a, bool need_comm) {
    RankSetup r;
    r.n_ranks = a.n_gpus > 0 ? a.n_gpus : 1;
    for (int i = 0; i < r.n_ranks; ++i) r.devices.push_back(a.gpu_ids.empty() ? i : a.gpu_ids[i]);
    // every ordinal is checked BEFORE any rank thread exists: a rank that cannot open its device would otherwise leave the
    // others waiting for it inside ncclCommInitRank
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) ndev = 0;
    for (int i = 0; i < r.n_ranks; ++i)
        if (r.devices[i] < 0 || r.devices[i] >= ndev)
            throw std::runtime_error("rank " + std::to_string(i) + " asks for GPU " + std::to_string(r.devices[i]) + " but " +
                                     std::to_string(ndev) + " GPU(s) are visible (--n-gpus / --gpu-ids)");
    const int total = std::max(a.n_threads, 1);
    for (int i = 0; i < r.n_ranks; ++i) r.threads.push_back(std::max(1, total / r.n_ranks + (i < total % r.n_ranks ? 1 : 0)));
    const char *e = std::getenv("PGH_COMM");
    r.host_comm = e && std::string(e) == "host";
    r.rccl = need_comm && a.n_gpus > 0 && !r.host_comm;
    if (r.rccl) {
        std::vector<int> d = r.devices;
        std::sort(d.begin(), d.end());
        if (std::adjacent_find(d.begin(), d.end()) != d.end())
            throw std::runtime_error("--gpu-ids lists a device twice: RCCL needs one GPU per rank (PGH_COMM=host rehearses the rank logic on fewer GPUs)");
        if (pg_comm_unique_id(r.id) != PG_OK) throw std::runtime_error(std::string("RCCL: ") + pg_last_error(nullptr));
    }
    return r;
}

// contiguous ranges of pieces per rank: rank r takes [first[r], first[r + 1])
inline std::vector<int> deal_pieces(int npieces, int n_ranks) {
    std::vector<int> first(n_ranks + 1);
    for (int r = 0; r <= n_ranks; ++r) first[r] = (int)((int64_t)npieces * r / n_ranks);
    return first;
}

template <typename F>
static void run_ranks(int n_ranks, F fn) { // fn(rank) on one thread per rank; the first exception is rethrown
    std::vector<std::exception_ptr> err(n_ranks);
    std::vector<std::thread> th;
    for (int r = 1; r < n_ranks; ++r)
        th.emplace_back([&, r] { try { fn(r); } catch (...) { err[r] = std::current_exception(); } });
    try { fn(0); } catch (...) { err[0] = std::current_exception(); }
    for (auto &t : th) t.join();
    for (auto &e : err) // the rank that failed first-hand, not the ones that stopped because of it
        if (e) { try { std::rethrow_exception(e); } catch (const RankAborted &) {} catch (...) { throw; } }
    for (auto &e : err) if (e) std::rethrow_exception(e);
}

// The loader on counts that are on the device (pg_load_plan_dev / pg_load_emit[_cov]_dev): filter + frequencies per locus, one
// column per surviving allele of a p x ld locus-major matrix in HBM, the loci in the order of `order_dev` (null: as they come),
// the n2 kept pools placed by `pool_map`.  The columns' labels come back to the host.  p == 0: nothing else is filled.
struct LoadedMatrix {
    int64_t p = 0;
    DeviceBuf<double> G, coverages;  // coverages: laid out like the matrix (pg_load_emit_cov_dev); only when asked for
    std::vector<int64_t> col_locus;  // per column: its locus (a row of the counts) ...
    std::vector<int32_t> col_allele; // ... and its allele (an index into ALLELES)
    DeviceBuf<int64_t> col_locus_dev; // the same two on the device, instead of the host's copies, when asked for (sync2csv formats there)
    DeviceBuf<int32_t> col_allele_dev;
};

inline LoadedMatrix load_matrix(Ctx &gpu, const uint32_t *counts_dev, int64_t L, int n, const std::vector<double> &pool_sizes,
                                const pg_filter &flt, bool keep_p_minus_1, const int64_t *order_dev, const std::vector<int32_t> &pool_map,
                                int n2, int64_t ld, bool with_coverages, bool labels_on_device = false) {
    LoadedMatrix m;
    gpu.ok(pg_load_plan_dev(gpu.c, counts_dev, L, n, pool_sizes.data(), &flt, keep_p_minus_1 ? 1 : 0, order_dev, &m.p), "load");
    if (m.p <= 0) return m;
    const size_t p = (size_t)m.p;
    m.G.reset(sizeof(double) * p * ld, "device memory for the genotype matrix");
    DeviceBuf<int64_t> col_locus_dev(sizeof(int64_t) * p, "device memory");
    DeviceBuf<int32_t> col_allele_dev(sizeof(int32_t) * p, "device memory");
    if (with_coverages) {
        m.coverages.reset(sizeof(double) * p * ld, "device memory for the coverages");
        gpu.ok(pg_load_emit_cov_dev(gpu.c, pool_map.data(), n2, m.G.get(), ld, col_locus_dev.get(), col_allele_dev.get(), m.coverages.get()), "load");
    } else
        gpu.ok(pg_load_emit_dev(gpu.c, pool_map.data(), n2, m.G.get(), ld, col_locus_dev.get(), col_allele_dev.get()), "load");
    if (labels_on_device) {
        m.col_locus_dev = std::move(col_locus_dev); m.col_allele_dev = std::move(col_allele_dev);
        return m;
    }
    m.col_locus.resize(p); m.col_allele.resize(p);
    hip_ok(hipMemcpy(m.col_locus.data(), col_locus_dev.get(), sizeof(int64_t) * p, hipMemcpyDeviceToHost), "D2H labels");
    hip_ok(hipMemcpy(m.col_allele.data(), col_allele_dev.get(), sizeof(int32_t) * p, hipMemcpyDeviceToHost), "D2H labels");
    return m;
}

// The CSV of ols_iter_with_kinship / mle_iter_with_kinship: p coefficients x k traits of beta / pval; `label(i, text)` appends
// the "chr,pos,allele" of coefficient i.
template <typename Label>
static void write_kinship_csv(const std::string &out, int64_t p, int k, const std::vector<double> &beta, const std::vector<double> &pval,
                              int n_threads, Label label) {
    FILE *fo = create_new(out);
    fputs("#chr,pos,alleles,phenotype,statistic,pvalue\n", fo); // ols.rs:409
    write_rows_parallel(fo, (int64_t)k * p, n_threads, [&](int64_t r, std::string &text) {
        const int64_t j = r / p, i = r - j * p; // rows are trait-major (ols.rs:411-433)
        label(i, text);
        text += ",Pheno_"; text += std::to_string(j); text.push_back(',');
        append_rust_display(text, beta[(size_t)i * k + j]); text.push_back(',');
        append_rust_display(text, pval[(size_t)i * k + j]); text.push_back('\n');
    });
    fclose(fo);
}

// GenotypesAndPhenotypes (base/structs_and_traits.rs:139-148) with the matrix resident in HBM: the reference's dense
// n x (1 + p) `intercept_and_allele_frequencies` is here p x ld locus-major on the device, the column of ones implied; the
// three label vectors keep the leading "intercept" entry (sync.rs:1121-1126).
struct GenotypesAndPhenotypes {
    std::vector<std::string> chromosome, allele; // 1 + p entries
    std::vector<uint64_t> position;
    DeviceBuf<double> intercept_and_allele_frequencies;
    int64_t p = 0, ld = 0;
    int n = 0, k = 0;
    std::vector<double> phenotypes;                     // n x k
    std::vector<std::string> pool_names;
    DeviceBuf<double> coverages;                        // laid out like the matrix (pg_load_emit_cov_dev); optional
};


// ---- the analyses: cli_streamed.cpp (run_kinship_streamed: -1 = load the whole file instead), cli_matrix.cpp, cli_popgen.cpp ----
int run_kinship_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, InputKind kind, const PileupFilter &pf, const pg_filter &flt,
                         const RankSetup &rs);
int run_batch_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, Analysis op, InputKind kind, const PileupFilter &pf,
                       const pg_filter &flt, const RankSetup &rs);
GenotypesAndPhenotypes into_genotypes_and_phenotypes(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt,
                                                     bool keep_p_minus_1, bool remove_missing, bool with_coverages, Lap &lap);
std::string ols_with_covariate(Ctx &gpu, GenotypesAndPhenotypes &g, double xxt_eigen_variance_explained,
                               const std::string &fname_input, const std::string &fname_output, int n_threads, Lap &lap, bool mle, bool gpu_writer = false, int64_t slab_rows = 0);
std::string sync2csv(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt, bool keep_p_minus_1, const std::string &out,
                     int64_t slab_rows, Lap &lap);
void write_freq_csv(Ctx &gpu, const SyncBatch &sb, const std::vector<std::string> &pool_names, const double *G, int64_t ld, int n, int64_t p,
                    const int64_t *col_locus_dev, const int32_t *col_allele_dev, const std::string &out, int64_t slab_rows, const char *what,
                    Lap &lap);
std::string impute(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt, const Args &a, const std::string &out, Lap &lap);
int run_popgen(const Args &a, Analysis analysis, Ctx &gpu, const GenotypesAndPhenotypes &g, const std::vector<double> &pool_sizes, Lap &lap);