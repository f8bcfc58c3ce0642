// main.cpp -- `poolgen` command line for the hot subcommands, flag-compatible with the
// reference CLI (src/main.rs:26-143): pileup2sync, fisher_exact_test, chisq_test, pearson_corr, ols_iter, ols_iter_with_kinship
// (and gp_ols as a plain coefficient dump).  Parsing/formatting/ordering follow the reference
// (base/sync.rs:606-970, :972-1180; gwas/ols.rs:255-275, :372-433); all arithmetic on the loci
// is done by libpoolgen_hip.so through its C ABI.  Anything else the reference CLI offers is out
// of scope and reported as such.
#include "host_util.h"
#include "pileup.h"
#include "gpu_mem.h"
#include "piece_reader.h"
#include "../../../include/poolgen_hip.h"
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <climits>
#include <map>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <exception>
#include "gp_cv.h"
#include "operators.h"
#include "rank_gate.h"
#include <numeric>
#include <sstream>
#include <stdexcept>
#include <thread>
#include <time.h>
#include <sys/stat.h>
#include <fcntl.h>
#include <unistd.h>

using namespace pgh;

struct Args {
    std::string analysis, fname, output, phen_fname, phen_delim = ",", phen_format = "default", gwalpha_method = "ML";
    double max_base_error_rate = 0.01, min_coverage_breadth = 1.0, min_allele_frequency = 0.001,
           max_missingness_rate = 0.0, xxt = 0.75;
    uint64_t min_coverage_depth = 1;
    bool keep_ns = false, keep_p_minus_1 = false, generate_plots = false, sig_only = false, keep_lowercase_reference = false;
    int phen_name_col = 0, phen_pool_size_col = 1, n_threads = 1;
    long stream_chunk_mb = -1; // ols_iter_with_kinship: pieces of this size are parsed / copied / loaded in turn (-1 = automatic)
    std::vector<int> phen_value_col{2};
    int k_folds = 10, n_reps = 3; // genomic_prediction_cross_validation (main.rs:104-109)
    uint64_t seed = 42;           // ... and the seed of its folds (an extension: the reference's folds are unrepeatable)
    uint64_t window_size_bp = 100, window_slide_size_bp = 50, min_loci_per_window = 10; // fst / heterozygosity (main.rs:110-118)
    // watterson_estimator / tajima_d (an extension): the pool sizes as the phenotype file has them and every locus of a window
    // counted, instead of the reference's fractions and its count
    bool popgen_as_documented = false;
    double sigma_threshold = 2.0, recombination_rate_cm_per_mb = 0.73; // gudmc (main.rs:119-128)
    // multi-GPU (an extension: the reference's parallel axis is --n-threads, one worker per file chunk, sync.rs:913-939):
    // the input is cut into one contiguous byte range per GPU, each with its own parser threads.  0 = flag absent.
    int n_gpus = 0;
    std::vector<int> gpu_ids; // device ordinals of the ranks (default 0, 1, .., n_gpus - 1)
};

static double parse_valid_freq(const std::string &v, const std::string &flag) { // helpers.rs:93-100
    double x = 0.0;
    if (!parse_f64_strict(v, x)) throw std::runtime_error("`" + v + "` isn't a valid number (" + flag + ")");
    if (x < 0.0 || x > 1.0) throw std::runtime_error("Value must be between 0.0 and 1.0, got `" + rust_display(x) + "` (" + flag + ")");
    return x;
}

// integer flag values as clap's `parse::<usize / u64>()` reads them: digits only, nothing after them, no sign for the unsigned
static uint64_t flag_u64(const std::string &v, const std::string &flag) {
    uint64_t x = 0;
    if (!parse_u64_strict(v, x)) throw std::runtime_error("invalid value `" + v + "` for " + flag + ": a non-negative integer is expected");
    return x;
}
static int flag_int(const std::string &v, const std::string &flag, int64_t lo = 0) {
    int64_t x = 0;
    if (!parse_i64_strict(v, x) || x < lo || x > INT32_MAX)
        throw std::runtime_error("invalid value `" + v + "` for " + flag + ": an integer >= " + std::to_string(lo) + " is expected");
    return (int)x;
}

static const char *USAGE =
    "poolgen <analysis> -f <input> -p <phenotypes.csv> [flags]      (MI355X build of the per-locus regression path)\n"
    "analyses: pileup2sync, fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship,\n"
    "          mle_iter_with_kinship, genomic_prediction_cross_validation, fst, heterozygosity, watterson_estimator, tajima_d,\n"
    "          gudmc\n"
    "  -f, --fname <file>                 *.sync, or *.pileup / *.mpileup (converted in memory: exactly what pileup2sync followed by the\n"
    "                                     analysis on its sync file gives -- including the reference's column quirk: pileup2sync\n"
    "                                     writes A:T:C:G:DEL:N, the sync reader labels the columns A,T,C,G,N,DEL, so on pileup-derived\n"
    "                                     counts the default N removal drops the DELETION column and --keep-ns keeps it)\n"
    "  -p, --phen-fname <file>            delimited file: pool name, pool size, trait value(s)\n"
    "  -o, --output <file>                must not exist; default: derived from the input name and the time\n"
    "      --phen-delim <,>  --phen-name-col <0>  --phen-pool-size-col <1>  --phen-value-col <2[,3..]>\n"
    "      --phen-format <default|gwalpha_fmt>   gwalpha_fmt: the GWAlpha.py file (Pheno_name=, sig=, MIN=, MAX=, perc=[..], q=[..]); gwalpha needs it\n"
    "      --gwalpha-method <ML|LS>        gwalpha: maximum likelihood (the default, and what any other value means) or least squares\n"
    "      --max-base-error-rate <0.01>  --min-coverage-depth <1>  --min-coverage-breadth <1.0>\n"
    "      --min-allele-frequency <0.001>  --max-missingness-rate <0.0>  --keep-ns  --keep-lowercase-reference\n"
    "      --keep-p-minus-1                drop the major allele of every locus when loading the matrix\n"
    "  -x, --xxt-eigen-variance-explained <0.75>   ols_iter_with_kinship: the n_eigenvecs rule's threshold\n"
    "      --k-folds <10>  --n-reps <3>  --seed <42>     genomic_prediction_cross_validation\n"
    "      --window-size-bp <100>  --window-slide-size-bp <50>  --min-loci-per-window <10>   fst, heterozygosity, watterson_estimator, tajima_d, gudmc\n"
    "      --sigma-threshold <2.0>  --recombination-rate-cm-per-mb <0.73>   gudmc: |D - mean| from which a window counts as a peak or\n"
    "                                      trough (not scaled by the fitted sd, as in the reference), and the rate behind the expected width\n"
    "      --popgen-as-documented          watterson_estimator, tajima_d, gudmc: use the pool sizes as the phenotype file has them and count\n"
    "                                      the polymorphic loci of every window.  Default: the reference's behaviour -- pool sizes as\n"
    "                                      fractions of their sum (its harmonic sums are then empty: every value is inf or NaN) and\n"
    "                                      its count, which looks the flag up at the window's index instead of the locus\n"
    "      --n-threads <1>                 parser / writer threads\n"
    "      --stream-chunk-mb <N>           size of the pieces the input is taken in (0: whole file, kinship path only)\n"
    "      --n-gpus <N>  [--gpu-ids a,b,..]  fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship: one contiguous\n"
    "                                      part of the input per GPU (own parser threads: --n-threads is the total); the kinship sums are\n"
    "                                      all-reduced over the GPUs with RCCL; the kinship path then needs an input sorted by\n"
    "                                      (chromosome, position)\n"
    "environment: PGH_TIMING=1 prints the phases' wall-clock on stderr\n";

static Args parse_args(int argc, char **argv) {
    Args a;
    for (int i = 1; i < argc; ++i)
        if (std::string(argv[i]) == "-h" || std::string(argv[i]) == "--help") { std::cout << USAGE; std::exit(0); }
    std::vector<std::string> pos;
    for (int i = 1; i < argc; ++i) {
        std::string k = argv[i], v;
        auto eq = k.find('=');
        bool has_v = false;
        if (k.rfind("--", 0) == 0 && eq != std::string::npos) { v = k.substr(eq + 1); k = k.substr(0, eq); has_v = true; }
        auto val = [&]() -> std::string {
            if (has_v) return v;
            if (i + 1 >= argc) throw std::runtime_error("missing value for " + k);
            return argv[++i];
        };
        if (k == "-f" || k == "--fname") a.fname = val();
        else if (k == "-o" || k == "--output") a.output = val();
        else if (k == "-p" || k == "--phen-fname") a.phen_fname = val();
        else if (k == "--phen-delim") a.phen_delim = val();
        else if (k == "--phen-format") a.phen_format = val();
        else if (k == "--gwalpha-method") a.gwalpha_method = val();
        else if (k == "--phen-name-col") a.phen_name_col = flag_int(val(), k);
        else if (k == "--phen-pool-size-col") a.phen_pool_size_col = flag_int(val(), k);
        else if (k == "--phen-value-col") {
            a.phen_value_col.clear();
            std::stringstream ss(val());
            std::string t;
            while (std::getline(ss, t, ',')) a.phen_value_col.push_back(flag_int(t, k));
        } else if (k == "--n-threads") a.n_threads = flag_int(val(), k, 1);
        else if (k == "--max-base-error-rate") a.max_base_error_rate = parse_valid_freq(val(), k);
        else if (k == "--min-coverage-breadth") a.min_coverage_breadth = parse_valid_freq(val(), k);
        else if (k == "--min-coverage-depth") a.min_coverage_depth = flag_u64(val(), k);
        else if (k == "--min-allele-frequency") a.min_allele_frequency = parse_valid_freq(val(), k);
        else if (k == "--max-missingness-rate") a.max_missingness_rate = parse_valid_freq(val(), k);
        else if (k == "-x" || k == "--xxt-eigen-variance-explained") a.xxt = parse_valid_freq(val(), k);
        else if (k == "--keep-ns") a.keep_ns = true;
        else if (k == "--keep-p-minus-1") a.keep_p_minus_1 = true;
        else if (k == "--generate-plots") a.generate_plots = true;
        else if (k == "--output-sig-snps-only") a.sig_only = true;
        else if (k == "--keep-lowercase-reference") a.keep_lowercase_reference = true; // pileup inputs only (pileup.rs:280-299)
        else if (k == "--stream-chunk-mb") a.stream_chunk_mb = flag_int(val(), k);
        else if (k == "--n-gpus") a.n_gpus = flag_int(val(), k, 1);
        else if (k == "--gpu-ids") {
            std::stringstream ss(val());
            std::string t;
            while (std::getline(ss, t, ',')) a.gpu_ids.push_back(flag_int(t, k));
        }
        else if (k == "--k-folds") a.k_folds = flag_int(val(), k, 1);
        else if (k == "--n-reps") a.n_reps = flag_int(val(), k, 1);
        else if (k == "--seed") a.seed = flag_u64(val(), k);
        else if (k == "--window-size-bp") a.window_size_bp = flag_u64(val(), k);
        else if (k == "--window-slide-size-bp") a.window_slide_size_bp = flag_u64(val(), k);
        else if (k == "--min-loci-per-window") a.min_loci_per_window = flag_u64(val(), k);
        else if (k == "--popgen-as-documented") a.popgen_as_documented = true;
        else if (k == "--sigma-threshold") {
            const std::string t = val();
            if (!parse_f64_strict(t, a.sigma_threshold)) throw std::runtime_error("`" + t + "` isn't a valid number (" + k + ")");
        } else if (k == "--recombination-rate-cm-per-mb") a.recombination_rate_cm_per_mb = parse_valid_freq(val(), k);
        else if (k.rfind("-", 0) == 0) throw std::runtime_error("unknown flag " + k);
        else pos.push_back(k);
    }
    if (pos.size() != 1) throw std::runtime_error("usage: poolgen <analysis> -f <sync> -p <phen.csv> [flags]   (--help lists them)");
    a.analysis = pos[0];
    if (a.fname.empty() || a.phen_fname.empty()) throw std::runtime_error("-f/--fname and -p/--phen-fname are required");
    if (!a.gpu_ids.empty()) {
        if (a.n_gpus == 0) a.n_gpus = (int)a.gpu_ids.size();
        if ((int)a.gpu_ids.size() != a.n_gpus) throw std::runtime_error("--gpu-ids must list exactly --n-gpus devices");
    }
    return a;
}

static PileupFilter pileup_filter(const Args &a, const std::vector<double> &pool_sizes) {
    PileupFilter pf;
    pf.remove_ns = !a.keep_ns;
    pf.keep_lowercase_reference = a.keep_lowercase_reference;
    pf.max_base_error_rate = a.max_base_error_rate;
    pf.min_coverage_depth = a.min_coverage_depth;
    pf.min_coverage_breadth = a.min_coverage_breadth;
    pf.min_allele_frequency = a.min_allele_frequency;
    pf.pool_sizes = pool_sizes;
    return pf;
}

static std::string basename_no_ext(const std::string &f) { // sync.rs:889-902
    const auto p = f.rfind('.');
    return p == std::string::npos ? std::string() : f.substr(0, p);
}

static std::string unix_time_string() {
    const double t = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    return rust_display(t);
}

// OpenOptions::create_new: refuse to overwrite (sync.rs:906, :942-947; ols.rs:285, :402-407)
static FILE *create_new(const std::string &path) {
    const int fd = ::open(path.c_str(), O_WRONLY | O_CREAT | O_EXCL, 0644);
    if (fd < 0) throw std::runtime_error("Unable to create file: " + path + " (it must not exist)");
    return fdopen(fd, "w");
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
static std::vector<int> complete_pools(const Phen &ph) {
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
static void stamp(const char *what) { // PGH_TIMING=1: the wall clock itself, so that a wrapper can see what lies outside the laps
    if (!std::getenv("PGH_TIMING")) return;
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    std::fprintf(stderr, "poolgen: clock at %-15s %lld.%09ld\n", what, (long long)ts.tv_sec, ts.tv_nsec);
}
static int done_ok() {
    stamp("exit");
    std::cout.flush();
    std::cerr.flush();
    std::fflush(nullptr);
    if (!std::getenv("PGH_CLEAN_EXIT")) ::_exit(0);
    return 0;
}

// ---------------------------------------------------------------------------------------------------------
// ols_iter_with_kinship on an input that is read in PIECES (config 5 of BASELINE.json: a file far larger than
// host memory): while the GPU takes piece c (H2D from pinned memory, loader, partial kinship), the worker
// threads already parse piece c + 1 into the other pinned buffer.  The frequency matrix stays resident in HBM
// piece by piece (288 GB hold 180 M columns of 200 pools); the host only keeps labels and results.
// The input must be sorted by (chromosome, position) -- what the whole-file path obtains by sorting
// (sync.rs:1092-1101) cannot be had across pieces -- and that is checked.
// ---------------------------------------------------------------------------------------------------------
struct UnsortedInput : std::runtime_error { using std::runtime_error::runtime_error; };

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

static RankSetup rank_setup(const Args &a, bool need_comm) {
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
static std::vector<int> deal_pieces(int npieces, int n_ranks) {
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
};

static LoadedMatrix load_matrix(Ctx &gpu, const uint32_t *counts_dev, int64_t L, int n, const std::vector<double> &pool_sizes,
                                const pg_filter &flt, bool keep_p_minus_1, const int64_t *order_dev, const std::vector<int32_t> &pool_map,
                                int n2, int64_t ld, bool with_coverages) {
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

struct KinRank {
    int rank = 0, device = 0, threads = 1, c0 = 0, c1 = 0;
    std::unique_ptr<Ctx> own;
    Ctx *gpu = nullptr;
    // the rank's pieces of the frequency matrix, resident in HBM (owned: an exception on the way -- unsorted input, out of memory --
    // must not leave the pieces behind: the caller may fall back to the whole-file path)
    std::vector<DeviceBuf<double>> Gs;
    std::vector<int64_t> ps;
    std::vector<std::string> chrom_names;             // the rank's dictionary
    std::vector<int32_t> lab_chr;                     // per column
    std::vector<uint64_t> lab_pos;
    std::vector<char> lab_al;
    std::vector<double> S_total;
    DeviceBuf<double> S_dev;
    std::string first_chrom, last_chrom;
    uint64_t first_pos = 0, last_pos = 0;
    bool have_last = false;
    int64_t p = 0, col0 = 0;
    int m = 0;
    double t_wait = 0, t_host = 0, t_gpu = 0;
};

static int run_kinship_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, size_t chunk_bytes, bool is_pileup,
                                const PileupFilter &pf, const pg_filter &flt, const RankSetup &rs) {
    const MappedFile mf(a.fname);
    const int R = rs.n_ranks;
    const size_t want_pieces = std::max<size_t>((size_t)R, (mf.size() + chunk_bytes - 1) / chunk_bytes);
    const std::vector<size_t> cuts = mf.cuts(want_pieces);
    const int nchunks = (int)cuts.size() - 1;
    const int n = ph.n, k = ph.k;
    const std::vector<int> keep = complete_pools(ph); // remove_missing (ols.rs:287)
    if (keep.empty()) throw std::runtime_error("All pools have missing data. Please check the phenotype file.");
    const int n2 = (int)keep.size();
    const int64_t ld = n2 + (n2 & 1);
    std::vector<int32_t> pool_map(n, -1);
    for (int i = 0; i < n2; ++i) pool_map[keep[i]] = i;
    const std::vector<int> first = deal_pieces(nchunks, R);
    std::vector<KinRank> ranks(R);
    for (int r = 0; r < R; ++r) {
        ranks[r].rank = r; ranks[r].device = rs.devices[r]; ranks[r].threads = rs.threads[r];
        ranks[r].c0 = first[r]; ranks[r].c1 = first[r + 1];
    }
    auto clk = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };

    // every rank's context is created here, on the main thread: a GPU that cannot be opened ends the run before any rank
    // thread exists
    for (int r = 0; r < R; ++r) {
        KinRank &K = ranks[r];
        hip_ok(hipSetDevice(K.device), "hipSetDevice");
        if (r == 0 && gpu0.device == K.device) K.gpu = &gpu0;
        else { K.own.reset(new Ctx(K.device)); K.gpu = K.own.get(); }
    }
    RankGate gate(R);
    // ---- phase A, per rank: parse piece c + 1 || H2D + loader + partial kinship of piece c -----------------------
    run_ranks(R, [&](int r) {
        KinRank &K = ranks[r];
        Ctx &gpu = *K.gpu;
        gate.pass([&] {
            hip_ok(hipSetDevice(K.device), "hipSetDevice");
            K.S_total.assign((size_t)n2 * n2, 0.0);
            K.S_dev.reset(sizeof(double) * n2 * n2);
        });
        if (rs.rccl) // collective over the rank threads: entered by all of them or by none, and its outcome agreed on
            gate.pass([&] { gpu.ok(pg_comm_init_rank(gpu.c, rs.id, R, r), "RCCL communicator"); });
        if (K.c0 >= K.c1) return;
        // (the pinned slots, the counts and the 16-bit scratch live to the end of this phase only)
        PieceReader pieces(mf, cuts, K.c0, K.c1, K.device, K.threads, is_pileup, pf, n, true);
        std::vector<double> S_piece((size_t)n2 * n2);
        DeviceBuf<uint32_t> counts_dev;
        CountsUpload upload;
        while (pieces.more()) {
            double t0 = clk();
            SyncBatch sb = pieces.next();
            K.t_wait += clk() - t0; t0 = clk();
            if (sb.L == 0) continue;
            if (sb.n != n) throw std::runtime_error("the number of pools in the input and in the phenotype file differ");
            for (int64_t l = 0; l < sb.L; ++l) { // sortedness, within and across the rank's pieces
                const std::string &ch = sb.chrom(l);
                if (K.have_last) {
                    const int cmp = K.last_chrom.compare(ch);
                    if (cmp > 0 || (cmp == 0 && K.last_pos > sb.pos[l]))
                        throw UnsortedInput("streamed ols_iter_with_kinship needs the input sorted by chromosome and position (line of " +
                                            ch + ":" + std::to_string(sb.pos[l]) + "); use --stream-chunk-mb 0 to load the whole file");
                    if (cmp != 0) K.last_chrom = ch;
                } else { K.last_chrom = ch; K.have_last = true; K.first_chrom = ch; K.first_pos = sb.pos[l]; }
                K.last_pos = sb.pos[l];
            }
            K.t_host += clk() - t0; t0 = clk();
            counts_dev.reserve(sizeof(uint32_t) * (size_t)sb.L * n * 6, "device memory for the counts");
            upload(gpu, sb, counts_dev.get());
            LoadedMatrix piece = load_matrix(gpu, counts_dev.get(), sb.L, n, ph.pool_sizes, flt, a.keep_p_minus_1, nullptr, pool_map, n2, ld, false);
            const int64_t pc = piece.p;
            if (pc == 0) continue;
            const double *G = piece.G.get();
            K.Gs.push_back(std::move(piece.G));
            K.ps.push_back(pc);
            K.t_gpu += clk() - t0; t0 = clk();
            std::vector<int32_t> remap(sb.chrom_names.size());
            for (size_t i = 0; i < sb.chrom_names.size(); ++i) {
                int g = -1;
                for (size_t j = 0; j < K.chrom_names.size(); ++j) if (K.chrom_names[j] == sb.chrom_names[i]) { g = (int)j; break; }
                if (g < 0) { K.chrom_names.push_back(sb.chrom_names[i]); g = (int)K.chrom_names.size() - 1; }
                remap[i] = g;
            }
            for (int64_t q = 0; q < pc; ++q) {
                K.lab_chr.push_back(remap[sb.chrom_id[piece.col_locus[q]]]);
                K.lab_pos.push_back(sb.pos[piece.col_locus[q]]);
                K.lab_al.push_back(ALLELES[piece.col_allele[q]]);
            }
            K.t_host += clk() - t0; t0 = clk();
            gpu.ok(pg_kinship_partial_dev(gpu.c, G, pc, n2, ld, K.S_dev.get()), "kinship");
            hip_ok(hipMemcpy(S_piece.data(), K.S_dev.get(), sizeof(double) * n2 * n2, hipMemcpyDeviceToHost), "D2H kinship");
            for (size_t i = 0; i < K.S_total.size(); ++i) K.S_total[i] += S_piece[i];
            K.p += pc;
            K.t_gpu += clk() - t0;
        }
    });
    if (std::getenv("PGH_TIMING"))
        for (const KinRank &K : ranks)
            std::fprintf(stderr, "poolgen: rank %d (GPU %d, pieces %d..%d, %d parser threads): waited for the parser %.3f s, host bookkeeping %.3f s, copies + device %.3f s\n",
                         K.rank, K.device, K.c0, K.c1, K.threads, K.t_wait, K.t_host, K.t_gpu);
    lap("pieces: parse | H2D + loader + partial kinship");
    // ---- between the phases: the order across ranks, the global column offsets ------------------------------------
    int64_t p = 0;
    const KinRank *prev = nullptr;
    for (KinRank &K : ranks) {
        K.col0 = p;
        p += K.p;
        if (!K.have_last) continue;
        if (prev) {
            const int cmp = prev->last_chrom.compare(K.first_chrom);
            if (cmp > 0 || (cmp == 0 && prev->last_pos > K.first_pos))
                throw UnsortedInput("streamed ols_iter_with_kinship needs the input sorted by chromosome and position (line of " +
                                    K.first_chrom + ":" + std::to_string(K.first_pos) + "); use --stream-chunk-mb 0 to load the whole file");
        }
        prev = &K;
    }
    if (p <= 0) throw std::runtime_error("no loci passed the filters");
    std::vector<double> Y;
    for (int i : keep) for (int j = 0; j < k; ++j) Y.push_back(ph.phen[(size_t)i * k + j]);
    if (!a.output.empty()) { FILE *t = create_new(a.output); fclose(t); ::unlink(a.output.c_str()); } // ols.rs:285
    std::vector<double> S_host; // PGH_COMM=host, or no communicator at all: the ranks' sums added in rank order
    if (!rs.rccl) {
        S_host.assign((size_t)n2 * n2, 0.0);
        for (const KinRank &K : ranks)
            for (size_t i = 0; i < S_host.size(); ++i) S_host[i] += K.S_total[i];
    }
    // ---- phase B, per rank: all-reduce of the kinship sums, the n x n step (replicated), the rank's sweeps ---------
    std::vector<double> beta((size_t)p * k), pval((size_t)p * k);
    run_ranks(R, [&](int r) {
        KinRank &K = ranks[r];
        Ctx &gpu = *K.gpu;
        gate.pass([&] {
            hip_ok(hipSetDevice(K.device), "hipSetDevice");
            hip_ok(hipMemcpy(K.S_dev.get(), rs.rccl ? K.S_total.data() : S_host.data(), sizeof(double) * n2 * n2, hipMemcpyHostToDevice), "H2D kinship");
        });
        if (rs.rccl) gpu.ok(pg_allreduce_sum_dev(gpu.c, K.S_dev.get(), (int64_t)n2 * n2), "RCCL all-reduce of the kinship sums");
        gpu.ok(pg_kinship_set(gpu.c, K.S_dev.get(), p, n2, Y.data(), k, a.xxt, -1, &K.m, nullptr, nullptr), "ols_iter_with_kinship");
        int64_t off = K.col0;
        for (size_t c = 0; c < K.Gs.size(); ++c) {
            const size_t cnt = (size_t)K.ps[c] * k;
            DeviceBuf<double> out_dev(sizeof(double) * 3 * cnt, "device memory for the results");
            gpu.ok(pg_ols_sweep_dev(gpu.c, K.Gs[c].get(), K.ps[c], n2, ld, out_dev.get(), out_dev.get() + cnt, out_dev.get() + 2 * cnt), "ols_iter_with_kinship");
            gpu.ok(pg_synchronize(gpu.c), "ols_iter_with_kinship");
            hip_ok(hipMemcpy(beta.data() + (size_t)off * k, out_dev.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
            hip_ok(hipMemcpy(pval.data() + (size_t)off * k, out_dev.get() + 2 * cnt, sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
            K.Gs[c].reset(); // a piece leaves HBM right after its sweep
            off += K.ps[c];
        }
        K.Gs.clear();
    });
    const int m = ranks[0].m;
    for (const KinRank &K : ranks)
        if (K.m != m) throw std::runtime_error("internal error: the ranks disagree on n_eigenvecs");
    lap("all-reduce + eigen rule + fits + D2H");
    std::string out = a.output;
    if (out.empty()) // ols.rs:393-398
        out = basename_no_ext(a.fname) + "-ols_iterative_xxt_" + std::to_string(m + 1) + "_eigens-" + unix_time_string() + ".csv";
    // label of global column q: the rank whose range holds it
    std::vector<int64_t> starts;
    for (const KinRank &K : ranks) starts.push_back(K.col0);
    write_kinship_csv(out, p, k, beta, pval, a.n_threads, [&](int64_t i, std::string &text) {
        // coefficient i carries label i of the (1+p)-long vectors whose entry 0 is "intercept" (ols.rs:421-425)
        if (i == 0) { text += "intercept,0,intercept"; return; }
        const int64_t q = i - 1;
        const int r = (int)(std::upper_bound(starts.begin(), starts.end(), q) - starts.begin()) - 1;
        const KinRank &K = ranks[r];
        const int64_t c = q - K.col0;
        text += K.chrom_names[K.lab_chr[c]]; text += ","; text += std::to_string(K.lab_pos[c]); text += ","; text.push_back(K.lab_al[c]);
    });
    lap("format + write CSV");
    std::cout << out << "\n";
    return done_ok();
}

// fisher_exact_test / chisq_test / pearson_corr / ols_iter / gwalpha (main.rs:245-271, :335-356): the per-locus operators know nothing beyond their own line, so
// the file is taken in pieces whatever its size -- the worker threads parse piece c + 1 into one of two pinned buffers
// (16-bit counts when they fit) while the GPU takes piece c and its rows are formatted and appended, in file order
// (sync.rs:927-946).  Nothing of the size of the input is ever allocated, pinned or copied in one go.
static int run_batch_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, Analysis op, size_t chunk_bytes, bool is_pileup,
                              const PileupFilter &pf, const pg_filter &flt, const RankSetup &rs) {
    const MappedFile mf(a.fname);
    const int R = rs.n_ranks;
    const std::vector<size_t> cuts = mf.cuts(std::max<size_t>((size_t)R, (mf.size() + chunk_bytes - 1) / chunk_bytes));
    const int nchunks = (int)cuts.size() - 1;
    const std::vector<int> first = deal_pieces(nchunks, R);
    // gwalpha: one statistic per row, no p-value; its phenotype matrix carries (bins, q', [sig, MIN, MAX]) instead of traits
    const bool gwa = op == Analysis::gwalpha;
    const int n = ph.n, k = gwa ? 1 : ph.k;
    std::vector<double> gw_q(gwa ? n : 0);
    for (int i = 0; gwa && i < n; ++i) gw_q[i] = ph.phen[(size_t)i * 3 + 1];
    const int gw_method = a.gwalpha_method == "LS" ? PG_GWALPHA_LS : PG_GWALPHA_ML; // main.rs:337-356: anything but LS is ML
    std::string out = a.output;
    if (out.empty()) out = basename_no_ext(a.fname) + "-" + unix_time_string() + "-" + a.analysis + ".csv"; // sync.rs:903
    { FILE *t = create_new(out); fclose(t); ::unlink(out.c_str()); } // probe, as the reference does before any work (sync.rs:906)
    // ols_iter drops the pools without phenotype first (ols.rs:206); pearson_corr keeps every pool (pairwise-complete inside)
    std::vector<int> keep(n);
    std::iota(keep.begin(), keep.end(), 0);
    std::vector<double> Y = ph.phen, ps = ph.pool_sizes;
    if (op == Analysis::ols_iter) {
        keep = complete_pools(ph);
        if (keep.empty()) throw std::runtime_error("All pools have missing data. Please check the phenotype file.");
        if ((int)keep.size() != n) {
            std::cerr << "warning: " << n - keep.size() << " pools without phenotype removed (pool sizes subset accordingly)\n";
            Y.clear(); ps.clear();
            for (int i : keep) { ps.push_back(ph.pool_sizes[i]); for (int j = 0; j < k; ++j) Y.push_back(ph.phen[(size_t)i * k + j]); }
        }
    }
    const int n2 = (int)keep.size();
    const bool subset = n2 != n;
    const bool tables = counts_only(op); // chisq_test, fisher_exact_test
    const char *header = tables ? "#chr,pos,alleles,statistic,pvalue\n"                    // sync.rs:766
                                   : "#chr,pos,alleles,freq,phenotype,statistic,pvalue\n"; // sync.rs:950
    // One rank = one contiguous range of pieces, one GPU, its own pinned buffers and parser threads, and -- when there are
    // several -- its own part file, like the reference's one `.tmp` file per worker thread (sync.rs:794-870), concatenated in
    // rank order afterwards (sync.rs:951-968).  No exchange between the ranks: a locus needs nothing beyond its own line.
    std::vector<int64_t> totals(R, 0);
    std::vector<std::string> part(R);
    for (int r = 0; r < R; ++r) part[r] = R == 1 ? out : out + ".rank" + std::to_string(r) + ".tmp";
    auto cleanup_parts = [&] { if (R > 1) for (auto &f : part) ::unlink(f.c_str()); };
    try {
    run_ranks(R, [&](int r) {
        const int device = rs.devices[r], threads = rs.threads[r];
        hip_ok(hipSetDevice(device), "hipSetDevice");
        std::unique_ptr<Ctx> own;
        Ctx *gp = &gpu0;
        if (!(r == 0 && gpu0.device == device)) { own.reset(new Ctx(device)); gp = own.get(); }
        Ctx &gpu = *gp;
        const int c0 = first[r], c1 = first[r + 1];
        if (c0 >= c1) return;
        PieceReader pieces(mf, cuts, c0, c1, device, threads, is_pileup, pf, 0, !subset);
        FILE *fo = nullptr;
        DeviceBuf<uint32_t> counts_dev;
        DeviceBuf<int32_t> n_out_dev, ids_dev;
        DeviceBuf<double> mf_dev, stat_dev, pv_dev;
        int64_t cap_loci = 0;
        CountsUpload upload;
        std::vector<uint32_t> counts2;
        std::vector<int32_t> n_out, ids;
        std::vector<double> mfq, stat, pv;
        const size_t per_stat = tables ? 1 : (size_t)PG_MAX_OUT * k;
        while (pieces.more()) {
            SyncBatch sb = pieces.next();
            if (sb.L == 0) continue;
            if (sb.n != n) throw std::runtime_error("the number of pools in the sync file and in the phenotype file differ");
            const int64_t L = sb.L;
            totals[r] += L;
            if (L > cap_loci) {
                cap_loci = L + L / 8;
                counts_dev.reset(sizeof(uint32_t) * (size_t)cap_loci * n * 6, "device memory for the counts");
                n_out_dev.reset(sizeof(int32_t) * cap_loci);
                ids_dev.reset(sizeof(int32_t) * cap_loci * PG_MAX_OUT);
                mf_dev.reset(sizeof(double) * cap_loci * PG_MAX_OUT);
                stat_dev.reset(sizeof(double) * cap_loci * per_stat);
                pv_dev.reset(sizeof(double) * cap_loci * per_stat);
            }
            if (subset) { // rare: drop the pools without phenotype on the host (32-bit counts), then one copy
                counts2.resize((size_t)L * n2 * 6);
                for (int64_t l = 0; l < L; ++l)
                    for (int i = 0; i < n2; ++i) std::memcpy(&counts2[((size_t)l * n2 + i) * 6], &sb.counts[((size_t)l * n + keep[i]) * 6], 24);
                hip_ok(hipMemcpy(counts_dev.get(), counts2.data(), sizeof(uint32_t) * counts2.size(), hipMemcpyHostToDevice), "H2D counts");
            } else
                upload(gpu, sb, counts_dev.get());
            if (gwa) // sig, MIN, MAX: rows 0..2 of the matrix' third column (gwalpha.rs:214-216)
                gpu.ok(pg_gwalpha_batch_dev(gpu.c, counts_dev.get(), L, n2, ps.data(), gw_q.data(), ph.phen[2], ph.phen[5], ph.phen[8], &flt, gw_method,
                                            n_out_dev.get(), ids_dev.get(), mf_dev.get(), stat_dev.get(), nullptr, nullptr, nullptr), "gwalpha");
            else if (op == Analysis::fisher_exact_test)
                gpu.ok(pg_fisher_batch_dev(gpu.c, counts_dev.get(), L, n2, ps.data(), &flt, n_out_dev.get(), ids_dev.get(), stat_dev.get(), pv_dev.get()),
                       "fisher_exact_test");
            else if (op == Analysis::chisq_test)
                gpu.ok(pg_chisq_batch_dev(gpu.c, counts_dev.get(), L, n2, ps.data(), &flt, n_out_dev.get(), ids_dev.get(), stat_dev.get(), pv_dev.get()),
                       "chisq_test");
            else if (op == Analysis::pearson_corr)
                gpu.ok(pg_pearson_batch_dev(gpu.c, counts_dev.get(), L, n2, ps.data(), &flt, Y.data(), k, n_out_dev.get(), ids_dev.get(), mf_dev.get(),
                                            stat_dev.get(), pv_dev.get()), "pearson_corr");
            else
                gpu.ok(pg_ols_iter_batch_dev(gpu.c, counts_dev.get(), L, n2, ps.data(), &flt, Y.data(), k, n_out_dev.get(), ids_dev.get(), mf_dev.get(),
                                             stat_dev.get(), pv_dev.get()), "ols_iter");
            n_out.resize(L); ids.resize((size_t)L * PG_MAX_OUT); mfq.resize((size_t)L * PG_MAX_OUT);
            stat.resize((size_t)L * per_stat); pv.resize((size_t)L * per_stat);
            hip_ok(hipMemcpy(n_out.data(), n_out_dev.get(), sizeof(int32_t) * L, hipMemcpyDeviceToHost), "D2H results");
            // slot-major arrays: the slots any locus of the piece uses are a prefix of every array (one slot on biallelic data)
            int used = 0;
            for (int64_t l = 0; l < L; ++l) used = std::max(used, (int)n_out[l]);
            used = std::min(used, (int)PG_MAX_OUT);
            const size_t per_stat_used = tables ? 1 : (size_t)used * k;
            hip_ok(hipMemcpy(ids.data(), ids_dev.get(), sizeof(int32_t) * L * used, hipMemcpyDeviceToHost), "D2H results");
            if (!tables) hip_ok(hipMemcpy(mfq.data(), mf_dev.get(), sizeof(double) * L * used, hipMemcpyDeviceToHost), "D2H results");
            hip_ok(hipMemcpy(stat.data(), stat_dev.get(), sizeof(double) * L * per_stat_used, hipMemcpyDeviceToHost), "D2H results");
            if (!gwa) hip_ok(hipMemcpy(pv.data(), pv_dev.get(), sizeof(double) * L * per_stat_used, hipMemcpyDeviceToHost), "D2H results");
            if (!fo) {
                fo = create_new(part[r]);
                if (R == 1) fputs(header, fo);
            }
            write_rows_parallel(fo, L, threads, [&](int64_t l, std::string &line) {
                // slot-major arrays: slot i of locus l sits i * L elements after its slot 0
                const size_t so = tables ? (size_t)l : (size_t)l * k;
                format_locus_rows(op, sb.chrom(l), sb.pos[l], n_out[l], &ids[(size_t)l], &mfq[(size_t)l], &stat[so], &pv[so], k, line, (size_t)L);
            });
        }
        if (fo) fclose(fo);
    });
    } catch (...) { cleanup_parts(); throw; }
    int64_t total = 0;
    for (int64_t t : totals) total += t;
    if (total == 0) { cleanup_parts(); throw std::runtime_error("no loci in " + a.fname); }
    if (R > 1) { // header + the ranks' parts in rank order = file order
        FILE *fo = create_new(out);
        fputs(header, fo);
        std::vector<char> buf(8 << 20);
        for (int r = 0; r < R; ++r) {
            if (totals[r] == 0) continue;
            FILE *fi = std::fopen(part[r].c_str(), "rb");
            if (!fi) { fclose(fo); cleanup_parts(); throw std::runtime_error("cannot reopen " + part[r]); }
            size_t got;
            while ((got = std::fread(buf.data(), 1, buf.size(), fi)) > 0)
                if (std::fwrite(buf.data(), 1, got, fo) != got) { fclose(fi); fclose(fo); cleanup_parts(); throw std::runtime_error("write failed (disk full?)"); }
            fclose(fi);
        }
        fclose(fo);
        cleanup_parts();
    }
    lap("pieces: parse | H2D + operator + D2H + format + write");
    std::cout << out << "\n"; // main.rs:507
    return done_ok();
}

// fst (popgen/fst.rs:10-261), heterozygosity = pi (popgen/pi.rs:115-190), watterson_estimator (popgen/watterson_theta.rs:191-289)
// and tajima_d (popgen/tajima_d.rs:10-171) on the loaded matrix: loci and windows on the host (count_loci,
// define_sliding_windows), the per-locus arithmetic and the means on the GPU, the files as written by the reference.
// pool_sizes: watterson_estimator / tajima_d only -- the reference's fractions, or the file's column (--popgen-as-documented).
static int run_popgen(const Args &a, Analysis analysis, Ctx &gpu, const double *G_dev, const double *cov_dev, int64_t p, int n,
                      int64_t ld, const std::vector<std::string> &lab_chr, const std::vector<uint64_t> &lab_pos,
                      const std::vector<std::string> &pool_names, const std::vector<double> &pool_sizes, Lap &lap) {
    const bool is_fst = analysis == Analysis::fst;
    // count_loci (sync.rs:73-97) without the intercept entry: column starts, and each locus' coordinates
    std::vector<int64_t> locus_col;
    std::vector<int32_t> chr_id;
    std::vector<uint64_t> loc_pos;
    std::vector<std::string> loc_chr;
    for (int64_t c = 0; c < p; ++c)
        if (c == 0 || lab_chr[c] != lab_chr[c + 1] || lab_pos[c] != lab_pos[c + 1]) { // labels carry the intercept at [0]
            locus_col.push_back(c);
            if (!loc_chr.empty() && loc_chr.back() == lab_chr[c + 1]) chr_id.push_back(chr_id.back());
            else chr_id.push_back(chr_id.empty() ? 0 : chr_id.back() + 1);
            loc_chr.push_back(lab_chr[c + 1]);
            loc_pos.push_back(lab_pos[c + 1]);
        }
    locus_col.push_back(p);
    const int64_t L = (int64_t)loc_pos.size();
    std::vector<int64_t> wh(L), wt(L);
    const int64_t nw = pg_host_sliding_windows(chr_id.data(), loc_pos.data(), L, a.window_size_bp, a.window_slide_size_bp,
                                               a.min_loci_per_window, wh.data(), wt.data());
    wh.resize(nw); wt.resize(nw);
    const std::string win = std::to_string(a.window_size_bp);
    const std::string time = unix_time_string();
    if (analysis == Analysis::gudmc) {
        // gudmc (popgen/gudmc.rs:64-462): tajima_d and fst as above, then the fits, widths and p-values on the GPU, one row per
        // (pair, row of population b).  The reference reads both tables back from text and takes their labels apart:
        for (const std::string &c : loc_chr)
            if (c.find('-') != std::string::npos) // "Window-<chr>_<ini>_<fin>".split("-")[1] (:169)
                throw std::runtime_error("gudmc: chromosome name `" + c + "` contains `-`; the reference splits its window labels at `-` and fails on it");
        for (int i = 0; i < n; ++i) {
            if (pool_names[i].find("_vs_") != std::string::npos) // "<a>_vs_<b>".split("_vs_") (:231)
                throw std::runtime_error("gudmc: pool name `" + pool_names[i] + "` contains `_vs_`; the reference splits its pair labels there");
            for (int j = 0; j < i; ++j)
                if (pool_names[i] == pool_names[j]) // position() finds the first of them (:298)
                    throw std::runtime_error("gudmc: pool name `" + pool_names[i] + "` occurs twice; the reference matches populations by name");
        }
        if (nw <= 0) throw std::runtime_error("There were no windows defined. Please check the sync file, the window size, slide size, and the minimum number of loci per window.");
        std::vector<int64_t> wc, wseed, wslot;
        if (!a.popgen_as_documented) {
            std::cerr << "note: gudmc reproduces the reference: the pool sizes are fractions of their sum, so every Tajima's D is NaN, no population has a row "
                         "and the file is the header alone; --popgen-as-documented uses the pool sizes as written and counts every locus\n";
            std::vector<int64_t> h2(L), t2(L);
            wc.resize(L); wseed.resize(L); wslot.resize(L);
            const int64_t nw2 = pg_host_watterson_windows(chr_id.data(), loc_pos.data(), L, a.window_size_bp, a.window_slide_size_bp,
                                                          a.min_loci_per_window, h2.data(), t2.data(), wc.data(), wseed.data(), wslot.data());
            h2.resize(nw2); t2.resize(nw2);
            if (h2 != wh || t2 != wt) throw std::runtime_error("internal error: the two window loops disagree");
        }
        const size_t nn = (size_t)n * n, wn = (size_t)nw * n, rows_all = nn * (size_t)nw;
        // A window whose tail lies before its head (the stale tail of a ditched last slot; the reference's own gudmc test has one,
        // gudmc.rs:500-510) is an empty slice there: mean_axis gives None and both tables hold NaN (pi.rs:87-90, fst.rs:194-197).
        // The tajima_d and fst entry points refuse such a window, so they see the others and its rows stay NaN.
        std::vector<int64_t> keep, kh, kt, kc, ksd, ksl;
        for (int64_t w = 0; w < nw; ++w)
            if (wh[w] <= wt[w]) {
                keep.push_back(w); kh.push_back(wh[w]); kt.push_back(wt[w]);
                if (!wc.empty()) { kc.push_back(wc[w]); ksd.push_back(wseed[w]); ksl.push_back(wslot[w]); }
            }
        const int64_t nk = (int64_t)keep.size();
        const int64_t *c = kc.empty() ? nullptr : kc.data(), *sd = kc.empty() ? nullptr : ksd.data(), *sl = kc.empty() ? nullptr : ksl.data();
        std::vector<double> dw(wn, std::nan("")), fw((size_t)nw * nn, std::nan(""));
        if (nk > 0) {
            std::vector<double> dk((size_t)nk * n), dm(n), fm(nn), fk((size_t)nk * nn);
            gpu.ok(pg_tajima_d_dev(gpu.c, G_dev, cov_dev, p, n, ld, locus_col.data(), L, kh.data(), kt.data(), c, sd, sl, nk, pool_sizes.data(),
                                   dk.data(), dm.data(), nullptr, nullptr), "gudmc (tajima_d)");
            gpu.ok(pg_fst_dev(gpu.c, G_dev, cov_dev, p, n, ld, locus_col.data(), L, kh.data(), kt.data(), nk, fm.data(), fk.data()), "gudmc (fst)");
            for (int64_t q = 0; q < nk; ++q) {
                std::copy(dk.begin() + (size_t)q * n, dk.begin() + (size_t)(q + 1) * n, dw.begin() + (size_t)keep[q] * n);
                std::copy(fk.begin() + (size_t)q * nn, fk.begin() + (size_t)(q + 1) * nn, fw.begin() + (size_t)keep[q] * nn);
            }
        }
        std::vector<int32_t> wchr(nw);
        std::vector<uint64_t> wini(nw), wfin(nw);
        for (int64_t w = 0; w < nw; ++w) { wchr[w] = chr_id[wh[w]]; wini[w] = loc_pos[wh[w]]; wfin[w] = loc_pos[wt[w]]; }
        // device: [D | Fst] in, [per population: 2 n | per pair: 4 nn | per row: 6 n^2 w] doubles and [rows: n | window: n^2 w] integers out
        const size_t n_f64 = 2 * (size_t)n + 4 * nn + 6 * rows_all, n_i64 = (size_t)n + rows_all;
        DeviceBuf<double> tabs(sizeof(double) * (wn + (size_t)nw * nn), "gudmc: tables"), of(sizeof(double) * n_f64, "gudmc: the rows' values");
        DeviceBuf<int64_t> oi(sizeof(int64_t) * n_i64, "gudmc: the rows' windows");
        hip_ok(hipMemcpy(tabs.get(), dw.data(), sizeof(double) * wn, hipMemcpyHostToDevice), "gudmc: H2D");
        hip_ok(hipMemcpy(tabs.get() + wn, fw.data(), sizeof(double) * (size_t)nw * nn, hipMemcpyHostToDevice), "gudmc: H2D");
        double *o = of.get();
        gpu.ok(pg_gudmc_dev(gpu.c, tabs.get(), tabs.get() + wn, nw, n, wchr.data(), wini.data(), wfin.data(), a.sigma_threshold,
                            a.recombination_rate_cm_per_mb, oi.get(), o, o + n, o + 2 * n, o + 2 * n + nn, o + 2 * n + 2 * nn, o + 2 * n + 3 * nn,
                            oi.get() + n, o + 2 * n + 4 * nn, o + 2 * n + 4 * nn + rows_all, o + 2 * n + 4 * nn + 2 * rows_all,
                            o + 2 * n + 4 * nn + 3 * rows_all, o + 2 * n + 4 * nn + 4 * rows_all, o + 2 * n + 4 * nn + 5 * rows_all), "gudmc");
        std::vector<double> hf(n_f64);
        std::vector<int64_t> hi(n_i64);
        hip_ok(hipMemcpy(hf.data(), of.get(), sizeof(double) * n_f64, hipMemcpyDeviceToHost), "gudmc: D2H");
        hip_ok(hipMemcpy(hi.data(), oi.get(), sizeof(int64_t) * n_i64, hipMemcpyDeviceToHost), "gudmc: D2H");
        lap("gudmc on the GPU");
        const double *d_mean = hf.data(), *d_sd = d_mean + n, *f_mean = d_sd + n, *f_sd = f_mean + nn;
        const double *r_d = hf.data() + 2 * n + 4 * nn, *r_width = r_d + rows_all, *r_wdev = r_width + rows_all, *r_wp = r_wdev + rows_all,
                     *r_delta = r_wp + rows_all, *r_fp = r_delta + rows_all;
        const int64_t *r_win = hi.data() + n;
        std::vector<int64_t> first(nn + 1, 0); // the first line of every pair (:433-434)
        for (size_t i = 0; i < nn; ++i) first[i + 1] = first[i] + hi[i % n];
        std::string out = a.output;
        if (out.empty()) out = basename_no_ext(a.fname) + "-gudmc-" + time + ".csv"; // :383-401
        FILE *fo = create_new(out);
        fputs("pop_a,pop_b,chr,pos_ini,pos_fin,mean_tajima_d_pop_b,mean_fst,sd_tajima_d_pop_b,sd_fst,tajima_d_pop_b,tajima_width_pop_b,"
              "tajima_width_deviation_from_r_pop_b,tajima_width_one_tail_pval_pop_b,fst_delta,fst_delta_one_tail_pval\n", fo);
        write_rows_parallel(fo, first[nn], a.n_threads, [&](int64_t r, std::string &text) { // :435-455
            const size_t i = (size_t)(std::upper_bound(first.begin(), first.end(), r) - first.begin()) - 1;
            const size_t e = i * (size_t)nw + (size_t)(r - first[i]);
            const int pa = (int)(i / n), pb = (int)(i % n);
            const int64_t w = r_win[e];
            text += pool_names[pa] + "," + pool_names[pb] + "," + loc_chr[wh[w]] + "," + std::to_string(loc_pos[wh[w]]) + "," +
                    std::to_string(loc_pos[wt[w]]) + ",";
            append_roundup_own(text, d_mean[pb], 7); text.push_back(',');
            append_roundup_own(text, f_mean[i], 7); text.push_back(',');
            append_roundup_own(text, d_sd[pb], 7); text.push_back(',');
            append_roundup_own(text, f_sd[i], 7); text.push_back(',');
            append_rust_display(text, r_d[e]); text.push_back(',');
            append_rust_display(text, r_width[e]); text.push_back(',');
            append_rust_display(text, r_wdev[e]); text.push_back(',');
            append_roundup_own(text, r_wp[e], 7); text.push_back(',');
            append_roundup_own(text, r_delta[e], 7); text.push_back(',');
            append_roundup_own(text, r_fp[e], 7); text.push_back('\n');
        });
        fclose(fo);
        lap("write CSV");
        std::cout << out << "\n";
        return done_ok();
    }
    if (!is_fst) {
        // one row per pool: name, mean across windows, the windows (pi.rs:160-188, watterson_theta.rs:244-287, tajima_d.rs:127-169)
        std::string out = a.output;
        std::vector<double> pw((size_t)nw * n), pm(n);
        const char *tag = "-pi-", *what = "heterozygosity"; // pi.rs:135-159
        if (analysis == Analysis::heterozygosity)
            gpu.ok(pg_pi_dev(gpu.c, G_dev, cov_dev, p, n, ld, locus_col.data(), L, wh.data(), wt.data(), nw, pw.data(), pm.data()), what);
        else {
            const bool tajima = analysis == Analysis::tajima_d;
            tag = tajima ? "-Tajimas_D-" : "-watterson-"; // tajima_d.rs:120-125, watterson_theta.rs:237-242
            what = tajima ? "tajima_d" : "watterson_estimator";
            std::vector<int64_t> wc, wseed, wslot;
            if (!a.popgen_as_documented) { // the reference's own loop: the same windows, and what its count is made of
                std::cerr << "note: " << what << " reproduces the reference: the pool sizes are fractions of their sum, so every value is inf or NaN, "
                             "and the segregating sites are counted its way; --popgen-as-documented uses the pool sizes as written and counts every locus\n";
                std::vector<int64_t> h2(L), t2(L);
                wc.resize(L); wseed.resize(L); wslot.resize(L);
                const int64_t nw2 = pg_host_watterson_windows(chr_id.data(), loc_pos.data(), L, a.window_size_bp, a.window_slide_size_bp,
                                                              a.min_loci_per_window, h2.data(), t2.data(), wc.data(), wseed.data(), wslot.data());
                h2.resize(nw2); t2.resize(nw2);
                if (h2 != wh || t2 != wt) throw std::runtime_error("internal error: the two window loops disagree"); // tajima_d.rs:46-47
            }
            const int64_t *c = wc.empty() ? nullptr : wc.data(), *sd = wc.empty() ? nullptr : wseed.data(), *sl = wc.empty() ? nullptr : wslot.data();
            if (tajima)
                gpu.ok(pg_tajima_d_dev(gpu.c, G_dev, cov_dev, p, n, ld, locus_col.data(), L, wh.data(), wt.data(), c, sd, sl, nw, pool_sizes.data(),
                                       pw.data(), pm.data(), nullptr, nullptr), what);
            else
                gpu.ok(pg_watterson_dev(gpu.c, G_dev, p, n, ld, locus_col.data(), L, wh.data(), wt.data(), c, sd, sl, nw, pool_sizes.data(), pw.data(),
                                        pm.data(), nullptr), what);
        }
        if (out.empty()) out = basename_no_ext(a.fname) + tag + win + "_bp_windows-" + time + ".csv";
        lap("windows on the GPU");
        FILE *fo = create_new(out);
        std::string line = "Pool,Mean_across_windows";
        for (int64_t w = 0; w < nw; ++w)
            line += ",Window-" + loc_chr[wh[w]] + "_" + std::to_string(loc_pos[wh[w]]) + "_" + std::to_string(loc_pos[wt[w]]);
        fputs((line + "\n").c_str(), fo);
        for (int i = 0; i < n; ++i) {
            line = pool_names[i] + "," + rust_display(pm[i]);
            for (int64_t w = 0; w < nw; ++w) line += "," + roundup_own(pw[(size_t)w * n + i], 8);
            fputs((line + "\n").c_str(), fo);
        }
        fclose(fo);
        lap("write CSV");
        std::cout << out << "\n";
        return done_ok();
    }
    std::string out = a.output, out_win;
    if (out.empty()) { // fst.rs:93-131
        out = basename_no_ext(a.fname) + "-fst-averaged_across_genome-" + time + ".csv";
        out_win = basename_no_ext(a.fname) + "-fst-" + win + "_bp_windows-" + time + ".csv";
    } else
        out_win = basename_no_ext(out) + "-fst-" + win + "_bp_windows.csv";
    const size_t nn = (size_t)n * n;
    std::vector<double> mean(nn), fw((size_t)nw * nn);
    gpu.ok(pg_fst_dev(gpu.c, G_dev, cov_dev, p, n, ld, locus_col.data(), L, wh.data(), wt.data(), nw, mean.data(), fw.data()), "fst");
    lap("fst on the GPU");
    FILE *fo = create_new(out);
    std::string line;
    for (int i = 0; i < n; ++i) line += "," + pool_names[i];
    fputs((line + "\n").c_str(), fo);
    for (int i = 0; i < n; ++i) {
        line = pool_names[i];
        for (int j = 0; j < n; ++j) line += "," + roundup_own(mean[(size_t)i * n + j], 8);
        fputs((line + "\n").c_str(), fo);
    }
    fclose(fo);
    if (nw <= 0) // fst.rs:180, after the genome-wide file has been written
        throw std::runtime_error("There were no windows defined. Please check the sync file, the window size, slide size, and the minimum number of loci per window.");
    fo = create_new(out_win);
    line = "chr,pos_ini,pos_fin";
    for (int j = 0; j < n; ++j)
        for (int k2 = 0; k2 < n; ++k2) line += "," + pool_names[j] + "_vs_" + pool_names[k2];
    fputs((line + "\n").c_str(), fo);
    write_rows_parallel(fo, nw, a.n_threads, [&](int64_t w, std::string &text) {
        text += loc_chr[wh[w]] + "," + std::to_string(loc_pos[wh[w]]) + "," + std::to_string(loc_pos[wt[w]]);
        for (size_t q = 0; q < nn; ++q) text += "," + rust_display(fw[(size_t)w * nn + q]);
        text += "\n";
    });
    fclose(fo);
    lap("write CSV");
    std::cout << out << " and " << out_win << "\n"; // main.rs:441
    return done_ok();
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

// FileSyncPhen::into_genotypes_and_phenotypes (base/sync.rs:1106-1179) = load (:1044-1104: filter + frequencies per locus,
// sorted by (chromosome, position)) + the dense fill.  The host only sorts the locus order; filter, frequencies and the
// column layout run on the GPU from the parsed counts (pg_load_plan_dev / pg_load_emit[_cov]_dev), and the matrix never
// exists in host memory.  `remove_missing`: drop the pools without phenotype (what ols_with_covariate does first,
// gwas/ols.rs:287); the popgen tools keep every pool.
static GenotypesAndPhenotypes into_genotypes_and_phenotypes(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt,
                                                            bool keep_p_minus_1, bool remove_missing, bool with_coverages, Lap &lap) {
    const int n = sb.n, k = ph.k;
    const int64_t L = sb.size();
    std::vector<int64_t> order(L);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const int c = sb.chrom(x).compare(sb.chrom(y));
        return c != 0 ? c < 0 : sb.pos[x] < sb.pos[y];
    });
    std::vector<int> keep(n);
    std::iota(keep.begin(), keep.end(), 0);
    if (remove_missing) keep = complete_pools(ph);
    if (keep.empty()) throw std::runtime_error("All pools have missing data. Please check the phenotype file.");
    GenotypesAndPhenotypes g;
    g.n = (int)keep.size();
    g.k = k;
    g.ld = g.n + (g.n & 1);
    std::vector<int32_t> pool_map(n, -1);
    for (int i = 0; i < g.n; ++i) pool_map[keep[i]] = i;
    LoadedMatrix m;
    {
        DeviceBuf<uint32_t> counts_dev(sizeof(uint32_t) * (size_t)L * n * 6, "device memory for the counts");
        DeviceBuf<int64_t> order_dev(sizeof(int64_t) * L, "device memory");
        CountsUpload upload;
        upload(gpu, sb, counts_dev.get());
        hip_ok(hipMemcpy(order_dev.get(), order.data(), sizeof(int64_t) * L, hipMemcpyHostToDevice), "H2D order");
        m = load_matrix(gpu, counts_dev.get(), L, n, ph.pool_sizes, flt, keep_p_minus_1, order_dev.get(), pool_map, g.n, g.ld, with_coverages);
        if (m.p <= 0) throw std::runtime_error("no loci passed the filters");
        lap("sort + H2D + GPU loader");
    }
    g.p = m.p;
    g.intercept_and_allele_frequencies = std::move(m.G);
    g.coverages = std::move(m.coverages);
    g.chromosome.assign(1, "intercept"); g.allele.assign(1, "intercept"); g.position.assign(1, 0);
    g.chromosome.reserve(g.p + 1); g.allele.reserve(g.p + 1); g.position.reserve(g.p + 1);
    for (int64_t c = 0; c < g.p; ++c) {
        g.chromosome.push_back(sb.chrom(m.col_locus[c])); g.position.push_back(sb.pos[m.col_locus[c]]);
        g.allele.push_back(std::string(1, ALLELES[m.col_allele[c]]));
    }
    for (int i : keep) {
        g.pool_names.push_back(ph.pool_names[i]);
        for (int j = 0; j < k; ++j) g.phenotypes.push_back(ph.phen[(size_t)i * k + j]);
    }
    return g;
}

// gwas::ols_with_covariate (gwas/ols.rs:278-436): kinship, eigen rule, one fit per (column, trait), the CSV; returns the
// name of the file it wrote.
// ... and gwas::mle_with_covariate (gwas/mle.rs:307-463) when `mle`: same preamble, Nelder-Mead fits, same writer with its own file name
// (the reference also prints its index arrays, the covariates, y, g, beta and pval to stdout, mle.rs:364-368, :402-405: debug output,
// not reproduced).
static std::string ols_with_covariate(Ctx &gpu, GenotypesAndPhenotypes &g, double xxt_eigen_variance_explained,
                                      const std::string &fname_input, const std::string &fname_output, int n_threads, Lap &lap,
                                      bool mle = false) {
    const int64_t p = g.p;
    const int k = g.k;
    if (!fname_output.empty()) { FILE *t = create_new(fname_output); fclose(t); ::unlink(fname_output.c_str()); } // ols.rs:285
    std::vector<double> beta((size_t)p * k), pval((size_t)p * k);
    int m = 0;
    const size_t cnt = (size_t)p * k;
    {
        DeviceBuf<double> out_dev(sizeof(double) * 3 * cnt, "device memory for the results");
        const double *G = g.intercept_and_allele_frequencies.get();
        if (mle)
            gpu.ok(pg_mle_kinship_dev(gpu.c, G, p, g.n, g.ld, g.phenotypes.data(), k, xxt_eigen_variance_explained, -1, &m, nullptr, out_dev.get(),
                                      out_dev.get() + cnt, out_dev.get() + 2 * cnt), "mle_iter_with_kinship");
        else
            gpu.ok(pg_ols_kinship_dev(gpu.c, G, p, g.n, g.ld, g.phenotypes.data(), k, xxt_eigen_variance_explained, -1, &m, nullptr, out_dev.get(),
                                      out_dev.get() + cnt, out_dev.get() + 2 * cnt), "ols_iter_with_kinship");
        gpu.ok(pg_synchronize(gpu.c), "ols_iter_with_kinship");
        hip_ok(hipMemcpy(beta.data(), out_dev.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
        hip_ok(hipMemcpy(pval.data(), out_dev.get() + 2 * cnt, sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
    }
    lap("kinship + fits + D2H");
    std::string out = fname_output;
    if (out.empty()) // ols.rs:393-398
        out = basename_no_ext(fname_input) + (mle ? "-mle_iterative_xxt_" : "-ols_iterative_xxt_") + std::to_string(m + 1) + "_eigens-" +
              unix_time_string() + ".csv"; // ols.rs:393-398, mle.rs:423-427
    write_kinship_csv(out, p, k, beta, pval, n_threads, [&](int64_t i, std::string &text) {
        // the reference labels coefficient i with entry i of the (1+p)-long label vectors, i.e.
        // shifted by the intercept entry (ols.rs:421-425) -- reproduced as is
        text += g.chromosome[i]; text.push_back(','); text += std::to_string(g.position[i]); text.push_back(','); text += g.allele[i];
    });
    lap("format + write CSV");
    return out;
}

static int run(int argc, char **argv) {
    stamp("main");
    const Args a = parse_args(argc, argv);
    Lap lap;
    const std::map<std::string, Analysis> known{
        {"chisq_test", Analysis::chisq_test}, {"pearson_corr", Analysis::pearson_corr}, {"ols_iter", Analysis::ols_iter},
        {"fisher_exact_test", Analysis::fisher_exact_test}, {"gwalpha", Analysis::gwalpha}, {"ols_iter_with_kinship", Analysis::ols_iter_with_kinship},
        {"mle_iter_with_kinship", Analysis::mle_iter_with_kinship},
        {"genomic_prediction_cross_validation", Analysis::genomic_prediction_cross_validation}, {"fst", Analysis::fst},
        {"heterozygosity", Analysis::heterozygosity}, {"watterson_estimator", Analysis::watterson_estimator},
        {"tajima_d", Analysis::tajima_d}, {"gudmc", Analysis::gudmc}, {"pileup2sync", Analysis::pileup2sync}};
    const auto found = known.find(a.analysis);
    if (found == known.end())
        throw std::runtime_error("Invalid analysis utility for this build: `" + a.analysis +
                                 "` (available: pileup2sync, fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship, "
                                 "mle_iter_with_kinship, genomic_prediction_cross_validation, fst, heterozygosity, watterson_estimator, tajima_d, gudmc)");
    const Analysis analysis = found->second;
    if (a.popgen_as_documented && analysis != Analysis::watterson_estimator && analysis != Analysis::tajima_d && analysis != Analysis::gudmc)
        throw std::runtime_error("--popgen-as-documented applies to watterson_estimator, tajima_d and gudmc");
    if (a.generate_plots || a.sig_only)
        throw std::runtime_error("--generate-plots / --output-sig-snps-only call the reference's python scripts and are out of scope here");
    if (a.phen_format != "default" && a.phen_format != "gwalpha_fmt")
        throw std::runtime_error("Invalid phenotype format. Please select: 'default' or 'gwalpha_fmt'"); // phen.rs:161-164
    const bool gwalpha_fmt = a.phen_format == "gwalpha_fmt";
    if (analysis == Analysis::gwalpha && !gwalpha_fmt)
        throw std::runtime_error("gwalpha needs the GWAlpha.py phenotype file: give it with --phen-format gwalpha_fmt "
                                 "(Pheno_name=, sig=, MIN=, MAX=, perc=[..], q=[..])");
    if (gwalpha_fmt && analysis != Analysis::gwalpha && analysis != Analysis::pileup2sync)
        throw std::runtime_error("--phen-format gwalpha_fmt is read by gwalpha and pileup2sync; `" + a.analysis + "` needs the default phenotype file");
    Phen ph = gwalpha_fmt ? parse_phen_gwalpha(a.phen_fname)
                          : parse_phen(a.phen_fname, a.phen_delim, a.phen_name_col, a.phen_pool_size_col, a.phen_value_col);
    if (analysis == Analysis::gwalpha && ph.n < 3) // the reference's check() panics: its matrix has 3 rows, the counts fewer
        throw std::runtime_error("gwalpha needs at least 3 pools; the phenotype file describes " + std::to_string(ph.n));
    if (gwalpha_fmt) ph.pool_names.resize(ph.n); // (the reference names max(n, 3) pools; fewer than 3 are refused by the operator)
    const PileupFilter pf = pileup_filter(a, ph.pool_sizes);
    // the counts are parsed straight into pinned memory: the copy to the device needs no staging pass
    SyncAlloc pinned;
    pinned.alloc = PinnedBuf::alloc;
    pinned.release = PinnedBuf::release;
    if (analysis == Analysis::pileup2sync) { // main.rs:212-225; text to text, no GPU involved
        std::string out = a.output;
        if (out.empty()) out = basename_no_ext(a.fname) + "-" + unix_time_string() + ".sync"; // pileup.rs:478-494
        const int64_t kept = pileup_to_sync_file(a.fname, ph.pool_names, pf, out, a.n_threads);
        lap("pileup2sync");
        std::cerr << kept << " loci written\n";
        std::cout << out << "\n"; // main.rs:507
        return done_ok();
    }
    if (a.n_gpus > 0 && !per_locus(analysis) && analysis != Analysis::ols_iter_with_kinship)
        throw std::runtime_error("--n-gpus applies to fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha and ols_iter_with_kinship; `" + a.analysis + "` runs on one GPU");
    const RankSetup ranks = rank_setup(a, analysis == Analysis::ols_iter_with_kinship);
    Ctx gpu(ranks.devices[0]); // first: the pinned allocator below needs a HIP context
    lap("start-up");
    // A pileup input (*.pileup / *.mpileup) is converted in memory -- the counts pileup2sync would write and the
    // sync reader would read back, without the text in between (an extension: the reference needs the sync file).
    auto ends_with = [](const std::string &x, const char *suf) {
        const size_t m = std::strlen(suf);
        return x.size() >= m && x.compare(x.size() - m, m, suf) == 0;
    };
    const bool is_pileup = ends_with(a.fname, ".pileup") || ends_with(a.fname, ".mpileup");
    pg_filter flt{};
    flt.remove_ns = a.keep_ns ? 0 : 1;
    flt.min_coverage_depth = a.min_coverage_depth;
    flt.min_allele_frequency = a.min_allele_frequency;
    flt.max_missingness_rate = a.max_missingness_rate;
    if (analysis == Analysis::ols_iter_with_kinship) {
        // inputs above 256 MiB are taken in pieces of 128 MiB of text, above 1 GiB in pieces of 256 MiB (parse of piece c + 1 overlaps the GPU work on
        // piece c, and the pinned buffers stay small); an unsorted input falls back to the whole-file path unless
        // the pieces were asked for explicitly
        struct stat st;
        const size_t fsize = ::stat(a.fname.c_str(), &st) == 0 ? (size_t)st.st_size : 0;
        const bool automatic = a.stream_chunk_mb < 0 && !std::getenv("PGH_STREAM_CHUNK_BYTES");
        long mb = a.stream_chunk_mb;
        if (mb < 0) mb = fsize > ((size_t)1 << 30) ? 256 : (fsize > ((size_t)256 << 20) ? 128 : 0); // no whole-file pinned buffer beyond 256 MiB
        size_t piece = (size_t)(mb > 0 ? mb : 0) << 20;
        if (const char *e = std::getenv("PGH_STREAM_CHUNK_BYTES")) piece = (size_t)std::strtoull(e, nullptr, 10); // tests: small pieces
        if (a.n_gpus > 0 && piece == 0) piece = std::max<size_t>(1, (fsize + ranks.n_ranks - 1) / ranks.n_ranks); // one piece per rank at least
        if (piece > 0 && (fsize > piece || a.n_gpus > 0)) {
            try {
                return run_kinship_streamed(a, ph, gpu, lap, piece, is_pileup, pf, flt, ranks);
            } catch (const UnsortedInput &e) {
                if (!automatic || a.n_gpus > 0) throw;
                std::cerr << "note: input is not sorted by (chromosome, position); loading the whole file instead\n";
            }
        }
    }
    if (per_locus(analysis)) {
        size_t piece = (size_t)(a.stream_chunk_mb > 0 ? a.stream_chunk_mb : 128) << 20;
        if (const char *e = std::getenv("PGH_STREAM_CHUNK_BYTES")) piece = (size_t)std::strtoull(e, nullptr, 10); // tests: small pieces
        return run_batch_streamed(a, ph, gpu, lap, analysis, piece, is_pileup, pf, flt, ranks);
    }
    SyncBatch sb;
    if (is_pileup) {
        sb = parse_pileup_file(a.fname, a.n_threads, pf, pinned);
        lap("pileup -> counts");
    } else {
        // the analyses on the loaded matrix copy the counts themselves: 16-bit counts when they fit
        sb = parse_sync_file(a.fname, a.n_threads, pinned, /*compact16=*/true);
        lap("parse sync");
    }
    if (sb.size() == 0) throw std::runtime_error("no loci in " + a.fname);
    if (sb.n != ph.n) throw std::runtime_error("the number of pools in the sync file and in the phenotype file differ");
    const int k = ph.k;
    const bool popgen = pgh::popgen(analysis);

    // ---------------- the analyses on the loaded matrix (main.rs:280-298, :397-455) ---------------------------
    const bool kpm1 = popgen && analysis != Analysis::fst ? false : a.keep_p_minus_1; // "we need all alleles in each locus" (main.rs:445, :460, :475)
    GenotypesAndPhenotypes genotypes_and_phenotypes =
        into_genotypes_and_phenotypes(gpu, sb, ph, flt, kpm1, /*remove_missing=*/!popgen, /*with_coverages=*/popgen, lap);
    GenotypesAndPhenotypes &g = genotypes_and_phenotypes;
    if (popgen) // fst / heterozygosity / watterson_estimator / tajima_d / gudmc use every pool (main.rs:427-502)
        return run_popgen(a, analysis, gpu, g.intercept_and_allele_frequencies.get(), g.coverages.get(), g.p, g.n, g.ld, g.chromosome, g.position,
                          g.pool_names, a.popgen_as_documented ? ph.pool_sizes_as_written : ph.pool_sizes, lap);
    if (analysis == Analysis::genomic_prediction_cross_validation) { // genomic_prediction_cross_validation (main.rs:397-426)
        CvLabels labels{g.chromosome, g.allele, g.position};
        CvArgs ca;
        ca.k_folds = a.k_folds; ca.n_reps = a.n_reps; ca.seed = a.seed; ca.n_threads = a.n_threads;
        ca.fname_input = a.fname; ca.fname_output = a.output;
        const std::string out = gp_cross_validate(gpu.c, g.intercept_and_allele_frequencies.get(), g.p, g.n, g.ld, g.phenotypes, k, g.pool_names,
                                                  labels, ca);
        lap("cross-validation");
        std::cout << out << "\n";
        return done_ok();
    }
    const std::string out = ols_with_covariate(gpu, g, a.xxt, a.fname, a.output, a.n_threads, lap, /*mle=*/analysis == Analysis::mle_iter_with_kinship);
    std::cout << out << "\n";
    return done_ok();
}

int main(int argc, char **argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception &e) {
        std::cerr << "poolgen: " << e.what() << "\n";
        return 1;
    }
}
