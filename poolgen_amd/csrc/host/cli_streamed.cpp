// cli_streamed.cpp -- the analyses that take the input in PIECES, one rank per GPU: ols_iter_with_kinship, the per-locus operators.
#include "cli.h"
#include "piece_reader.h"
#include <cstring>
#include <memory>
#include <numeric>
#include <sys/stat.h>

// The size of the pieces: --stream-chunk-mb, else 128 MiB for the per-locus operators; the kinship path takes inputs above 256 MiB
// in pieces of 128 MiB of text, above 1 GiB in pieces of 256 MiB (parse of piece c + 1 overlaps the GPU work on piece c, and no
// whole-file pinned buffer beyond 256 MiB), one piece per rank at least, and 0 = load the file whole.  PGH_STREAM_CHUNK_BYTES
// overrides the size (tests: small pieces).  *automatic: nobody asked for pieces.
static size_t piece_bytes(const Args &a, bool kinship, int n_ranks, bool *automatic = nullptr) {
    const char *e = std::getenv("PGH_STREAM_CHUNK_BYTES");
    struct stat st;
    const size_t fsize = ::stat(a.fname.c_str(), &st) == 0 ? (size_t)st.st_size : 0;
    long mb = a.stream_chunk_mb;
    if (automatic) *automatic = mb < 0 && !e;
    if (!kinship && mb <= 0) mb = 128;
    if (mb < 0) mb = fsize > ((size_t)1 << 30) ? 256 : (fsize > ((size_t)256 << 20) ? 128 : 0);
    size_t piece = e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)mb << 20;
    if (kinship && a.n_gpus > 0 && piece == 0) piece = std::max<size_t>(1, (fsize + n_ranks - 1) / n_ranks);
    return kinship && fsize <= piece && a.n_gpus == 0 ? 0 : piece; // one GPU and the file within one piece: load it whole
}

// The input, cut at line starts into pieces of about `bytes` (one per rank at least), and the ranks' ranges of pieces
struct PiecedInput {
    const MappedFile mf;
    const std::vector<size_t> cuts;
    const std::vector<int> first; // rank r takes the pieces [first[r], first[r + 1])
    PiecedInput(const std::string &fname, size_t bytes, int n_ranks)
        : mf(fname), cuts(mf.cuts(std::max<size_t>((size_t)n_ranks, (mf.size() + bytes - 1) / bytes))),
          first(deal_pieces((int)cuts.size() - 1, n_ranks)) {}
};

// Selects the rank's device on the calling thread and returns the rank's context: gpu0 for rank 0 on gpu0's device, else a new one in `own`
static Ctx *rank_ctx(int rank, int device, Ctx &gpu0, std::unique_ptr<Ctx> &own) {
    hip_ok(hipSetDevice(device), "hipSetDevice");
    if (rank == 0 && gpu0.device == device) return &gpu0;
    own.reset(new Ctx(device));
    return own.get();
}

// ---------------------------------------------------------------------------------------------------------
// ols_iter_with_kinship on an input that is read in PIECES (config 5 of BASELINE.json: a file far larger than
// host memory): while the GPU takes piece c (H2D from pinned memory, loader, partial kinship), the worker
// threads already parse piece c + 1 into the other pinned buffer.  The frequency matrix stays resident in HBM
// piece by piece (288 GB hold 180 M columns of 200 pools); the host only keeps labels and results.
// The input must be sorted by (chromosome, position) -- what the whole-file path obtains by sorting
// (sync.rs:1092-1101) cannot be had across pieces -- and that is checked.
// ---------------------------------------------------------------------------------------------------------
struct UnsortedInput : std::runtime_error {
    UnsortedInput(const std::string &chrom, uint64_t pos)
        : std::runtime_error("streamed ols_iter_with_kinship needs the input sorted by chromosome and position (line of " + chrom + ":" +
                             std::to_string(pos) + "); use --stream-chunk-mb 0 to load the whole file") {}
};

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

// ---- phase A, per rank: parse piece c + 1 || H2D + loader + partial kinship of piece c -----------------------
static void kin_load_pieces(KinRank &K, RankGate &gate, const Args &a, const Phen &ph, const PiecedInput &in, InputKind kind, const PileupFilter &pf,
                            const pg_filter &flt, const RankSetup &rs, const std::vector<int32_t> &pool_map, int n2, int64_t ld) {
    const int n = ph.n, R = rs.n_ranks;
    auto clk = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    Ctx &gpu = *K.gpu;
    gate.pass([&] {
        hip_ok(hipSetDevice(K.device), "hipSetDevice");
        K.S_total.assign((size_t)n2 * n2, 0.0);
        K.S_dev.reset(sizeof(double) * n2 * n2);
    });
    if (rs.rccl) // collective over the rank threads: entered by all of them or by none, and its outcome agreed on
        gate.pass([&] { gpu.ok(pg_comm_init_rank(gpu.c, rs.id, R, K.rank), "RCCL communicator"); });
    if (K.c0 >= K.c1) return;
    // (the pinned slots, the counts and the 16-bit scratch live to the end of this phase only)
    PieceReader pieces(in.mf, in.cuts, K.c0, K.c1, K.device, K.threads, kind, pf, n, true, a.sync_parser == "gpu" ? SyncOnGpu::device : SyncOnGpu::no,
                       a.pileup_parser == "gpu");
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
                if (cmp > 0 || (cmp == 0 && K.last_pos > sb.pos[l])) throw UnsortedInput(ch, sb.pos[l]);
                if (cmp != 0) K.last_chrom = ch;
            } else { K.last_chrom = ch; K.have_last = true; K.first_chrom = ch; K.first_pos = sb.pos[l]; }
            K.last_pos = sb.pos[l];
        }
        K.t_host += clk() - t0; t0 = clk();
        const uint32_t *counts = sb.counts_dev; // --sync-parser gpu: the piece's counts are on the device already
        if (!counts) {
            counts_dev.reserve(sizeof(uint32_t) * (size_t)sb.L * n * 6, "device memory for the counts");
            upload(gpu, sb, counts_dev.get());
            counts = counts_dev.get();
        }
        LoadedMatrix piece = load_matrix(gpu, counts, sb.L, n, ph.pool_sizes, flt, a.keep_p_minus_1, nullptr, pool_map, n2, ld, false);
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
}

// ---- phase B, per rank: all-reduce of the kinship sums, the n x n step (replicated), the rank's sweeps ---------
// S_host: the ranks' sums added on the host (no communicator); Y: the kept pools' phenotypes; beta, pval: p x k, a rank fills its columns
static void kin_fit_pieces(KinRank &K, RankGate &gate, const RankSetup &rs, const std::vector<double> &S_host, int64_t p, int n2, int64_t ld,
                           const std::vector<double> &Y, int k, double xxt, std::vector<double> &beta, std::vector<double> &pval,
                           double *res_dev = nullptr) { // --result-writer gpu (one rank): beta at res_dev, pval p * k further on; nothing copied down
    Ctx &gpu = *K.gpu;
    gate.pass([&] {
        hip_ok(hipSetDevice(K.device), "hipSetDevice");
        hip_ok(hipMemcpy(K.S_dev.get(), rs.rccl ? K.S_total.data() : S_host.data(), sizeof(double) * n2 * n2, hipMemcpyHostToDevice), "H2D kinship");
    });
    if (rs.rccl) gpu.ok(pg_allreduce_sum_dev(gpu.c, K.S_dev.get(), (int64_t)n2 * n2), "RCCL all-reduce of the kinship sums");
    gpu.ok(pg_kinship_set(gpu.c, K.S_dev.get(), p, n2, Y.data(), k, xxt, -1, &K.m, nullptr, nullptr), "ols_iter_with_kinship");
    int64_t off = K.col0;
    for (size_t c = 0; c < K.Gs.size(); ++c) {
        const size_t cnt = (size_t)K.ps[c] * k;
        DeviceBuf<double> out_dev(sizeof(double) * 3 * cnt, "device memory for the results");
        gpu.ok(pg_ols_sweep_dev(gpu.c, K.Gs[c].get(), K.ps[c], n2, ld, out_dev.get(), out_dev.get() + cnt, out_dev.get() + 2 * cnt), "ols_iter_with_kinship");
        gpu.ok(pg_synchronize(gpu.c), "ols_iter_with_kinship");
        if (res_dev) { // the rank's results stay on the device, 16 bytes per coefficient and trait
            hip_ok(hipMemcpy(res_dev + (size_t)off * k, out_dev.get(), sizeof(double) * cnt, hipMemcpyDeviceToDevice), "keeping the results");
            hip_ok(hipMemcpy(res_dev + (size_t)(p + off) * k, out_dev.get() + 2 * cnt, sizeof(double) * cnt, hipMemcpyDeviceToDevice), "keeping the results");
        } else {
            hip_ok(hipMemcpy(beta.data() + (size_t)off * k, out_dev.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
            hip_ok(hipMemcpy(pval.data() + (size_t)off * k, out_dev.get() + 2 * cnt, sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
        }
        K.Gs[c].reset(); // a piece leaves HBM right after its sweep
        off += K.ps[c];
    }
    K.Gs.clear();
}

static int kinship_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, size_t chunk_bytes, InputKind kind, const PileupFilter &pf,
                            const pg_filter &flt, const RankSetup &rs) {
    const int R = rs.n_ranks, n = ph.n, k = ph.k;
    const PiecedInput in(a.fname, chunk_bytes, R);
    const std::vector<int> keep = complete_pools(ph); // remove_missing (ols.rs:287)
    if (keep.empty()) throw std::runtime_error("All pools have missing data. Please check the phenotype file.");
    const int n2 = (int)keep.size();
    const int64_t ld = n2 + (n2 & 1);
    std::vector<int32_t> pool_map(n, -1);
    for (int i = 0; i < n2; ++i) pool_map[keep[i]] = i;
    std::vector<KinRank> ranks(R);
    // every rank's context is created here, on the main thread: a GPU that cannot be opened ends the run before any rank
    // thread exists
    for (int r = 0; r < R; ++r) {
        KinRank &K = ranks[r];
        K.rank = r; K.device = rs.devices[r]; K.threads = rs.threads[r];
        K.c0 = in.first[r]; K.c1 = in.first[r + 1];
        K.gpu = rank_ctx(r, K.device, gpu0, K.own);
    }
    RankGate gate(R);
    run_ranks(R, [&](int r) { kin_load_pieces(ranks[r], gate, a, ph, in, kind, pf, flt, rs, pool_map, n2, ld); });
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
            if (cmp > 0 || (cmp == 0 && prev->last_pos > K.first_pos)) throw UnsortedInput(K.first_chrom, K.first_pos);
        }
        prev = &K;
    }
    if (p <= 0) throw std::runtime_error("no loci passed the filters");
    std::vector<double> Y, S_host;
    for (int i : keep) for (int j = 0; j < k; ++j) Y.push_back(ph.phen[(size_t)i * k + j]);
    if (!a.output.empty()) probe_output(a.output); // ols.rs:285
    if (!rs.rccl) { // PGH_COMM=host, or no communicator at all: the ranks' sums added in rank order
        S_host.assign((size_t)n2 * n2, 0.0);
        for (const KinRank &K : ranks)
            for (size_t i = 0; i < S_host.size(); ++i) S_host[i] += K.S_total[i];
    }
    const bool gpu_writer = a.result_writer == "gpu"; // one rank: checked with the flags
    std::vector<double> beta(gpu_writer ? 0 : (size_t)p * k), pval(beta.size());
    DeviceBuf<double> res_dev;
    if (gpu_writer) {
        hip_ok(hipSetDevice(ranks[0].device), "hipSetDevice");
        res_dev.reset(sizeof(double) * 2 * (size_t)p * k, "device memory for the results");
    }
    run_ranks(R, [&](int r) { kin_fit_pieces(ranks[r], gate, rs, S_host, p, n2, ld, Y, k, a.xxt, beta, pval, res_dev.get()); });
    const int m = ranks[0].m;
    for (const KinRank &K : ranks)
        if (K.m != m) throw std::runtime_error("internal error: the ranks disagree on n_eigenvecs");
    lap(gpu_writer ? "all-reduce + eigen rule + fits" : "all-reduce + eigen rule + fits + D2H");
    std::string out = a.output;
    if (out.empty()) // ols.rs:393-398
        out = basename_no_ext(a.fname) + "-ols_iterative_xxt_" + std::to_string(m + 1) + "_eigens-" + unix_time_string() + ".csv";
    if (gpu_writer) { // after the last piece: the rows in their trait-major order, formatted on the device a slab of rows per turn
        const KinRank &K = ranks[0];
        std::vector<int32_t> col_allele(K.lab_al.size());
        for (size_t c = 0; c < K.lab_al.size(); ++c) col_allele[c] = (int32_t)(std::strchr(ALLELES, K.lab_al[c]) - ALLELES);
        { // (a scope of its own: done_ok below does not return, and the writer reports its timing when it goes)
        DeviceResultWriter writer;
        writer.set_column_labels(K.lab_chr, K.lab_pos, col_allele, K.chrom_names);
        FILE *fo = create_new(out);
        try {
            fputs("#chr,pos,alleles,phenotype,statistic,pvalue\n", fo); // ols.rs:409
            const int64_t total = (int64_t)k * p, step = result_slab_rows((int)std::min<int64_t>(a.result_slab_rows, INT32_MAX));
            for (int64_t row0 = 0; row0 < total; row0 += step)
                writer.kinship_rows(K.gpu->c, p, k, row0, std::min(step, total - row0), res_dev.get(), res_dev.get() + (size_t)p * k, fo);
            if (fclose(fo) != 0) { fo = nullptr; throw std::runtime_error("write error on " + out); }
        } catch (...) { // a failure on the way leaves no file
            if (fo) fclose(fo);
            ::unlink(out.c_str());
            throw;
        }
        }
        lap("format (gpu) + write CSV");
        return done_ok(out);
    }
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
    return done_ok(out);
}

int run_kinship_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, InputKind kind, const PileupFilter &pf, const pg_filter &flt,
                         const RankSetup &rs) {
    bool automatic = false;
    const size_t piece = piece_bytes(a, true, rs.n_ranks, &automatic);
    if (piece == 0) return -1;
    try {
        return kinship_streamed(a, ph, gpu0, lap, piece, kind, pf, flt, rs);
    } catch (const UnsortedInput &) { // falls back to the whole-file path unless the pieces were asked for explicitly
        if (!automatic || a.n_gpus > 0) throw;
    }
    std::cerr << "note: input is not sorted by (chromosome, position); loading the whole file instead\n";
    return -1;
}

// fisher_exact_test / chisq_test / pearson_corr / ols_iter / gwalpha (main.rs:245-271, :335-356): the per-locus operators know nothing beyond their own line, so
// the file is taken in pieces whatever its size -- the worker threads parse piece c + 1 into one of two pinned buffers
// (16-bit counts when they fit) while the GPU takes piece c and its rows are formatted and appended, in file order
// (sync.rs:927-946).  Nothing of the size of the input is ever allocated, pinned or copied in one go.
int run_batch_streamed(const Args &a, const Phen &ph, Ctx &gpu0, Lap &lap, Analysis op, InputKind kind, const PileupFilter &pf,
                       const pg_filter &flt, const RankSetup &rs) {
    const int R = rs.n_ranks;
    const PiecedInput in(a.fname, piece_bytes(a, false, R), R);
    // gwalpha: one statistic per row, no p-value; its phenotype matrix carries (bins, q', [sig, MIN, MAX]) instead of traits
    const bool gwa = op == Analysis::gwalpha;
    const int n = ph.n, k = gwa ? 1 : ph.k;
    std::vector<double> gw_q(gwa ? n : 0);
    for (int i = 0; gwa && i < n; ++i) gw_q[i] = ph.phen[(size_t)i * 3 + 1];
    const int gw_method = a.gwalpha_method == "LS" ? PG_GWALPHA_LS : PG_GWALPHA_ML; // main.rs:337-356: anything but LS is ML
    std::string out = a.output;
    if (out.empty()) out = basename_no_ext(a.fname) + "-" + unix_time_string() + "-" + a.analysis + ".csv"; // sync.rs:903
    probe_output(out); // as the reference does before any work (sync.rs:906)
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
    const bool gpu_writer = a.result_writer == "gpu";
    const int result_op = op == Analysis::fisher_exact_test ? PG_RESULT_FISHER : op == Analysis::chisq_test ? PG_RESULT_CHISQ
                          : gwa ? PG_RESULT_GWALPHA : op == Analysis::pearson_corr ? PG_RESULT_PEARSON : PG_RESULT_OLS_ITER;
    const char *header = tables ? "#chr,pos,alleles,statistic,pvalue\n"                    // sync.rs:766
                                   : "#chr,pos,alleles,freq,phenotype,statistic,pvalue\n"; // sync.rs:950
    // One rank = one contiguous range of pieces, one GPU, its own pinned buffers and parser threads, and -- when there are
    // several -- its own part file, like the reference's one `.tmp` file per worker thread (sync.rs:794-870), concatenated in
    // rank order afterwards (sync.rs:951-968).  No exchange between the ranks: a locus needs nothing beyond its own line.
    std::vector<int64_t> totals(R, 0);
    std::vector<std::string> part(R);
    for (int r = 0; r < R; ++r) part[r] = R == 1 ? out : out + ".rank" + std::to_string(r) + ".tmp";
    std::vector<char> created(R, 0); // the part files this run made: a run that fails leaves none of them behind, one rank's output included
    auto cleanup_parts = [&] { for (int r = 0; r < R; ++r) if (R > 1 || created[r]) ::unlink(part[r].c_str()); };
    try {
    run_ranks(R, [&](int r) {
        const int device = rs.devices[r], threads = rs.threads[r];
        std::unique_ptr<Ctx> own;
        Ctx &gpu = *rank_ctx(r, device, gpu0, own);
        const int c0 = in.first[r], c1 = in.first[r + 1];
        if (c0 >= c1) return;
        // --sync-parser gpu: the counts stay on the device, except where pools are dropped on the host below
        const SyncOnGpu sync_gpu = a.sync_parser != "gpu" ? SyncOnGpu::no : subset ? SyncOnGpu::host : SyncOnGpu::device;
        PieceReader pieces(in.mf, in.cuts, c0, c1, device, threads, kind, pf, 0, !subset, sync_gpu, a.pileup_parser == "gpu");
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
        DeviceResultWriter writer; // (its timing line, under PGH_TIMING, comes when the rank is done)
        while (pieces.more()) {
            SyncBatch sb = pieces.next();
            if (sb.L == 0) continue;
            if (sb.n != n) throw std::runtime_error("the number of pools in the sync file and in the phenotype file differ");
            const int64_t L = sb.L;
            totals[r] += L;
            if (L > cap_loci) {
                cap_loci = L + L / 8;
                if (!sb.counts_dev) counts_dev.reset(sizeof(uint32_t) * (size_t)cap_loci * n * 6, "device memory for the counts");
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
            } else if (!sb.counts_dev)
                upload(gpu, sb, counts_dev.get());
            const uint32_t *counts = sb.counts_dev ? sb.counts_dev : counts_dev.get();
            if (gwa) // sig, MIN, MAX: rows 0..2 of the matrix' third column (gwalpha.rs:214-216)
                gpu.ok(pg_gwalpha_batch_dev(gpu.c, counts, L, n2, ps.data(), gw_q.data(), ph.phen[2], ph.phen[5], ph.phen[8], &flt, gw_method,
                                            n_out_dev.get(), ids_dev.get(), mf_dev.get(), stat_dev.get(), nullptr, nullptr, nullptr), "gwalpha");
            else if (op == Analysis::fisher_exact_test)
                gpu.ok(pg_fisher_batch_dev(gpu.c, counts, L, n2, ps.data(), &flt, n_out_dev.get(), ids_dev.get(), stat_dev.get(), pv_dev.get()),
                       "fisher_exact_test");
            else if (op == Analysis::chisq_test)
                gpu.ok(pg_chisq_batch_dev(gpu.c, counts, L, n2, ps.data(), &flt, n_out_dev.get(), ids_dev.get(), stat_dev.get(), pv_dev.get()),
                       "chisq_test");
            else if (op == Analysis::pearson_corr)
                gpu.ok(pg_pearson_batch_dev(gpu.c, counts, L, n2, ps.data(), &flt, Y.data(), k, n_out_dev.get(), ids_dev.get(), mf_dev.get(),
                                            stat_dev.get(), pv_dev.get()), "pearson_corr");
            else
                gpu.ok(pg_ols_iter_batch_dev(gpu.c, counts, L, n2, ps.data(), &flt, Y.data(), k, n_out_dev.get(), ids_dev.get(), mf_dev.get(),
                                             stat_dev.get(), pv_dev.get()), "ols_iter");
            if (gpu_writer) { // --result-writer gpu: the piece's results stay on the device, only their text comes back
                if (!fo) {
                    fo = create_new(part[r]);
                    created[r] = 1;
                    if (R == 1) fputs(header, fo);
                }
                writer.set_locus_labels(sb.chrom_id, sb.pos, sb.chrom_names, L);
                writer.locus_rows(gpu.c, result_op, L, k, n_out_dev.get(), ids_dev.get(), tables ? nullptr : mf_dev.get(), stat_dev.get(),
                                  gwa ? nullptr : pv_dev.get(), fo);
                continue;
            }
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
                created[r] = 1;
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
    if (total == 0) { cleanup_parts(); throw std::runtime_error("no loci in " + a.fname); } // (no part was made)
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
    return done_ok(out);
}

