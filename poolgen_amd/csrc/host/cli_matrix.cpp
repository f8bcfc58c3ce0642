// cli_matrix.cpp -- the analyses' common start, the matrix loaded into HBM, and the kinship GWAS on it.
#include "cli.h"
#include <numeric>

// FileSyncPhen::into_genotypes_and_phenotypes (base/sync.rs:1106-1179) = load (:1044-1104: filter + frequencies per locus,
// sorted by (chromosome, position)) + the dense fill.  The host only sorts the locus order; filter, frequencies and the
// column layout run on the GPU from the parsed counts (pg_load_plan_dev / pg_load_emit[_cov]_dev), and the matrix never
// exists in host memory.  `remove_missing`: drop the pools without phenotype (what ols_with_covariate does first,
// gwas/ols.rs:287); the popgen tools keep every pool.
static std::vector<int64_t> sorted_locus_order(const SyncBatch &sb) { // the (chromosome, position) sort of sync.rs:1092-1101
    std::vector<int64_t> order(sb.size());
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
        const int c = sb.chrom(x).compare(sb.chrom(y));
        return c != 0 ? c < 0 : sb.pos[x] < sb.pos[y];
    });
    return order;
}

GenotypesAndPhenotypes into_genotypes_and_phenotypes(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt,
                                                     bool keep_p_minus_1, bool remove_missing, bool with_coverages, Lap &lap) {
    const int n = sb.n, k = ph.k;
    const int64_t L = sb.size();
    const std::vector<int64_t> order = sorted_locus_order(sb);
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
std::string ols_with_covariate(Ctx &gpu, GenotypesAndPhenotypes &g, double xxt_eigen_variance_explained,
                               const std::string &fname_input, const std::string &fname_output, int n_threads, Lap &lap,
                               bool mle) {
    const int64_t p = g.p;
    const int k = g.k;
    if (!fname_output.empty()) probe_output(fname_output); // ols.rs:285
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


// FileSyncPhen::write_csv (base/sync.rs:1182-1262): the loaded table -- every pool of the phenotype file (:1222, :1236), a row per
// surviving allele in (chromosome, position) order -- as "#chr,pos,allele,<pools>" and one line of frequencies per row.  The
// matrix is loaded as for the other analyses and stays in HBM; its text is formatted there too (pg_csv_freq_rows_dev), a slab of
// rows at a time: format into a device buffer, copy to pinned memory, write.  `out` has been probed by the caller; the file does
// not depend on slab_rows (0 = what CSV_SLAB_BYTES of text hold).  PGH_TIMING=1 splits the last lap into its three parts.
std::string sync2csv(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt, bool keep_p_minus_1, const std::string &out,
                     int64_t slab_rows, Lap &lap) {
    const int n = sb.n;
    const int64_t L = sb.size(), ld = n + (n & 1);
    std::vector<int32_t> pool_map(n);
    std::iota(pool_map.begin(), pool_map.end(), 0);
    LoadedMatrix m;
    {
        const std::vector<int64_t> order = sorted_locus_order(sb);
        DeviceBuf<uint32_t> counts_dev(sizeof(uint32_t) * (size_t)L * n * 6, "device memory for the counts");
        DeviceBuf<int64_t> order_dev(sizeof(int64_t) * L, "device memory");
        CountsUpload upload;
        upload(gpu, sb, counts_dev.get());
        hip_ok(hipMemcpy(order_dev.get(), order.data(), sizeof(int64_t) * L, hipMemcpyHostToDevice), "H2D order");
        m = load_matrix(gpu, counts_dev.get(), L, n, ph.pool_sizes, flt, keep_p_minus_1, order_dev.get(), pool_map, n, ld, false,
                        /*labels_on_device=*/true);
    }
    if (m.p <= 0) // sync.rs:1220
        throw std::runtime_error("No data passed the filtering variables. Please decrease minimum depth, and/or minimum allele frequency.");
    lap("sort + H2D + GPU loader");
    // the loci's labels and the name table, once
    std::string names;
    std::vector<int32_t> name_off(1, 0);
    size_t longest = 0;
    for (const std::string &c : sb.chrom_names) {
        names += c;
        name_off.push_back((int32_t)names.size());
        longest = std::max(longest, c.size());
    }
    DeviceBuf<int32_t> chrom_dev(sizeof(int32_t) * L, "device memory"), off_dev(sizeof(int32_t) * name_off.size(), "device memory");
    DeviceBuf<uint64_t> pos_dev(sizeof(uint64_t) * L, "device memory");
    DeviceBuf<char> names_dev(std::max<size_t>(1, names.size()), "device memory");
    hip_ok(hipMemcpy(chrom_dev.get(), sb.chrom_id.data(), sizeof(int32_t) * L, hipMemcpyHostToDevice), "H2D labels");
    hip_ok(hipMemcpy(pos_dev.get(), sb.pos.data(), sizeof(uint64_t) * L, hipMemcpyHostToDevice), "H2D labels");
    hip_ok(hipMemcpy(off_dev.get(), name_off.data(), sizeof(int32_t) * name_off.size(), hipMemcpyHostToDevice), "H2D labels");
    if (!names.empty()) hip_ok(hipMemcpy(names_dev.get(), names.data(), names.size(), hipMemcpyHostToDevice), "H2D labels");
    // a slab's text is at most rows x (longest name + 24 + 9 n) bytes
    const int64_t row_max = (int64_t)longest + 24 + 9 * (int64_t)n;
    if (slab_rows <= 0) slab_rows = std::max<int64_t>(1, CSV_SLAB_BYTES / row_max);
    slab_rows = std::min(slab_rows, m.p);
    const int64_t cap = slab_rows * row_max;
    DeviceBuf<char> text_dev((size_t)cap, "device memory for the text");
    PinnedBuf text_host;
    if (!text_host.reset((size_t)cap)) throw std::runtime_error("out of pinned host memory for the text");
    FILE *fo = create_new(out);
    std::string header = "#chr,pos,allele,";
    for (int i = 0; i < n; ++i) { header += ph.pool_names[i]; header.push_back(i + 1 < n ? ',' : '\n'); }
    fputs(header.c_str(), fo);
    std::fflush(fo);
    const int fd = fileno(fo);
    off_t at = (off_t)header.size();
    double t_format = 0, t_copy = 0, t_write = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); };
    try {
        for (int64_t row0 = 0; row0 < m.p; row0 += slab_rows) {
            const int64_t rows = std::min(slab_rows, m.p - row0);
            int64_t bytes = 0;
            auto t0 = now();
            gpu.ok(pg_csv_freq_rows_dev(gpu.c, m.G.get(), ld, n, row0, rows, m.col_locus_dev.get(), m.col_allele_dev.get(), chrom_dev.get(),
                                        pos_dev.get(), names_dev.get(), off_dev.get(), (int)sb.chrom_names.size(), text_dev.get(), cap, &bytes),
                   "sync2csv");
            gpu.ok(pg_synchronize(gpu.c), "sync2csv");
            t_format += since(t0); t0 = now();
            hip_ok(hipMemcpy(text_host.get(), text_dev.get(), (size_t)bytes, hipMemcpyDeviceToHost), "D2H text");
            t_copy += since(t0); t0 = now();
            const char *q = static_cast<const char *>(text_host.get());
            for (size_t left = (size_t)bytes; left > 0;) { // one writer
                const ssize_t w = ::pwrite(fd, q, left, at);
                if (w <= 0) throw std::runtime_error("write failed (disk full?)");
                q += w; at += w; left -= (size_t)w;
            }
            t_write += since(t0);
        }
    } catch (...) { // no partly written file stays behind: a later run with the same name would be refused
        fclose(fo);
        ::unlink(out.c_str());
        throw;
    }
    fclose(fo);
    if (lap.on)
        std::fprintf(stderr, "poolgen: %-24s %.3f s  D2H %.3f s  write %.3f s  (%lld rows, %lld bytes)\n", "GPU format", t_format, t_copy, t_write,
                     (long long)m.p, (long long)at);
    lap("format + write CSV");
    return out;
}
