// cli_matrix.cpp -- the analyses' common start, the matrix loaded into HBM, and the kinship GWAS on it.
#include "cli.h"
#include <numeric>

// FileSyncPhen::into_genotypes_and_phenotypes (base/sync.rs:1106-1179) = load (:1044-1104: filter + frequencies per locus,
// sorted by (chromosome, position)) + the dense fill.  The host only sorts the locus order; filter, frequencies and the
// column layout run on the GPU from the parsed counts (pg_load_plan_dev / pg_load_emit[_cov]_dev), and the matrix never
// exists in host memory.  `remove_missing`: drop the pools without phenotype (what ols_with_covariate does first,
// gwas/ols.rs:287); the popgen tools keep every pool.
GenotypesAndPhenotypes into_genotypes_and_phenotypes(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt,
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

