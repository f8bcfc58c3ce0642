// cli_matrix.cpp -- the analyses' common start, the matrix loaded into HBM, and the kinship GWAS on it.
#include "cli.h"
#include <cstring>
#include <map>
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
                               bool mle, bool gpu_writer, int64_t slab_rows) {
    const int64_t p = g.p;
    const int k = g.k;
    if (!fname_output.empty()) probe_output(fname_output); // ols.rs:285
    std::vector<double> beta((size_t)p * k), pval((size_t)p * k);
    int m = 0;
    const size_t cnt = (size_t)p * k;
    DeviceBuf<double> out_dev(sizeof(double) * 3 * cnt, "device memory for the results");
    {
        const double *G = g.intercept_and_allele_frequencies.get();
        if (mle)
            gpu.ok(pg_mle_kinship_dev(gpu.c, G, p, g.n, g.ld, g.phenotypes.data(), k, xxt_eigen_variance_explained, -1, &m, nullptr, out_dev.get(),
                                      out_dev.get() + cnt, out_dev.get() + 2 * cnt), "mle_iter_with_kinship");
        else
            gpu.ok(pg_ols_kinship_dev(gpu.c, G, p, g.n, g.ld, g.phenotypes.data(), k, xxt_eigen_variance_explained, -1, &m, nullptr, out_dev.get(),
                                      out_dev.get() + cnt, out_dev.get() + 2 * cnt), "ols_iter_with_kinship");
        gpu.ok(pg_synchronize(gpu.c), "ols_iter_with_kinship");
        if (!gpu_writer) {
            hip_ok(hipMemcpy(beta.data(), out_dev.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
            hip_ok(hipMemcpy(pval.data(), out_dev.get() + 2 * cnt, sizeof(double) * cnt, hipMemcpyDeviceToHost), "D2H results");
        }
    }
    if (!gpu_writer) out_dev.reset();
    lap(gpu_writer ? "kinship + fits" : "kinship + fits + D2H");
    std::string out = fname_output;
    if (out.empty()) // ols.rs:393-398
        out = basename_no_ext(fname_input) + (mle ? "-mle_iterative_xxt_" : "-ols_iterative_xxt_") + std::to_string(m + 1) + "_eigens-" +
              unix_time_string() + ".csv"; // ols.rs:393-398, mle.rs:423-427
    if (gpu_writer) { // --result-writer gpu: beta and pval stay on the device; their rows are formatted there, a slab of rows per turn
        std::vector<std::string> names;
        std::map<std::string, int32_t> id_of;
        std::vector<int32_t> col_chrom(p), col_allele(p);
        std::vector<uint64_t> col_pos(p);
        for (int64_t c = 0; c < p; ++c) { // column c carries entry c + 1 of the (1+p)-long label vectors; the shift is the formatter's
            const auto it = id_of.emplace(g.chromosome[c + 1], (int32_t)names.size());
            if (it.second) names.push_back(g.chromosome[c + 1]);
            col_chrom[c] = it.first->second;
            col_pos[c] = g.position[c + 1];
            const char *at = g.allele[c + 1].size() == 1 ? std::strchr(ALLELES, g.allele[c + 1][0]) : nullptr;
            if (!at || !*at) throw std::runtime_error("--result-writer gpu: the allele label `" + g.allele[c + 1] + "` is none of " + ALLELES);
            col_allele[c] = (int32_t)(at - ALLELES);
        }
        DeviceResultWriter writer;
        writer.set_column_labels(col_chrom, col_pos, col_allele, names);
        FILE *fo = create_new(out);
        try {
            fputs("#chr,pos,alleles,phenotype,statistic,pvalue\n", fo); // ols.rs:409
            const int64_t total = (int64_t)k * p, step = result_slab_rows((int)std::min<int64_t>(slab_rows, INT32_MAX));
            for (int64_t row0 = 0; row0 < total; row0 += step)
                writer.kinship_rows(gpu.c, p, k, row0, std::min(step, total - row0), out_dev.get(), out_dev.get() + 2 * cnt, fo);
            if (fclose(fo) != 0) { fo = nullptr; throw std::runtime_error("write error on " + out); }
        } catch (...) { // a failure on the way leaves no file
            if (fo) fclose(fo);
            ::unlink(out.c_str());
            throw;
        }
        lap("format (gpu) + write CSV");
        return out;
    }
    write_kinship_csv(out, p, k, beta, pval, n_threads, [&](int64_t i, std::string &text) {
        // the reference labels coefficient i with entry i of the (1+p)-long label vectors, i.e.
        // shifted by the intercept entry (ols.rs:421-425) -- reproduced as is
        text += g.chromosome[i]; text.push_back(','); text += std::to_string(g.position[i]); text.push_back(','); text += g.allele[i];
    });
    lap("format + write CSV");
    return out;
}


// The rows of a resident frequency table as the allele-frequency CSV (the line loops of sync.rs:1239-1259 and :1315-1332): the
// header "#chr,pos,allele,<pools>", then the text of pg_csv_freq_rows_dev, a slab of rows at a time: format into a device buffer,
// copy to pinned memory, write.  `out` has been probed by the caller; the file does not depend on slab_rows (0 = what CSV_SLAB_BYTES
// of text hold); a failure leaves no file.  PGH_TIMING=1 splits the lap into its three parts.
void write_freq_csv(Ctx &gpu, const SyncBatch &sb, const std::vector<std::string> &pool_names, const double *G, int64_t ld, int n, int64_t p,
                    const int64_t *col_locus_dev, const int32_t *col_allele_dev, const std::string &out, int64_t slab_rows, const char *what,
                    Lap &lap) {
    const int64_t L = sb.size();
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
    slab_rows = std::min(slab_rows, p);
    const int64_t cap = slab_rows * row_max;
    DeviceBuf<char> text_dev((size_t)cap, "device memory for the text");
    PinnedBuf text_host;
    if (!text_host.reset((size_t)cap)) throw std::runtime_error("out of pinned host memory for the text");
    FILE *fo = create_new(out);
    std::string header = "#chr,pos,allele,";
    for (int i = 0; i < n; ++i) { header += pool_names[i]; header.push_back(i + 1 < n ? ',' : '\n'); }
    fputs(header.c_str(), fo);
    std::fflush(fo);
    const int fd = fileno(fo);
    off_t at = (off_t)header.size();
    double t_format = 0, t_copy = 0, t_write = 0;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto since = [&](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double>(now() - t0).count(); };
    try {
        for (int64_t row0 = 0; row0 < p; row0 += slab_rows) {
            const int64_t rows = std::min(slab_rows, p - row0);
            int64_t bytes = 0;
            auto t0 = now();
            gpu.ok(pg_csv_freq_rows_dev(gpu.c, G, ld, n, row0, rows, col_locus_dev, col_allele_dev, chrom_dev.get(),
                                        pos_dev.get(), names_dev.get(), off_dev.get(), (int)sb.chrom_names.size(), text_dev.get(), cap, &bytes),
                   what);
            gpu.ok(pg_synchronize(gpu.c), what);
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
                     (long long)p, (long long)at);
}

// FileSyncPhen::write_csv (base/sync.rs:1182-1262): the loaded table -- every pool of the phenotype file (:1222, :1236), a row per
// surviving allele in (chromosome, position) order -- as "#chr,pos,allele,<pools>" and one line of frequencies per row.  The
// matrix is loaded as for the other analyses and stays in HBM; its text is formatted there too (write_freq_csv).  `out` has been
// probed by the caller.
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
    write_freq_csv(gpu, sb, ph.pool_names, m.G.get(), ld, n, m.p, m.col_locus_dev.get(), m.col_allele_dev.get(), out, slab_rows, "sync2csv", lap);
    lap("format + write CSV");
    return out;
}

// impute_mean / impute_aLDkNN (imputation/mean_imputation.rs:65-162, adaptive_ld_knn_imputation.rs:371-477): the matrix is loaded
// with every allele and its coverages, in sorted locus order, and stays in HBM through every step -- missing by depth, the sparsest
// pools and loci out, the imputation, the coverage mark, the loci still missing everywhere out (the pg_impute entry points; the
// host only applies the keep rule to the NaN counts and plans the windows) -- and is printed by the GPU formatter of sync2csv
// (GenotypesAndPhenotypes::write_csv, sync.rs:1264-1335).  The six progress lines go to stdout as in the reference.
std::string impute(Ctx &gpu, const SyncBatch &sb, const Phen &ph, const pg_filter &flt, const Args &a, const std::string &out, Lap &lap) {
    const bool mean = a.imputation_method == "mean";
    int n = sb.n;
    int64_t ld = n + (n & 1);
    const int64_t L0 = sb.size();
    std::vector<int32_t> pool_map(n);
    std::iota(pool_map.begin(), pool_map.end(), 0);
    auto t0 = std::chrono::steady_clock::now();
    LoadedMatrix m;
    {
        const std::vector<int64_t> order = sorted_locus_order(sb);
        DeviceBuf<uint32_t> counts_dev(sizeof(uint32_t) * (size_t)L0 * n * 6, "device memory for the counts");
        DeviceBuf<int64_t> order_dev(sizeof(int64_t) * L0, "device memory");
        CountsUpload upload;
        upload(gpu, sb, counts_dev.get());
        hip_ok(hipMemcpy(order_dev.get(), order.data(), sizeof(int64_t) * L0, hipMemcpyHostToDevice), "H2D order");
        m = load_matrix(gpu, counts_dev.get(), L0, n, ph.pool_sizes, flt, /*keep_p_minus_1=*/false, order_dev.get(), pool_map, n, ld,
                        /*with_coverages=*/true, /*labels_on_device=*/true);
    }
    if (m.p <= 0) throw std::runtime_error("no loci passed the filters");
    lap("sort + H2D + GPU loader");
    // the table as it stands: matrix, coverages and column labels on the device, the loci's first columns and labels on the host
    int64_t p = m.p;
    DeviceBuf<double> G = std::move(m.G), cov = std::move(m.coverages);
    DeviceBuf<int64_t> cl = std::move(m.col_locus_dev);
    DeviceBuf<int32_t> ca = std::move(m.col_allele_dev);
    std::vector<int64_t> locus_col, locus_id; // count_loci (sync.rs:73-97): a new locus where (chromosome, position) changes
    {
        std::vector<int64_t> col_locus((size_t)p);
        hip_ok(hipMemcpy(col_locus.data(), cl.get(), sizeof(int64_t) * p, hipMemcpyDeviceToHost), "D2H labels");
        for (int64_t c = 0; c < p; ++c) {
            const int64_t l = col_locus[c], k = c ? col_locus[c - 1] : -1;
            if (c == 0 || sb.chrom_id[l] != sb.chrom_id[k] || sb.pos[l] != sb.pos[k]) { locus_col.push_back(c); locus_id.push_back(l); }
        }
        locus_col.push_back(p);
    }
    std::vector<std::string> pool_names = ph.pool_names;
    pool_names.resize(n);
    std::vector<int64_t> pool_nan, locus_nan;
    auto count = [&](bool pools) { // the NaN counts of the table as it stands
        const int64_t L = (int64_t)locus_id.size();
        pool_nan.assign(n, 0); locus_nan.assign(L, 0);
        gpu.ok(pg_missingness_dev(gpu.c, G.get(), cov.get(), p, n, ld, locus_col.data(), L, pools ? pool_nan.data() : nullptr, locus_nan.data()), "impute");
    };
    auto report = [&](const char *what) { // "{what}: {n} pools x {l} loci | Missingness: {missing_rate()}% | Duration: {secs} seconds"
        const int64_t L = (int64_t)locus_id.size();
        double sum = 0.0;
        for (int64_t x : locus_nan) sum += (double)x;
        const double rate = std::round(sum * 100.0 / (double)((int64_t)n * L) * 100.0) / 100.0; // sensible_round(.., 2)
        const auto t1 = std::chrono::steady_clock::now();
        std::cout << what << ": " << n << " pools x " << L << " loci | Missingness: " << rust_display(rate) << "% | Duration: "
                  << std::chrono::duration_cast<std::chrono::seconds>(t1 - t0).count() << " seconds\n";
        t0 = t1;
    };
    auto compact = [&](const std::vector<int64_t> &keep_pools, const std::vector<int64_t> &keep_loci) {
        const int n2 = (int)keep_pools.size();
        const int64_t ld2 = n2 + (n2 & 1), L2 = (int64_t)keep_loci.size();
        int64_t p2 = 0;
        for (int64_t l : keep_loci) p2 += locus_col[l + 1] - locus_col[l];
        DeviceBuf<double> G2(sizeof(double) * (size_t)p2 * ld2, "device memory for the genotype matrix"), cov2(sizeof(double) * (size_t)p2 * ld2, "device memory for the coverages");
        DeviceBuf<int64_t> cl2(sizeof(int64_t) * p2, "device memory");
        DeviceBuf<int32_t> ca2(sizeof(int32_t) * p2, "device memory");
        std::vector<int64_t> lc2((size_t)L2 + 1), id2;
        gpu.ok(pg_impute_compact_dev(gpu.c, G.get(), cov.get(), p, n, ld, cl.get(), ca.get(), locus_col.data(), (int64_t)locus_id.size(), keep_pools.data(),
                                     n2, keep_loci.data(), L2, G2.get(), cov2.get(), ld2, cl2.get(), ca2.get(), lc2.data()), "impute");
        for (int64_t l : keep_loci) id2.push_back(locus_id[l]);
        std::vector<std::string> names2;
        for (int64_t i : keep_pools) names2.push_back(pool_names[i]);
        G = std::move(G2); cov = std::move(cov2); cl = std::move(cl2); ca = std::move(ca2);
        locus_col = std::move(lc2); locus_id = std::move(id2); pool_names = std::move(names2);
        n = n2; ld = ld2; p = p2;
    };
    auto keep_of = [&](const std::vector<int64_t> &nan_count, double frac, const char *what) {
        std::vector<int64_t> keep(nan_count.size());
        const int64_t left = pg_host_top_missing_keep(nan_count.data(), (int64_t)nan_count.size(), frac, keep.data());
        if (left <= 0) throw std::runtime_error(std::string("No ") + what + " left after filtering, please reduce 'frac_top_missing_" + what + "'");
        keep.resize((size_t)left);
        return keep;
    };
    auto all = [](int64_t count) { std::vector<int64_t> v((size_t)count); std::iota(v.begin(), v.end(), (int64_t)0); return v; };

    count(false);
    report("Parsed the sync file into allele frequncies");
    gpu.ok(pg_set_missing_by_depth_dev(gpu.c, G.get(), cov.get(), p, n, ld, locus_col.data(), (int64_t)locus_id.size(), a.min_depth_set_to_missing), "impute");
    count(true);
    report("Set missing loci below the minimum depth");
    compact(keep_of(pool_nan, a.frac_top_missing_pools, "pools"), all((int64_t)locus_id.size()));
    count(false);
    report("Filtered out sparsest pools");
    compact(all(n), keep_of(locus_nan, a.frac_top_missing_loci, "loci"));
    count(false);
    report("Filtered out sparsest loci");
    lap("missing data filters");
    const int64_t L = (int64_t)locus_id.size();
    if (mean) {
        gpu.ok(pg_impute_mean_dev(gpu.c, G.get(), p, n, ld, locus_col.data(), L), "impute");
    } else {
        std::vector<int32_t> chr((size_t)L);
        std::vector<uint64_t> pos((size_t)L);
        for (int64_t l = 0; l < L; ++l) { chr[l] = sb.chrom_id[locus_id[l]]; pos[l] = sb.pos[locus_id[l]]; }
        std::vector<int64_t> head((size_t)L), tail((size_t)L);
        const int64_t nw = pg_host_sliding_windows(chr.data(), pos.data(), L, a.window_size_bp, a.window_slide_size_bp, a.min_loci_per_window, head.data(),
                                                   tail.data());
        if (nw < 0) throw std::runtime_error("impute: the sliding windows could not be defined");
        DeviceBuf<double> G2(sizeof(double) * (size_t)p * ld, "device memory for the imputed matrix");
        gpu.ok(pg_impute_aldknn_dev(gpu.c, G.get(), p, n, ld, locus_col.data(), L, head.data(), tail.data(), nw, (int64_t)a.n_loci_to_estimate_distance,
                                    (int64_t)a.k_neighbours, 0, G2.get()), "impute");
        G = std::move(G2);
    }
    gpu.ok(pg_impute_mark_cov_dev(gpu.c, cov.get(), p, n, ld, locus_col.data(), L), "impute");
    count(false);
    report(mean ? "Mean value imputation" : "Adaptive LD-kNN imputation");
    lap("imputation");
    compact(all(n), keep_of(locus_nan, 1.0, "loci"));
    count(false);
    report("Missing data removed, i.e. loci which cannot be imputed because of extreme sparsity");
    write_freq_csv(gpu, sb, pool_names, G.get(), ld, n, p, cl.get(), ca.get(), out, a.csv_slab_rows, "impute", lap);
    lap("format + write CSV");
    return out;
}
