// cli_popgen.cpp -- fst (popgen/fst.rs:10-261), heterozygosity = pi (popgen/pi.rs:115-190), watterson_estimator
// (popgen/watterson_theta.rs:191-289), tajima_d (popgen/tajima_d.rs:10-171) and gudmc on the loaded matrix: loci and windows on the
// host (popgen_plan.h), the per-locus arithmetic and the means on the GPU, the files as written by the reference.
#include "cli.h"
#include "popgen_plan.h"
#include "result_writer.h"

// What pg_gudmc_dev fills, as it lies in one block of doubles (2 values per population, 4 per pair, 6 per row, n^2 w rows) and
// one of integers (rows per population, the rows' windows): over the device blocks for the call, over their host copies for the writer.
struct GudmcResults {
    double *d_mean, *d_sd, *f_mean, *f_sd, *w_mean, *w_sd, *r_d, *r_width, *r_wdev, *r_wp, *r_delta, *r_fp;
    int64_t *rows, *r_win;
    static size_t n_f64(size_t n, size_t nw) { return 2 * n + 4 * n * n + 6 * n * n * nw; }
    static size_t n_i64(size_t n, size_t nw) { return n + n * n * nw; }
    GudmcResults(double *f, int64_t *i, size_t n, size_t nw) : rows(i), r_win(i + n) {
        const size_t nn = n * n, rows_all = nn * nw;
        d_mean = f; d_sd = d_mean + n; f_mean = d_sd + n; f_sd = f_mean + nn; w_mean = f_sd + nn; w_sd = w_mean + nn; r_d = w_sd + nn;
        r_width = r_d + rows_all; r_wdev = r_width + rows_all; r_wp = r_wdev + rows_all; r_delta = r_wp + rows_all; r_fp = r_delta + rows_all;
    }
};

// --popgen-writer gpu: a new file written by body(fo), its text formatted on the device (pg_f64_table_dev, pg_gudmc_rows_dev); a
// failure on the way leaves no file.
template <class Body>
static void write_new_file(const std::string &out, Body body) {
    FILE *fo = create_new(out);
    try {
        body(fo);
        if (fclose(fo) != 0) { fo = nullptr; throw std::runtime_error("write error on " + out); }
    } catch (...) {
        if (fo) fclose(fo);
        ::unlink(out.c_str());
        throw;
    }
}

// byte strings with offsets, on the device: the labels of a table's rows (int64 offsets) or a name table (int32 offsets)
template <typename Off>
struct DeviceStrings {
    DeviceBuf<char> text;
    DeviceBuf<Off> off;
    explicit DeviceStrings(const std::vector<std::string> &items) {
        std::string all;
        std::vector<Off> o{0};
        for (const std::string &s : items) { all += s; o.push_back((Off)all.size()); }
        text.reset(all.size() + 1, "the labels");
        off.reset(sizeof(Off) * o.size(), "the labels");
        if (!all.empty()) hip_ok(hipMemcpy(text.get(), all.data(), all.size(), hipMemcpyHostToDevice), "H2D labels");
        hip_ok(hipMemcpy(off.get(), o.data(), sizeof(Off) * o.size(), hipMemcpyHostToDevice), "H2D labels");
    }
};

// rows per turn: the flag, or what fits the writer's text budget at `row_bytes` a row
static int64_t popgen_slab_rows(const Args &a, int64_t row_bytes) {
    return a.popgen_slab_rows > 0 ? a.popgen_slab_rows : std::max<int64_t>(1, RESULT_SLAB_BYTES / std::max<int64_t>(1, row_bytes));
}

constexpr int64_t POPGEN_CELL_TYPICAL = 24; // bytes of a cell for the default slab: 17 digits, "0.", a sign, the separator and some room

// the rows of a device table (cell (r, c) at x[r * row_stride + c * col_stride]) with their labels, appended to fo slab by slab
static void table_rows_to_file(DeviceResultWriter &writer, Ctx &gpu, const Args &a, FILE *fo, const double *x_dev, int64_t rows, int64_t cols,
                               int64_t row_stride, int64_t col_stride, int n_digits, int first_col_digits, const std::vector<std::string> &labels) {
    const DeviceStrings<int64_t> lab(labels);
    const int64_t step = popgen_slab_rows(a, cols * POPGEN_CELL_TYPICAL + 32);
    for (int64_t row0 = 0; row0 < rows; row0 += step)
        writer.text(gpu.c, fo, [&](char *text, int64_t cap, int64_t *need) {
            return pg_f64_table_dev(gpu.c, x_dev, rows, cols, row_stride, col_stride, row0, std::min(step, rows - row0), n_digits, first_col_digits,
                                    lab.text.get(), lab.off.get(), text, cap, need);
        });
}

static std::string window_label(const PopgenPlan &pl, int64_t w, char sep) {
    return pl.loc_chr[pl.wh[w]] + sep + std::to_string(pl.loc_pos[pl.wh[w]]) + sep + std::to_string(pl.loc_pos[pl.wt[w]]);
}

static const char *GUDMC_HEADER =
    "pop_a,pop_b,chr,pos_ini,pos_fin,mean_tajima_d_pop_b,mean_fst,sd_tajima_d_pop_b,sd_fst,tajima_d_pop_b,tajima_width_pop_b,"
    "tajima_width_deviation_from_r_pop_b,tajima_width_one_tail_pval_pop_b,fst_delta,fst_delta_one_tail_pval\n";

// gudmc (popgen/gudmc.rs:64-462): tajima_d and fst as below, then the fits, widths and p-values on the GPU, one row per
// (pair, row of population b).  D and Fst go from the tables entry points into pg_gudmc_dev on the device; then the writer: host
// takes the results down and formats them here, gpu formats the rows there and takes down only rows[n], for the number of rows.
static int popgen_gudmc(const Args &a, Ctx &gpu, const GenotypesAndPhenotypes &g, const std::vector<double> &pool_sizes, const PopgenPlan &pl, Lap &lap) {
    const double *G_dev = g.intercept_and_allele_frequencies.get(), *cov_dev = g.coverages.get();
    const int n = g.n;
    const int64_t nw = pl.nw();
    const std::string time = unix_time_string();
    // The reference reads both tables back from text and takes their labels apart:
    for (const std::string &c : pl.loc_chr)
        if (c.find('-') != std::string::npos) // "Window-<chr>_<ini>_<fin>".split("-")[1] (:169)
            throw std::runtime_error("gudmc: chromosome name `" + c + "` contains `-`; the reference splits its window labels at `-` and fails on it");
    for (int i = 0; i < n; ++i) {
        if (g.pool_names[i].find("_vs_") != std::string::npos) // "<a>_vs_<b>".split("_vs_") (:231)
            throw std::runtime_error("gudmc: pool name `" + g.pool_names[i] + "` contains `_vs_`; the reference splits its pair labels there");
        for (int j = 0; j < i; ++j)
            if (g.pool_names[i] == g.pool_names[j]) // position() finds the first of them (:298)
                throw std::runtime_error("gudmc: pool name `" + g.pool_names[i] + "` occurs twice; the reference matches populations by name");
    }
    if (nw <= 0) throw std::runtime_error(NO_WINDOWS);
    if (!a.popgen_as_documented)
        std::cerr << "note: gudmc reproduces the reference: the pool sizes are fractions of their sum, so every Tajima's D is NaN, no population has a row "
                     "and the file is the header alone; --popgen-as-documented uses the pool sizes as written and counts every locus\n";
    const bool on_gpu = a.popgen_writer == "gpu";
    const size_t nn = (size_t)n * n, wn = (size_t)nw * n;
    std::string out = a.output;
    if (out.empty()) out = basename_no_ext(a.fname) + "-gudmc-" + time + ".csv"; // :383-401
    if (on_gpu) probe_output(out);
    // The tajima_d and fst entry points refuse a window whose tail lies before its head, so they see the others (pl.keep) and its
    // rows stay NaN: mean_axis of the empty slice gives None there and both tables hold NaN (pi.rs:87-90, fst.rs:194-197).
    const int64_t nk = (int64_t)pl.keep.size();
    const bool ref = pl.reference_count;
    const int64_t *c = ref ? pl.kc.data() : nullptr, *sd = ref ? pl.kseed.data() : nullptr, *sl = ref ? pl.kslot.data() : nullptr;
    DeviceBuf<double> tabs(sizeof(double) * (wn + (size_t)nw * nn), "gudmc: tables"), means(sizeof(double) * (n + nn), "gudmc: tables");
    double *d_tab = tabs.get(), *f_tab = tabs.get() + wn;
    {
        // the kept windows' tables; where every window is kept they are the tables themselves
        DeviceBuf<double> kept;
        double *dk = d_tab, *fk = f_tab;
        if (nk < nw) {
            kept.reset(sizeof(double) * std::max<size_t>(1, (size_t)nk * (n + nn)), "gudmc: tables");
            dk = kept.get(); fk = kept.get() + (size_t)nk * n;
        }
        if (nk > 0) {
            gpu.ok(pg_tajima_d_tables_dev(gpu.c, G_dev, cov_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.kh.data(), pl.kt.data(), c, sd, sl, nk,
                                          pool_sizes.data(), dk, means.get(), nullptr, nullptr), "gudmc (tajima_d)");
            gpu.ok(pg_fst_tables_dev(gpu.c, G_dev, cov_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.kh.data(), pl.kt.data(), nk, means.get() + n, fk),
                   "gudmc (fst)");
        }
        if (nk < nw) { // the NaN rows and the kept ones at their places
            gpu.ok(pg_window_scatter_dev(gpu.c, dk, nk, pl.keep.data(), nw, n, d_tab), "gudmc (tables)");
            gpu.ok(pg_window_scatter_dev(gpu.c, fk, nk, pl.keep.data(), nw, (int64_t)nn, f_tab), "gudmc (tables)");
        }
    }
    std::vector<int32_t> wchr(nw);
    std::vector<uint64_t> wini(nw), wfin(nw);
    for (int64_t w = 0; w < nw; ++w) { wchr[w] = pl.chr_id[pl.wh[w]]; wini[w] = pl.loc_pos[pl.wh[w]]; wfin[w] = pl.loc_pos[pl.wt[w]]; }
    const size_t n_f64 = GudmcResults::n_f64(n, nw), n_i64 = GudmcResults::n_i64(n, nw);
    DeviceBuf<double> of(sizeof(double) * n_f64, "gudmc: the rows' values");
    DeviceBuf<int64_t> oi(sizeof(int64_t) * n_i64, "gudmc: the rows' windows");
    const GudmcResults o(of.get(), oi.get(), n, nw);
    gpu.ok(pg_gudmc_dev(gpu.c, d_tab, f_tab, nw, n, wchr.data(), wini.data(), wfin.data(), a.sigma_threshold, a.recombination_rate_cm_per_mb, o.rows,
                        o.d_mean, o.d_sd, o.f_mean, o.f_sd, o.w_mean, o.w_sd, o.r_win, o.r_d, o.r_width, o.r_wdev, o.r_wp, o.r_delta, o.r_fp), "gudmc");
    if (on_gpu) {
        std::vector<int64_t> rows(n);
        hip_ok(hipMemcpy(rows.data(), o.rows, sizeof(int64_t) * n, hipMemcpyDeviceToHost), "gudmc: D2H");
        lap("gudmc on the GPU");
        int64_t total = 0;
        for (int i = 0; i < n; ++i) total += rows[i];
        total *= n; // every pair (a, b) carries the rows of b (:433-434)
        std::vector<std::string> chrom_names; // by id: plan_popgen numbers the runs of one name
        for (int64_t l = 0; l < pl.L(); ++l)
            if ((size_t)pl.chr_id[l] == chrom_names.size()) chrom_names.push_back(pl.loc_chr[l]);
        DeviceBuf<int32_t> wchr_dev(sizeof(int32_t) * nw, "gudmc: the windows");
        DeviceBuf<uint64_t> wpos_dev(sizeof(uint64_t) * 2 * nw, "gudmc: the windows");
        hip_ok(hipMemcpy(wchr_dev.get(), wchr.data(), sizeof(int32_t) * nw, hipMemcpyHostToDevice), "gudmc: H2D");
        hip_ok(hipMemcpy(wpos_dev.get(), wini.data(), sizeof(uint64_t) * nw, hipMemcpyHostToDevice), "gudmc: H2D");
        hip_ok(hipMemcpy(wpos_dev.get() + nw, wfin.data(), sizeof(uint64_t) * nw, hipMemcpyHostToDevice), "gudmc: H2D");
        const DeviceStrings<int32_t> pools(g.pool_names), chroms(chrom_names);
        {
            DeviceResultWriter writer("popgen");
            write_new_file(out, [&](FILE *fo) {
                fputs(GUDMC_HEADER, fo);
                const int64_t step = popgen_slab_rows(a, 192);
                for (int64_t row0 = 0; row0 < total; row0 += step)
                    writer.text(gpu.c, fo, [&](char *text, int64_t cap, int64_t *need) {
                        return pg_gudmc_rows_dev(gpu.c, n, nw, row0, std::min(step, total - row0), o.rows, o.d_mean, o.d_sd, o.f_mean, o.f_sd, o.r_win,
                                                 o.r_d, o.r_width, o.r_wdev, o.r_wp, o.r_delta, o.r_fp, wchr_dev.get(), wpos_dev.get(),
                                                 wpos_dev.get() + nw, pools.text.get(), pools.off.get(), chroms.text.get(), chroms.off.get(),
                                                 (int)chrom_names.size(), text, cap, need);
                    });
            });
        }
        lap("format (gpu) + write CSV");
        return done_ok(out);
    }
    std::vector<double> hf(n_f64);
    std::vector<int64_t> hi(n_i64);
    hip_ok(hipMemcpy(hf.data(), of.get(), sizeof(double) * n_f64, hipMemcpyDeviceToHost), "gudmc: D2H");
    hip_ok(hipMemcpy(hi.data(), oi.get(), sizeof(int64_t) * n_i64, hipMemcpyDeviceToHost), "gudmc: D2H");
    lap("gudmc on the GPU");
    const GudmcResults h(hf.data(), hi.data(), n, nw);
    std::vector<int64_t> first(nn + 1, 0); // the first line of every pair (:433-434)
    for (size_t i = 0; i < nn; ++i) first[i + 1] = first[i] + h.rows[i % n];
    FILE *fo = create_new(out);
    fputs(GUDMC_HEADER, fo);
    write_rows_parallel(fo, first[nn], a.n_threads, [&](int64_t r, std::string &text) { // :435-455
        const size_t i = (size_t)(std::upper_bound(first.begin(), first.end(), r) - first.begin()) - 1;
        const size_t e = i * (size_t)nw + (size_t)(r - first[i]);
        const int pa = (int)(i / n), pb = (int)(i % n);
        text += g.pool_names[pa] + "," + g.pool_names[pb] + "," + window_label(pl, h.r_win[e], ',') + ",";
        append_roundup_own(text, h.d_mean[pb], 7); text.push_back(',');
        append_roundup_own(text, h.f_mean[i], 7); text.push_back(',');
        append_roundup_own(text, h.d_sd[pb], 7); text.push_back(',');
        append_roundup_own(text, h.f_sd[i], 7); text.push_back(',');
        append_rust_display(text, h.r_d[e]); text.push_back(',');
        append_rust_display(text, h.r_width[e]); text.push_back(',');
        append_rust_display(text, h.r_wdev[e]); text.push_back(',');
        append_roundup_own(text, h.r_wp[e], 7); text.push_back(',');
        append_roundup_own(text, h.r_delta[e], 7); text.push_back(',');
        append_roundup_own(text, h.r_fp[e], 7); text.push_back('\n');
    });
    fclose(fo);
    lap("write CSV");
    return done_ok(out);
}

// one row per pool: name, mean across windows, the windows (pi.rs:160-188, watterson_theta.rs:244-287, tajima_d.rs:127-169)
static int popgen_diversity(const Args &a, Ctx &gpu, const GenotypesAndPhenotypes &g, const std::vector<double> &pool_sizes, const PopgenPlan &pl, Lap &lap, Analysis analysis) {
    const double *G_dev = g.intercept_and_allele_frequencies.get(), *cov_dev = g.coverages.get();
    const int n = g.n;
    const int64_t nw = pl.nw();
    const std::string win = std::to_string(a.window_size_bp), time = unix_time_string();
    std::string out = a.output;
    const bool on_gpu = a.popgen_writer == "gpu";
    if (on_gpu && !out.empty()) probe_output(out);
    // [mean: n | windows: nw x n] in one block on the device, so that cell (pool i, column c) of the file's table, the mean in
    // column 0, is block[i + c * n]
    const size_t cells = (size_t)n + (size_t)std::max<int64_t>(nw, 0) * n;
    DeviceBuf<double> block(sizeof(double) * cells, "the windows' table");
    double *const pm_dev = block.get(), *const pw_dev = block.get() + n;
    const char *tag = "-pi-", *what = "heterozygosity"; // pi.rs:135-159
    if (analysis == Analysis::heterozygosity)
        gpu.ok(pg_pi_tables_dev(gpu.c, G_dev, cov_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.wh.data(), pl.wt.data(), nw, pw_dev, pm_dev), what);
    else {
        const bool tajima = analysis == Analysis::tajima_d;
        tag = tajima ? "-Tajimas_D-" : "-watterson-"; // tajima_d.rs:120-125, watterson_theta.rs:237-242
        what = tajima ? "tajima_d" : "watterson_estimator";
        if (!a.popgen_as_documented)
            std::cerr << "note: " << what << " reproduces the reference: the pool sizes are fractions of their sum, so every value is inf or NaN, "
                         "and the segregating sites are counted its way; --popgen-as-documented uses the pool sizes as written and counts every locus\n";
        const bool ref = pl.reference_count;
        const int64_t *c = ref ? pl.wc.data() : nullptr, *sd = ref ? pl.wseed.data() : nullptr, *sl = ref ? pl.wslot.data() : nullptr;
        if (tajima)
            gpu.ok(pg_tajima_d_tables_dev(gpu.c, G_dev, cov_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.wh.data(), pl.wt.data(), c, sd, sl, nw,
                                          pool_sizes.data(), pw_dev, pm_dev, nullptr, nullptr), what);
        else
            gpu.ok(pg_watterson_tables_dev(gpu.c, G_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.wh.data(), pl.wt.data(), c, sd, sl, nw,
                                           pool_sizes.data(), pw_dev, pm_dev, nullptr), what);
    }
    std::vector<double> host(on_gpu ? 0 : cells); // the host writer's copy of the block
    if (!on_gpu) hip_ok(hipMemcpy(host.data(), block.get(), sizeof(double) * cells, hipMemcpyDeviceToHost), "the windows' table: D2H");
    if (out.empty()) out = basename_no_ext(a.fname) + tag + win + "_bp_windows-" + time + ".csv";
    lap("windows on the GPU");
    std::string line = "Pool,Mean_across_windows";
    for (int64_t w = 0; w < nw; ++w) line += ",Window-" + window_label(pl, w, '_');
    if (on_gpu) {
        {
            DeviceResultWriter writer("popgen");
            write_new_file(out, [&](FILE *fo) {
                fputs((line + "\n").c_str(), fo);
                std::vector<std::string> labels;
                for (int i = 0; i < n; ++i) labels.push_back(g.pool_names[i] + ",");
                table_rows_to_file(writer, gpu, a, fo, block.get(), n, 1 + nw, 1, n, 8, -1, labels); // name,D(mean),R(w_0,8),...
            });
        }
        lap("format (gpu) + write CSV");
        return done_ok(out);
    }
    FILE *fo = create_new(out);
    fputs((line + "\n").c_str(), fo);
    for (int i = 0; i < n; ++i) {
        line = g.pool_names[i] + "," + rust_display(host[i]);
        for (int64_t w = 0; w < nw; ++w) line += "," + roundup_own(host[(size_t)(1 + w) * n + i], 8);
        fputs((line + "\n").c_str(), fo);
    }
    fclose(fo);
    lap("write CSV");
    return done_ok(out);
}

// fst: the genome-wide means, then one row per window.  The host writer takes the tables through pg_fst_dev, which never holds more
// than a slab of the window table on the device; the gpu writer needs the whole table there.
static int popgen_fst(const Args &a, Ctx &gpu, const GenotypesAndPhenotypes &g, const std::vector<double> &pool_sizes, const PopgenPlan &pl, Lap &lap) {
    const double *G_dev = g.intercept_and_allele_frequencies.get(), *cov_dev = g.coverages.get();
    const int n = g.n;
    const int64_t nw = pl.nw();
    const std::string win = std::to_string(a.window_size_bp), time = unix_time_string();
    std::string out = a.output, out_win;
    if (out.empty()) { // fst.rs:93-131
        out = basename_no_ext(a.fname) + "-fst-averaged_across_genome-" + time + ".csv";
        out_win = basename_no_ext(a.fname) + "-fst-" + win + "_bp_windows-" + time + ".csv";
    } else
        out_win = basename_no_ext(out) + "-fst-" + win + "_bp_windows.csv";
    const size_t nn = (size_t)n * n;
    // both files' header lines and their rows' labels, each label with its separator
    std::string head_mean, head_win = "chr,pos_ini,pos_fin";
    std::vector<std::string> pool_labels, win_labels;
    for (int i = 0; i < n; ++i) { head_mean += "," + g.pool_names[i]; pool_labels.push_back(g.pool_names[i] + ","); }
    for (int j = 0; j < n; ++j)
        for (int k2 = 0; k2 < n; ++k2) head_win += "," + g.pool_names[j] + "_vs_" + g.pool_names[k2];
    for (int64_t w = 0; w < nw; ++w) win_labels.push_back(window_label(pl, w, ',') + ",");
    head_mean += "\n"; head_win += "\n";
    if (a.popgen_writer == "gpu") {
        probe_output(out);
        DeviceBuf<double> mean_dev(sizeof(double) * nn, "fst: the means"), fw_dev(sizeof(double) * std::max<size_t>(1, (size_t)std::max<int64_t>(nw, 0) * nn), "fst: the windows' table");
        gpu.ok(pg_fst_tables_dev(gpu.c, G_dev, cov_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.wh.data(), pl.wt.data(), nw, mean_dev.get(), fw_dev.get()),
               "fst");
        lap("fst on the GPU");
        {
            DeviceResultWriter writer("popgen");
            write_new_file(out, [&](FILE *fo) {
                fputs(head_mean.c_str(), fo);
                table_rows_to_file(writer, gpu, a, fo, mean_dev.get(), n, n, n, 1, 8, 8, pool_labels);
            });
            if (nw <= 0) throw std::runtime_error(NO_WINDOWS); // fst.rs:180, after the genome-wide file has been written
            write_new_file(out_win, [&](FILE *fo) {
                fputs(head_win.c_str(), fo);
                table_rows_to_file(writer, gpu, a, fo, fw_dev.get(), nw, (int64_t)nn, (int64_t)nn, 1, -1, -1, win_labels);
            });
        }
        lap("format (gpu) + write CSV");
        std::cout << out << " and " << out_win << "\n"; // main.rs:441
        return done_ok();
    }
    std::vector<double> mean(nn), fw((size_t)nw * nn);
    gpu.ok(pg_fst_dev(gpu.c, G_dev, cov_dev, g.p, n, g.ld, pl.locus_col.data(), pl.L(), pl.wh.data(), pl.wt.data(), nw, mean.data(), fw.data()), "fst");
    lap("fst on the GPU");
    FILE *fo = create_new(out);
    fputs(head_mean.c_str(), fo);
    for (int i = 0; i < n; ++i) {
        std::string line = pool_labels[i];
        for (int j = 0; j < n; ++j) line += roundup_own(mean[(size_t)i * n + j], 8) + ",";
        line.back() = '\n'; // in place of the last separator
        fputs(line.c_str(), fo);
    }
    fclose(fo);
    if (nw <= 0) throw std::runtime_error(NO_WINDOWS); // fst.rs:180, after the genome-wide file has been written
    fo = create_new(out_win);
    fputs(head_win.c_str(), fo);
    write_rows_parallel(fo, nw, a.n_threads, [&](int64_t w, std::string &text) {
        text += win_labels[w];
        for (size_t q = 0; q < nn; ++q) text += rust_display(fw[(size_t)w * nn + q]) + ",";
        text.back() = '\n';
    });
    fclose(fo);
    lap("write CSV");
    std::cout << out << " and " << out_win << "\n"; // main.rs:441
    return done_ok();
}


int run_popgen(const Args &a, Analysis analysis, Ctx &gpu, const GenotypesAndPhenotypes &g, const std::vector<double> &pool_sizes, Lap &lap) {
    const bool reference_count = !a.popgen_as_documented && analysis != Analysis::fst && analysis != Analysis::heterozygosity;
    const PopgenPlan pl = plan_popgen(g.chromosome, g.position, a.window_size_bp, a.window_slide_size_bp, a.min_loci_per_window, reference_count,
                                      pg_host_sliding_windows, pg_host_watterson_windows);
    if (analysis == Analysis::gudmc) return popgen_gudmc(a, gpu, g, pool_sizes, pl, lap);
    if (analysis == Analysis::fst) return popgen_fst(a, gpu, g, pool_sizes, pl, lap);
    return popgen_diversity(a, gpu, g, pool_sizes, pl, lap, analysis);
}
