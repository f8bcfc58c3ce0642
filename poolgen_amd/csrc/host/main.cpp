// main.cpp -- `poolgen`, the command line over libpoolgen_hip.so: run() reads the flags (cli_args.h) and the phenotype file,
// answers pileup2sync on the host (or, with --pileup-parser gpu, with the GPU's parser) and vcf2sync with the GPU's parser (either
// with the GPU's writer under --sync-writer gpu), sets up the ranks and hands over to the analysis' translation unit -- the drivers that take
// the input in pieces (cli_streamed.cpp), or the loaded matrix (cli_matrix.cpp) and on it the popgen tools (cli_popgen.cpp), the
// cross-validation (gp_cv.h) or the kinship GWAS.  Parsing / formatting / ordering follow the reference (base/sync.rs:606-970,
// :972-1180; gwas/ols.rs:255-275, :372-433); anything else the reference CLI offers is out of scope and reported as such.
#include "cli.h"
#include "gp_cv.h"
#include "pileup_reader.h"
#include "sync_reader.h"
#include "vcf.h"
#include <cstring>

static int run(int argc, char **argv) {
    stamp("main");
    const Args a = parse_args(argc, argv);
    Lap lap;
    bool gwalpha_fmt = false;
    const Analysis analysis = checked_analysis(a, gwalpha_fmt);
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
    if (analysis == Analysis::pileup2sync) { // main.rs:212-225; text to text, no GPU involved unless --pileup-parser gpu asks for it
        std::string out = a.output;
        if (out.empty()) out = basename_no_ext(a.fname) + "-" + unix_time_string() + ".sync"; // pileup.rs:478-494
        int64_t kept;
        if (a.pileup_parser == "gpu") {
            probe_output(out); // before any work
            check_n_gpus(a, analysis);
            kept = pileup_to_sync_file_gpu(a.gpu_ids.empty() ? 0 : a.gpu_ids[0], a.fname, ph.pool_names, pf, out, a.n_threads, a.sync_writer == "gpu");
        } else
            kept = pileup_to_sync_file(a.fname, ph.pool_names, pf, out, a.n_threads);
        lap("pileup2sync");
        std::cerr << kept << " loci written\n";
        return done_ok(out);
    }
    if (analysis == Analysis::vcf2sync) { // main.rs:226-238; the text is parsed on the GPU (no GPU: an error, there is no host fallback)
        std::string out = a.output;
        if (out.empty()) out = basename_no_ext(a.fname) + "-" + unix_time_string() + ".sync"; // vcf.rs:317-337
        probe_output(out);                                                                    // :339, before any work
        check_n_gpus(a, analysis);
        const int64_t kept = vcf_to_sync_file(a.gpu_ids.empty() ? 0 : a.gpu_ids[0], a.fname, pf, out, a.n_threads, a.sync_writer == "gpu");
        lap("vcf2sync");
        std::cerr << kept << " loci written\n";
        return done_ok(out);
    }
    check_n_gpus(a, analysis);
    const RankSetup ranks = rank_setup(a, analysis == Analysis::ols_iter_with_kinship);
    Ctx gpu(ranks.devices[0]); // first: the pinned allocator below needs a HIP context
    lap("start-up");
    // A pileup input (*.pileup / *.mpileup) is converted in memory -- the counts pileup2sync would write and the
    // sync reader would read back, without the text in between (an extension: the reference needs the sync file).
    const InputKind kind = input_kind(a.fname); // a VCF input likewise: the counts vcf2sync would write, parsed on the GPU
    pg_filter flt{};
    flt.remove_ns = a.keep_ns ? 0 : 1;
    flt.min_coverage_depth = a.min_coverage_depth;
    flt.min_allele_frequency = a.min_allele_frequency;
    flt.max_missingness_rate = a.max_missingness_rate;
    if (analysis == Analysis::ols_iter_with_kinship) { // in pieces where the input is large or several GPUs take it
        const int rc = run_kinship_streamed(a, ph, gpu, lap, kind, pf, flt, ranks);
        if (rc >= 0) return rc;
    }
    if (per_locus(analysis)) return run_batch_streamed(a, ph, gpu, lap, analysis, kind, pf, flt, ranks);
    std::string csv_out; // sync2csv: the file is refused before any work is done (sync.rs:1191-1216)
    if (analysis == Analysis::sync2csv) {
        csv_out = a.output.empty() ? basename_no_ext(a.fname) + "-" + unix_time_string() + "-allele_frequencies.csv" : a.output;
        probe_output(csv_out);
    }
    if (analysis == Analysis::impute) { // GenotypesAndPhenotypes::write_csv's default name (sync.rs:1288-1299), probed as early
        csv_out = a.output.empty() ? "genotypes_and_phenotypes-" + unix_time_string() + "-allele_frequencies.csv" : a.output;
        probe_output(csv_out);
    }
    SyncBatch sb;
    if (kind == InputKind::pileup && a.pileup_parser == "gpu") {
        sb = parse_pileup_file_gpu(ranks.devices[0], a.fname, a.n_threads, pf, pinned);
        lap("pileup -> counts (gpu)");
    } else if (kind == InputKind::pileup) {
        sb = parse_pileup_file(a.fname, a.n_threads, pf, pinned);
        lap("pileup -> counts");
    } else if (kind == InputKind::vcf) {
        sb = parse_vcf_file(ranks.devices[0], a.fname, a.n_threads, pf, pinned);
        lap("vcf -> counts");
    } else if (a.sync_parser == "gpu") { // the text parsed on the GPU, the counts copied back: the batch below, 32-bit
        sb = parse_sync_file_gpu(ranks.devices[0], a.fname, a.n_threads, pinned);
        lap("parse sync (gpu)");
    } else {
        // the analyses on the loaded matrix copy the counts themselves: 16-bit counts when they fit
        sb = parse_sync_file(a.fname, a.n_threads, pinned, /*compact16=*/true);
        lap("parse sync");
    }
    if (sb.size() == 0) throw std::runtime_error("no loci in " + a.fname);
    if (sb.n != ph.n) throw std::runtime_error("the number of pools in the sync file and in the phenotype file differ");
    if (analysis == Analysis::sync2csv) // sync2csv (main.rs:357-366): every pool, whatever its phenotype
        return done_ok(sync2csv(gpu, sb, ph, flt, a.keep_p_minus_1, csv_out, a.csv_slab_rows, lap));
    if (analysis == Analysis::impute) // impute (main.rs:367-396): every pool, all alleles, coverages
        return done_ok(impute(gpu, sb, ph, flt, a, csv_out, lap));
    const int k = ph.k;
    const bool popgen = pgh::popgen(analysis);

    // ---------------- the analyses on the loaded matrix (main.rs:280-298, :397-455) ---------------------------
    const bool kpm1 = popgen && analysis != Analysis::fst ? false : a.keep_p_minus_1; // "we need all alleles in each locus" (main.rs:445, :460, :475)
    GenotypesAndPhenotypes genotypes_and_phenotypes =
        into_genotypes_and_phenotypes(gpu, sb, ph, flt, kpm1, /*remove_missing=*/!popgen, /*with_coverages=*/popgen, lap);
    GenotypesAndPhenotypes &g = genotypes_and_phenotypes;
    if (popgen) // fst / heterozygosity / watterson_estimator / tajima_d / gudmc use every pool (main.rs:427-502)
        return run_popgen(a, analysis, gpu, g, a.popgen_as_documented ? ph.pool_sizes_as_written : ph.pool_sizes, lap);
    if (analysis == Analysis::genomic_prediction_cross_validation) { // genomic_prediction_cross_validation (main.rs:397-426)
        CvLabels labels{g.chromosome, g.allele, g.position};
        CvArgs ca;
        ca.k_folds = a.k_folds; ca.n_reps = a.n_reps; ca.seed = a.seed; ca.n_threads = a.n_threads;
        ca.fname_input = a.fname; ca.fname_output = a.output;
        const std::string out = gp_cross_validate(gpu.c, g.intercept_and_allele_frequencies.get(), g.p, g.n, g.ld, g.phenotypes, k, g.pool_names,
                                                  labels, ca);
        lap("cross-validation");
        return done_ok(out);
    }
    const std::string out = ols_with_covariate(gpu, g, a.xxt, a.fname, a.output, a.n_threads, lap, /*mle=*/analysis == Analysis::mle_iter_with_kinship,
                                               a.result_writer == "gpu", a.result_slab_rows);
    return done_ok(out);
}

int main(int argc, char **argv) {
    try {
        return run(argc, argv);
    } catch (const std::exception &e) {
        std::cerr << "poolgen: " << e.what() << "\n";
        return 1;
    }
}
