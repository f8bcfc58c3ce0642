// cli_args.cpp -- the flags of `poolgen`, compatible with the reference CLI's (src/main.rs:26-143): parser, usage, checks.  No HIP.
#include "cli_args.h"
#include "host_util.h"
#include <algorithm>
#include <climits>
#include <iostream>
#include <sstream>
#include <stdexcept>

using namespace pgh;

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

// the names of the analyses that `pick` takes, as the messages list them: "a, b, c", or "a, b and c" with last = " and "
static std::string analysis_names(bool (*pick)(Analysis), const char *last = ", ") {
    std::vector<std::string> names;
    for (const AnalysisName &x : ANALYSES) if (pick(x.id)) names.push_back(x.name);
    std::string text;
    for (size_t i = 0; i < names.size(); ++i) text += (i == 0 ? "" : i + 1 == names.size() ? last : ", ") + names[i];
    return text;
}
static bool takes_n_gpus(Analysis a) { return per_locus(a) || a == Analysis::ols_iter_with_kinship; }

// (the help text also names analyses in prose, here and at the --window-*, --popgen-as-documented and --n-gpus flags)
static const char *USAGE =
    "poolgen <analysis> -f <input> -p <phenotypes.csv> [flags]      (MI355X build of the per-locus regression path)\n"
    "analyses: pileup2sync, vcf2sync, fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship,\n"
    "          mle_iter_with_kinship, genomic_prediction_cross_validation, fst, heterozygosity, watterson_estimator, tajima_d,\n"
    "          gudmc, sync2csv, impute\n"
    "  -f, --fname <file>                 *.sync, or *.pileup / *.mpileup / *.vcf (converted in memory: exactly what pileup2sync or vcf2sync\n"
    "                                     followed by the analysis on its sync file gives -- including the reference's column quirk: both\n"
    "                                     write A:T:C:G:DEL:N, the sync reader labels the columns A,T,C,G,N,DEL, so on such counts the\n"
    "                                     default N removal drops the DELETION column and --keep-ns keeps it).  A VCF is parsed on the\n"
    "                                     GPU (the AD field of every sample; vcf2sync needs a GPU too) and taken by one GPU\n"
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
    "      --imputation-method <aLD-kNNi|mean>   impute: adaptive LD-kNN imputation over the --window-* windows, or the mean of the pools\n"
    "      --min-depth-set-to-missing <5>  --frac-top-missing-pools <0.1>  --frac-top-missing-loci <0.1>   impute: the depth below which\n"
    "                                      a pool is missing at a locus, and the shares of the pools / loci with missing data dropped\n"
    "      --n-loci-to-estimate-distance <10>  --k-neighbours <5>   impute, aLD-kNNi: linked columns per column, neighbours per pool\n"
    "      --csv-slab-rows <N>             sync2csv, impute: rows of the table formatted on the GPU, copied and written per turn; default: as\n"
    "                                      many as hold 256 MB of text at their longest.  The file does not depend on it\n"
    "      --n-threads <1>                 parser / writer threads\n"
    "      --sync-parser <host|gpu>        who parses a *.sync input: the host's --n-threads threads (the default), or the GPU that analyses\n"
    "                                      it (the text goes over the link, the counts stay on the device).  The output is the same\n"
    "      --pileup-parser <host|gpu>      who parses a *.pileup / *.mpileup input, pileup2sync's included: the host's --n-threads threads (the\n"
    "                                      default), or the GPU (the text goes over the link, the counts come back).  The output is the same\n"
    "      --sync-writer <host|gpu>        pileup2sync (with --pileup-parser gpu), vcf2sync: who formats the sync lines: the host's --n-threads\n"
    "                                      threads (the default), or the GPU that parsed the input (the counts then never leave the device,\n"
    "                                      only the text comes back).  The output is the same\n"
    "      --result-writer <host|gpu>      fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship,\n"
    "                                      mle_iter_with_kinship: who formats the rows of the result CSV: the host's --n-threads threads (the\n"
    "                                      default), or the GPU that computed them (the statistics then never leave the device, only the\n"
    "                                      text comes back).  The GPU prints a number as the reference does (the shortest digits that read\n"
    "                                      back as the same double); the file is the host writer's byte for byte whenever every printed\n"
    "                                      |value| is below 2^53, and above that it is the one of the two that matches the reference.  The\n"
    "                                      kinship analyses take it on one GPU, in the whole-file path and in the streamed one (the\n"
    "                                      coefficients then stay on the device, 16 bytes each per trait, until the last piece)\n"
    "      --result-slab-rows <N>          --result-writer gpu, kinship analyses: rows formatted, copied and written per turn; default: as\n"
    "                                      many as hold 256 MB of text at 128 bytes a row.  The file does not depend on it (the per-locus\n"
    "                                      analyses format the rows of one piece of the input per turn: --stream-chunk-mb)\n"
    "      --popgen-writer <host|gpu>      fst, heterozygosity, watterson_estimator, tajima_d, gudmc: who formats the tables and gudmc's rows:\n"
    "                                      the host (the default), or the GPU that computed them (the tables then never leave the device --\n"
    "                                      gudmc's D and Fst go straight into its fits -- and only the text comes back).  Numbers print as with\n"
    "                                      --result-writer gpu; the file is the host writer's byte for byte below 2^53\n"
    "      --popgen-slab-rows <N>          --popgen-writer gpu: rows formatted, copied and written per turn; default: as many as hold 256 MB of\n"
    "                                      text.  The file does not depend on it\n"
    "      --stream-chunk-mb <N>           size of the pieces the input is taken in (0: whole file, kinship path only)\n"
    "      --n-gpus <N>  [--gpu-ids a,b,..]  fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship: one contiguous\n"
    "                                      part of the input per GPU (own parser threads: --n-threads is the total); the kinship sums are\n"
    "                                      all-reduced over the GPUs with RCCL; the kinship path then needs an input sorted by\n"
    "                                      (chromosome, position)\n"
    "environment: PGH_TIMING=1 prints the phases' wall-clock on stderr\n";

Args parse_args(int argc, char **argv) {
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
        else if (k == "--csv-slab-rows") a.csv_slab_rows = flag_int(val(), k, 1);
        else if (k == "--imputation-method") a.imputation_method = val();
        else if (k == "--sync-parser") a.sync_parser = val();
        else if (k == "--pileup-parser") a.pileup_parser = val();
        else if (k == "--sync-writer") a.sync_writer = val();
        else if (k == "--result-writer") a.result_writer = val();
        else if (k == "--result-slab-rows") a.result_slab_rows = flag_int(val(), k, 1);
        else if (k == "--popgen-writer") a.popgen_writer = val();
        else if (k == "--popgen-slab-rows") a.popgen_slab_rows = flag_int(val(), k, 1);
        else if (k == "--min-depth-set-to-missing") {
            const std::string t = val();
            if (!parse_f64_strict(t, a.min_depth_set_to_missing)) throw std::runtime_error("`" + t + "` isn't a valid number (" + k + ")");
        } else if (k == "--frac-top-missing-pools") a.frac_top_missing_pools = parse_valid_freq(val(), k);
        else if (k == "--frac-top-missing-loci") a.frac_top_missing_loci = parse_valid_freq(val(), k);
        else if (k == "--n-loci-to-estimate-distance") a.n_loci_to_estimate_distance = flag_u64(val(), k);
        else if (k == "--k-neighbours") a.k_neighbours = flag_u64(val(), k);
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

PileupFilter pileup_filter(const Args &a, const std::vector<double> &pool_sizes) {
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

Analysis checked_analysis(const Args &a, bool &gwalpha_fmt) {
    const AnalysisName *found = std::find_if(std::begin(ANALYSES), std::end(ANALYSES), [&](const AnalysisName &x) { return a.analysis == x.name; });
    if (found == std::end(ANALYSES))
        throw std::runtime_error("Invalid analysis utility for this build: `" + a.analysis + "` (available: " + analysis_names([](Analysis) { return true; }) + ")");
    const Analysis analysis = found->id;
    if (a.popgen_as_documented && analysis != Analysis::watterson_estimator && analysis != Analysis::tajima_d && analysis != Analysis::gudmc)
        throw std::runtime_error("--popgen-as-documented applies to watterson_estimator, tajima_d and gudmc");
    if (a.generate_plots || a.sig_only)
        throw std::runtime_error("--generate-plots / --output-sig-snps-only call the reference's python scripts and are out of scope here");
    if (a.phen_format != "default" && a.phen_format != "gwalpha_fmt")
        throw std::runtime_error("Invalid phenotype format. Please select: 'default' or 'gwalpha_fmt'"); // phen.rs:161-164
    if (analysis == Analysis::impute) {
        if (a.imputation_method != "mean" && a.imputation_method != "aLD-kNNi")
            throw std::runtime_error("Invalid imputation method `" + a.imputation_method + "`. Please select: 'mean' or 'aLD-kNNi'");
        if (a.n_loci_to_estimate_distance < 1 || a.k_neighbours < 1)
            throw std::runtime_error("--n-loci-to-estimate-distance and --k-neighbours must be at least 1");
    }
    if (a.sync_parser != "host" && a.sync_parser != "gpu")
        throw std::runtime_error("Invalid value `" + a.sync_parser + "` for --sync-parser. Please select: 'host' or 'gpu'");
    if (a.sync_parser == "gpu" && input_kind(a.fname) != InputKind::sync)
        throw std::runtime_error("--sync-parser gpu applies to a *.sync input; `" + a.fname + "` is converted by its own reader");
    if (a.pileup_parser != "host" && a.pileup_parser != "gpu")
        throw std::runtime_error("Invalid value `" + a.pileup_parser + "` for --pileup-parser. Please select: 'host' or 'gpu'");
    if (a.pileup_parser == "gpu" && input_kind(a.fname) != InputKind::pileup)
        throw std::runtime_error("--pileup-parser gpu applies to a *.pileup / *.mpileup input; `" + a.fname + "` is read by its own reader");
    if (a.sync_writer != "host" && a.sync_writer != "gpu")
        throw std::runtime_error("Invalid value `" + a.sync_writer + "` for --sync-writer. Please select: 'host' or 'gpu'");
    if (a.sync_writer == "gpu" && analysis != Analysis::pileup2sync && analysis != Analysis::vcf2sync)
        throw std::runtime_error("--sync-writer gpu applies to pileup2sync and vcf2sync, which write a sync file; `" + a.analysis + "` writes none");
    if (a.sync_writer == "gpu" && analysis == Analysis::pileup2sync && a.pileup_parser != "gpu")
        throw std::runtime_error("--sync-writer gpu on pileup2sync needs --pileup-parser gpu: with the host's parser the rows are not on the device");
    if (a.result_writer != "host" && a.result_writer != "gpu")
        throw std::runtime_error("Invalid value `" + a.result_writer + "` for --result-writer. Please select: 'host' or 'gpu'");
    const bool kinship_rows = analysis == Analysis::ols_iter_with_kinship || analysis == Analysis::mle_iter_with_kinship;
    const bool locus_rows = analysis == Analysis::fisher_exact_test || analysis == Analysis::chisq_test || analysis == Analysis::pearson_corr ||
                            analysis == Analysis::ols_iter || analysis == Analysis::gwalpha;
    if ((a.result_writer == "gpu" || a.result_slab_rows > 0) && !kinship_rows && !locus_rows)
        throw std::runtime_error("--result-writer gpu applies to fisher_exact_test, chisq_test, pearson_corr, ols_iter, gwalpha, ols_iter_with_kinship and "
                                 "mle_iter_with_kinship, which write result rows; `" + a.analysis + "` writes none");
    if (a.result_slab_rows > 0 && a.result_writer != "gpu")
        throw std::runtime_error("--result-slab-rows needs --result-writer gpu: the host writer has no slabs");
    if (a.result_writer == "gpu" && kinship_rows && a.n_gpus > 1)
        throw std::runtime_error("--result-writer gpu on `" + a.analysis + "` takes one GPU: with --n-gpus " + std::to_string(a.n_gpus) +
                                 " the rows of one trait would interleave the ranks' coefficients; run it without --n-gpus, or with --result-writer host");
    const bool popgen_tables = analysis == Analysis::fst || analysis == Analysis::heterozygosity || analysis == Analysis::watterson_estimator ||
                               analysis == Analysis::tajima_d || analysis == Analysis::gudmc;
    if (a.popgen_writer != "host" && a.popgen_writer != "gpu")
        throw std::runtime_error("Invalid value `" + a.popgen_writer + "` for --popgen-writer (fst, heterozygosity, watterson_estimator, tajima_d and gudmc "
                                 "take it). Please select: 'host' or 'gpu'");
    if ((a.popgen_writer == "gpu" || a.popgen_slab_rows > 0) && !popgen_tables)
        throw std::runtime_error("--popgen-writer gpu applies to fst, heterozygosity, watterson_estimator, tajima_d and gudmc, which write popgen tables; `" +
                                 a.analysis + "` writes none");
    if (a.popgen_slab_rows > 0 && a.popgen_writer != "gpu")
        throw std::runtime_error("--popgen-slab-rows needs --popgen-writer gpu: the host writer has no slabs");
    gwalpha_fmt = a.phen_format == "gwalpha_fmt";
    if (analysis == Analysis::gwalpha && !gwalpha_fmt)
        throw std::runtime_error("gwalpha needs the GWAlpha.py phenotype file: give it with --phen-format gwalpha_fmt "
                                 "(Pheno_name=, sig=, MIN=, MAX=, perc=[..], q=[..])");
    if (gwalpha_fmt && analysis != Analysis::gwalpha && analysis != Analysis::pileup2sync)
        throw std::runtime_error("--phen-format gwalpha_fmt is read by gwalpha and pileup2sync; `" + a.analysis + "` needs the default phenotype file");
    return analysis;
}

void check_n_gpus(const Args &a, Analysis analysis) {
    if (a.n_gpus > 1 && input_kind(a.fname) == InputKind::vcf) // its pieces are parsed on the device that analyses them; sharing them out is left for later
        throw std::runtime_error("--n-gpus " + std::to_string(a.n_gpus) + ": a VCF input is taken by one GPU; convert it with vcf2sync first to use several");
    if (analysis == Analysis::sync2csv || analysis == Analysis::impute) { // one table in (chromosome, position) order: the sort is global
        if (a.n_gpus > 1) throw std::runtime_error("--n-gpus " + std::to_string(a.n_gpus) + ": `" + a.analysis + "` sorts the whole table and runs on one GPU");
        return;
    }
    if (a.n_gpus > 0 && !takes_n_gpus(analysis))
        throw std::runtime_error("--n-gpus applies to " + analysis_names(takes_n_gpus, " and ") + "; `" + a.analysis + "` runs on one GPU");
}
