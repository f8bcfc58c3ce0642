// cli_args.h -- the flags of `poolgen` and the checks that need nothing but the flags (cli_args.cpp; no HIP in either).
#pragma once
#include "operators.h"
#include "pileup.h"
#include <cstdint>
#include <string>
#include <vector>

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
    int64_t csv_slab_rows = 0; // sync2csv, impute: rows formatted per call (0 = as many as CSV_SLAB_BYTES of text hold)
    // impute (main.rs:125-142)
    std::string pileup_parser = "host"; // who parses a *.pileup / *.mpileup input: the host's threads, or the GPU (the counts come back)
    std::string result_writer = "host"; // who formats the result rows of the GWAS analyses: the host's threads, or the GPU that computed them
    int64_t result_slab_rows = 0;       // --result-writer gpu, kinship analyses: rows formatted, copied and written per turn (0 = a byte budget's worth)
    std::string popgen_writer = "host"; // who formats the tables of fst and the diversity analyses and gudmc's rows: the host, or the GPU that computed them
    int64_t popgen_slab_rows = 0;       // --popgen-writer gpu: rows formatted, copied and written per turn (0 = a byte budget's worth)
    std::string sync_writer = "host"; // who formats the sync lines pileup2sync / vcf2sync write: the host's threads, or the GPU that parsed the input
    std::string sync_parser = "host"; // who parses a *.sync input: the host's threads, or the GPU (the counts then stay on the device)
    std::string imputation_method = "aLD-kNNi";
    double min_depth_set_to_missing = 5.0, frac_top_missing_pools = 0.1, frac_top_missing_loci = 0.1;
    uint64_t n_loci_to_estimate_distance = 10, k_neighbours = 5;
};

constexpr int64_t CSV_SLAB_BYTES = 256ll << 20; // sync2csv: the text budget of one slab of rows (device buffer + pinned copy)

Args parse_args(int argc, char **argv); // --help prints the usage and ends the process
pgh::Analysis checked_analysis(const Args &a, bool &gwalpha_fmt); // the analysis `a` names, once its flags agree with one another
void check_n_gpus(const Args &a, pgh::Analysis analysis); // --n-gpus on an analysis that runs on one GPU is refused
pgh::PileupFilter pileup_filter(const Args &a, const std::vector<double> &pool_sizes);
