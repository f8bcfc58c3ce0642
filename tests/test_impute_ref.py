"""The restatement of the reference's imputation (tests/impute_ref.py) reproduces the literal answers of the reference's
own three tests on the golden fixture, and the library's host keep rule agrees with it.  No GPU."""
import json
from pathlib import Path

import numpy as np
import pytest

import impute_ref as R

ROOT = Path(__file__).resolve().parent.parent
LIT = json.loads((ROOT / "tests" / "golden" / "imputation_literals.json").read_text())


def cell(G, c):
    """the reference's [pool, column incl. intercept] in the p x n restatement"""
    return G[c[1] - 1, c[0]]


def load(oracle, f):
    return R.load_fixture(oracle, f["remove_ns"], f["min_coverage_depth"], f["min_allele_frequency"], f["max_missingness_rate"])


def test_filtering_missing_literals(oracle):
    lit = LIT["filtering_missing"]
    fx = load(oracle, lit["filter"])
    G, cov = R.set_missing_by_depth(fx["G"], fx["cov"], fx["locus_col"], lit["min_depth_set_to_missing"])
    for c in lit["nan_cells"]:
        assert np.isnan(cell(G, c)), c
    for v in lit["value_cells"]:
        assert cell(G, v["cell"]) == v["num"] / v["den"], v
    G, cov, pools = R.filter_out_top_missing_pools(G, cov, lit["frac_top_missing_pools"])
    assert G.shape[1] == lit["pools_left"] == len(pools)
    G, cov, lc, loci = R.filter_out_top_missing_loci(G, cov, fx["locus_col"], lit["frac_top_missing_loci"])
    assert G.shape[0] + 1 == lit["columns_left_with_intercept"]
    assert lc[-1] == G.shape[0] and len(loci) == cov.shape[0]


def test_last_locus_keeps_its_frequencies(oracle):
    """idx_fin = loci_idx[l - 1] (filtering_missing.rs:30-34): an empty range for the last locus"""
    G = np.array([[0.5, 0.5], [0.5, 0.5], [0.25, 0.75], [0.75, 0.25]])
    cov = np.array([[1.0, 9.0], [2.0, 9.0]])
    G2, cov2 = R.set_missing_by_depth(G, cov, [0, 2, 4], 5.0)
    assert np.isnan(G2[:2, 0]).all() and (G2[2:] == G[2:]).all() and np.isnan(cov2[:, 0]).all() and (cov2[:, 1] == 9.0).all()


def test_mean_imputation_literals(oracle):
    lit = LIT["mean_imputation"]
    fx = load(oracle, lit["filter"])
    G, cov = R.set_missing_by_depth(fx["G"], fx["cov"], fx["locus_col"], lit["min_depth_set_to_missing"])
    G = R.mean_imputation(oracle, G, fx["locus_col"])
    for grp in lit["cells"]:
        want = R.ndsum(oracle, grp["mean_of"]) / float(len(grp["mean_of"]))     # Array1::mean = sum() / len
        for c in grp["cells"]:
            assert cell(G, c) == want, (c, cell(G, c), want)


def test_adaptive_ld_knn_literals(oracle):
    lit = LIT["adaptive_ld_knn_imputation"]
    fx = load(oracle, lit["filter"])
    G, cov = R.set_missing_by_depth(fx["G"], fx["cov"], fx["locus_col"], lit["min_depth_set_to_missing"])
    head, tail = oracle.sliding_windows(fx["chrom"], fx["pos"], lit["window_size_bp"], lit["window_slide_size_bp"],
                                        lit["min_loci_per_window"])
    out = R.adaptive_ld_knn_imputation(oracle, G, fx["locus_col"], head.tolist(), tail.tolist(),
                                       lit["n_loci_to_estimate_distance"], lit["k_neighbours"])
    assert np.isnan(G).sum() > 1000 and np.isnan(out).sum() < np.isnan(G).sum()
    for a, b in lit["column_ranges_whose_pool_sums_round_to_one"]:
        for i in range(5):
            s = R.ndsum(oracle, out[a - 1:b - 1, i])                               # sum_axis over a lane of 2 or 3
            assert oracle.lib.orc_sensible_round(s, lit["round_digits"]) == 1.0, (a, b, i, s)


@pytest.mark.parametrize("frac", [0.0, 0.1, 0.5, 1.0])
def test_host_keep_rule_matches_the_restatement(native, frac):
    rng = np.random.default_rng(int(frac * 10) + 3)
    for trial in range(60):
        N = int(rng.integers(1, 80))
        denom = int(rng.integers(1, 7))
        counts = rng.integers(0, denom + 1, size=N).astype(np.int64)               # few distinct values: many ties
        if trial % 5 == 0:
            counts[:] = 0
        keep = np.empty(N, dtype=np.int64)
        got = native.pg_host_top_missing_keep(counts.ctypes.data, N, float(frac), keep.ctypes.data)
        try:
            want = R.top_missing_keep([float(c) / float(denom) for c in counts], frac)
        except R.NothingLeft:
            assert got == 0
            continue
        assert got == len(want) and keep[:got].tolist() == want
    assert native.pg_host_top_missing_keep(None, 0, 0.5, None) < 0
