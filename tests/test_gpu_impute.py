"""Imputation on the GPU (pg_impute.hip through the Engine) against the literal restatement tests/impute_ref.py: every stage
and the composed call, bit for bit (NaN = NaN); then the reference's own literals through the Engine on the full fixture.

Shapes are the smallest at which the kernels can go wrong: n in {3, 5, 9, 17, 65} (the smallest count with n - 2 > 0; the
8-lane sum with 8, 9, 16, 17 shared pools; more pools than a wave), K in {1, 7, 8, 9, 10} against windows narrower than, as
wide as and wider than K, k_neighbours in {1, 3, n}, and the special cases each test names."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import csv_expect as E
import impute_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LIT = json.loads((ROOT / "tests" / "golden" / "imputation_literals.json").read_text())
NAN = float("nan")


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def to_dev(M, n):
    """p x n host array -> p x ld device tensor (ld even, padding zero)"""
    ld = n + (n & 1)
    out = np.zeros((M.shape[0], ld))
    out[:, :n] = M
    return torch.from_numpy(out).cuda()


def cov_rows(cov, locus_col):
    """L x n coverages -> one row per column, as the loader lays them out"""
    reps = np.diff(np.asarray(locus_col))
    return np.repeat(cov, reps, axis=0)


def host(T, n):
    return T.cpu().numpy()[:, :n]


def make_case(seed, n, alleles, nan_locus=0.25, nan_cell=0.03, empty_rows=(), empty_pools=(), twin_pools=None, step=40):
    """alleles: columns per locus.  Frequencies are counts over depths (a locus sums to one in a pool); a (locus, pool) is
    missing as set_missing_by_depth leaves it (every allele), a few single cells on top.  Returns G p x n, locus_col, chrom, pos."""
    rng = np.random.default_rng(seed)
    rows, lc = [], [0]
    for a in alleles:
        c = rng.integers(0, 30, size=(a, n)).astype(np.float64) + (rng.random((a, n)) < 0.7)
        c[0] += 1.0
        f = c / c.sum(axis=0)
        f[:, rng.random(n) < nan_locus] = NAN
        rows.append(f)
        lc.append(lc[-1] + a)
    G = np.concatenate(rows)
    G[rng.random(G.shape) < nan_cell] = NAN
    for r in empty_rows:
        G[r] = NAN
    for (r0, r1, i) in empty_pools:
        G[r0:r1, i] = NAN
    if twin_pools is not None:
        a, b = twin_pools
        G[:, b] = G[:, a]
    L = len(alleles)
    chrom = [0] * L
    pos = (np.arange(L) * step + 1).tolist()
    return G, lc, chrom, pos


# ---- the elementwise and reduction stages, the keep rule, the compaction, the mean pass ---------------------------------
@pytest.mark.parametrize("n", [3, 5, 9, 17, 65])
def test_stages_match_the_restatement(engine, oracle, n):
    rng = np.random.default_rng(n)
    alleles = [int(a) for a in rng.choice([1, 2, 2, 2, 3, 4], size=300)] + [3]      # more than one block of loci; tri-allelic last
    G, lc, _, _ = make_case(100 + n, n, alleles, nan_locus=0.0, nan_cell=0.0)
    L = len(alleles)
    cov = rng.integers(0, 12, size=(L, n)).astype(np.float64)
    cov[rng.random(cov.shape) < 0.05] = NAN                                          # an uncovered pool the loader let through
    cov[5] = 2.0                                                                      # a locus below the depth in every pool
    G[lc[7]:lc[8]] = NAN; cov[7] = NAN                                               # ... and one that arrives missing
    cov[L - 1, 0] = 1.0                                                               # the last-locus quirk
    Gd, cd = to_dev(G, n), to_dev(cov_rows(cov, lc), n)
    # set_missing_by_depth
    engine.set_missing_by_depth(Gd, cd, lc, 5.0, n=n)
    G1, cov1 = R.set_missing_by_depth(G, cov, lc, 5.0)
    assert same(host(Gd, n), G1) and same(host(cd, n), cov_rows(cov1, lc))
    assert np.isnan(cov1[L - 1, 0]) and not np.isnan(G1[lc[L - 1]:, 0]).any()        # coverage gone, frequencies kept
    assert (Gd.cpu().numpy()[:, n:] == 0).all()
    # NaN counts and the keep rule
    pool_nan, locus_nan = engine.missingness(Gd, cd, lc, n=n)
    assert pool_nan.tolist() == np.isnan(G1).sum(axis=0).tolist() and locus_nan.tolist() == np.isnan(cov1).sum(axis=1).tolist()
    from poolgen_amd import NativeError
    for frac in (0.0, 0.2, 0.5, 1.0):
        try:
            pools = R.top_missing_keep((pool_nan / float(G.shape[0])).tolist(), frac)
        except R.NothingLeft:
            with pytest.raises(NativeError, match="No pools left"):
                engine.top_missing_keep(pool_nan, frac, "pools")
            continue
        assert engine.top_missing_keep(pool_nan, frac, "pools").tolist() == pools
    G2, cov2, pools = R.filter_out_top_missing_pools(G1, cov1, 0.2)
    Gd2, cd2, lc2, _, _ = engine.impute_compact(Gd, cd, lc, pools, np.arange(L), n=n)
    n2 = len(pools)
    assert same(host(Gd2, n2), G2) and same(host(cd2, n2), cov_rows(cov2, lc)) and lc2.tolist() == lc
    assert (Gd2.cpu().numpy()[:, n2:] == 0).all()
    G3, cov3, lc3, loci = R.filter_out_top_missing_loci(G2, cov2, lc, 0.3)
    locus_nan2 = engine.missingness(Gd2, cd2, lc2, n=n2)[1]
    keep_loci = engine.top_missing_keep(locus_nan2, 0.3, "loci")
    assert keep_loci.tolist() == loci
    labels = torch.arange(G.shape[0], dtype=torch.int64).cuda()
    alle = (torch.arange(G.shape[0], dtype=torch.int32) % 6).cuda()
    Gd3, cd3, lcd3, cl3, ca3 = engine.impute_compact(Gd2, cd2, lc2, np.arange(n2), keep_loci, labels, alle, n=n2)
    assert same(host(Gd3, n2), G3) and same(host(cd3, n2), cov_rows(cov3, lc3)) and lcd3.tolist() == lc3
    rows = [c for l in loci for c in range(lc[l], lc[l + 1])]
    assert cl3.cpu().tolist() == rows and ca3.cpu().tolist() == [r % 6 for r in rows]
    # mean imputation and the coverage mark: before the locus filter (loci missing in every pool stay NaN) and after it
    for Gx, cx, lcx, Gr, cr in ((Gd2.clone(), cd2.clone(), lc, G2, cov2), (Gd3, cd3, lc3, G3, cov3)):
        engine.impute_mean(Gx, lcx, n=n2)
        G4 = R.mean_imputation(oracle, Gr, lcx)
        assert same(host(Gx, n2), G4) and np.isnan(G4).sum() < np.isnan(Gr).sum()
        engine.impute_mark_cov(cx, lcx, n=n2)
        cov4 = R.mark_coverages(cr)
        assert same(host(cx, n2), cov_rows(cov4, lcx)) and np.isinf(cov4).any()
        if Gr is G2:
            assert np.isnan(G4[lc[7]:lc[8]]).all() and np.isnan(cov4[5]).all() and np.isnan(cov4[7]).all()


def test_mean_imputation_sums_and_wide_loci(engine, oracle):
    """loci of 8, 9, 16 and 17 allele columns put ndarray's 8-lane order into the sum of the means; those of 33 and 40 are wider
    than a tile of the mean pass and take its wave-per-locus kernel, between loci that are tiled"""
    n = 9
    G, lc, _, _ = make_case(7, n, [8, 9, 17, 40, 1, 2, 16, 33, 3], nan_locus=0.3, nan_cell=0.1)
    Gd = to_dev(G, n)
    engine.impute_mean(Gd, lc, n=n)
    assert same(host(Gd, n), R.mean_imputation(oracle, G, lc))


# ---- adaptive LD-kNN ----------------------------------------------------------------------------------------------------
def run_aldknn(engine, oracle, G, lc, chrom, pos, n, K, kn, wsize, wslide, wmin, scratch=0):
    head, tail = oracle.sliding_windows(chrom, pos, wsize, wslide, wmin)
    h2, t2 = engine.sliding_windows(chrom, pos, wsize, wslide, wmin)
    assert h2.tolist() == head.tolist() and t2.tolist() == tail.tolist()
    want = R.adaptive_ld_knn_imputation(oracle, G, lc, head.tolist(), tail.tolist(), K, kn)
    got = host(engine.impute_aldknn(to_dev(G, n), lc, head, tail, K, kn, scratch, n=n), n)
    return got, want, head, tail


ALDKNN = [  # n, K, k_neighbours, loci per window (positions step 40: window_size = 40 * that), seed
    (3, 1, 1, 3, 1), (3, 10, 3, 4, 2), (5, 7, 3, 3, 3), (5, 8, 5, 3, 4), (9, 9, 1, 4, 5), (9, 8, 9, 3, 6),
    (17, 10, 3, 5, 7), (17, 7, 17, 3, 8), (65, 9, 3, 3, 9), (65, 1, 65, 2, 10),
]


@pytest.mark.parametrize("n,K,kn,per,seed", ALDKNN)
def test_aldknn_matches_the_restatement(engine, oracle, n, K, kn, per, seed):
    """windows of `per` loci with 1 to 3 allele columns each: narrower than, as wide as and wider than K"""
    L = 4 * per if n == 65 else 8 * per
    rng = np.random.default_rng(seed)
    alleles = [int(a) for a in rng.choice([1, 2, 2, 3], size=L)]
    alleles[0] = 1                                                                   # a window that starts with a one-allele locus
    G, lc, chrom, pos = make_case(seed, n, alleles, nan_locus=0.3, nan_cell=0.05)
    G[0, 0] = NAN                                                                     # ... missing in its first column: j = 0 skips the renormalisation
    got, want, head, tail = run_aldknn(engine, oracle, G, lc, chrom, pos, n, K, kn, 40 * per, 40 * per, 1)
    assert len(head) >= 4
    widths = {lc[t + 1] - lc[h] for h, t in zip(head, tail)}
    if K in (7, 8, 9):
        assert min(widths) < K <= max(widths)
    assert same(got, want)
    assert np.isnan(G).sum() > np.isnan(want).sum()


def test_aldknn_sparse_corners(engine, oracle):
    """a column missing in every pool; a pool with no data in a whole window (its distances are all NaN, so k grows to n);
    two identical pools (dist_sum = EPS); tri-allelic loci throughout"""
    n = 9
    alleles = [3] * 12
    G, lc, chrom, pos = make_case(21, n, alleles, nan_locus=0.2, nan_cell=0.02, empty_rows=(4, 5, 20),
                                  empty_pools=((9, 18, 2),), twin_pools=(3, 6))
    G[13, 6] = 0.25                                                                   # the twins differ in one cell that pool 3 lacks
    G[13, 3] = NAN
    got, want, head, tail = run_aldknn(engine, oracle, G, lc, chrom, pos, n, 10, 3, 120, 120, 1)
    assert same(got, want)
    assert not np.isnan(want[9:18, 2]).all()


def test_aldknn_all_linked_columns_empty(engine, oracle):
    """K = 1 and a column that is missing in every pool: its NaN correlations sort first, the one linked column holds nothing,
    no distance exists (all_missing) and every pool gets the count of present values over n"""
    n = 5
    G, lc, chrom, pos = make_case(31, n, [2, 2, 2, 2, 2, 2], nan_locus=0.3, nan_cell=0.0, empty_rows=(0, 6))
    got, want, head, tail = run_aldknn(engine, oracle, G, lc, chrom, pos, n, 1, 3, 120, 120, 1)
    assert same(got, want)
    assert np.isnan(G[0]).all() and want[0, 0] == 0.0 and not np.isnan(want).any()  # 0 present values over n, then 1 / n ...


def test_aldknn_overlapping_windows_and_loci_in_no_window(engine, oracle):
    """slide < size: the last window that holds a column wins; min_loci_per_window > 1: loci in no window stay NaN"""
    n = 5
    rng = np.random.default_rng(5)
    alleles = [int(a) for a in rng.choice([1, 2, 3], size=30)]
    G, lc, chrom, pos = make_case(41, n, alleles, nan_locus=0.3, nan_cell=0.03)
    chrom = [0] * 18 + [1] * 12                                                       # runs of close loci, lone loci and a pair between them
    pos = [10 + 30 * i for i in range(14)] + [1000, 1500, 2000, 2030] + [5 + 30 * i for i in range(8)] + [500, 900, 930, 960]
    got, want, head, tail = run_aldknn(engine, oracle, G, lc, chrom, pos, n, 7, 3, 300, 100, 3)
    covered = np.zeros(30, dtype=bool)
    for h, t in zip(head, tail):
        covered[h:t + 1] = True
    assert len(head) >= 3 and (np.diff(head) >= 0).all() and (head[1:] <= tail[:-1]).any() and not covered.all()
    assert same(got, want)
    outside = [c for l in np.flatnonzero(~covered) for c in range(lc[l], lc[l + 1])]
    assert same(want[outside], G[outside]) and np.isnan(G[outside]).any()


def test_aldknn_window_batches_and_refusals(engine, oracle):
    """a scratch budget of one byte puts every window into a batch of its own: same result; k_neighbours > n is refused"""
    from poolgen_amd import NativeError
    n = 5
    G, lc, chrom, pos = make_case(51, n, [2] * 24, nan_locus=0.3, nan_cell=0.02)
    got, want, head, tail = run_aldknn(engine, oracle, G, lc, chrom, pos, n, 10, 3, 160, 80, 1, scratch=1)
    assert len(head) > 3 and same(got, want)
    assert same(host(engine.impute_aldknn(to_dev(G, n), lc, head, tail, 10, 3, n=n), n), want)
    with pytest.raises(NativeError, match="k_neighbours"):
        engine.impute_aldknn(to_dev(G, n), lc, head, tail, 10, n + 1, n=n)
    with pytest.raises(ValueError):
        R.adaptive_ld_knn_imputation(oracle, G, lc, head.tolist(), tail.tolist(), 10, n + 1)
    assert same(host(engine.impute_aldknn(to_dev(G, n), lc, [], [], 10, 3, n=n), n), G)   # no windows: a copy


# ---- the composed call on a slice of the fixture ------------------------------------------------------------------------
@pytest.mark.parametrize("method,win", [("mean", (100, 50, 10)), ("aLD-kNNi", (1000000, 1000000, 1)), ("aLD-kNNi", (3000000, 1000000, 2))])
def test_composed_call_matches_the_restatement(engine, oracle, method, win):
    fx = R.load_fixture(oracle, True, 1, 0.001, 0.0, max_loci=300)
    n = 5
    names = sorted(set(fx["chrom"]), key=fx["chrom"].index)
    chrom_ids = [names.index(c) for c in fx["chrom"]]
    trace = []
    want = R.impute(oracle, fx["G"], fx["cov"], fx["locus_col"], fx["chrom"], fx["pos"], method, 5.0, 0.2, 0.1, win[0], win[1], win[2],
                    10, 3, trace=trace)
    p = fx["G"].shape[0]
    cl = torch.from_numpy(np.repeat(np.arange(len(fx["pos"])), np.diff(fx["locus_col"]))).cuda()
    ca = torch.tensor(fx["alleles"], dtype=torch.int32).cuda()
    Gd, cd = to_dev(fx["G"], n), to_dev(cov_rows(fx["cov"], fx["locus_col"]), n)
    before = Gd.clone()
    got = engine.impute(Gd, cd, fx["locus_col"], chrom_ids, fx["pos"], method, 5.0, 0.2, 0.1, win[0], win[1], win[2], 10, 3,
                        col_locus=cl, col_allele=ca, n=n)
    assert torch.equal(before, Gd)
    n2 = len(want["pools"])
    assert got["pools"].tolist() == want["pools"] and got["loci"].tolist() == want["loci"] and n2 == 4
    assert got["locus_col"].tolist() == want["locus_col"]
    assert same(host(got["G"], n2), want["G"]) and same(host(got["cov"], n2), cov_rows(want["cov"], want["locus_col"]))
    assert got["col_locus"].cpu().tolist() == [l for l, a in zip(want["loci"], np.diff(want["locus_col"])) for _ in range(a)]
    assert got["missing_rate"] == [t[2] for t in trace]
    assert not np.isnan(want["G"]).all() and len(want["loci"]) < 300


# ---- the reference's literals through the Engine on the full fixture ----------------------------------------------------
def load_on_gpu(engine, oracle, f):
    from poolgen_amd import Filter
    counts, chrom_ids, pos, names, order = E.golden_fixture(oracle)
    dev = torch.from_numpy(np.stack(counts).astype(np.int32)).cuda()
    flt = Filter(f["remove_ns"], f["min_coverage_depth"], f["min_allele_frequency"], f["max_missingness_rate"])
    G, col_locus, col_allele, cov = engine.load_frequencies(dev, np.full(5, 20.0), flt, keep_p_minus_1=False, order=torch.from_numpy(order),
                                                            coverages=True)
    cl = col_locus.cpu().numpy()
    starts = np.flatnonzero(np.r_[True, cl[1:] != cl[:-1]])
    lc = np.r_[starts, len(cl)].astype(np.int64)
    loci = cl[starts]
    return G, cov, lc, chrom_ids[loci], pos[loci]


def cell(G, c):
    return float(G[c[1] - 1, c[0]])


def test_reference_literals_filtering_missing(engine, oracle):
    lit = LIT["filtering_missing"]
    G, cov, lc, _, _ = load_on_gpu(engine, oracle, lit["filter"])
    engine.set_missing_by_depth(G, cov, lc, lit["min_depth_set_to_missing"], n=5)
    for c in lit["nan_cells"]:
        assert np.isnan(cell(G, c))
    for v in lit["value_cells"]:
        assert cell(G, v["cell"]) == v["num"] / v["den"]
    pool_nan, _ = engine.missingness(G, cov, lc, n=5)
    pools = engine.top_missing_keep(pool_nan, lit["frac_top_missing_pools"], "pools")
    assert len(pools) == lit["pools_left"]
    G2, cov2, lc2, _, _ = engine.impute_compact(G, cov, lc, pools, np.arange(len(lc) - 1), n=5)
    locus_nan = engine.missingness(G2, cov2, lc2, n=len(pools))[1]
    loci = engine.top_missing_keep(locus_nan, lit["frac_top_missing_loci"], "loci")
    G3 = engine.impute_compact(G2, cov2, lc2, np.arange(len(pools)), loci, n=len(pools))[0]
    assert G3.shape[0] + 1 == lit["columns_left_with_intercept"]


def test_reference_literals_mean_imputation(engine, oracle):
    lit = LIT["mean_imputation"]
    G, cov, lc, _, _ = load_on_gpu(engine, oracle, lit["filter"])
    engine.set_missing_by_depth(G, cov, lc, lit["min_depth_set_to_missing"], n=5)
    engine.impute_mean(G, lc, n=5)
    for grp in lit["cells"]:
        want = R.ndsum(oracle, grp["mean_of"]) / float(len(grp["mean_of"]))
        for c in grp["cells"]:
            assert cell(G, c) == want


def test_reference_literals_adaptive_ld_knn(engine, oracle):
    lit = LIT["adaptive_ld_knn_imputation"]
    G, cov, lc, chrom_ids, pos = load_on_gpu(engine, oracle, lit["filter"])
    engine.set_missing_by_depth(G, cov, lc, lit["min_depth_set_to_missing"], n=5)
    head, tail = engine.sliding_windows(chrom_ids, pos, lit["window_size_bp"], lit["window_slide_size_bp"], lit["min_loci_per_window"])
    out = engine.impute_aldknn(G, lc, head, tail, lit["n_loci_to_estimate_distance"], lit["k_neighbours"], n=5).cpu().numpy()
    assert np.isnan(out).sum() < int(torch.isnan(G).sum())
    for a, b in lit["column_ranges_whose_pool_sums_round_to_one"]:
        for i in range(5):
            s = R.ndsum(oracle, out[a - 1:b - 1, i])
            assert oracle.lib.orc_sensible_round(s, lit["round_digits"]) == 1.0, (a, b, i, s)
