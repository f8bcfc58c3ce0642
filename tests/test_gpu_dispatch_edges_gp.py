"""Both sides of the dispatch rules of the genomic-prediction and MLE paths, against the CPU oracle: the four routes of the
coefficient pass pg_gp_beta_cols, the batched passes of the fused cross-validation, every path length, the geometry of the prediction
pass and the block count of the mass step.  Every shape names the rule it sits on and the source line of that rule, and asserts the
rule as restated in tests/dispatch_rules.py before anything is launched: when a rule moves, its points fail instead of sliding off
their edge.  Tolerances are the suite's own (tests/test_gpu_kinship_path.py): selected alphas and lambdas equal, error indices rtol
1e-10 / atol 2.6e-8 with fewer than 2 % of the cells off by more than 1e-10, coefficients rtol 1e-10 / atol 1e-11 max|ref|, the m = 0
MLE fits 2e-5 from the analytic optimum.

The dispatch goes by the pool count n of the matrix, not by the number of training pools: from ~70 pools up the fits train on a
spread subset of the pools (the first, the last three, both sides of every 32 / 64 / 128 / 256 / 512 boundary), so the oracle's
pseudo-inverses stay small while the kernels run the full width (the other pools' rows of Z are zero, their predictions unused)."""
import numpy as np
import pytest
import torch

import dispatch_rules as R

pytestmark = pytest.mark.gpu

PG_ERR_INVALID, PG_ERR_UNSUPPORTED = -1, -5
ENV = {"OLD": "POOLGEN_GP_BETA_OLD", "VALU": "POOLGEN_GP_BETA_VALU", "SCALAR": "POOLGEN_GP_BETA_SCALAR"}


def design(n, p, k, seed):
    from poolgen_amd import synth
    G = synth.genotype_matrix(p, n, "cuda", seed=seed)
    return G, synth.phenotypes(G, n, k=k, seed=seed)


def spread_rows(n, m=64):
    if n <= m + 8:
        return np.arange(n)
    keep = set(np.rint(np.linspace(0, n - 1, m)).astype(int).tolist()) | {n - 3, n - 2, n - 1}
    keep |= {b + d for b in (32, 64, 128, 256, 512) for d in (-1, 0, 1) if b + 1 < n}
    return np.array(sorted(keep))


def make_folds(n_rows, n_folds, n_reps, seed):
    rng = np.random.default_rng(seed)
    assert n_rows >= 3 * n_folds                       # three validation pools per fold at least: a defined error index
    return np.stack([rng.permutation(np.arange(n_rows) % n_folds) for _ in range(n_reps)])


def host_xt(G, n):
    return np.vstack([np.ones((1, n)), G.cpu().numpy()[:, :n]])


def assert_path(got, ref, what):
    """(beta, lambdas, perf) or (beta, alphas, lambdas, perf) against the oracle's, at the suite's tolerances"""
    b, rb = got[0].cpu().numpy(), ref[0]
    perf, rp = got[-1], ref[-1]
    off = np.abs(perf - rp) > 1e-10
    print(f"[{what}] perf: max |diff| {np.abs(perf - rp).max():.2e}, {off.mean():.4f} of {perf.size} cells off by > 1e-10, max index "
          f"{np.abs(rp).max():.2f}; beta: max |diff| / max|ref| {np.abs(b - rb).max() / np.abs(rb).max():.2e}")
    assert perf.shape == rp.shape and np.isfinite(rp).all(), what
    for g, r in zip(got[1:-1], ref[1:-1]):
        assert np.array_equal(g, r), what + " selected alpha / lambda"
    assert np.allclose(perf, rp, rtol=1e-10, atol=2.6e-8) and off.mean() < 0.02, what + " perf"
    assert np.allclose(b, rb, rtol=1e-10, atol=1e-11 * np.abs(rb).max()), what + " beta"


def launches(engine, call):
    """call() with the library's launch counters on -> (result, {kernel family: launches})"""
    engine.profile(True)
    engine.profile_reset()
    try:
        res = call()
        cnt = {name: engine.profile_get(name)[1] for name in ("gp_xxt", "gp_beta", "gp_predict", "kinship")}
    finally:
        engine.profile(False)
    return res, cnt


def same_bits(a, b):
    return all(np.array_equal(x.cpu().numpy() if torch.is_tensor(x) else x, y.cpu().numpy() if torch.is_tensor(y) else y)
               for x, y in zip(a, b))


# ---- A. the routes of the coefficient pass -----------------------------------------------------------------------------------
# pg_gp_beta_cols (pg_sweep.hip:1484-1544), in this order: the matrix-core products mode while ms_fits(n, ncol, 1) (:1520; from 33
# pools up to 1176 / 728 / 288 / 144 / 240 pools for 2 / 16 / 20 / 30 / 33-34 columns); k_gp_beta_mfma for column-major output, 5 ..
# 16 columns and at most 608 pools (:1523: zrows * 16 + 4 tiles of 64 x 36 doubles within 150 KiB); k_gp_beta_lds<C> for even C in 6 ..
# 24, Z above 12 KiB and Z + 4 tiles of 64 x 34 within 150 KiB (:1530); else the scalar k_gp_beta<C> (:1537).  C = round_cols(ncol).
# With n_reps = 1 the n_folds * k columns of the one repetition go in one pass (pg_gp.hip:874, :926).
# (n, p, n_folds, k, route)
ROUTE_POINTS = [
    (30, 600, 3, 2, ("beta_mfma", 16)),       # C = 6 below 33 pools (ms_fits: nc >= 5, :971): the LDS-staged MFMA form
    (32, 640, 4, 4, ("beta_mfma", 16)),       # C = 16, the last pool count below the matrix-core mode
    (33, 660, 3, 2, ("matrix-core", 6)),      # C = 6, the first matrix-core count
    (30, 600, 2, 2, ("beta_scalar", 4)),      # C = 4 < 5 columns (:1523): scalar k_gp_beta<4>
    (40, 800, 2, 2, ("matrix-core", 4)),      # C = 4 in the matrix-core mode
    (48, 900, 2, 4, ("matrix-core", 8)),      # C = 8
    (32, 640, 4, 5, ("beta_scalar", 24)),     # C = 20 > 16 columns below 33 pools, Z = 32 * 24 * 8 = 6 KiB <= 12 KiB (:1530): scalar k_gp_beta<24>
    (40, 900, 10, 2, ("matrix-core", 24)),    # C = 20 in one pass: the shapes of test_gp_ridge_many_fold_columns with n_reps = 1
    (80, 1500, 10, 2, ("matrix-core", 24)),
    (728, 1500, 4, 4, ("matrix-core", 16)),   # C = 16: last matrix-core count (one column group)
    (729, 1500, 4, 4, ("beta_scalar", 16)),   # C = 16 above it: past k_gp_beta_mfma (608 pools) and k_gp_beta_lds<16> (656): scalar k_gp_beta<16>
    (288, 1200, 4, 5, ("matrix-core", 24)),   # C = 20: last matrix-core count (two column groups)
    (289, 1200, 4, 5, ("beta_lds", 24)),      # C = 20 above it: k_gp_beta_lds<24>
    (436, 1200, 4, 5, ("beta_lds", 24)),      # the last pool count whose Z (436 * 24 doubles) fits beside the tiles
    (437, 1200, 4, 5, ("beta_scalar", 24)),   # C = 20 past the LDS form (n_even = 438): scalar k_gp_beta<24>
    (144, 1000, 5, 6, ("matrix-core", 34)),   # C = 30: last matrix-core count
    (145, 1000, 5, 6, ("beta_scalar", 34)),   # C = 30 above it: no LDS form beyond 24 columns, scalar k_gp_beta<34>
    (240, 1200, 17, 2, ("matrix-core", 34)),  # C = 34 (three column groups): last matrix-core count
    (241, 1200, 17, 2, ("beta_scalar", 34)),  # C = 34 above it
]
for _n, _p, _nf, _k, _route in ROUTE_POINTS:
    assert R.beta_route(_n, _nf * _k) == _route and R.cv_route(_n, _p, _nf * _k, 1) == "per_rep", (_n, _nf, _k)
assert [R.last_ms_count(c, 1) for c in (6, 16, 20, 30, 34)] == [1056, 728, 288, 144, 240]
assert not R.ms_fits(32, 6, 1) and R.ms_fits(33, 6, 1)


def route_case(n, p, n_folds, k, n_reps=1):
    G, Y = design(n, p, k, seed=700 + n + n_folds)
    rows = spread_rows(n, max(64, 5 * n_folds))
    return G, Y, rows, make_folds(len(rows), n_folds, n_reps, seed=n)


@pytest.mark.parametrize("n,p,n_folds,k,route", ROUTE_POINTS)
def test_coefficient_pass_routes(engine, oracle, n, p, n_folds, k, route):
    G, Y, rows, folds = route_case(n, p, n_folds, k)
    got, cnt = launches(engine, lambda: engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n))
    assert cnt["gp_beta"] == 2 and cnt["gp_predict"] == k     # one pass for the folds, one for the all-rows fit; one prediction pass per trait
    assert_path(got, oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, n=n), f"n={n} C={n_folds * k} {route}")


def test_more_columns_than_one_pass_takes_the_per_fold_route(engine, oracle):
    """C = 5 folds x 7 traits = 35 > PG_MAX_SWEEP_COLS: penalised_path (pg_gp.hip:1045) leaves the fused passes for one fit per fold
    (cv_per_fold: pg_gp_ols_dev per fold, 7 columns -> matrix-core, width 8) and still matches the oracle; C = 34 is fused (ROUTE_POINTS)."""
    n, p, n_folds, k = 60, 1000, 5, 7
    assert R.cv_route(n, p, n_folds * k, 1) == "per_fold" and R.cv_route(n, p, 34, 1) == "per_rep"
    assert R.beta_route(n, k, colmajor=False) == ("matrix-core", 8)
    G, Y, rows, folds = route_case(n, p, n_folds, k)
    got, cnt = launches(engine, lambda: engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n))
    assert cnt["gp_beta"] == n_folds + 1 and cnt["gp_predict"] == 0        # no fused prediction pass ran
    assert_path(got, oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, n=n), "C=35 per fold")


# gp_ols hands its k columns over row-major (pg_gp.hip:1127): never k_gp_beta_mfma; below 33 pools the scalar kernel of width
# round_cols(k) = 2, 3, 6, 8
@pytest.mark.parametrize("k,cols", [(1, 2), (3, 3), (5, 6), (8, 8)])
def test_gp_ols_below_the_matrix_core_mode(engine, oracle, k, cols):
    n, p = 24, 700
    assert R.beta_route(n, k, colmajor=False) == ("beta_scalar", cols)
    G, Y = design(n, p, k, seed=24 + k)
    idx = np.array([i for i in range(n) if i % 7 != 3])
    beta = engine.gp_ols(G, Y, idx, n=n).cpu().numpy()
    rc, ref = oracle.gp_ols(host_xt(G, n), Y, idx, n=n)
    assert rc == 0
    assert np.allclose(beta, ref, rtol=1e-10, atol=1e-11 * np.abs(ref).max())


def test_gp_ols_trait_limit_is_refused(engine, oracle):
    """k = 9 traits: PG_ERR_UNSUPPORTED (pg_gp.hip:1085), and the context goes on working"""
    from poolgen_amd import NativeError
    n, p = 24, 300
    G, Y = design(n, p, 9, seed=9)
    idx = np.arange(n)
    with pytest.raises(NativeError, match=rf"failed \({PG_ERR_UNSUPPORTED}\)"):
        engine.gp_ols(G, Y, idx, n=n)
    beta = engine.gp_ols(G, Y[:, :8], idx, n=n).cpu().numpy()
    rc, ref = oracle.gp_ols(host_xt(G, n), Y[:, :8], idx, n=n)
    assert rc == 0 and np.allclose(beta, ref, rtol=1e-10, atol=1e-11 * np.abs(ref).max())


# The older forms behind their switches (pg_sweep.hip:1520-1531), on shapes the matrix-core mode takes by default.  POOLGEN_GP_BETA_OLD
# alone falls to k_gp_beta_mfma (5 .. 16 columns); with _VALU to k_gp_beta_lds<C> (Z above 12 KiB: n_even * C > 1536); _SCALAR only
# switches the LDS form off, so _OLD + _SCALAR is k_gp_beta_mfma again and the scalar kernel needs all three.
# (n, p, n_folds, k) -> {switches: route}
FORCED_SHAPES = {
    (200, 2000, 5, 2): {(): ("matrix-core", 12), ("OLD",): ("beta_mfma", 16), ("OLD", "VALU"): ("beta_lds", 12),
                        ("OLD", "SCALAR"): ("beta_mfma", 16), ("OLD", "VALU", "SCALAR"): ("beta_scalar", 12)},
    (260, 2000, 3, 2): {("OLD", "VALU"): ("beta_lds", 6), ("OLD", "VALU", "SCALAR"): ("beta_scalar", 6)},     # 260 * 6 = 1560 > 1536
    (260, 2000, 4, 2): {("OLD", "VALU"): ("beta_lds", 8)},
    (260, 2000, 4, 4): {("OLD",): ("beta_mfma", 16), ("OLD", "VALU"): ("beta_lds", 16)},
}
FORCED_POINTS = [(shape, sw, route) for shape, by in FORCED_SHAPES.items() for sw, route in by.items()]
for (_n, _p, _nf, _k), _sw, _route in FORCED_POINTS:
    assert R.beta_route(_n, _nf * _k, env=set(_sw)) == _route and R.beta_route(_n, _nf * _k)[0] == "matrix-core", (_n, _nf, _k, _sw)
_forced_ref = {}


@pytest.mark.parametrize("shape,switches,route", FORCED_POINTS,
                         ids=["-".join(map(str, sh)) + "-" + ("+".join(sw) or "default") for sh, sw, _ in FORCED_POINTS])
def test_forced_coefficient_pass_routes(engine, oracle, monkeypatch, shape, switches, route):
    n, p, n_folds, k = shape
    G, Y, rows, folds = route_case(n, p, n_folds, k)
    if shape not in _forced_ref:                                  # one oracle run per shape, shared and left unchanged
        _forced_ref[shape] = oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, n=n)
    for s in switches:
        monkeypatch.setenv(ENV[s], "1")
    got = engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n)
    assert_path(got, _forced_ref[shape], f"n={n} C={n_folds * k} {switches} {route}")


# The batched passes (n_reps > 1, pg_gp.hip:874, :894-916): the n_reps * C + k columns of all repetitions and of the all-rows fit, 16
# per pass; the first pass takes repetition 0 alone when that costs no extra pass (short_first, :898-899).
# (n, p, n_folds, k, n_reps, total columns, passes, short_first)
BATCH_POINTS = [
    (60, 1200, 5, 1, 3, 16, [16], False),            # exactly one full pass, the all-rows fit in its last column
    (48, 1000, 8, 1, 2, 17, [8, 9], True),           # one column past a pass: repetition 0 alone first
    (32, 640, 8, 1, 2, 17, [8, 9], True),            # the same below 33 pools: both passes k_gp_beta_mfma
    (80, 1500, 16, 1, 2, 33, [16, 16, 1], False),    # C = 16: never short; the all-rows fit alone in a one-column pass (width 2)
    (60, 1200, 5, 3, 2, 33, [15, 16, 2], True),      # C = 15: short first, the second pass straddles repetition 1 and the all-rows fit
]
for _n, _p, _nf, _k, _reps, _total, _passes, _short in BATCH_POINTS:
    assert _reps * _nf * _k + _k == _total and R.batched_passes(_nf * _k, _k, _reps) == (_passes, _short)
    assert R.cv_route(_n, _p, _nf * _k, _reps) == "batched" and R.cv_route(_n, _p, _nf * _k, _reps, {"POOLGEN_RIDGE_PER_REP"}) == "per_rep"
assert R.beta_route(32, 8) == R.beta_route(32, 9) == ("beta_mfma", 16) and R.beta_route(80, 1) == ("matrix-core", 2)


@pytest.mark.parametrize("n,p,n_folds,k,n_reps,total,passes,short_first", BATCH_POINTS)
def test_batched_coefficient_passes(engine, oracle, monkeypatch, n, p, n_folds, k, n_reps, total, passes, short_first):
    G, Y, rows, folds = route_case(n, p, n_folds, k, n_reps)
    got, cnt = launches(engine, lambda: engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n))
    assert cnt["gp_beta"] == len(passes)
    assert_path(got, oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, n=n), f"batched {passes}")
    monkeypatch.setenv("POOLGEN_RIDGE_PER_REP", "1")
    per_rep, cnt = launches(engine, lambda: engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n))
    assert cnt["gp_beta"] == n_reps + 1
    assert same_bits(got, per_rep), "batched passes and one pass per repetition: the same bits"


# The MLE sums (pg_mle.hip:464) go through the same pass row-major with ss_out_dev: matrix-core from 33 to 1176 pools for the two
# columns [1 | y]; below and above, the scalar k_gp_beta<2>, the one kernel besides it that writes g'g (pg_sweep.hip:649).
# The assertions are those of test_mle_against_the_oracle_and_the_analytic_optimum (tests/test_gpu_mle.py) for m = 0; the oracle gets
# an n x 0 covariate, so that it forms no kinship and solves no 1200 x 1200 eigenproblem for fits that use neither.
@pytest.mark.parametrize("n", [24, 1200])
def test_mle_sums_through_the_scalar_kernel(engine, oracle, n):
    assert R.mle_sums_route(n, 0, 1) == ("beta_scalar", 2) and R.mle_sums_route(33, 0, 1) == R.mle_sums_route(1176, 0, 1) == ("matrix-core", 2)
    assert R.mle_sums_route(32, 0, 1) == R.mle_sums_route(1177, 0, 1) == ("beta_scalar", 2)
    p, k, tol = 300, 1, 2e-5
    G, Y = design(n, p, k, seed=101)
    Gh = G.cpu().numpy()
    m, K, beta, var, pv = engine.mle_with_covariate(G, Y, 0.75, force_m=0, n=n)
    beta, var, pv = beta.cpu().numpy(), var.cpu().numpy(), pv.cpu().numpy()
    assert m == 0
    none = np.zeros((n, 0))
    ref = oracle.mle_with_covariate(Gh, Y, covariate=none, n=n, threads=8)
    ols = oracle.ols_with_covariate(Gh, Y, covariate=none, n=n)
    assert ref["m"] == ols["m"] == 0
    scale = np.abs(ols["beta"]).max()
    d_go = np.abs(beta - ref["beta"]).max() / scale
    d_g = np.abs(beta - ols["beta"]).max() / scale
    d_o = np.abs(ref["beta"] - ols["beta"]).max() / scale
    vb_opt = ols["var"] * 2.0 * (n - 2) / n
    rv_g = np.abs(var / vb_opt - 1.0).max()
    rv_o = np.abs(ref["var"] / vb_opt - 1.0).max()
    print(f"[mle n={n} p={p} m=0] beta / max|beta|: |GPU - oracle| {d_go:.1e}  |GPU - optimum| {d_g:.1e}  |oracle - optimum| {d_o:.1e}   "
          f"var: rel |GPU / optimum - 1| {rv_g:.1e}  |oracle / optimum - 1| {rv_o:.1e}")
    assert d_g <= tol and d_o <= tol and d_go <= 2 * tol
    assert rv_g <= 50 * tol and rv_o <= 50 * tol
    t = np.abs(beta / var)                                         # p-values as written: t = b / v_b, df = n - 1 (mle.rs:175)
    want = np.array([2.0 * (1.0 - oracle.lib.orc_students_t_cdf(float(x), float(n - 1))) for x in t.reshape(-1)]).reshape(t.shape)
    assert np.max(np.abs(pv - want)) <= 1e-10


def test_mle_refusals_leave_the_engine_usable(engine):
    """pg_mle.hip:392 (k = 5: PG_ERR_INVALID), :419-421 (m + 2 beyond the 10 design columns of the simplex kernels, no residual
    degrees of freedom: PG_ERR_UNSUPPORTED); after each, the same small fit gives the same bits"""
    from poolgen_amd import NativeError
    n, p = 24, 200
    G, Y = design(n, p, 5, seed=5)
    first = engine.mle_with_covariate(G, Y[:, :1], 0.75, force_m=0, n=n)
    want = [x.clone() for x in first[2:]]
    assert all(bool(torch.isfinite(x).all()) for x in want)
    G4, Y4 = design(4, p, 1, seed=4)
    for refused, code in ((lambda: engine.mle_with_covariate(G, Y[:, :1], 0.75, force_m=9, n=n), PG_ERR_UNSUPPORTED),
                          (lambda: engine.mle_with_covariate(G4, Y4, 0.75, force_m=2, n=4), PG_ERR_UNSUPPORTED),
                          (lambda: engine.mle_with_covariate(G, Y, 0.75, force_m=0, n=n), PG_ERR_INVALID)):
        with pytest.raises(NativeError, match=rf"failed \({code}\)"):
            refused()
        again = engine.mle_with_covariate(G, Y[:, :1], 0.75, force_m=0, n=n)
        assert all(torch.equal(a, b) for a, b in zip(want, again[2:]))


# ---- B. path lengths ---------------------------------------------------------------------------------------------------------
# L = llround(1 / lambda_step) + 1 lambdas (pg_gp.hip:1030-1033); with_path_len (:502-506) picks the kernels compiled for LP = L
# rounded up to even (k_gp_path_sums_cols<LP>, k_gp_predict_folds<LP, ., .>, and k_gp_path_sums<LP> for the all-rows fit), odd and even
# L separate variants of the prediction pass (:835-836), as are several locus groups per block (n <= 256) and one (n = 260).
PATH_LENGTHS = list(range(2, 17))
for _L in PATH_LENGTHS:
    assert R.path_len(1.0 / (_L - 1)) == _L and R.path_lp(_L) == _L + (_L & 1) <= R.GP_LMAX
    assert R.predict_geometry(40, 4, _L)["variant"] == (R.path_lp(_L), True, bool(_L & 1))
    assert R.predict_geometry(260, 4, _L)["variant"] == (R.path_lp(_L), False, bool(_L & 1))
assert {R.path_lp(L) for L in PATH_LENGTHS} == set(range(2, 17, 2))


@pytest.mark.parametrize("L", PATH_LENGTHS)
def test_every_path_length(engine, oracle, L):
    """ridge-like and glmnet (alpha < 0: the L x L grid) at n = 40 (four locus groups per block), ridge-like at n = 260 (one group,
    40 training pools)"""
    step = 1.0 / (L - 1)
    n, p, k, n_folds, n_reps = 40, 1500, 2, 4, 2
    G, Y, rows, folds = route_case(n, p, n_folds, k, n_reps)
    Xt = host_xt(G, n)
    got = engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, lambda_step=step, n=n)
    assert got[2].shape == (n_reps, n_folds, L, k)
    assert_path(got, oracle.penalised_lambda_path(Xt, Y, rows, folds, n_folds, alpha=0.0, lambda_step=step, n=n), f"L={L} ridge n=40")
    got = engine.gp_penalised(G, Y, rows, folds, n_folds, -0.1, False, lambda_step=step, n=n)
    assert got[3].shape == (n_reps, n_folds, L, L, k)
    assert_path(got, oracle.penalised_path_general(Xt, Y, rows, folds, n_folds, -0.1, False, lambda_step=step, n=n), f"L={L} glmnet n=40")
    n = 260
    G, Y = design(n, p, k, seed=260)
    rows = spread_rows(n, 40)
    folds = make_folds(len(rows), n_folds, n_reps, seed=L)
    got = engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, lambda_step=step, n=n)
    assert_path(got, oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, lambda_step=step, n=n), f"L={L} ridge n=260")


def test_path_longer_than_sixteen_is_refused(engine):
    """L = 17 (lambda_step = 1 / 16): PG_ERR_INVALID before anything is launched (pg_gp.hip:1031)"""
    from poolgen_amd import NativeError
    assert R.path_len(1.0 / 16) == 17 > R.GP_LMAX
    n, p, k, n_folds = 40, 1500, 2, 4
    G, Y, rows, folds = route_case(n, p, n_folds, k, 2)
    for call in (lambda: engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, lambda_step=1.0 / 16, n=n),
                 lambda: engine.gp_penalised(G, Y, rows, folds, n_folds, -0.1, False, lambda_step=1.0 / 16, n=n)):
        def refused():
            with pytest.raises(NativeError, match=rf"failed \({PG_ERR_INVALID}\)"):
                call()
        _, cnt = launches(engine, refused)
        assert set(cnt.values()) == {0}, cnt
    beta, lam, perf = engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, lambda_step=1.0 / 15, n=n)    # L = 16 runs
    assert perf.shape == (2, n_folds, 16, k) and np.isfinite(perf).all()


# ---- C. prediction-pass geometry and the mass step ---------------------------------------------------------------------------
# PredictPipeline::launch (pg_gp.hip:820-826): 256 threads up to 128 pools, 512 above; 4 locus groups per block up to 64 pools, 2 up to
# 256, 1 above, where grid.y = ceil(n / 512) takes over.
# (n, n_reps, threads, groups, grid.y)
GEOMETRY_POINTS = [
    (64, 1, 256, 4, 1),     # last pool count with four locus groups
    (65, 2, 256, 2, 1),     # first with two (two waves per group)
    (128, 1, 256, 2, 1),    # last 256-thread count
    (129, 2, 512, 2, 1),    # first 512-thread count: groups of 192 threads, 128 threads idle
    (192, 1, 512, 2, 1),    # last with groups of 192
    (193, 2, 512, 2, 1),    # first with groups of 256
    (256, 1, 512, 2, 1),    # last grouped count
    (257, 2, 512, 1, 1),    # first ungrouped count
    (512, 1, 512, 1, 1),    # last with one block row
    (513, 2, 512, 1, 2),    # grid.y = 2: the second block row holds one pool
]
for _n, _reps, _threads, _groups, _gy in GEOMETRY_POINTS:
    _g = R.predict_geometry(_n, 4, 11)
    assert (_g["threads"], _g["groups"], _g["grid_y"], _g["chunk"]) == (_threads, _groups, _gy, 64), _n


@pytest.mark.parametrize("n,n_reps,threads,groups,grid_y", GEOMETRY_POINTS)
def test_prediction_pass_geometry(engine, oracle, n, n_reps, threads, groups, grid_y):
    p, k, n_folds = 1000, 1, 4
    G, Y, rows, folds = route_case(n, p, n_folds, k, n_reps)
    assert {n - 1, min(n - 1, 63), min(n - 1, 64)} <= set(rows.tolist())            # pools on both sides of the group boundaries validate
    got = engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n)
    assert_path(got, oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, n=n), f"n={n} {threads}x{groups} y={grid_y}")


# chunk = clamp((49152 - 264 n_folds) / (8 n_folds (LPr + 2)), 4, 64) loci staged per step (:821-822), here with L = 16 (LPr = 16).  The
# fused passes carry at most 34 fold x trait columns (:1045), so 34 folds (chunk 8) is as near the lower clamp as a launch gets: the
# clamp to 4 itself needs 59 folds and more, which take the per-fold route.
# (n_folds, chunk, clamped)
CHUNK_POINTS = [
    (5, 64, True),      # 66 before the clamp: on the upper clamp
    (6, 55, False),     # the first fold count below it
    (17, 18, False),    # strictly between
    (34, 8, False),     # the most folds one fused pass carries
]
for _nf, _chunk, _clamped in CHUNK_POINTS:
    _g = R.predict_geometry(110, _nf, 16)
    assert _g["chunk"] == _chunk and ((49152 - 264 * _nf) // (8 * _nf * 18) > 64) == _clamped and _g["lds"] <= 49152
    assert R.cv_route(110, 1200, _nf, 1) == "per_rep"
assert (49152 - 264 * 58) // (8 * 58 * 18) == 4 and (49152 - 264 * 59) // (8 * 59 * 18) == 3 and R.predict_geometry(110, 59, 16)["chunk"] == 4
assert R.cv_route(110, 1200, 35, 1) == "per_fold"


@pytest.mark.parametrize("n_folds,chunk,clamped", CHUNK_POINTS)
def test_prediction_pass_chunk(engine, oracle, n_folds, chunk, clamped):
    n, p, k, step = 110, 1200, 1, 1.0 / 15
    G, Y = design(n, p, k, seed=110)
    rows = np.arange(n)
    folds = make_folds(n, n_folds, 1, seed=n_folds)
    got = engine.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, lambda_step=step, n=n)
    assert_path(got, oracle.penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, lambda_step=step, n=n), f"{n_folds} folds chunk {chunk}")


# ridge_path_params_cols (pg_gp.hip:631): nb = clamp(p / 2048, 32, 1024) blocks per column of the mass step.  The other tests have
# p <= 5000 (nb = 32) or p = 5 M (nb = 1024).
# (p, nb, alpha, proxy)
MASS_POINTS = [
    (67583, 32, 0.0, False),     # the last locus count on the lower clamp
    (67584, 33, 1.0, True),      # the first past it; the Proxy branch of k_gp_norm_max_cols
    (409600, 200, 1.0, False),   # well inside: several blocks per lane of k_gp_reduce_parts (64 lanes); ~5 s of oracle
]
for _p, _nb, _alpha, _proxy in MASS_POINTS:
    assert R.mass_nb(_p) == _nb
assert R.mass_nb(5000) == 32 and R.mass_nb(5_000_000) == 1024


@pytest.mark.parametrize("p,nb,alpha,proxy", MASS_POINTS)
def test_mass_step_block_count(engine, oracle, exact, p, nb, alpha, proxy):
    n, k, n_folds = 40, 1, 4
    G, Y, rows, folds = route_case(n, p, n_folds, k)
    Xt = host_xt(G, n)
    got = engine.gp_penalised(G, Y, rows, folds, n_folds, alpha, proxy, n=n)
    if proxy:                         # the proxy models' fits and proxy coefficients from binary128, as test_gp_penalised_family_matches_oracle
        exact.install_into_oracle(oracle, True)
    try:
        ref = oracle.penalised_path_general(Xt, Y, rows, folds, n_folds, alpha, proxy, n=n)
    finally:
        if proxy:
            exact.install_into_oracle(oracle, False)
    assert_path(got, ref, f"p={p} nb={nb} alpha={alpha} proxy={proxy}")
