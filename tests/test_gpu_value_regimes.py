"""Every route of the ols_iter_with_kinship regression sweep on the loci real pool-seq data is made of (tests/value_regimes.py:
singletons, near-fixed major-allele columns, rare alleles, tiny spreads, fixed differences, monomorphic rows) and on a ladder of planted
signals whose p-values run from 1 down to 1e-16 and below -- against BINARY128 (oracle/poolgen_exact.c), never against the literal oracle:
on these rows the reference's own normal equations are 1e-7 .. 1e-5 off (tests/test_value_regimes.py measures it), so the oracle is
the noisy side.

Each sweep kernel subtracts the locus' first pool before it sums; the copies of that step are written separately (sweep_chunk, the
super-row kernel, the matrix-core kernel in MODE 0 and MODE 2, the fused sums of the generic and of the 13-tile kinship kernel), and on
the rows the rest of the suite runs (synth: frequencies inside [0.02, 0.98]) losing any of them costs 1e-14.  Here it costs 1e-7.

Asserted per case, per locus and trait:
  NaN exactly on the monomorphic rows, in beta, var and p;
  |beta - exact| <= 1e-10 beta_scale and |var - exact| <= 1e-10 var_scale with the natural scales sqrt(s_yy / s_gg) and
      s_yy / (s_gg dfe) of the fit (one corpus mixes coefficients ten orders of magnitude apart: the per-run scale of
      test_gpu_exact.assert_close, applied per locus);
  the p-function alone: |p - formula(t_gpu)| <= 1e-10 with t_gpu = beta / sqrt(var) formed on the host from the returned arrays (the
      two IEEE operations of ols_close), its special cases applied, and the reference's formula as statrs evaluates it;
  the tail: |p - binary128 tail(|t_exact|)| <= 2e-12 wherever |t_exact| >= 1 (5 and 6 pools included: the formula itself stays inside
      2e-12 of the tail there, tests/test_value_regimes.py).
The worst error per tag is printed for every case.  Measured on one MI355X, worst over the 35 cases: beta 1.7e-13 and var 1.9e-12 of
their scales (singletons and near-fixed rows at 200 and 201 pools; every other tag below 4e-14), p against the formula 1.2e-13, p
against the tail 4.5e-13.  (Before PG_T_H_IS_ONE, pg_stats_device.h, the weakest ladder rungs missed the formula by 2.2e-8 .. 4.0e-8:
statrs returns exactly 1 where h = nu / (nu + t^2) is within four ulps of 1.)"""
import ctypes
import os

import numpy as np
import pytest
import torch

import dispatch_rules as R
import value_regimes as V

pytestmark = pytest.mark.gpu

TOL = 1e-10        # coefficients and variances over their natural scale; p against the formula (absolute)
TAIL = 2e-12       # p against the binary128 tail where |t| >= 1

_REF = {}


def covariates(n, m):
    """m well-conditioned covariates: an orthonormalised normal draw, as in test_sweep_random_shapes"""
    return None if m == 0 else np.linalg.qr(np.random.default_rng([n, m]).normal(size=(n, m)))[0]


def reference(exact, n, which, m=0):
    """binary128 fits and natural scales of the corpus at n pools for the trait set `which` beside m covariates; once per session"""
    key = (n, which, m)
    if key not in _REF:
        c = V.corpus(n)
        Y, C = getattr(c, which), covariates(n, m)
        ex = exact.ols_covariate(c.G, Y, C)
        bs, vs = V.scales(c.G, Y, C)
        _REF[key] = (ex, bs, vs)
    return _REF[key]


def device_matrix(n, reps=1, ld=None, nan_padding=False):
    """the corpus rows `reps` times over, p x ld on the device (ld even; the columns behind the pools zero, or NaN)"""
    G = V.corpus(n).G
    ld = n + (n & 1) if ld is None else ld
    host = np.full((len(G) * reps, ld), np.nan if nan_padding else 0.0)
    host[:, :n] = np.tile(G, (reps, 1))
    return torch.from_numpy(host).cuda(), host


def check(what, got, n, which, cols, oracle, exact, capsys, m=0, reps=1):
    """got = (beta, var, p), each (reps p) x len(cols), for the traits `cols` of the trait set `which`"""
    c = V.corpus(n)
    ex, bs, vs = reference(exact, n, which, m)
    tile = lambda a: np.tile(a[:, cols], (reps, 1))
    eb_, ev_, et_, ep_, bs, vs = (tile(a) for a in (ex["beta"], ex["var"], ex["t"], ex["pval"], bs, vs))
    tags = np.tile(c.tags, reps)
    b, v, p = (np.asarray(x.cpu() if torch.is_tensor(x) else x).reshape(len(tags), len(cols)) for x in got)
    mono = tags == "monomorphic"
    live = ~mono
    for name, a in (("beta", b), ("var", v), ("p", p)):
        assert np.array_equal(np.isnan(a), np.repeat(mono[:, None], len(cols), axis=1)), f"{what}: NaN pattern of {name}"
    db = np.abs(b - eb_) / bs
    dv = np.abs(v - ev_) / vs
    pf, tg = V.host_p(oracle, b, v, n)
    dpf = np.abs(p - pf)
    tail = live[:, None] & (np.abs(et_) >= 1.0)
    dpt = np.where(tail, np.abs(p - ep_), 0.0)
    lines = [f"\n[{what}] worst per tag: |beta - exact| / scale, |var - exact| / scale, |p - formula(t_gpu)|, |p - exact tail| where |t| >= 1"]
    for tag in V.TAGS:
        r = tags == tag
        if tag != "monomorphic":
            lines.append(f"    {tag:14s} {db[r].max():.2e}  {dv[r].max():.2e}  {dpf[r].max():.2e}  {dpt[r].max():.2e}")
    with capsys.disabled():
        print("\n".join(lines))
    assert db[live].max() <= TOL, f"{what}: beta, {db[live].max():.2e} of its scale at locus {np.unravel_index(np.argmax(np.where(live[:, None], db, 0)), db.shape)}"
    assert dv[live].max() <= TOL, f"{what}: var, {dv[live].max():.2e} of its scale at locus {np.unravel_index(np.argmax(np.where(live[:, None], dv, 0)), dv.shape)}"
    assert dpf[live].max() <= TOL, f"{what}: p against the formula at the GPU's own t: {dpf[live].max():.2e}"
    worst = np.unravel_index(np.argmax(dpt), dpt.shape)
    assert dpt.max() <= TAIL, f"{what}: p against the binary128 tail: {dpt.max():.2e} at |t| = {abs(et_[worst]):.6g}, df = {n - 1}: {p[worst]!r} vs {ep_[worst]!r}"
    assert np.all((p[live] >= 0.0) & (p[live] <= 1.0))


def sweep(engine, n, which, cols, m=0, ld=None, nan_padding=False):
    c = V.corpus(n)
    Y = np.ascontiguousarray(getattr(c, which)[:, cols])
    G, _ = device_matrix(n, ld=ld, nan_padding=nan_padding)
    engine.set_phenotypes(None)
    engine.covariates_set(n, covariates(n, m), Y)
    return engine.ols_sweep(G, len(cols), n)


# ---- the sweep kernels, m = 0 --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 6, 24, 32])
def test_rows_kernel(engine, oracle, exact, capsys, n):
    """k_ols_sweep_rows / sweep_chunk: up to 32 pools (launch_sweep; below the matrix-core kernel's 5 chunks)"""
    assert n <= R.SW_CH and not R.ms_fits(n, 1 + 3, 0)
    check(f"rows kernel n={n}", sweep(engine, n, "Y", [0, 1, 2]), n, "Y", [0, 1, 2], oracle, exact, capsys)


@pytest.mark.parametrize("n,ld", [(33, None), (40, 44), (200, None), (201, None)])
def test_matrix_core_kernel(engine, oracle, exact, capsys, n, ld):
    """k_ols_sweep_mfma MODE 0: the first pool count it takes, a row pitch with NaN padding behind the pools, the headline pool count
    and an odd one with a masked last group"""
    assert R.ms_fits(n, 1 + 3, 0)
    check(f"matrix-core kernel n={n} ld={ld}", sweep(engine, n, "Y", [0, 1, 2], ld=ld, nan_padding=ld is not None), n, "Y", [0, 1, 2],
          oracle, exact, capsys)


@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("forced", ["POOLGEN_SWEEP_V1", "POOLGEN_SWEEP_V2"])
def test_lane_per_locus_kernels_as_shipped(engine, oracle, exact, capsys, monkeypatch, forced, n):
    """k_ols_sweep_rows (V1) and the super-row kernel k_ols_sweep (V2) at pool counts the matrix-core kernel takes by default, through
    the library's own switch"""
    monkeypatch.setenv(forced, "1")
    check(f"{forced} n={n}", sweep(engine, n, "Y", [0, 1, 2]), n, "Y", [0, 1, 2], oracle, exact, capsys)


@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("m", [3, 8])
def test_sweep_with_covariates(engine, oracle, exact, capsys, n, m):
    """Z = [1 | C]: the shift cancels through the intercept column of the basis, s_gg = g'g' - |Q'g'|^2"""
    assert R.ms_fits(n, m + 1 + 3, 0)
    check(f"covariates n={n} m={m}", sweep(engine, n, "Y", [0, 1, 2], m=m), n, "Y", [0, 1, 2], oracle, exact, capsys, m=m)


# ---- the fused intercept-only sums of the kinship pass ---------------------------------------------------------------------------
def fused(engine, n, which, cols):
    c = V.corpus(n)
    Y = np.ascontiguousarray(getattr(c, which)[:, cols])
    G, _ = device_matrix(n)
    engine.profile(True)
    try:
        engine.profile_reset()
        m, K, beta, var, pv = engine.ols_with_covariate(G, Y, 0.0, force_m=0, n=n)
        torch.cuda.synchronize()
        n_finish, n_sweep = engine.profile_get("sweep_finish")[1], engine.profile_get("sweep")[1]
    finally:
        engine.profile(False)
    assert m == 0 and n_finish == 1 and n_sweep == 0, "the fits must have been closed from the fused sums (k_sweep_finish*), not by a sweep"
    return beta, var, pv


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [24, 40, 100])
def test_fused_sums_generic_kinship_kernel(engine, oracle, exact, capsys, n, k):
    """the generic kinship kernel's sums (8-wave build up to 64 pools, 16-wave above) closed by k_sweep_finish_x2 (k = 1) and
    k_sweep_finish (k = 2)"""
    lay = R.kin_layout(n)
    assert R.kin_fuses(n, k) and not lay["spec13"] and lay["w8"] == (n <= 64)
    cols = [0, 1][:k]
    check(f"fused sums, generic kernel n={n} k={k}", fused(engine, n, "Y", cols), n, "Y", cols, oracle, exact, capsys)


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n,small", [(193, 3), (200, 3), (201, 1), (208, 1)])
def test_fused_sums_13_tile_kernel(engine, oracle, exact, capsys, n, small, k):
    """the 13-tile kinship kernels: one pool in the last tile column, the last count with the narrow last column, the first without
    it, all 13 tile columns full"""
    lay = R.kin_layout(n)
    assert R.kin_fuses(n, k) and lay["spec13"] and lay["small"] == small
    cols = [0, 2][:k]
    check(f"fused sums, 13-tile kernel n={n} k={k}", fused(engine, n, "Y", cols), n, "Y", cols, oracle, exact, capsys)


# ---- the lazy route and the host-buffer form ---------------------------------------------------------------------------------------
def test_lazy_kinship_route(engine, oracle, exact, capsys):
    """pg_ols_kinship_dev without K: the matrix-core kernel in MODE 2, which also hands the shift back to the closing lane"""
    n, cols = 200, [0, 1, 2]
    c = V.corpus(n)
    assert R.ms_fits(n, 1 + len(cols), 2)
    G, host = device_matrix(n)
    bound = float((host[:, :n].sum(axis=1) ** 2).sum() / n / (host[:, :n] ** 2).sum())
    assert bound >= 0.75 + 1e-6, "the ones vector must decide m = 0 for this matrix"
    engine.profile(True)
    try:
        engine.profile_reset()
        m, K, beta, var, pv = engine.ols_with_covariate(G, c.Y, 0.75, n=n, want_K=False)
        torch.cuda.synchronize()
        n_kin, n_sweep = engine.profile_get("kinship")[1], engine.profile_get("sweep")[1]
    finally:
        engine.profile(False)
    assert m == 0 and K is None and n_kin == 0 and n_sweep == 1, "the lazy route forms no kinship matrix"
    check("lazy kinship route n=200", (beta, var, pv), n, "Y", cols, oracle, exact, capsys)


def test_host_buffer_form_in_slabs(native, oracle, exact, capsys):
    """pg_ols_kinship on host buffers with the smallest slab (1024 loci at 200 pools): the corpus ten times over is two whole slabs
    and a ragged one, swept slab by slab"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    n, reps, cols = 200, 10, [0, 2]
    c = V.corpus(n)
    host = np.ascontiguousarray(np.tile(c.G, (reps, 1)))
    p, k = len(host), len(cols)
    assert p > 2 * 1024 and p % 1024
    Y = np.ascontiguousarray(c.Y[:, cols])
    beta, var, pv = (np.full((p, k), -7.0) for _ in range(3))
    K = np.empty((n, n)); m = ctypes.c_int(-1)
    ctx = ctypes.c_void_p()
    assert native.pg_create(ctypes.byref(ctx), 0, None) == 0, native.pg_last_error(None)
    os.environ["POOLGEN_HOST_SLAB_MB"] = "1"
    try:
        rc = native.pg_ols_kinship(ctx, host.ctypes.data, p, n, n, Y.ctypes.data, k, 0.75, 0, ctypes.byref(m), K.ctypes.data,
                                   beta.ctypes.data, var.ctypes.data, pv.ctypes.data)
        err = native.pg_last_error(ctx)
    finally:
        del os.environ["POOLGEN_HOST_SLAB_MB"]
        native.pg_destroy(ctx)
    assert rc == 0, err
    assert m.value == 0
    check("host buffers, 3 slabs n=200", (beta, var, pv), n, "Y", cols, oracle, exact, capsys, reps=reps)


# ---- traits scaled by 1e-6 and 1e6 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,n", [("rows", 24), ("matrix-core", 200), ("fused", 100)])
def test_scaled_traits(engine, oracle, exact, capsys, route, n):
    """trait 0 times 1e-6 and times 1e6 in one call: the same t and p as trait 0, coefficients twelve orders of magnitude apart (and
    the reference's |beta| <= eps rule, which sets t = 0 for the weakest rungs of the small trait)"""
    cols = [0, 1]
    assert R.kin_fuses(n, 2) if route == "fused" else R.ms_fits(n, 1 + 2, 0) == (route == "matrix-core")
    got = fused(engine, n, "Y_scaled", cols) if route == "fused" else sweep(engine, n, "Y_scaled", cols)
    check(f"scaled traits, {route} n={n}", got, n, "Y_scaled", cols, oracle, exact, capsys)
