"""CPU tests of the value-regime corpus (tests/value_regimes.py): the rows are what their tags say, the fp64 restatement of the sweep
kernels' arithmetic WITH the subtraction of the first pool sits within 1e-12 of binary128 on the natural scale of every fit, the same
arithmetic WITHOUT it -- and the literal oracle, the reference's normal equations -- are worse than 1e-8 on the near-fixed and the
tiny-spread rows (so a GPU test on this corpus, held to 1e-10 against binary128, fails for a kernel that lost its shift, and cannot be
held to the oracle), and the reference's p-value formula agrees with the binary128 tail down the ladder.

Measured (24, 40, 200 and 201 pools; error against binary128 over the natural scale of the fit):
    with the shift        beta <= 2.0e-13, var <= 1.5e-13 over every tag and both trait sets
    without the shift     near-fixed: beta 0.8e-7 .. 4.5e-7, var 1.7e-7 .. 1.4e-6;   tiny-spread: beta 1.1e-7 .. 5.3e-7, var 0.9e-6 .. 2.1e-6
    the literal oracle    near-fixed: beta 0.8e-7 .. 1.6e-7, var 1.8e-7 .. 1.4e-6;   tiny-spread: beta 2.0e-7 .. 1.7e-6, var 1.3e-6 .. 9.9e-6"""
import numpy as np
import pytest

import value_regimes as V

POOLS = (24, 40, 200, 201)
GPU_POOLS = (5, 6, 24, 32, 33, 40, 100, 193, 200, 201, 208)     # every pool count tests/test_gpu_value_regimes.py runs
_EXACT = {}


def exact_fit(exact, n, which="Y"):
    """binary128 fits of the corpus at n pools, computed once per session"""
    if (n, which) not in _EXACT:
        c = V.corpus(n)
        _EXACT[(n, which)] = exact.ols_covariate(c.G, getattr(c, which), None)
    return _EXACT[(n, which)]


def worst(got, want, scale, rows):
    """largest |got - want| / scale over the given rows and every trait; a NaN on either side counts as infinitely wrong"""
    e = np.abs(got[rows] - want[rows]) / scale[rows]
    return float(np.max(np.where(np.isnan(e), np.inf, e)))


@pytest.mark.parametrize("n", GPU_POOLS)
def test_rows_are_what_their_tags_say(exact, n):
    c = V.corpus(n)
    G, tags = c.G, c.tags
    p = len(G)
    assert G.shape == (p, n) and p % 64 != 0 and p > 128 and set(tags) == set(V.TAGS)
    assert np.all((G >= 0.0) & (G <= 1.0))
    assert all(len(set(tags[g:g + 64])) >= 4 for g in range(0, p - 63, 64)), "shuffled, not grouped by tag"
    const = G.min(axis=1) == G.max(axis=1)
    assert np.array_equal(const, tags == "monomorphic")
    assert sorted(G[tags == "monomorphic"][:, 0].tolist()) == [0.0, 0.5, 1.0]
    pos = V.odd_pool_positions(n)
    assert pos[0] == 0 and pos[-1] == n - 1
    for tag, flip in (("singleton", False), ("near-fixed", True)):
        rows = G[tags == tag]
        rows = 1.0 - rows if flip else rows
        seen = set()
        for r in rows:
            (nz,) = np.nonzero(r)
            assert len(nz) == 1
            d = [d for d in V.DEPTHS if (1.0 - (1.0 - 1.0 / d) if flip else 1.0 / d) == r[nz[0]]]
            assert len(d) == 1, r[nz[0]]
            seen.add((d[0], int(nz[0])))
        assert seen == {(d, i) for d in V.DEPTHS for i in pos}
    for tag, flip in (("rare", False), ("common-near-1", True)):
        rows = G[tags == tag]
        rows = 1.0 - rows if flip else rows
        assert len(rows) == 24
        for r in rows:
            assert any(np.allclose(r * d, np.round(r * d), rtol=0, atol=1e-9) for d in (70, 1000)) and r.max() <= 0.1 and r.min() != r.max()
    assert set(np.unique(G[tags == "tiny-spread"]).tolist()) == {0.5 - 1e-5, 0.5, 0.5 + 1e-5}
    two = G[tags == "two-valued"]
    assert set(np.unique(two).tolist()) == {0.0, 1.0} and np.all(two.sum(axis=1) == n - n // 2)
    assert not np.all(np.diff(two, axis=1) >= 0), "shuffled order"
    # the traits
    Y = c.Y
    assert Y.shape == (n, 3) and set(np.unique(Y[:, 2]).tolist()) == {0.0, 1.0}
    assert np.all(np.abs(Y.mean(axis=0)) / Y.std(axis=0) <= 100.0)
    assert np.array_equal(c.Y_scaled, np.column_stack([Y[:, 0] * 1e-6, Y[:, 0] * 1e6]))
    # the ladder: the binary128 t of trait 0 is the target (the rows are rounded to fp64 once: 1e-5 relative while the residual is
    # not itself rounding noise), both signs, and every decade of p from [0.1, 1) down to [1e-15, 1e-14) holds a rung
    ex = exact_fit(exact, n)
    lad = tags == "ladder"
    t, want = ex["t"][lad, 0], c.t_target[lad]
    assert np.all(np.isnan(c.t_target[~lad])) and want.min() <= 1e-9 and want.max() >= 1e9
    mid = (want >= 1e-6) & (want <= 1e4)
    assert np.allclose(np.abs(t[mid]), want[mid], rtol=1e-5, atol=0)
    assert (t > 0).sum() >= 20 and (t < 0).sum() >= 20
    pv = ex["pval"][lad, 0]
    decades = set(np.floor(np.log10(pv[pv > 0])).astype(int).tolist())
    assert set(range(-15, 0)) <= decades, sorted(decades)
    assert all(abs(pv[i] - exact.t_two_sided_p(abs(t[i]), n - 1)) <= 1e-15 for i in range(len(t)) if abs(t[i]) > 1e-3)


@pytest.mark.parametrize("which", ["Y", "Y_scaled"])
@pytest.mark.parametrize("n", POOLS)
def test_shifted_restatement_is_within_1e_12_of_binary128(exact, n, which, capsys):
    c = V.corpus(n)
    Y = getattr(c, which)
    ex = exact_fit(exact, n, which)
    bs, vs = V.scales(c.G, Y)
    b, v, _ = V.restated_fit(c.G, Y)
    mono = c.tags == "monomorphic"
    assert np.array_equal(np.isnan(b), np.repeat(mono[:, None], Y.shape[1], axis=1)) and np.array_equal(np.isnan(b), np.isnan(v))
    eb, ev = worst(b, ex["beta"], bs, ~mono), worst(v, ex["var"], vs, ~mono)
    with capsys.disabled():
        print(f"\n[restatement with the shift, n={n} {which}] |beta - exact| / scale {eb:.2e}   |var - exact| / scale {ev:.2e}")
    assert eb <= 1e-12 and ev <= 1e-12


@pytest.mark.parametrize("n", POOLS)
def test_without_the_shift_and_in_the_oracle_these_rows_are_worse_than_1e_8(oracle, exact, n, capsys):
    """The premise of the GPU tests: on near-fixed and tiny-spread rows the kernels' arithmetic without the subtraction of the first
    pool, and the literal oracle, miss binary128 by more than 1e-8 of the natural scale -- a hundred times the 1e-10 the GPU is held
    to -- in the coefficient and in its variance."""
    c = V.corpus(n)
    ex = exact_fit(exact, n)
    bs, vs = V.scales(c.G, c.Y)
    bu, vu, _ = V.restated_fit(c.G, c.Y, shift=False)
    ref = oracle.ols_with_covariate(c.G, c.Y, covariate=np.zeros((n, 0)))
    for tag in ("near-fixed", "tiny-spread"):
        rows = c.tags == tag
        eu = (worst(bu, ex["beta"], bs, rows), worst(vu, ex["var"], vs, rows))
        eo = (worst(ref["beta"], ex["beta"], bs, rows), worst(ref["var"], ex["var"], vs, rows))
        with capsys.disabled():
            print(f"\n[{tag} n={n}] without the shift: beta {eu[0]:.2e} var {eu[1]:.2e}   literal oracle: beta {eo[0]:.2e} var {eo[1]:.2e}")
        assert min(eu) >= 1e-8 and min(eo) >= 1e-8


def formula(oracle, t, n):
    return 2.0 * (1.0 - oracle.lib.orc_students_t_cdf(abs(float(t)), float(n - 1)))


@pytest.mark.parametrize("n", (5, 6) + POOLS)
def test_reference_formula_follows_the_binary128_tail_down_the_ladder(oracle, exact, n, capsys):
    """|t| >= 1: 2 (1 - StudentsT(n - 1).cdf(|t|)) as statrs evaluates it, at the binary128 t, against the binary128 tail, at the
    2e-12 of test_host_rule_and_pvalue_match_oracle.  Measured: at most 9.8e-14 over 24 .. 201 pools; 5 and 6 pools (4 and 5 degrees
    of freedom) stay inside it too (2.2e-15 and 2.8e-16), so the GPU tests assert the tail at those pool counts as well."""
    c = V.corpus(n)
    ex = exact_fit(exact, n)
    lad = np.nonzero(c.tags == "ladder")[0]
    rows = [l for l in lad if abs(ex["t"][l, 0]) >= 1.0]
    assert len(rows) >= 30
    err = max(abs(formula(oracle, ex["t"][l, 0], n) - ex["pval"][l, 0]) for l in rows)
    with capsys.disabled():
        print(f"\n[tail n={n}] {len(rows)} rungs with |t| >= 1: max |formula - binary128 tail| = {err:.2e}")
    assert err <= 2e-12


@pytest.mark.parametrize("n", POOLS)
def test_no_ladder_rung_sits_on_a_quantisation_edge(oracle, exact, n):
    """|t| < 1: statrs' h = nu / (nu + t^2) rounds next to 1 and its p is quantised; a rung whose fp64 t and binary128 t fall on two
    sides of a step would differ by the step.  None does with value_regimes.SEED (the GPU assertions take the formula at the GPU's own
    t, so they do not depend on this)."""
    c = V.corpus(n)
    ex = exact_fit(exact, n)
    b, v, t = V.restated_fit(c.G, c.Y[:, :1])
    p_fp64 = V.host_p(oracle, b, v, n)[0]
    rows = [l for l in np.nonzero(c.tags == "ladder")[0] if abs(ex["t"][l, 0]) < 1.0]
    assert len(rows) >= 15
    for l in rows:
        te = ex["t"][l, 0]
        p_exact_t = 1.0 if abs(te) <= V.EPS else formula(oracle, te, n)
        assert abs(p_fp64[l, 0] - p_exact_t) <= 1e-10, (l, t[l, 0], te, p_fp64[l, 0], p_exact_t)


@pytest.mark.parametrize("df", [1, 2, 4, 5, 23, 39, 199, 200, 499])
def test_host_twin_of_the_device_tail_follows_the_formula_through_the_quantised_region(native, oracle, df):
    """pg_host_t_two_sided_p evaluates the device's series in the device's order.  Below |t| ~ 1e-6 the reference's p moves in steps
    (h = nu / (nu + t^2) rounds next to 1), and within four ulps of h = 1 statrs takes h for 1 and returns exactly 1 -- up to
    2.4e-7 (200 pools) above the true tail.  The weakest ladder rungs sit there; 2000 values of t across the region, 1e-10."""
    worst = 0.0
    for t in np.logspace(-10, -5, 2000):
        want = 2.0 * (1.0 - oracle.lib.orc_students_t_cdf(float(t), float(df)))
        worst = max(worst, abs(native.pg_host_t_two_sided_p(float(t), df) - want))
    assert worst <= 1e-10, worst
