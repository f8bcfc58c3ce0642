"""pg_beta_reg_dev (the regularised incomplete Beta function the gwalpha fit evaluates: statrs' beta_reg behind Beta::cdf's
guards) against the oracle's restatement orc_beta_reg on a grid: a, b in {1e-3, 0.3, 1, 2.5, 10}^2; x = 0, 1e-12, seventeen
interior points -- thirteen fixed ones and four around the symmetry switch (a + 1) / (a + b + 2) of the pair, two on either
side --, 1 - 1e-12, 1 and 1 + 1e-15 (what the cumulative percentiles of the ML cost reach; Beta::cdf answers 1 there).
Absolute difference <= 1e-10, the project's contract for its statistical functions.

The side of the switch a point takes is not visible in the result; both sides evaluate the same expression
x >= (a + 1) / (a + b + 2) in IEEE arithmetic, and the points 1e-9 away from the switch on either side, which agree with the
oracle like every other point, are where a differently formed threshold would show as a jump of the fraction's truncation."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
SHAPES = [1e-3, 0.3, 1.0, 2.5, 10.0]
FIXED = [0.01, 0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99]


def grid():
    a, b, x = [], [], []
    for sa in SHAPES:
        for sb in SHAPES:
            s = (sa + 1.0) / (sa + sb + 2.0)
            xs = [0.0, 1e-12] + FIXED + [s - 1e-3, s - 1e-9, s + 1e-9, s + 1e-3] + [1.0 - 1e-12, 1.0, 1.0 + 1e-15]
            assert len(xs) == 2 + 17 + 3 and all(0.0 < v < 1.0 for v in xs[2:19])
            a += [sa] * len(xs); b += [sb] * len(xs); x += xs
    return np.array(a), np.array(b), np.array(x)


def test_beta_reg_matches_the_oracle_on_the_grid(engine, oracle):
    a, b, x = grid()
    got = engine.beta_reg(a, b, x).cpu().numpy()
    want = np.array([oracle.lib.orc_beta_reg(float(p), float(q), min(max(float(v), 0.0), 1.0)) for p, q, v in zip(a, b, x)])
    d = np.abs(got - want)
    i = int(np.argmax(d))
    print(f"beta_reg: {len(x)} points, max |device - oracle| = {d[i]:.3g} at a={a[i]} b={b[i]} x={x[i]!r}")
    assert np.all(np.isfinite(got)) and d[i] <= 1e-10
    assert np.all(got[x <= 0.0] == 0.0) and np.all(got[x >= 1.0] == 1.0)
    assert np.all((got >= 0.0) & (got <= 1.0 + 1e-15))


def test_beta_reg_rejects_what_the_reference_rejects(engine):
    got = engine.beta_reg([0.0, -1.0, 1.0, 1.0, float("nan")], [1.0, 1.0, 0.0, 1.0, 1.0], [0.5, 0.5, 0.5, float("nan"), 0.5]).cpu().numpy()
    assert np.all(np.isnan(got))
    assert engine.beta_reg(np.zeros(0), np.zeros(0), np.zeros(0)).numel() == 0
    with pytest.raises(ValueError):
        engine.beta_reg([1.0, 2.0], [1.0], [0.5])
