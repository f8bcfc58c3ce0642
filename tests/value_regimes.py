"""A deterministic corpus of allele-frequency rows chosen by their VALUES, for the regression sweep of ols_iter_with_kinship.

`synth.genotype_matrix` keeps every locus well inside (0, 1) and `synth.phenotypes` keeps |t| at O(1): g'g / s_gg stays below ~100 and
p-values stay in (1e-3, 1).  Real pool-seq matrices are dominated by the opposite: loci that are 0 (or 1) in every pool but one, and the
only p-values anybody reports are the small ones.  The rows here are those loci, tagged:

  singleton       all pools 0, one pool 1 / d (d = 30, 70, 1000, 10000), the odd pool at index 0, 1, 15, 16, n // 2, n - 1
  near-fixed      1 - singleton: the major-allele column the loader emits next to a singleton
  rare            Binomial(d, 0.003) / d at d = 70 and 1000 (constant draws discarded)
  common-near-1   1 - such a row
  tiny-spread     0.5 + {-1, 0, 1} * 1e-5 per pool
  two-valued      half the pools 0, half 1 (fixed differences), shuffled
  monomorphic     all 0, all 1, all 0.5: rank-deficient, NaN in beta, var and p
  ladder          g = 0.5 + 0.2 (r yhat + sqrt(1 - r^2) uhat) with yhat the centred, normalised trait 0, uhat a unit vector orthogonal
                  to 1 and yhat, and r = t / sqrt(n - 2 + t^2): the regression of trait 0 on g has the t statistic t.  Forty targets
                  log-spaced over 1e-9 .. 1e9 with alternating signs, plus one rung per decade of p (the middle of every decade from
                  [0.1, 1) down to [1e-16, 1e-15) at n - 1 degrees of freedom, the df of the reported p), so that every pool count has
                  a locus in every decade of p a GWAS reports
  plain           64 rows in the style of poolgen_amd.synth (numpy draws): the anchor to what the rest of the suite runs

The loci are shuffled (a 64-locus group holds a mix of tags) and their number is not a multiple of 64.  numpy only; the CPU tests
(test_value_regimes.py) and the GPU tests (test_gpu_value_regimes.py) see the same rows.

Also here: the natural scale of every (locus, trait) fit in np.longdouble, and two plain fp64 restatements of the m = 0 closing arithmetic
of the sweep kernels (ols_close, pg_sweep.hip) -- with the subtraction of the locus' first pool that every kernel performs before it
sums, and without it."""
from collections import namedtuple
from functools import lru_cache

import numpy as np

TAGS = ("singleton", "near-fixed", "rare", "common-near-1", "tiny-spread", "two-valued", "monomorphic", "ladder", "plain")
DEPTHS = (30, 70, 1000, 10000)
SEED = 20261021          # (every ladder rung clears the quantisation-edge test of test_value_regimes.py with this seed)
EPS = 2.220446049250313e-16
TAU = 1e-12              # the kernels' relative singularity threshold on s_gg / sum g'^2 (pg_sweep.hip: A.D.tau)

Corpus = namedtuple("Corpus", "G tags Y Y_scaled t_target")


def odd_pool_positions(n):
    """index of the odd pool of a singleton: the shift element itself (0), its neighbour, both sides of a 16-pool tile column, the
    middle and the last pool"""
    return sorted({i for i in (0, 1, 15, 16, n // 2, n - 1) if 0 <= i < n})


def t_tail(t, df):
    """P(|T_df| > t) by the finite series of Abramowitz & Stegun 26.7.3 / 26.7.4 in np.longdouble: good to ~1e-19 absolute, which is
    all the ladder needs to aim at the middle of a decade of p"""
    L = np.longdouble
    pi = 4 * np.arctan(L(1))
    th = np.arctan(L(t) / np.sqrt(L(df)))
    c, s = np.cos(th), np.sin(th)
    c2 = c * c
    if df == 1:
        return L(1) - 2 * th / pi
    if df & 1:
        term = tot = c
        for j in range(3, df - 1, 2):
            term = term * c2 * L(j - 1) / L(j)
            tot = tot + term
        return L(1) - 2 / pi * (th + s * tot)
    term = tot = L(1)
    for j in range(2, df - 1, 2):
        term = term * c2 * L(j - 1) / L(j)
        tot = tot + term
    return L(1) - s * tot


def t_for_p(p, df):
    """the t with P(|T_df| > t) = p, by bisection on log t"""
    lo, hi = np.log(1e-3), np.log(1e7)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        if t_tail(np.exp(mid), df) > p:
            lo = mid
        else:
            hi = mid
    return float(np.exp(0.5 * (lo + hi)))


def ladder_targets(n):
    """signed target t statistics of the ladder rows at n pools"""
    wide = np.logspace(-9, 9, 40) * np.where(np.arange(40) % 2 == 0, 1.0, -1.0)
    rungs = [t_for_p(10.0 ** -(d - 0.5), n - 1) * (1.0 if d % 2 else -1.0) for d in range(1, 17)]
    return np.concatenate([wide, np.array(rungs)])


def _traits(n, rng):
    y0 = rng.standard_normal(n)
    y1 = 170.0 + 7.0 * rng.standard_normal(n)       # a measured quantity with an offset: |mean| / sd ~ 24
    y2 = np.zeros(n)
    y2[rng.permutation(n)[: n // 2]] = 1.0          # case / control
    Y = np.column_stack([y0, y1, y2])
    return Y, np.column_stack([y0 * 1e-6, y0 * 1e6])


def _plain_rows(rng, rows, n):
    b = np.clip(rng.beta(0.5, 0.5, size=(rows, 1)), 0.02, 0.98)
    pr = np.clip(b + 0.08 * rng.standard_normal((rows, n)), 0.0, 1.0)
    depth = rng.poisson(60.0, size=(rows, n)) + 10
    return rng.binomial(depth, pr) / depth


def _nonconstant(draw, rows):
    out = []
    while len(out) < rows:
        for r in draw(rows):
            if r.min() != r.max() and len(out) < rows:
                out.append(r)
    return np.array(out)


@lru_cache(maxsize=None)
def corpus(n, seed=SEED):
    """-> Corpus(G[p, n] float64, tags[p], Y[n, 3], Y_scaled[n, 2], t_target[p]): the rows and their tags, the traits of the first
    call (standard normal; 170 + 7 N(0, 1); 0 / 1), the traits of the second call (trait 0 times 1e-6 and times 1e6) and, for ladder
    rows, the |t| the row was built for (NaN elsewhere).  The arrays are shared between callers and read-only."""
    rng = np.random.default_rng([seed, n])
    Y, Ys = _traits(n, rng)
    rows, tags, tt = [], [], []

    def add(tag, block, t=None):
        block = np.atleast_2d(np.asarray(block, dtype=np.float64))
        rows.extend(block)
        tags.extend([tag] * len(block))
        tt.extend([np.nan] * len(block) if t is None else list(np.abs(t)))

    pos = odd_pool_positions(n)
    single = np.zeros((len(DEPTHS) * len(pos), n))
    for a, d in enumerate(DEPTHS):
        for b, i in enumerate(pos):
            single[a * len(pos) + b, i] = 1.0 / d
    add("singleton", single)
    add("near-fixed", 1.0 - single)
    for d in (70, 1000):
        r = _nonconstant(lambda k: rng.binomial(d, 0.003, size=(k, n)) / d, 12)
        add("rare", r)
        r = _nonconstant(lambda k: rng.binomial(d, 0.003, size=(k, n)) / d, 12)
        add("common-near-1", 1.0 - r)
    add("tiny-spread", _nonconstant(lambda k: 0.5 + rng.integers(-1, 2, size=(k, n)) * 1e-5, 8))
    two = np.zeros((8, n))
    two[:, n // 2:] = 1.0
    add("two-valued", rng.permuted(two, axis=1))
    add("monomorphic", np.stack([np.zeros(n), np.ones(n), np.full(n, 0.5)]))
    # the ladder: in np.longdouble up to the one rounding of g to fp64
    L = np.longdouble
    yc = Y[:, 0].astype(L) - Y[:, 0].astype(L).mean()
    yh = yc / np.sqrt((yc * yc).sum())
    one = np.full(n, 1 / np.sqrt(L(n)))
    t = ladder_targets(n)
    lad = np.empty((len(t), n))
    for j, tj in enumerate(t):
        u = rng.standard_normal(n).astype(L)
        for _ in range(2):
            u = u - one * (one * u).sum()
            u = u - yh * (yh * u).sum()
        u = u / np.sqrt((u * u).sum())
        den = np.sqrt(L(n - 2) + L(tj) * L(tj))
        lad[j] = (L(0.5) + L(0.2) * (L(tj) / den * yh + np.sqrt(L(n - 2)) / den * u)).astype(np.float64)
    add("ladder", lad, t)
    add("plain", _nonconstant(lambda k: _plain_rows(rng, k, n), 64))
    if len(rows) % 64 == 0:
        add("plain", _nonconstant(lambda k: _plain_rows(rng, k, n), 1))
    order = rng.permutation(len(rows))
    out = Corpus(np.ascontiguousarray(np.array(rows)[order]), np.array(tags)[order], Y, Ys, np.array(tt)[order])
    for a in out:
        a.flags.writeable = False
    return out


def scales(G, Y, C=None):
    """natural scales of the fits of every row of G (p x n) on every column of Y (n x k) beside Z = [1 | C], in np.longdouble:
    beta_scale = sqrt(s_yy / s_gg) and var_scale = s_yy / (s_gg dfe) with s_gg = |(I - P_Z) g|^2, s_yy = |(I - P_Z) y|^2 and
    dfe = n - (m + 2).  -> (beta_scale, var_scale), each p x k fp64; inf where s_gg = 0."""
    L = np.longdouble
    G = np.asarray(G, dtype=L)
    Y = np.asarray(Y, dtype=L).reshape(G.shape[1], -1)
    n = G.shape[1]
    Z = [np.ones(n, dtype=L)] + ([] if C is None else [c for c in np.asarray(C, dtype=L).reshape(n, -1).T])
    Q = []
    for z in Z:                                    # Gram-Schmidt, twice
        for _ in range(2):
            for q in Q:
                z = z - q * (q * z).sum()
        Q.append(z / np.sqrt((z * z).sum()))
    Gr, Yr = G.copy(), Y.copy()
    for _ in range(2):
        for q in Q:
            Gr = Gr - np.outer(Gr @ q, q)
            Yr = Yr - np.outer(q, q @ Yr)
    sgg = (Gr * Gr).sum(axis=1)[:, None]
    syy = (Yr * Yr).sum(axis=0)[None, :]
    dfe = L(n - (len(Z) + 1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(syy / sgg).astype(np.float64), (syy / (sgg * dfe)).astype(np.float64)


def restated_fit(G, Y, shift=True):
    """The m = 0 closing arithmetic of the sweep kernels in plain fp64, operation for operation (ols_close and k_sweep_finish,
    pg_sweep.hip): subtract the locus' first pool (shift = False: do not), sum g', g'^2 and g' y_c (numpy's pairwise sums along a
    row; summed left to right instead, as one lane of a lane-per-locus kernel does, the 200-pool singletons whose odd pool is the
    shift element reach 1.5e-12 of the variance's scale: s_gg cancels by a factor n there), then
    s_gg = s2 - s1^2 / n, b = s_gy / s_gg, rss = s_yy - s_gy b (not below 0), var = rss / dfe / s_gg, t = b / sqrt(var).
    -> (beta, var, t), each p x k; NaN where s_gg is not above TAU s2, as in the kernels."""
    G = np.asarray(G, dtype=np.float64)
    p, n = G.shape
    Y = np.asarray(Y, dtype=np.float64).reshape(n, -1)
    k = Y.shape[1]
    yc = Y - Y.mean(axis=0)
    syy = (yc * yc).sum(axis=0)
    Gs = G - G[:, :1] if shift else G
    s1 = Gs.sum(axis=1)
    s2 = (Gs * Gs).sum(axis=1)
    sgy = np.stack([(Gs * yc[:, j]).sum(axis=1) for j in range(k)], axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sgg = s2 - s1 * s1 / float(n)
        bad = ~(sgg > TAU * s2)
        b = sgy / sgg[:, None]
        rss = np.maximum(syy[None, :] - sgy * b, 0.0)
        var = (rss / float(n - 2)) / sgg[:, None]
        t = np.where(np.abs(b) <= EPS, 0.0, b / np.sqrt(var))
    for a in (b, var, t):
        a[bad] = np.nan
    return b, var, t


def host_p(oracle, beta, var, n):
    """The sweep's p-value from a returned (beta, var) by the reference's formula, with the special cases of ols_close: t = 0 where
    |beta| <= eps, p = 1 where |t| <= eps or t is NaN, else 2 (1 - StudentsT(n - 1).cdf(|t|)) as statrs evaluates it
    (orc_students_t_cdf); NaN where beta is NaN.  -> (p, t)"""
    beta, var = np.asarray(beta, dtype=np.float64), np.asarray(var, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(np.abs(beta) <= EPS, 0.0, beta / np.sqrt(var))
    p = np.array([1.0 if (abs(x) <= EPS or np.isnan(x)) else 2.0 * (1.0 - oracle.lib.orc_students_t_cdf(abs(float(x)), float(n - 1)))
                  for x in t.reshape(-1)]).reshape(t.shape)
    p[np.isnan(beta)] = np.nan
    return p, t
