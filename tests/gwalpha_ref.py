"""GWAlpha restated in Python (gwas/gwalpha.rs of the reference), for the tests of the gwalpha operator.

Everything numerical that the reference takes from a crate goes through the oracle's restatements: statrs' beta_reg
(orc_beta_reg), ndarray's sum (orc_ndarray_sum), the filter / to_frequencies / sort_by_allele_freq of base/sync.rs and the
rounding of parse_f64_roundup_and_own.  The Nelder-Mead is the one of oracle/poolgen_oracle.c (mle_nelder_mead) with D = 4.
The reference's test literals (gwalpha.rs:389-390, tests/golden/gwalpha_literals.json) pin the whole.
"""
from __future__ import annotations

import math

import numpy as np

import oracle_lib

EPS = 2.220446049250313e-16      # f64::EPSILON = PARAMETER_LOWER_LIMIT (gwalpha.rs:8)
UPPER = 10.00                    # PARAMETER_UPPER_LIMIT (gwalpha.rs:9)
MAX_ITERS = 1000                 # .configure(|state| state.max_iters(1_000)) (gwalpha.rs:120, :148)
ALLELES = "ATCGND"


def bound(x: float) -> float:
    """bound_parameters_with_logit(x, EPSILON, 10) (base/helpers.rs:120-130)."""
    return EPS + ((UPPER - EPS) / (1.00 + math.exp(-x)))


def beta_cdf(o, a: float, b: float, x: float) -> float:
    """statrs Beta::cdf: 0 below the support, 1 from x = 1 on, beta_reg between."""
    if x <= 0.0:
        return 0.0
    if x >= 1.0:
        return 1.0
    return o.lib.orc_beta_reg(a, b, x)


def nd_sum(o, x) -> float:
    a = np.ascontiguousarray(x, dtype=np.float64)
    return o.lib.orc_ndarray_sum(a.ctypes.data, len(a))


def cost_ls(o, shapes, percs_a, percs_b, q_prime) -> float:
    """least_squares_beta (gwalpha.rs:11-41) at bounded shapes."""
    sa = sb = 0.0
    for i in range(len(percs_a)):
        sa += (percs_a[i] - beta_cdf(o, shapes[0], shapes[1], q_prime[i])) ** 2
        sb += (percs_b[i] - beta_cdf(o, shapes[2], shapes[3], q_prime[i])) ** 2
    return sa + sb


def cost_ml(o, shapes, percs_a, percs_b, percs_a0, percs_b0) -> float:
    """maximum_likelihood_beta (gwalpha.rs:43-79) at bounded shapes."""
    la = lb = 0.0
    for i in range(len(percs_a)):
        da = beta_cdf(o, shapes[0], shapes[1], percs_a[i]) - beta_cdf(o, shapes[0], shapes[1], percs_a0[i])
        db = beta_cdf(o, shapes[2], shapes[3], percs_b[i]) - beta_cdf(o, shapes[2], shapes[3], percs_b0[i])
        da = EPS if da < EPS else da
        db = EPS if db < EPS else db
        la += math.log10(da)
        lb += math.log10(db)
    return -la - lb


def nelder_mead(cost, D: int = 4):
    """argmin 0.8's Nelder-Mead as oracle/poolgen_oracle.c words it, from prepare_solver_neldermead(D, 1)
    (base/helpers.rs:132-146).  Returns (best parameters, best cost, iterations done)."""
    V = D + 1
    sx = [[1.5 if i == j else 1.0 for j in range(D)] for i in range(V)]
    cs = [cost(v) for v in sx]

    def sort():
        order = sorted(range(V), key=lambda i: cs[i])  # stable
        sx[:] = [sx[i] for i in order]
        cs[:] = [cs[i] for i in order]

    sort()
    it = 0
    while it < MAX_ITERS:
        mean = 0.0
        for c in cs:
            mean += c
        mean /= V
        sd = 0.0
        for c in cs:
            sd += (c - mean) * (c - mean)
        sd = math.sqrt(sd / (V - 1.0))
        if sd < EPS:
            break
        x0 = []
        for j in range(D):
            c = sx[0][j]
            for i in range(1, V - 1):
                c += sx[i][j]
            x0.append(c * (1.0 / (V - 1.0)))
        xw = sx[V - 1]
        xr = [x0[j] + (x0[j] - xw[j]) * 1.0 for j in range(D)]
        cr = cost(xr)
        if cr < cs[V - 2] and cr >= cs[0]:
            sx[V - 1], cs[V - 1] = xr, cr
        elif cr < cs[0]:
            xe = [x0[j] + (xr[j] - x0[j]) * 2.0 for j in range(D)]
            ce = cost(xe)
            if ce < cr:
                sx[V - 1], cs[V - 1] = xe, ce
            else:
                sx[V - 1], cs[V - 1] = xr, cr
        else:
            xc = [x0[j] + (xw[j] - x0[j]) * 0.5 for j in range(D)]
            cc = cost(xc)
            if cc < cs[V - 1]:
                sx[V - 1], cs[V - 1] = xc, cc
            else:
                for i in range(1, V):
                    sx[i] = [sx[0][j] + (sx[i][j] - sx[0][j]) * 0.5 for j in range(D)]
                    cs[i] = cost(sx[i])
        sort()
        it += 1
    return sx[0], cs[0], it


def prepare_locus(o, counts, bins, flt):
    """prepare_geno_and_pheno_stats (gwalpha.rs:162-225): filter -> to_frequencies -> sort_by_allele_freq(true) -> drop the
    first allele.  counts: n x 6 in sync column order; bins are the pool sizes the filter sees (main.rs:210, phen.rs:157).
    Returns None (locus dropped) or (allele ids of the rows, n x rows frequencies, id of the dropped allele)."""
    r = o.filter_locus(np.asarray(counts, dtype=np.uint64), bins, flt)
    if r is None:
        return None
    ids, fc = r
    fr = o.to_frequencies(fc)
    fr, ids = o.sort_by_allele_freq(fr, ids, True)
    dropped = -1
    if fr.shape[1] >= 2:
        dropped = int(ids[0])
        fr, ids = fr[:, 1:], ids[1:]
    return ids, fr, dropped


def row_inputs(o, f, bins, q, mn, mx):
    """prepare_freqs_and_qprime (gwalpha.rs:227-279) for one column f of the frequency matrix."""
    n = len(f)
    p_a = 0.0
    for i in range(n):      # a strided column's dot: ndarray's plain loop
        p_a = p_a + f[i] * bins[i]
    q_prime = [0.0] * n
    for i in range(1, n):
        q_prime[i] = (q[i] - mn) / (mx - mn)
    with np.errstate(all="ignore"):
        bins_a = [float(np.float64(f[i]) * bins[i] / np.float64(p_a)) for i in range(n)]
        bins_b = [float((1.0 - np.float64(f[i])) * bins[i] / (1.0 - np.float64(p_a))) for i in range(n)]
    percs_a, percs_b = list(bins_a), list(bins_b)
    for i in range(1, n):
        percs_a[i] = nd_sum(o, bins_a[: i + 1])
        percs_b[i] = nd_sum(o, bins_b[: i + 1])
    percs_a0, percs_b0 = [0.0] * n, [0.0] * n
    for i in range(n - 1):
        percs_a0[i + 1] = percs_a[i]
        percs_b0[i + 1] = percs_b[i]
    return dict(p_a=p_a, q_prime=q_prime, percs_a=percs_a, percs_b=percs_b, percs_a0=percs_a0, percs_b0=percs_b0)


def cost_at(o, method: str, shapes, ri) -> float:
    """The cost of `method` at bounded shapes for the row inputs `ri`."""
    if method == "LS":
        return cost_ls(o, shapes, ri["percs_a"], ri["percs_b"], ri["q_prime"])
    return cost_ml(o, shapes, ri["percs_a"], ri["percs_b"], ri["percs_a0"], ri["percs_b0"])


def mu_diff(shapes, mn, mx) -> float:
    a_mu = mn + (mx - mn) * (shapes[0] / (shapes[0] + shapes[1]))
    b_mu = mn + (mx - mn) * (shapes[2] / (shapes[2] + shapes[3]))
    return a_mu - b_mu


def alpha_of(shapes, p_a, sig, mn, mx) -> float:
    return (2.00 * math.sqrt(p_a * (1.0 - p_a))) * mu_diff(shapes, mn, mx) / sig


def fit_row(o, method: str, ri, sig, mn, mx):
    par, c, it = nelder_mead(lambda p: cost_at(o, method, [bound(x) for x in p], ri))
    shapes = [bound(x) for x in par]
    return dict(alpha=alpha_of(shapes, ri["p_a"], sig, mn, mx), shapes=shapes, cost=c, iters=it,
                mu_diff=mu_diff(shapes, mn, mx))


def gwalpha_locus(o, counts, bins, q, sig, mn, mx, flt, method: str = "ML", fit: bool = True):
    """gwalpha_ls / gwalpha_ml (gwalpha.rs:281-380) on one locus: None, or a list of rows (dicts: allele id, mean_freq,
    inputs, and with fit=True alpha, shapes, cost, iters, mu_diff)."""
    n = len(bins)
    if n < 3:
        raise ValueError("gwalpha: the reference's phenotype matrix needs at least 3 pools (check() panics)")
    pl = prepare_locus(o, counts, bins, flt)
    if pl is None:
        return None
    ids, fr, dropped = pl
    rows = []
    for j in range(fr.shape[1]):
        f = [float(v) for v in fr[:, j]]
        ri = row_inputs(o, f, bins, q, mn, mx)
        s = 0.0
        for v in f:
            s = s + v
        row = dict(allele=int(ids[j]), mean_freq=s / n, inputs=ri, dropped=dropped)
        p_a = ri["p_a"]
        if fit and p_a > 0.0 and p_a < 1.0:
            row.update(fit_row(o, method, ri, sig, mn, mx))
        rows.append(row)
    return rows


def csv_lines(o, chrom: str, pos: int, rows) -> str:
    """The output line(s) of a locus (gwalpha.rs:318-328)."""
    out = ""
    for r in rows:
        out += f"{chrom},{pos},{ALLELES[r['allele']]},{o.round_own(r['mean_freq'], 6)},Pheno_0,{o.round_own(r['alpha'], 6)},Unknown\n"
    return out


def parse_gwalpha_fmt(text: str):
    """The gwalpha_fmt phenotype file as base/phen.rs:111-158 reads it: (bins, q column of the phenotype matrix, sig, min,
    max, pool names).  q is normalised here once; the operator normalises it again (gwalpha.rs:248-251)."""
    lines = text.splitlines()

    def rhs(i):
        return lines[i].split("=")[1].replace(";", "")

    def vec(i):
        return [float(x.strip()) for x in rhs(i).replace("[", "").replace("]", "").strip().split(",")]

    sig, mn, mx = float(rhs(1).strip()), float(rhs(2).strip()), float(rhs(3).strip())
    perc, q = vec(4), vec(5)
    p0, p1 = perc + [1.0], [0.0] + perc
    bins = [a - b for a, b in zip(p0, p1)]
    n = max(len(bins), 3)
    q_prime = [0.0] * n
    for i in range(len(q)):
        q_prime[i + 1] = (q[i] - mn) / (mx - mn)
    return bins, q_prime[: len(bins)], sig, mn, mx, [f"pool-{i}" for i in range(n)]


def gwalpha_fmt_text(name, sig, mn, mx, perc, q) -> str:
    return (f'Pheno_name="{name}";\nsig={sig!r};\nMIN={mn!r};\nMAX={mx!r};\n'
            f'perc=[{",".join(repr(float(v)) for v in perc)}];\nq=[{",".join(repr(float(v)) for v in q)}];\n')


def make_case(seed: int, L: int, n: int):
    """The input recipe of the gwalpha tests: coverage 20-59, frequencies linear in pool rank with a N(0, 0.3) slope clipped to
    [0.03, 0.97]; a fifth of the loci carry a third allele above the MAF, a fifth misread bases below it; locus 1 has a pool
    without reads, locus 2 the same counts in every pool.  Returns counts (L x n x 6 uint32), bins, q, sig, min, max."""
    rng = np.random.default_rng(seed)
    counts = np.zeros((L, n, 6), dtype=np.uint32)
    rank = np.arange(n) / (n - 1) - 0.5
    for l in range(L):
        a, b = rng.choice(4, size=2, replace=False)        # the two main alleles among A, T, C, G
        f = np.clip(rng.uniform(0.25, 0.75) + rng.normal(0.0, 0.3) * rank, 0.03, 0.97)
        cov = rng.integers(20, 60, size=n)
        ca = rng.binomial(cov, f)
        counts[l, :, a] = ca
        counts[l, :, b] = cov - ca
        others = [j for j in range(4) if j not in (a, b)]
        kind = l % 5
        if kind == 3:      # a third allele well above the MAF
            c3 = rng.binomial(cov, 0.15)
            counts[l, :, others[0]] = c3
        elif kind == 4:    # one misread base, below the MAF
            counts[l, rng.integers(0, n), others[1]] = 1
    if L > 2:
        counts[1, n // 2, :] = 0
        counts[2, :, :] = counts[2, 0, :]
    w = rng.uniform(0.6, 1.4, size=n)
    bins = w / w.sum()
    q = np.concatenate([[0.0], np.sort(rng.uniform(0.05, 0.95, size=n - 1))])
    return counts, bins, q, 0.25, 0.02, 0.98


def load_oracle():
    return oracle_lib.load()
