"""gudmc restated in Python (popgen/gudmc.rs of the reference), for the tests of pg_normal_fit_dev, pg_gudmc_dev and `poolgen gudmc`.

The fits are the reference's own cost -- the left-to-right sum of -ln_pdf over the column (gudmc.rs:15-29) -- through a copy of
gwalpha_ref.nelder_mead with D = 2 and the 10 000-iteration cap (:42).  `reverse=True` sums the same terms from the other end: a
second legitimate evaluation of the same cost, whose distance from the first one is the resolution of the solver (T below).
`cost="moments"` is the closed form the library evaluates; it is here to be compared, the tests' reference is the sum.
"""
from __future__ import annotations

import functools
import math

import numpy as np

import rustfmt

EPS = 2.220446049250313e-16      # PARAMETER_LOWER_LIMIT = f64::EPSILON (gudmc.rs:12)
UPPER = 1e24                     # PARAMETER_UPPER_LIMIT (gudmc.rs:13)
MAX_ITERS = 10_000               # .configure(|state| state.max_iters(10_000)) (gudmc.rs:42)
LN_SQRT_2PI = 0.91893853320467274178032973640561763986139747363778341281715154  # statrs consts::LN_SQRT_2PI
HEADER = ("pop_a,pop_b,chr,pos_ini,pos_fin,mean_tajima_d_pop_b,mean_fst,sd_tajima_d_pop_b,sd_fst,tajima_d_pop_b,"
          "tajima_width_pop_b,tajima_width_deviation_from_r_pop_b,tajima_width_one_tail_pval_pop_b,fst_delta,fst_delta_one_tail_pval")

# The tolerance of the fitted values, measured, not chosen: 10 x the largest |d mu| / sigma and |d sigma| / sigma between the
# restatement summed forward and summed in reverse, over the whole corpus of the tests (fit_table() and every stage_cases() entry;
# columns whose forward sigma is <= 1e-12 sit at the logit's lower bound and are compared otherwise).  Produced by
#     python -m pytest tests/test_gudmc_ref.py -k tolerance -s
# which prints the two spreads (1.02e-7 and 8.0e-8 when this was written); T is 10 x the larger, rounded up to two digits.
T = 1.1e-6
DEGENERATE_SD = 1e-12


def sigma_of(x: float) -> float:
    """bound_parameters_with_logit(x, EPSILON, 1e24) (base/helpers.rs:120-130)."""
    try:
        e = math.exp(-x)
    except OverflowError:
        e = math.inf
    return EPS + ((UPPER - EPS) / (1.00 + e))


def cost_sum(mu: float, x: float, q, reverse: bool = False) -> float:
    """maximum_likelihood_normal (gudmc.rs:15-29): fold(0.0, |sum, x| sum + x) over -1.00 * ln_pdf, statrs' ln_pdf."""
    s = sigma_of(x)
    ln_s = math.log(s)
    total = 0.0
    for v in (reversed(q) if reverse else q):
        d = (v - mu) / s
        total = total + (-1.00 * ((-0.5 * d * d) - LN_SQRT_2PI - ln_s))
    return total


def moments(q):
    cnt = len(q)
    s = 0.0
    for v in q:
        s = s + v
    mean = s / cnt if cnt else math.nan
    ss = 0.0
    for v in q:
        ss = ss + (v - mean) * (v - mean)
    return float(cnt), mean, ss


def cost_moments(mu: float, x: float, mom) -> float:
    cnt, mean, ss = mom
    if cnt == 0.0:
        return 0.0
    s = sigma_of(x)
    dm = mean - mu
    return cnt * (LN_SQRT_2PI + math.log(s)) + (0.5 * (ss + cnt * (dm * dm))) / (s * s)


def nelder_mead(cost, D: int = 2, max_iters: int = MAX_ITERS):
    """gwalpha_ref.nelder_mead (argmin 0.8's Nelder-Mead as oracle/poolgen_oracle.c words it, from
    prepare_solver_neldermead(D, 1)) with the cap as a parameter.  Returns (best parameters, best cost, iterations done)."""
    V = D + 1
    sx = [[1.5 if i == j else 1.0 for j in range(D)] for i in range(V)]
    cs = [cost(v) for v in sx]

    def sort():
        order = sorted(range(V), key=lambda i: cs[i])  # stable
        sx[:] = [sx[i] for i in order]
        cs[:] = [cs[i] for i in order]

    sort()
    it = 0
    while it < max_iters:
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


def fit_normal(q, reverse: bool = False, cost: str = "sum"):
    """ml_normal_1d (gudmc.rs:39-60) on the values q (NaN already removed): (mu, sigma, iterations done)."""
    q = [float(v) for v in q]
    if any(math.isinf(v) for v in q):
        raise ValueError("the cost is NaN and Normal::new panics (gudmc.rs:22-25)")
    if cost == "sum":
        f = lambda p: cost_sum(p[0], p[1], q, reverse)
    else:
        mom = moments(q)
        f = lambda p: cost_moments(p[0], p[1], mom)
    par, _, it = nelder_mead(f)
    return par[0], sigma_of(par[1]), it


def fit_column(col, reverse: bool = False, cost: str = "sum"):
    return fit_normal([v for v in col if not math.isnan(v)], reverse, cost)


def round8(x: float) -> float:
    """What gudmc reads back for a D that tajima_d printed with parse_f64_roundup_and_own(x, 8) (tajima_d.rs:164)."""
    x = float(x)
    if math.isnan(x) or math.isinf(x):
        return x
    return float(rustfmt.roundup_own(x, 8))


def normal_cdf(x: float, mean: float, sd: float) -> float:
    """statrs Normal::cdf"""
    return 0.5 * math.erfc((mean - x) / (sd * math.sqrt(2.0)))


def one_tail(x: float, mean: float, sd: float) -> float:
    """gudmc.rs:353-357, :370-374"""
    if math.isnan(x):
        return math.nan
    return normal_cdf(x, mean, sd) if x < mean else 1.0 - normal_cdf(x, mean, sd)


def width_scan(d, mean, chrom, ini, fin, thr):
    """gudmc.rs:168-208 for one population: d = its non-NaN D; row j takes the label of window j of the unfiltered list."""
    width = []
    for j in range(len(d)):
        if abs(d[j] - mean) >= thr:
            wj = int(fin[j]) - int(ini[j])
            if j > 0 and chrom[j] == chrom[j - 1] and int(ini[j]) <= int(fin[j - 1]):
                wj += width[j - 1]
            width.append(wj)
        else:
            width.append(0)
    return width


def gudmc_stage(d_win, fst_win, chrom, ini, fin, sigma_threshold=2.0, rate=0.73, reverse=False, cost="sum"):
    """gudmc.rs:124-378 from the two tables: a dict of what pg_gudmc_dev returns, the per-row values as lists per pair."""
    d_win = np.asarray(d_win, dtype=np.float64)
    fst_win = np.asarray(fst_win, dtype=np.float64)
    w, n = d_win.shape
    assert fst_win.shape == (w, n * n)
    pops = []
    for b in range(n):
        d = [round8(v) for v in d_win[:, b]]
        d = [v for v in d if not math.isnan(v)]
        mu, sd, it = fit_normal(d, reverse, cost)
        width = width_scan(d, mu, chrom, ini, fin, sigma_threshold)
        wmu, wsd, wit = fit_normal([float(x) for x in width], reverse, cost)
        pops.append(dict(d=d, mean=mu, sd=sd, iters=it, width=width, width_mean=wmu, width_sd=wsd, width_iters=wit))
    rec = (rate / 100.0) * 1.0e6
    out = dict(rows=[len(p["d"]) for p in pops], d_mean=[p["mean"] for p in pops], d_sd=[p["sd"] for p in pops],
               fst_mean=[], fst_sd=[], fst_iters=[], width_mean=[], width_sd=[], window=[], d=[], width=[], width_dev=[],
               width_p=[], fst_delta=[], fst_p=[])
    for i in range(n * n):
        p = pops[i % n]
        fm, fs, fit = fit_column(fst_win[:, i], reverse, cost)
        out["fst_mean"].append(fm); out["fst_sd"].append(fs); out["fst_iters"].append(fit)
        out["width_mean"].append(p["width_mean"]); out["width_sd"].append(p["width_sd"])
        rows = len(p["d"])
        out["window"].append(list(range(rows)))
        out["d"].append(list(p["d"]))
        out["width"].append([float(x) for x in p["width"]])
        out["width_dev"].append([float(x) - rec for x in p["width"]])
        out["width_p"].append([one_tail(float(x), p["width_mean"], p["width_sd"]) for x in p["width"]])
        out["fst_delta"].append([float(fst_win[j, i]) - fm for j in range(rows)])
        out["fst_p"].append([one_tail(float(fst_win[j, i]), fm, fs) for j in range(rows)])
    out["pops"] = pops
    return out


def csv_rows(res, pool_names, chrom_names, ini, fin):
    """The lines of the output file after the header (gudmc.rs:433-456): a list of 15 fields each."""
    n = len(pool_names)
    lines = []
    r7 = lambda x: rustfmt.roundup_own(x, 7)
    for i in range(n * n):
        a, b = divmod(i, n)
        for j in range(res["rows"][b]):
            lines.append([pool_names[a], pool_names[b], chrom_names[j], str(int(ini[j])), str(int(fin[j])),
                          r7(res["d_mean"][b]), r7(res["fst_mean"][i]), r7(res["d_sd"][b]), r7(res["fst_sd"][i]),
                          rustfmt.display(res["d"][i][j]), rustfmt.display(res["width"][i][j]),
                          rustfmt.display(res["width_dev"][i][j]), r7(res["width_p"][i][j]), r7(res["fst_delta"][i][j]),
                          r7(res["fst_p"][i][j])])
    return lines


# ---- the corpus of the tests ---------------------------------------------------------------------------------------------

FIT_ROWS, FIT_COLS = 48, 130


@functools.lru_cache(maxsize=None)
def fit_table():
    """One 48 x 130 table: non-NaN counts 0, 1, 2, 3, 12 and 40 with the NaN interleaved, a constant column, then D-like,
    Fst-like (values in [0, 1]) and width-like (mostly 0, a few in 20..400) columns of 2..40 values.  Returns (table,
    {column: constant value} for the columns whose every value is the same)."""
    rng = np.random.default_rng(20240611)
    t = np.full((FIT_ROWS, FIT_COLS), np.nan)
    const = {}

    def put(c, vals):
        at = np.sort(rng.choice(FIT_ROWS, size=len(vals), replace=False))  # NaN in between
        t[at, c] = vals

    def kind(c, k, cnt):
        if k == 0:
            return rng.normal(rng.normal(0.0, 0.5), rng.uniform(0.3, 1.5), size=cnt)
        if k == 1:
            return np.clip(rng.beta(2.0, 8.0, size=cnt) + rng.uniform(0.0, 0.3), 0.0, 1.0)
        v = np.zeros(cnt)
        hit = rng.choice(cnt, size=max(1, cnt // 5), replace=False)
        v[hit] = rng.integers(20, 401, size=len(hit)).astype(np.float64)
        return v

    for c, cnt in enumerate((0, 1, 2, 3, 12, 40)):
        put(c, kind(c, 0, cnt))
    const[1] = float(t[~np.isnan(t[:, 1]), 1][0])
    put(6, np.full(12, 0.37)); const[6] = 0.37
    for c in range(7, FIT_COLS):
        put(c, kind(c, c % 3, int(rng.integers(2, 41))))
    # width-like columns whose few non-zero draws left them constant would be degenerate: there are none by construction
    for c in range(7, FIT_COLS):
        v = t[~np.isnan(t[:, c]), c]
        assert len(set(v.tolist())) > 1, c
    t.setflags(write=False)
    return t, const


def make_stage_case(seed: int, n: int, w: int, overlap: bool, thr: float = 0.4, all_insignificant: bool = False):
    """Synthetic tables of the stage: w windows on two chromosomes (100 bp every 50 bp, or 60..100 bp every 150 bp), D ~ N(0, 1)
    in runs, Fst in [0, 1] with a zero diagonal and one NaN; population 1 has a NaN window in the middle, population n - 1 only
    NaN windows.  The seed is advanced until every population with rows has a run of >= 3 significant windows and two distinct
    non-zero widths (decided on the restatement's own scan around the sample mean)."""
    half = w // 2
    chrom = np.array([0] * half + [1] * (w - half), dtype=np.int32)
    for s in range(seed, seed + 1000):
        rng = np.random.default_rng(s)
        step = 50 if overlap else 150
        ini = np.concatenate([1 + step * np.arange(half), 7 + step * np.arange(w - half)]).astype(np.uint64)
        fin = (ini + rng.integers(60, 100, size=w).astype(np.uint64)).astype(np.uint64)
        d = rng.normal(0.0, 1.0, size=(w, n)) + np.repeat(rng.normal(0.0, 0.8, size=((w + 2) // 3, n)), 3, axis=0)[:w]
        if all_insignificant:
            d = rng.normal(0.0, 0.05, size=(w, n))
        d[w // 2, 1] = np.nan
        d[:, n - 1] = np.nan
        base = rng.uniform(0.05, 0.4, size=(n, n))
        fst = np.clip(base.reshape(1, n * n) + rng.normal(0.0, 0.08, size=(w, n * n)), 0.0, 1.0)
        for a in range(n):
            fst[:, a * n + a] = 0.0
        fst[w // 3, 1] = np.nan
        if all_insignificant:
            return dict(n=n, w=w, d=d, fst=fst, chrom=chrom, ini=ini, fin=fin, thr=thr, rate=0.73)
        ok = True
        for b in range(n - 1):
            col = [round8(v) for v in d[:, b] if not math.isnan(v)]
            m = sum(col) / len(col)
            wd = width_scan(col, m, chrom, ini, fin, thr)
            sig = [abs(v - m) >= thr for v in col]
            run = best = 0
            for j, f in enumerate(sig):
                run = run + 1 if f and (j == 0 or (sig[j - 1] and chrom[j] == chrom[j - 1])) else (1 if f else 0)
                best = max(best, run)
            # values within 1e-3 of the threshold could fall on the other side with the fitted mean: keep clear of them
            clear = all(abs(abs(v - m) - thr) > 1e-3 for v in col)
            ok = ok and best >= 3 and len({x for x in wd if x > 0}) >= 2 and clear
        if ok:
            return dict(n=n, w=w, d=d, fst=fst, chrom=chrom, ini=ini, fin=fin, thr=thr, rate=0.73)
    raise AssertionError("no seed gives the runs the stage tests need")


STAGE_SHAPES = ((3, 12, True), (4, 40, False), (3, 40, True), (4, 12, False))


@functools.lru_cache(maxsize=None)
def stage_cases():
    return tuple(make_stage_case(100 * k, n, w, ov, thr=(0.3, 0.5, 0.4, 0.45)[k]) for k, (n, w, ov) in enumerate(STAGE_SHAPES))


@functools.lru_cache(maxsize=None)
def insignificant_case():
    return make_stage_case(7, 3, 12, True, thr=2.0, all_insignificant=True)


@functools.lru_cache(maxsize=None)
def fit_table_reference(reverse: bool = False):
    """(mu, sigma, iterations) of every column of fit_table() by the restatement."""
    t, _ = fit_table()
    return tuple(fit_column(t[:, c].tolist(), reverse) for c in range(t.shape[1]))


@functools.lru_cache(maxsize=None)
def stage_reference(k: int, reverse: bool = False):
    c = stage_cases()[k] if k >= 0 else insignificant_case()
    return gudmc_stage(c["d"], c["fst"], c["chrom"], c["ini"], c["fin"], c["thr"], c["rate"], reverse)


def spread(fwd, rev):
    """(largest |d mu| / sigma, largest |d sigma| / sigma) over pairs of (mu, sigma, ..) with a forward sigma above 1e-12."""
    dm = ds = 0.0
    for a, b in zip(fwd, rev):
        if a[1] <= DEGENERATE_SD:
            continue
        dm = max(dm, abs(a[0] - b[0]) / a[1])
        ds = max(ds, abs(a[1] - b[1]) / a[1])
    return dm, ds


def stage_fits(res):
    """every fit of a stage result as (mu, sigma): D per population, Fst per pair, width per population"""
    return (list(zip(res["d_mean"], res["d_sd"])) + list(zip(res["fst_mean"], res["fst_sd"])) +
            [(p["width_mean"], p["width_sd"]) for p in res["pops"]])
