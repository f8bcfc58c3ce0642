"""Literal restatement of the reference's imputation (src/imputation/: filtering_missing.rs, mean_imputation.rs,
adaptive_ld_knn_imputation.rs), quirks included, on the loader's matrix.  Test-side only.

Orientation: the reference's matrix is n x (1 + p) with an intercept column; here G is p x n (a row per allele column, no
intercept) and cov is L x n (a row per locus).  locus_col (L + 1 entries, 0 .. p) is count_loci (sync.rs:73-97) minus the
intercept.  Sums follow the reference's orders: sequential folds where it folds, ndarray's 8-lane sum where it calls sum().
"""
from __future__ import annotations

import math

import numpy as np

EPS = 2.220446049250313e-16
NAN = float("nan")
INF = float("inf")


class NothingLeft(Exception):
    pass


def ndsum(oracle, xs) -> float:
    a = np.ascontiguousarray(xs, dtype=np.float64)
    return oracle.lib.orc_ndarray_sum(a.ctypes.data, len(a))


# ---- filtering_missing.rs ---------------------------------------------------------------------------------------------
def missing_rate(oracle, cov) -> float:
    """:7-13"""
    l, n = cov.shape
    return oracle.lib.orc_sensible_round(float(np.isnan(cov).sum()) * 100.0 / float(n * l), 2)


def set_missing_by_depth(G, cov, locus_col, min_depth):
    """:15-44.  The last locus keeps its frequencies (idx_fin = loci_idx[l - 1] is its own start); its coverage still goes."""
    G = G.copy(); cov = cov.copy()
    L, n = cov.shape
    for i in range(n):
        for j in range(L):
            if cov[j, i] < min_depth:
                cov[j, i] = NAN
                ini = locus_col[j]
                fin = locus_col[j + 1] if j < L - 1 else locus_col[L - 1]
                for k in range(ini, fin):
                    G[k, i] = NAN
    return G, cov


def top_missing_keep(missingness, frac):
    """the keep rule of :63-86 and :146-170: indices kept, ascending"""
    N = len(missingness)
    n_missing = 0.0
    for x in missingness:
        if x > 0.0:
            n_missing += 1.0
    left = N - int(math.ceil(n_missing * frac))
    if left <= 0:
        raise NothingLeft()
    idx = sorted(range(N), key=lambda a: missingness[a])   # stable, as sort_by is
    return sorted(idx[:left])


def filter_out_top_missing_pools(G, cov, frac):
    """:46-122 -> G, cov, kept pool indices"""
    p, n = G.shape
    miss = [float(int(np.isnan(G[:, i]).sum())) / float(p) for i in range(n)]
    keep = top_missing_keep(miss, frac)
    return G[:, keep].copy(), cov[:, keep].copy(), keep


def filter_out_top_missing_loci(G, cov, locus_col, frac):
    """:125-226 -> G, cov, locus_col, kept locus indices.  Works on the NaN of cov."""
    L, n = cov.shape
    miss = [float(int(np.isnan(cov[l]).sum())) / float(n) for l in range(L)]
    keep = top_missing_keep(miss, frac)
    rows = [k for l in keep for k in range(locus_col[l], locus_col[l + 1])]
    new_lc = [0]
    for l in keep:
        new_lc.append(new_lc[-1] + locus_col[l + 1] - locus_col[l])
    return G[rows].copy(), cov[keep].copy(), new_lc, keep


def mark_coverages(cov):
    """mean_imputation.rs:42-59 = adaptive_ld_knn_imputation.rs:347-363"""
    cov = cov.copy()
    for l in range(cov.shape[0]):
        if (~np.isnan(cov[l])).any():
            cov[l][np.isnan(cov[l])] = INF
    return cov


# ---- mean_imputation.rs -----------------------------------------------------------------------------------------------
def mean_imputation(oracle, G, locus_col):
    """:6-41"""
    G = G.copy()
    L = len(locus_col) - 1
    n = G.shape[1]
    for l in range(L):
        ini, fin = locus_col[l], locus_col[l + 1]
        means = []
        for k in range(ini, fin):       # mean_axis_ignore_nan (helpers.rs:267-291): fold in pool order, then sum / count
            s, c = 0.0, 0.0
            for x in G[k].tolist():
                if x == x:
                    s = s + x; c += 1.0
            means.append(s / c if c > 0 else NAN)
        tot = ndsum(oracle, means)
        if tot != 1.0:
            with np.errstate(all="ignore"):
                means = (np.array(means) / np.float64(tot)).tolist()
        for a, k in enumerate(range(ini, fin)):
            for i in range(n):
                if G[k, i] != G[k, i]:
                    G[k, i] = means[a]
    return G


# ---- adaptive_ld_knn_imputation.rs ------------------------------------------------------------------------------------
def _key(x):
    return INF if x != x else x


def linked_columns(corr_col, K):
    """:17-36: stable sort by correlation, descending, NaN as +inf; the first K"""
    p = len(corr_col)
    K = min(p, K)
    return sorted(range(p), key=lambda j: -_key(corr_col[j]))[:K]


def euclidean_distances(oracle, W, links):
    """:38-73 on the current W (p_w x n) -> (dist n x n, all_missing)"""
    n = W.shape[1]
    dist = np.full((n, n), NAN)
    sel = W[links]
    all_missing = True
    for i0 in range(n):
        a = sel[:, i0]
        for i1 in range(i0, n):
            b = sel[:, i1]
            m = ~np.isnan(a) & ~np.isnan(b)
            if not m.any():
                continue
            d = a[m] - b[m]
            d = math.sqrt(ndsum(oracle, d * d))
            if d != d:
                continue
            dist[i0, i1] = d; dist[i1, i0] = d
            all_missing = False
    return dist, all_missing


def count_over_n(col):
    """mean_value_imputation (:76-82): the NUMBER of non-missing values over the length, as written"""
    s = 0.0
    for x in col:
        if x == x:
            s = s + 1.0
    return s / float(len(col))


def find_k_nearest_neighbours(k, col, dist_col):
    """:84-134 -> (values, distances) of the neighbours kept"""
    n = len(col)
    if k > n:
        raise ValueError("k_neighbours exceeds the number of pools")   # select(0..k) panics
    idx = sorted(range(n), key=lambda q: _key(dist_col[q]))
    fs = [col[q] for q in idx]
    fk = fs[:k]
    while k < n:
        if any(x != x for x in fk):
            break
        fk = fs[:k]
        k += 1
    dk = [dist_col[idx[t]] for t in range(k)]
    pairs = [(x, y) for x, y in zip(fk, dk) if x == x and y == y]
    return [x for x, _ in pairs], [y for _, y in pairs]


def impute_window(oracle, W, starts, K_links, k_neighbours):
    """One window's closure (:209-321).  W: pristine copy p_w x n; starts: local start columns of the window's loci plus
    the trailing p_w.  Returns the imputed copy."""
    pw, n = W.shape
    corr = np.full((pw, pw), NAN)
    need = [j for j in range(pw) if np.isnan(W[j]).any()]
    for j in need:                      # only the columns of corr that are read (the matrix is symmetric)
        for c in range(pw):
            j0, j1 = min(j, c), max(j, c)
            corr[c, j] = oracle.pearson(W[j0], W[j1])[0]
    W = W.copy()
    last_of = {starts[t] - 1: starts[t - 1] for t in range(1, len(starts))}
    for j in need:
        links = linked_columns(corr[:, j], K_links)
        dist, all_missing = euclidean_distances(oracle, W, links)
        for i in range(n):
            if W[j, i] == W[j, i]:
                continue
            if all_missing:
                W[j, i] = count_over_n(W[j].tolist())
            else:
                vals, ds = find_k_nearest_neighbours(k_neighbours, W[j].tolist(), dist[:, i].tolist())
                if len(vals) == 0:
                    W[j, i] = count_over_n(W[j].tolist())
                else:
                    dist_sum = 0.0
                    for d in ds:
                        dist_sum = dist_sum + d
                    dist_sum = dist_sum + EPS
                    w = [1.0 - (d / dist_sum) + EPS for d in ds]
                    ws = 0.0
                    for x in w:
                        ws = ws + x
                    w = [x / ws for x in w]
                    W[j, i] = ndsum(oracle, [v * x for v, x in zip(vals, w)])
            if j > 0 and j in last_of:  # correct_allele_frequencies_per_locus (:136-171)
                j_ini = last_of[j]
                s = 0.0
                for x in W[j_ini:j + 1, i].tolist():
                    if x == x:
                        s = s + x
                s = s + EPS
                if s != 1.0:
                    for jj in range(j_ini, j + 1):
                        W[jj, i] = W[jj, i] / s
    return W


def adaptive_ld_knn_imputation(oracle, G, locus_col, head, tail, K_links, k_neighbours):
    """:174-341: every window on its own copy of the input, written back in window order"""
    if k_neighbours > G.shape[1]:
        raise ValueError("k_neighbours exceeds the number of pools")
    out = G.copy()
    copies = []
    for a in range(len(head)):
        ini, fin = locus_col[head[a]], locus_col[tail[a] + 1]
        starts = [locus_col[l] - ini for l in range(head[a], tail[a] + 2)]
        copies.append((ini, fin, impute_window(oracle, G[ini:fin], starts, K_links, k_neighbours)))
    for ini, fin, W in copies:
        out[ini:fin] = W
    return out


# ---- impute_mean / impute_aLDkNN --------------------------------------------------------------------------------------
def impute(oracle, G, cov, locus_col, chrom, pos, method, min_depth=5.0, frac_pools=0.1, frac_loci=0.1, window_size_bp=100,
           window_slide_size_bp=50, min_loci_per_window=10, n_loci_to_estimate_distance=10, k_neighbours=5, trace=None):
    """mean_imputation.rs:65-162 / adaptive_ld_knn_imputation.rs:371-477 up to the writer.  chrom / pos: per locus.
    Returns dict(G, cov, pools, loci, locus_col): the imputed table, the kept pools and the kept loci (input indices).
    `trace` (a list) receives (rows, cols, missing_rate) after every step, as the progress lines print them."""
    def note(c):
        if trace is not None:
            trace.append((c.shape[1], c.shape[0], missing_rate(oracle, c)))
    locus_col = [int(x) for x in locus_col]
    note(cov)
    G, cov = set_missing_by_depth(G, cov, locus_col, min_depth); note(cov)
    G, cov, pools = filter_out_top_missing_pools(G, cov, frac_pools); note(cov)
    G, cov, locus_col, loci = filter_out_top_missing_loci(G, cov, locus_col, frac_loci); note(cov)
    if method == "mean":
        G = mean_imputation(oracle, G, locus_col)
    else:
        head, tail = oracle.sliding_windows([chrom[l] for l in loci], [pos[l] for l in loci], window_size_bp,
                                            window_slide_size_bp, min_loci_per_window)
        G = adaptive_ld_knn_imputation(oracle, G, locus_col, head.tolist(), tail.tolist(), n_loci_to_estimate_distance,
                                       k_neighbours)
    cov = mark_coverages(cov); note(cov)
    G, cov, locus_col, keep2 = filter_out_top_missing_loci(G, cov, locus_col, 1.0); note(cov)
    loci = [loci[l] for l in keep2]
    return dict(G=G, cov=cov, pools=pools, loci=loci, locus_col=locus_col)


# ---- the fixture through the oracle's loader steps --------------------------------------------------------------------
_fixture_memo = {}


def load_fixture(oracle, remove_ns, min_cov, maf, miss=0.0, max_loci=None):
    """tests/golden/test.sync as into_genotypes_and_phenotypes(keep_p_minus_1 = false) leaves it: dict(G p x n, cov L x n,
    locus_col, chrom, pos (per kept locus), alleles (per column, index into ATCGND), names)."""
    import csv_expect as E
    key = (remove_ns, min_cov, maf, miss, max_loci)
    if key in _fixture_memo:
        return _fixture_memo[key]
    counts, chrom_ids, pos, names, order = E.golden_fixture(oracle)
    ps = np.full(5, 20.0)
    fo = oracle.filt(remove_ns, min_cov, maf, miss)
    rows, covs, lc, ch, po, al = [], [], [0], [], [], []
    for l in order:
        if max_loci is not None and len(ch) >= max_loci:
            break
        res = oracle.filter_locus(counts[l], ps, fo)
        if res is None:
            continue
        ids, fc = res
        fr = oracle.to_frequencies(fc)
        for j, a in enumerate(ids):
            rows.append(fr[:, j]); al.append(int(a))
        covs.append(fc.sum(axis=1).astype(np.float64))     # sync.rs:1129-1152
        lc.append(len(rows)); ch.append(names[chrom_ids[l]]); po.append(int(pos[l]))
    out = dict(G=np.array(rows), cov=np.array(covs), locus_col=lc, chrom=ch, pos=po, alleles=al, names=names)
    _fixture_memo[key] = out
    return out
