"""Checker of fisher_exact_test: a line-by-line restatement of tables::fisher (tables/fisher_exact_test.rs:6-130) on an
already filtered n x p table of counts, and the compacted enumeration the GPU kernel's argument rests on.  Pure
numpy / math; the filter itself is the oracle's (oracle_lib.filter_locus)."""
import math

import numpy as np


def factorial_log10(x):
    """fisher_exact_test.rs:6-18"""
    if x > 34.0:
        raise ValueError("Input is far too big")
    out = 0.0
    for i in range(2, int(x + 1.0)):
        out = out + math.log10(float(i))
    return out


F = [factorial_log10(float(i)) for i in range(35)]


def hypergeom_ratio(c, lp):
    """fisher_exact_test.rs:20-30; c: 2-d array of cell values <= 34 (row-major iteration)."""
    s = 0.0
    for v in np.asarray(c).ravel():
        s = s + F[int(v)]
    s = s + F[int(np.asarray(c).sum())]
    return 10.0 ** (lp - s)


def scaled(mat):
    """:38-58: counts as f64, scaled to at most 34 reads with ONE division and, per cell, one multiply and floor."""
    c = np.asarray(mat).astype(np.float64).copy()
    tot = c.sum()
    if tot > 34.0:
        coef = 34.0 / tot
        c = np.floor(c * coef)
    return c


def _marginals(c):
    rs = c.sum(1)
    cs = c.sum(0)
    lp = 0.0
    for r in rs:
        lp = lp + F[int(r)]
    for q in cs:
        lp = lp + F[int(q)]
    return rs, cs, lp


class MarginalsBroken(AssertionError):
    """The reference's assert at :113-114 would fire."""


def fisher(mat):
    """The literal restatement: (p_observed, p_observed + p_extremes) of an n x p table of filtered counts.
    O((n p)^2) slice sums and more, like the reference."""
    c = scaled(mat)
    n, p = c.shape
    rs, cs, lp = _marginals(c)
    pobs = hypergeom_ratio(c, lp)
    pext = 0.0
    for mi in range(n):
        for mj in range(p):
            for i in range(n):
                for j in range(p):
                    a = rs[i] - c[i, :j].sum()
                    b = cs[j] - c[:i, j].sum()
                    mx = float(min(max(int(a), 0), max(int(b), 0)))  # `as usize`: negative -> 0
                    if i == n - 1 or j == p - 1:
                        c[i, j] = mx
                    elif i < mi or j < mj:
                        c[i, j] = 0.0
                    else:
                        c[i, j] = mx
            for ij in range(p):
                for ii in range(n):
                    j = p - (ij + 1)
                    i = n - (ii + 1)
                    a = rs[i] - c[i, :].sum()
                    b = cs[j] - c[:, j].sum()
                    mx = float(min(max(int(a), 0), max(int(b), 0)))
                    if mx > 0.0:
                        c[i, j] = mx
            if not (np.array_equal(rs, c.sum(1)) and np.array_equal(cs, c.sum(0))):
                raise MarginalsBroken(f"max_i={mi} max_j={mj} table={np.asarray(mat).tolist()}")
            pext += hypergeom_ratio(c, lp)
    return pobs, pobs + pext


def fisher_compact(mat):
    """The same two numbers from the non-zero rows / columns of the scaled table only: one table per (t_r, t_c) = (non-zero
    rows before max_i, non-zero columns before max_j), weighted by the number of (max_i, max_j) that map to it.  "Last row /
    column" are the TRUE last pool / allele: if that one is all zero after scaling, no compacted row / column is last."""
    c = scaled(mat)
    n, p = c.shape
    rs, cs, lp = _marginals(c)
    pobs = hypergeom_ratio(c, lp)
    R = [i for i in range(n) if rs[i] > 0]
    Cc = [j for j in range(p) if cs[j] > 0]
    rr, cc = rs[R], cs[Cc]
    nr, nc = len(R), len(Cc)
    lastr = nr - 1 if (nr and R[-1] == n - 1) else -1
    lastc = nc - 1 if (nc and Cc[-1] == p - 1) else -1
    mr = np.zeros(nr + 1, dtype=np.int64)
    for mi in range(n):
        mr[sum(1 for i in R if i < mi)] += 1
    mc = np.zeros(nc + 1, dtype=np.int64)
    for mj in range(p):
        mc[sum(1 for j in Cc if j < mj)] += 1
    ntot = int(c.sum())
    pext = 0.0
    for tr in range(nr + 1):
        if mr[tr] == 0:
            continue
        for tc in range(nc + 1):
            if mc[tc] == 0:
                continue
            t = np.zeros((nr, nc))
            rrem, crem = rr.copy(), cc.copy()
            for i in range(nr):
                for j in range(nc):
                    mx = min(rrem[i], crem[j])
                    v = mx if (i == lastr or j == lastc or not (i < tr or j < tc)) else 0.0
                    t[i, j] = v
                    rrem[i] -= v
                    crem[j] -= v
            for j in range(nc - 1, -1, -1):
                for i in range(nr - 1, -1, -1):
                    a = rr[i] - t[i].sum()
                    b = cc[j] - t[:, j].sum()
                    mx = min(max(a, 0.0), max(b, 0.0))
                    if mx > 0:
                        t[i, j] = mx
            s = 0.0
            for v in t.ravel():
                s = s + F[int(v)]
            s = s + F[ntot]
            pext += float(mr[tr] * mc[tc]) * 10.0 ** (lp - s)
    return pobs, pobs + pext


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)
