"""watterson_estimator (popgen/watterson_theta.rs:8-289) and tajima_d (popgen/tajima_d.rs:10-171) restated in numpy / plain
Python for the tests: the oracle has neither.  Everything the oracle has (theta_pi, sliding windows, count_loci, the two
number formats) is taken from it.  Conventions are the oracle's: Xt is (1 + p) x n with the intercept row first, loci_idx
the column starts of count_loci (so locus l is rows loci_idx[l] .. loci_idx[l + 1] of Xt).

Every arithmetic step is one IEEE double operation in the reference's order; `powf` is libm's pow = math.pow."""
import math

import numpy as np

EPS = np.finfo(np.float64).eps   # f64::EPSILON


def poly_flags(Xt, loci_idx):
    """polymorphic_loci_per_pool (:8-30) for every locus: L x n of 0 / 1.  The fold starts from 0.0 and replaces the
    maximum only where x > max, so a NaN never wins; the flag is max < 1.0."""
    Xt = np.asarray(Xt, dtype=np.float64)
    L, n = len(loci_idx) - 1, Xt.shape[1]
    out = np.zeros((L, n), dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for l in range(L):
            m = np.zeros(n)
            for c in range(loci_idx[l], loci_idx[l + 1]):
                x = Xt[c]
                m = np.where(x > m, x, m)
            out[l] = m < 1.0
    return out


def watterson_windows(chrom, pos, window_size_bp, window_slide_size_bp, min_loci_per_window):
    """The loop of theta_watterson (:56-164), line for line.  Instead of the polymorphic counts themselves each slot
    keeps the list of locus indices at which polymorphic_loci_per_pool was evaluated for it (`terms`): S is the sum of
    the flags at those indices.  Returns (head, tail, cov, seed, slot, terms) of the kept windows; seed = terms[0], and
    every later term is the slot's index (asserted)."""
    l = len(chrom)
    idx_head, idx_tail = [0], [0]
    chr_head, pos_head = [chrom[0]], [pos[0]]
    cov = [1]
    marker_next_window_head = False
    idx_next_head = 0
    i = 1
    terms = [[0]]                                                   # :74-75
    while i < l:
        c, p = chrom[i], pos[i]
        if c != chr_head[-1] or p > pos_head[-1] + window_size_bp:  # :84
            i = idx_next_head if marker_next_window_head else i     # :89-93
            c, p = chrom[i], pos[i]
            if cov[-1] >= min_loci_per_window:                      # :97-109
                idx_head.append(i); idx_tail.append(i)
                chr_head.append(c); pos_head.append(p)
                cov.append(1)
                terms.append([i])
            else:                                                   # :110-120
                i_ = len(idx_head) - 1
                idx_head[i_] = i
                chr_head[i_] = c; pos_head[i_] = p
                cov[i_] = 1
                terms[i_] = [i_]
            marker_next_window_head = False
        else:                                                       # :123-145
            i_ = len(idx_tail) - 1
            idx_tail[i_] = i
            cov[i_] += 1
            terms[i_].append(i_)
            if not marker_next_window_head and p >= pos_head[-1] + window_slide_size_bp:
                marker_next_window_head = True
                idx_next_head = i
        i += 1
    keep, out_tail = [0], [idx_tail[0]]                             # :152-164
    for w in range(1, len(idx_head)):
        if idx_tail[w] != out_tail[-1]:
            keep.append(w); out_tail.append(idx_tail[w])
    for w in keep:
        assert len(terms[w]) == cov[w] and all(t == w for t in terms[w][1:])
    a = lambda v: np.array([v[w] for w in keep], dtype=np.int64)
    return a(idx_head), a(idx_tail), a(cov), np.array([terms[w][0] for w in keep], dtype=np.int64), np.array(keep, dtype=np.int64), \
        [terms[w] for w in keep]


def segregating_sites(flags, head, tail, terms=None):
    """S per (window, pool) and the divisor cov: reference mode sums the flags at `terms`; counted mode (terms None) sums
    the window's own loci."""
    nw = len(head)
    S = np.zeros((nw, flags.shape[1]), dtype=np.int64)
    cov = np.zeros(nw, dtype=np.int64)
    for w in range(nw):
        idx = list(range(head[w], tail[w] + 1)) if terms is None else terms[w]
        for t in idx:
            S[w] += flags[t]
        cov[w] = len(idx)
    return S, cov


def as_usize(x):
    """Rust's `f64 as usize`: truncation, saturating, NaN -> 0"""
    x = float(x)
    if not x >= 1.0:
        return 0
    return min(int(x), 2 ** 64 - 1)


def constants(pool_size):
    """a1, a2, b1, b2, c1, c2, e1, e2 of tajima_d.rs:52-61 for one pool"""
    f = np.float64
    with np.errstate(all="ignore"):
        m = as_usize(pool_size)
        a1, a2 = f(0.0), f(0.0)
        for x in range(1, m):
            a1 = a1 + f(1.0) / f(x)
        for x in range(1, m):
            a2 = a2 + f(1.0) / f(math.pow(float(x), 2.0))
        n = f(m)
        b1 = (n + f(1.0)) / (f(3.0) * (n - f(1.0)))
        b2 = (f(2.0) * (f(math.pow(n, 2.0)) + n + f(3.0))) / (f(9.0) * n * (n - f(1.0)))
        c1 = b1 - (f(1.0) / a1)
        c2 = b2 - ((n + f(2.0)) / (a1 * n)) + (a2 / f(math.pow(a1, 2.0)))
        e1 = c1 / a1
        e2 = c2 / (f(math.pow(a1, 2.0)) + a2)
    return a1, a2, b1, b2, c1, c2, e1, e2


def mean_across_windows(win):
    """mean_axis(Axis(0)): summed left to right over the windows, divided by their number"""
    with np.errstate(all="ignore"):
        s = np.zeros(win.shape[1])
        for w in range(win.shape[0]):
            s = s + win[w]
        return s / np.float64(win.shape[0])


def theta_watterson(S, cov, pool_sizes):
    """(S as f64 / cov as f64) / a1 (:175-182) -> (per window [nw x n], mean across windows [n])"""
    a1 = np.array([constants(p)[0] for p in pool_sizes])
    with np.errstate(all="ignore"):
        theta = (S.astype(np.float64) / cov.astype(np.float64)[:, None]) / a1[None, :]
    return theta, mean_across_windows(theta)


def tajima_d(theta, pi, pool_sizes):
    """tajima_d.rs:62-96 -> (D per window [nw x n], mean across windows [n]); the branch order is the reference's, and a
    NaN fails every comparison and reaches the division."""
    k = [constants(p) for p in pool_sizes]
    a1 = np.array([c[0] for c in k])[None, :]; e1 = np.array([c[6] for c in k])[None, :]; e2 = np.array([c[7] for c in k])[None, :]
    with np.errstate(all="ignore"):
        s = np.where(theta <= EPS, 0.0, theta / a1)
        vd = (e1 * s) + ((e2 * s) * (s - 1.0))
        d = np.where(np.abs(pi - theta) <= EPS, 0.0, np.where(vd <= EPS, 0.0, (pi - theta) / np.sqrt(vd)))
    return d, mean_across_windows(d)


def file_text(oracle, names, win, mean, lc, lp, head, tail):
    """the CSV of watterson_estimator (:254-287) / tajima_d (:137-169): the lines without their newlines"""
    want = ["Pool,Mean_across_windows," + ",".join(f"Window-{lc[h]}_{lp[h]}_{lp[t]}" for h, t in zip(head, tail))]
    for i, name in enumerate(names):
        want.append(name + "," + oracle.fmt(mean[i]) + "," + ",".join(oracle.round_own(x, 8) for x in win[:, i]))
    return want
