"""The launch rules of the popgen kernels (pg_popgen.hip) on both sides of their edges, against the oracle (fst, theta_pi) and the
restatement of watterson_estimator / tajima_d (tests/popgen_diversity_restated.py): the 32 x 32 pool-pair tiles of k_fst_ranges, the
chunks of the genome-wide mean, the slabs of the per-window table, and the one-thread-per-(window, pool) kernels at block
boundaries.  G, the coverages and locus_col are handed to the engine directly, so the shapes do not depend on the loader: dyadic
frequencies a / 64, b / 64, 1 - (a + b) / 64 (they sum to one exactly, as k_pop_check demands), whole-number coverages, ~30 % of the
loci tri-allelic, ~15 % of the cells fixed (frequency exactly 1.0), and a row pitch ld > n with NaN in the padding columns of G and
of the coverages, which the oracle never sees.  Tolerances are those of tests/test_gpu_popgen.py: the per-window table and pi bit
for bit, the genome-wide mean rtol 1e-12 / atol 1e-15 (chunked partial sums instead of one left-to-right sum)."""
import numpy as np
import pytest
import torch

import dispatch_rules as R
import popgen_diversity_restated as D
from test_gpu_popgen_diversity import restate, same

pytestmark = pytest.mark.gpu


def build(n, L, seed):
    """-> G, cov (p x ld on the device), starts (locus_col), Xt ((1 + p) x n), loci_idx, covs (L x n)"""
    rng = np.random.default_rng(seed)
    ld = n + 2 + (n & 1)
    nall = np.where(rng.random(L) < 0.3, 3, 2)
    starts = np.concatenate([[0], np.cumsum(nall)]).astype(np.int64)
    p = int(starts[-1])
    a = np.where(rng.random((L, n)) < 0.15, 64, rng.integers(1, 64, size=(L, n)))
    b = np.where(nall[:, None] == 3, rng.integers(0, 64, size=(L, n)) % (65 - a), 64 - a)      # third allele: 64 - a - b >= 0
    depth = rng.integers(20, 90, size=(L, n)).astype(np.float64)
    G = np.full((p, ld), np.nan)
    cov = np.full((p, ld), np.nan)
    first, tri = starts[:-1], nall == 3
    G[first, :n] = a / 64.0
    G[first + 1, :n] = b / 64.0
    G[first[tri] + 2, :n] = (64 - a[tri] - b[tri]) / 64.0
    for j in range(3):
        rows = first[nall > j] + j
        cov[rows, :n] = depth[nall > j]
    assert not np.isnan(G[:, :n]).any() and np.isnan(G[:, n:]).all() and np.isnan(cov[:, n:]).all() and ld > n
    Xt = np.vstack([np.ones(n), G[:, :n]])
    return torch.from_numpy(G).cuda(), torch.from_numpy(cov).cuda(), starts, Xt, (starts + 1).tolist(), depth


def pool_sizes(n):
    return (2 + (np.arange(n) * 7) % 41).astype(np.float64)


def check_fst_and_pi(engine, oracle, case, wh, wt, n, what):
    G, cov, starts, Xt, loci_idx, covs = case
    rc, rmean, rwin = oracle.fst(Xt, loci_idx, covs, wh, wt)
    assert rc == 0
    mean, fwin = engine.fst(G, cov, starts, wh, wt, n=n)
    assert fwin.shape == (len(wh), n * n) and mean.shape == (n, n)
    print(f"[{what}] fst windows: {int((fwin != rwin).sum())} of {fwin.size} cells differ; mean: max |diff| {np.abs(mean - rmean).max():.2e}")
    assert np.isfinite(rwin).all() and np.array_equal(fwin, rwin), what + " fst windows"
    assert np.allclose(mean, rmean, rtol=1e-12, atol=1e-15), what + " fst mean"
    rpw, rpm = oracle.theta_pi(Xt, loci_idx, covs, wh, wt)
    pw, pm = engine.theta_pi(G, cov, starts, wh, wt, n=n)
    assert pw.shape == (len(wh), n) and pm.shape == (n,)
    assert np.array_equal(pw, rpw) and np.array_equal(pm, rpm), what + " pi"
    return pw


def check_diversity(engine, oracle, case, wh, wt, n, count, terms, what):
    """theta_watterson and tajima_d in one counting mode (count / terms None: the counted mode) against the restatement, bit for bit"""
    G, cov, starts, Xt, loci_idx, covs = case
    ps = pool_sizes(n)
    S, theta, tmean, pi, d, dmean = restate(oracle, Xt, loci_idx, covs, wh, wt, ps, terms)
    gtheta, gtmean, gS = engine.theta_watterson(G, starts, wh, wt, ps, count=count, n=n)
    assert gS.shape == gtheta.shape == (len(wh), n)
    assert np.array_equal(gS, S) and np.array_equal(gtheta, theta) and np.array_equal(gtmean, tmean), what
    gd, gdmean, gtheta2, gpi = engine.tajima_d(G, cov, starts, wh, wt, ps, count=count, n=n)
    assert gd.shape == gpi.shape == (len(wh), n)
    assert np.array_equal(gtheta2, theta) and np.array_equal(gpi, pi), what
    assert same(gd, d) and same(gdmean, dmean), what
    return S, d


# ---- the 32 x 32 tiles of pool pairs -----------------------------------------------------------------------------------------
# k_fst_ranges (pg_popgen.hip: FT, FR, FTILE; its launch in fst_ranges): ntile = ceil(n / 32) tiles per edge, the upper triangle of them as
# grid.y; a thread holds 4 x 4 pairs, pool indices past n - 1 are clamped for the loads and masked for the stores.
# (n, tiles per edge, tiles launched)
TILE_POINTS = [
    (1, 1, 1),     # one pair, 15 of a thread's 16 clamped away
    (2, 1, 1),
    (31, 1, 1),    # one short of a full tile: the last thread row / column holds 3 pools
    (32, 1, 1),    # exactly one tile
    (33, 2, 3),    # one pool in the second tile row: the off-diagonal tile is 32 x 1
    (63, 2, 3),
    (64, 2, 3),    # exactly 2 x 2 tiles
    (65, 3, 6),    # three tile rows: the tile id -> (tj, tk) walk (:181-183) goes past its first row
    (96, 3, 6),
    (97, 4, 10),
]
for _n, _ntile, _ntri in TILE_POINTS:
    assert R.fst_tiles(_n) == (_ntile, _ntri)


@pytest.mark.parametrize("n,ntile,ntri", TILE_POINTS)
def test_fst_tiles_and_diversity_across_pool_counts(engine, oracle, n, ntile, ntri):
    L = 300
    case = build(n, L, seed=n)
    chrom, pos = [0] * L, (100 + 13 * np.arange(L)).tolist()
    wh, wt, wc, wseed, wslot = engine.watterson_windows(chrom, pos, 13 * 40, 13 * 20, 5)          # overlapping windows of 41 loci
    rh, rt, rcov, rseed, rslot, terms = D.watterson_windows(chrom, pos, 13 * 40, 13 * 20, 5)
    assert (wh.tolist(), wt.tolist(), wc.tolist(), wseed.tolist(), wslot.tolist()) == \
        (rh.tolist(), rt.tolist(), rcov.tolist(), rseed.tolist(), rslot.tolist()) and len(wh) > 5
    assert R.fst_chunk(L) == (64, 5, 44)
    check_fst_and_pi(engine, oracle, case, wh, wt, n, f"n={n}")
    S_ref, d = check_diversity(engine, oracle, case, wh, wt, n, (wc, wseed, wslot), terms, f"n={n} reference count")
    S_cnt, d = check_diversity(engine, oracle, case, wh, wt, n, None, None, f"n={n} counted")
    assert (S_ref != S_cnt).any() and (n == 1 or (d != 0).any())                      # the two modes differ, and D is not all zero
    #                                                                                   (n = 1: the one pool's size is 2, where D is 0)


# ---- the chunks of the genome-wide mean --------------------------------------------------------------------------------------
# pg_fst_dev (pg_popgen.hip, fst_prepare): chunk = max(64, ceil(L / 2048)) loci per partial sum, ceil(L / chunk) chunks, the last one
# partial; k_chunk_reduce adds the partial sums in chunk order.
# (L, chunk, chunks, loci in the last chunk)
CHUNK_POINTS = [
    (63, 64, 1, 63),             # one chunk, not full
    (64, 64, 1, 64),             # exactly one chunk
    (65, 64, 2, 1),              # a second chunk of one locus
    (129, 64, 3, 1),
    (131072, 64, 2048, 64),      # the last locus count with 64-locus chunks: 2048 full chunks
    (131073, 65, 2017, 33),      # chunk 65: 2016 full chunks and a partial one
]
for _L, _chunk, _nchunks, _last in CHUNK_POINTS:
    assert R.fst_chunk(_L) == (_chunk, _nchunks, _last)


@pytest.mark.parametrize("L,chunk,nchunks,last", CHUNK_POINTS)
def test_fst_mean_across_the_chunk_rule(engine, oracle, L, chunk, nchunks, last):
    n = 5
    case = build(n, L, seed=L % 1000)
    # a window on each chunk seam and one that ends on the last locus
    wh = sorted({0, max(0, chunk - 2), max(0, L - last - 3), max(0, L - 7)})
    wt = [min(L - 1, h + 5) for h in wh[:-1]] + [L - 1]
    check_fst_and_pi(engine, oracle, case, wh, wt, n, f"L={L} chunk={chunk}")


# ---- the slabs of the per-window table ---------------------------------------------------------------------------------------
def test_fst_window_table_second_slab(engine, oracle):
    """pg_fst_dev produces the n_windows x n^2 table 2^30 / (8 n^2) windows at a time (pg_popgen.hip: fst_slab, the loop in pg_fst_dev).  n = 450 pools: slab =
    662 windows; 665 one-locus windows make a second trip with w0 = 662 (window offsets wh + w0, host offset w0 * n^2).  The table
    is 665 * 450^2 doubles = 1.08 GB of host memory.  The oracle is asked for the first two windows and the five around the seam
    only (bit for bit); every window of the second slab must be finite and symmetric, and differ from the first slab's windows."""
    n = 450
    slab = R.fst_slab(n, 10 ** 6)
    nw = slab + 3
    assert slab == (1 << 30) // (8 * n * n) == 662 and R.fst_slab(n, nw) == slab and R.fst_slab(n, 600) == 600
    L = nw + 2
    case = build(n, L, seed=450)
    G, cov, starts, Xt, loci_idx, covs = case
    wh = np.arange(nw)
    mean, win = engine.fst(G, cov, starts, wh, wh, n=n)
    assert win.shape == (nw, n * n)
    some = np.array([0, 1, slab - 2, slab - 1, slab, slab + 1, slab + 2])
    rc, rmean, rwin = oracle.fst(Xt, loci_idx, covs, some, some)
    assert rc == 0 and np.isfinite(rwin).all()
    print(f"[slab] windows {some.tolist()}: cells that differ {[(int((win[w] != rwin[i]).sum())) for i, w in enumerate(some)]}")
    for i, w in enumerate(some):
        assert np.array_equal(win[w], rwin[i]), f"window {w}"
    assert np.allclose(mean, rmean, rtol=1e-12, atol=1e-15)
    second = win[slab:].reshape(-1, n, n)
    assert np.isfinite(second).all() and np.array_equal(second, second.transpose(0, 2, 1))
    for w in range(slab, nw):                                  # a second trip that re-did the first slab's windows would repeat them
        assert not np.array_equal(win[w], win[w - slab])


# ---- one thread per (window, pool) -------------------------------------------------------------------------------------------
# k_range_mean_1d (theta_pi; launched in pi_tables of pg_popgen.hip) and k_diversity_windows (launched in diversity_tables): n_windows * n threads in blocks of
# 256, the tail of the last block masked.  The engine returns host arrays of exactly n_windows x n, so a thread that ran past the end
# would show as a wrong or missing value in the last window, not as an overwritten neighbour.
# (n, n_windows, blocks)
THREAD_POINTS = [
    (5, 51, 1),      # 255 threads' worth: one short of a block
    (4, 64, 1),      # exactly one block
    (1, 257, 2),     # one past: a second block with one live thread
    (7, 73, 2),      # 511
    (8, 64, 2),      # exactly two blocks
    (3, 171, 3),     # 513
]
for _n, _nw, _blocks in THREAD_POINTS:
    assert R.blocks_256(_n * _nw) == _blocks and (_n * _nw) % 256 in (255, 0, 1)


@pytest.mark.parametrize("n,nw,blocks", THREAD_POINTS)
def test_window_kernels_at_block_boundaries(engine, oracle, n, nw, blocks):
    L = nw + 2
    case = build(n, L, seed=100 * n + nw)
    wh = np.arange(nw)
    wt = wh + 2                                                # three loci per window, the last one ends on the last locus
    assert wt[-1] == L - 1
    check_fst_and_pi(engine, oracle, case, wh, wt, n, f"n={n} windows={nw}")
    S, d = check_diversity(engine, oracle, case, wh, wt, n, None, None, f"n={n} windows={nw}")
    assert S.any() and (S[-1] >= 0).all()
