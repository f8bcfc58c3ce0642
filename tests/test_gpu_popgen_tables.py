"""The tables forms of the popgen entry points (pg_pi_tables_dev, pg_fst_tables_dev, pg_watterson_tables_dev,
pg_tajima_d_tables_dev): each leaves on the device exactly the bits that the host-output entry point returns -- which the tests
beside this one hold against the oracle and the restatement -- at the shapes of test_gpu_popgen.py / test_gpu_popgen_diversity.py
(n below and above one wave and no multiple of 64, overlapping windows, both counting modes).  The host forms are the tables forms
plus a copy, so the mean across windows is also held against numpy over the table returned with it.  pg_window_scatter_dev: the
kept windows at their places, NaN elsewhere."""
import numpy as np
import pytest
import torch

from test_gpu_popgen_diversity import make_counts

pytestmark = pytest.mark.gpu


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def same_bits(dev, host):
    return dev.is_cuda and tuple(dev.shape) == host.shape and np.array_equal(bits(dev), bits(host))


def tables_case(engine, n, L, win, slide, minl):
    """the matrix, the loci's first columns, watterson_windows' five arrays and the pool sizes of one shape"""
    from poolgen_amd import Filter
    counts = make_counts(L, n, 23)
    rng = np.random.default_rng(2)
    chrom = np.sort(rng.integers(0, 3, size=L))
    pos = np.concatenate([np.sort(rng.choice(np.arange(1, 40 * L), size=int((chrom == c).sum()), replace=False)) for c in range(3)])
    ps = (2 + (np.arange(n) * 7) % 41).astype(np.float64)
    G, col_locus, col_allele, cov = engine.load_frequencies(counts, ps, Filter(), coverages=True)
    cl = col_locus.cpu().numpy()
    starts = [0] + [i for i in range(1, len(cl)) if cl[i] != cl[i - 1]] + [len(cl)]
    loci = cl[starts[:-1]]
    wh, wt, wc, wseed, wslot = engine.watterson_windows(chrom[loci], pos[loci], win, slide, minl)
    assert len(wh) > 3
    return G, cov, starts, (wh, wt, wc, wseed, wslot), ps


@pytest.mark.parametrize("n,L,win,slide,minl", [(12, 600, 400, 200, 2), (37, 1500, 1000, 500, 3), (200, 800, 5000, 2500, 10)])
def test_tables_forms_return_the_host_forms_bits(engine, n, L, win, slide, minl):
    G, cov, starts, (wh, wt, wc, wseed, wslot), ps = tables_case(engine, n, L, win, slide, minl)
    for dev, host in zip(engine.theta_pi_tables(G, cov, starts, wh, wt, n=n), engine.theta_pi(G, cov, starts, wh, wt, n=n)):
        assert same_bits(dev, host)
    fm, fw = engine.fst(G, cov, starts, wh, wt, n=n)
    dm, dw = engine.fst_tables(G, cov, starts, wh, wt, n=n)
    assert same_bits(dm, fm) and same_bits(dw, fw) and np.isfinite(fw).any() and (fw != 0).any()
    for count in ((wc, wseed, wslot), None):
        for dev, host in zip(engine.theta_watterson_tables(G, starts, wh, wt, ps, count=count, n=n),
                             engine.theta_watterson(G, starts, wh, wt, ps, count=count, n=n)):
            assert same_bits(dev, host)
        got = engine.tajima_d_tables(G, cov, starts, wh, wt, ps, count=count, n=n)
        want = engine.tajima_d(G, cov, starts, wh, wt, ps, count=count, n=n)
        for dev, host in zip(got, want):
            assert same_bits(dev, host)
        assert (want[0] != 0).any()


def is_mean_of(mean, win):
    """mean [n] is mean_axis(Axis(0)) of win [nw x n] bit for bit: the windows added left to right from 0.0, one division;
    a NaN equals a NaN whatever its payload"""
    mean, win = mean.cpu().numpy(), win.cpu().numpy()
    with np.errstate(all="ignore"):
        s = np.zeros(win.shape[1])
        for w in range(win.shape[0]):
            s = s + win[w]
        want = s / win.shape[0]
    nan = np.isnan(want)
    return mean.shape == want.shape and np.array_equal(np.isnan(mean), nan) and np.array_equal(bits(mean)[~nan], bits(want)[~nan])


@pytest.mark.parametrize("n,L,win,slide,minl", [(12, 600, 400, 200, 2), (37, 1500, 1000, 500, 3)])
def test_window_means_are_the_means_of_the_tables_returned(engine, n, L, win, slide, minl):
    """The host forms copy the tables forms' results, so tables against host no longer holds two mean computations against
    each other: the device mean (k_window_mean) against numpy over the very table returned with it, at all windows and at
    a single one."""
    G, cov, starts, windows, ps = tables_case(engine, n, L, win, slide, minl)
    for nw in (len(windows[0]), 1):
        wh, wt, wc, wseed, wslot = (x[:nw] for x in windows)
        pw, pm = engine.theta_pi_tables(G, cov, starts, wh, wt, n=n)
        assert pw.shape == (nw, n) and is_mean_of(pm, pw)
        for count in ((wc, wseed, wslot), None):
            tw, tm, seg = engine.theta_watterson_tables(G, starts, wh, wt, ps, count=count, n=n)
            assert tw.shape == (nw, n) and is_mean_of(tm, tw)
            d, dm, theta, pi = engine.tajima_d_tables(G, cov, starts, wh, wt, ps, count=count, n=n)
            assert d.shape == (nw, n) and is_mean_of(dm, d)


def test_fst_tables_without_windows_and_refusals(engine):
    from poolgen_amd import Filter, NativeError
    counts = make_counts(60, 5, 3)
    ps = np.full(5, 10.0)
    G, col_locus, col_allele, cov = engine.load_frequencies(counts, ps, Filter(), coverages=True)
    cl = col_locus.cpu().numpy()
    starts = [0] + [i for i in range(1, len(cl)) if cl[i] != cl[i - 1]] + [len(cl)]
    none = np.zeros(0, dtype=np.int64)
    mean, win = engine.fst_tables(G, cov, starts, none, none, n=5)                       # the genome-wide means alone
    assert same_bits(mean, engine.fst(G, cov, starts, none, none, n=5)[0]) and win.numel() == 0
    for call in (lambda: engine.theta_pi_tables(G, cov, starts, none, none, n=5),         # "There were no windows defined."
                 lambda: engine.tajima_d_tables(G, cov, starts, none, none, ps, n=5),
                 lambda: engine.theta_watterson_tables(G, starts, [3], [2], ps, n=5)):     # a tail before its head
        with pytest.raises(NativeError):
            call()


def test_window_scatter(engine):
    import ctypes as C
    dev = torch.device("cuda", engine.device)
    for w, cols, keep in ((7, 3, [0, 2, 3, 6]), (5, 300, []), (4, 1, [0, 1, 2, 3]), (300, 9, list(range(1, 300, 2)))):
        kept = torch.arange(1, len(keep) * cols + 1, dtype=torch.float64, device=dev).reshape(len(keep), cols)
        table = torch.full((w, cols), 7.0, dtype=torch.float64, device=dev)
        k = np.array(keep, dtype=np.int64)
        rc = engine._lib.pg_window_scatter_dev(engine._ctx, kept.data_ptr() if keep else None, len(keep), k.ctypes.data if keep else None, w, cols,
                                               table.data_ptr())
        assert rc == 0
        want = np.full((w, cols), np.nan)
        want[keep] = kept.cpu().numpy()
        assert np.array_equal(bits(table), bits(want))                                   # the NaN is the host's std::nan("") too
    k = np.array([2, 1], dtype=np.int64)
    assert engine._lib.pg_window_scatter_dev(engine._ctx, kept.data_ptr(), 2, k.ctypes.data, 300, 9, table.data_ptr()) != 0    # not increasing
