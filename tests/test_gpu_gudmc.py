"""pg_normal_fit_dev and pg_gudmc_dev against the restatement of popgen/gudmc.rs (tests/gudmc_ref.py).

What the reference fixes exactly -- the rows per pair, their windows, d, the widths and their deviation -- is compared exactly.
The fitted values are compared at the solver's resolution T (gudmc_ref.T: 10 x the spread between two summation orders of the
reference's own cost): mu and sigma at T sigma, fst_delta at T sigma_fst, the p-values at T absolute
(|dp| <= phi(z) (|d mu| / sigma + |z| |d sigma| / sigma) < T).  Columns whose RESTATED sigma is <= 1e-12 sit at the logit's lower
bound: only sigma <= 1e-12 and |mu - value| <= 1e-12 are asked of them."""
import math

import numpy as np
import pytest

import gudmc_ref as R

pytestmark = pytest.mark.gpu


def bits(t):
    return t.cpu().numpy().view(np.int64) if t.dtype.is_floating_point else t.cpu().numpy()


@pytest.fixture(scope="module")
def batch(engine):
    """the fits of the whole 130-column table, once"""
    t, _ = R.fit_table()
    return engine.normal_fit(t)


def check_fit(name, mu, sd, ref_mu, ref_sd, value=None):
    if ref_sd <= R.DEGENERATE_SD:
        assert value is not None, f"{name}: a degenerate column the test did not expect"
        assert sd <= R.DEGENERATE_SD and abs(mu - value) <= 1e-12, (name, mu, sd, value)
        return 0.0
    e = max(abs(mu - ref_mu), abs(sd - ref_sd)) / ref_sd
    assert e <= R.T, (name, mu, ref_mu, sd, ref_sd, e)
    return e


def test_fits_match_the_restatement(batch):
    t, const = R.fit_table()
    ref = R.fit_table_reference()
    mu, sd, count, iters = (x.cpu().numpy() for x in batch)
    assert count.tolist() == (~np.isnan(t)).sum(axis=0).tolist()
    assert (mu[0], sd[0], iters[0]) == (1.5, R.sigma_of(1.0), 0)                     # the empty column
    assert any(r[2] == R.MAX_ITERS for r in ref) and any(0 < r[2] < R.MAX_ITERS for r in ref)
    worst = max(check_fit(f"column {c}", mu[c], sd[c], ref[c][0], ref[c][1], const.get(c)) for c in range(t.shape[1]))
    capped = int((iters == R.MAX_ITERS).sum())
    print(f"normal_fit: {t.shape[1]} columns, worst |d| / sigma {worst:.3g} (T = {R.T:.3g}); {capped} fits at the cap here, "
          f"{sum(r[2] == R.MAX_ITERS for r in ref)} in the restatement")
    assert iters.min() >= 0 and iters.max() <= R.MAX_ITERS


@pytest.mark.parametrize("cols", [1, 63, 64, 65, 130])
def test_a_fit_does_not_depend_on_its_batch(engine, batch, cols):
    t, _ = R.fit_table()
    got = engine.normal_fit(np.ascontiguousarray(t[:, :cols]))
    for g, b in zip(got, batch):
        assert np.array_equal(bits(g), bits(b)[:cols])
    # ... nor on where the column stands: the last column of the prefix, fitted alone
    alone = engine.normal_fit(np.ascontiguousarray(t[:, cols - 1:cols]))
    for a, b in zip(alone, batch):
        assert np.array_equal(bits(a), bits(b)[cols - 1:cols])


def check_stage(engine, k):
    c = R.stage_cases()[k] if k >= 0 else R.insignificant_case()
    ref = R.stage_reference(k)
    n, w = c["n"], c["w"]
    out = engine.gudmc_from_tables(c["d"], c["fst"], c["chrom"], c["ini"], c["fin"], c["thr"], c["rate"])
    got = {name: v.cpu().numpy() for name, v in out.items()}
    assert got["rows"].tolist() == ref["rows"]
    degenerate = 0
    worst = 0.0
    for b in range(n):
        worst = max(worst, check_fit(f"D of population {b}", got["d_mean"][b], got["d_sd"][b], ref["d_mean"][b], ref["d_sd"][b]))
    for i in range(n * n):
        a, b = divmod(i, n)
        rows = ref["rows"][b]
        fst_degenerate = ref["fst_sd"][i] <= R.DEGENERATE_SD
        degenerate += fst_degenerate
        width_degenerate = ref["width_sd"][i] <= R.DEGENERATE_SD
        assert width_degenerate == (k < 0 and rows > 0), (i, ref["width_sd"][i])
        worst = max(worst, check_fit(f"Fst of pair {i}", got["fst_mean"][i], got["fst_sd"][i], ref["fst_mean"][i], ref["fst_sd"][i],
                                     0.0 if a == b else None))
        worst = max(worst, check_fit(f"width of pair {i}", got["width_mean"][i], got["width_sd"][i], ref["width_mean"][i],
                                     ref["width_sd"][i], 0.0 if k < 0 else None))
        # exact: the rows' windows, d, the widths and their deviation
        assert got["window"][i, :rows].tolist() == ref["window"][i]
        for name in ("d", "width", "width_dev"):
            want = np.array(ref[name][i], dtype=np.float64)
            assert np.array_equal(got[name][i, :rows].view(np.int64), want.view(np.int64)), (name, i)
        # within the tolerance: fst_delta and the two p-values
        for j in range(rows):
            if not fst_degenerate:
                fd, fp = ref["fst_delta"][i][j], ref["fst_p"][i][j]
                if math.isnan(fd):
                    assert math.isnan(got["fst_delta"][i, j]) and math.isnan(got["fst_p"][i, j])
                else:
                    assert abs(got["fst_delta"][i, j] - fd) <= R.T * ref["fst_sd"][i], (i, j)
                    assert abs(got["fst_p"][i, j] - fp) <= R.T, (i, j, got["fst_p"][i, j], fp)
            if not width_degenerate:
                assert abs(got["width_p"][i, j] - ref["width_p"][i][j]) <= R.T, (i, j, got["width_p"][i, j], ref["width_p"][i][j])
    assert degenerate == n          # exactly the diagonal pairs: nothing else hides behind the degenerate rule
    print(f"gudmc stage n={n} w={w}: rows {ref['rows']}, worst |d| / sigma of the fits {worst:.3g} (T = {R.T:.3g})")


@pytest.mark.parametrize("k", range(len(R.STAGE_SHAPES)))
def test_stage_matches_the_restatement(engine, k):
    c = R.stage_cases()[k]
    assert (c["n"], c["w"]) == R.STAGE_SHAPES[k][:2] and 0.3 <= c["thr"] <= 0.5
    check_stage(engine, k)


def test_stage_all_insignificant(engine):
    """every width 0: the width fits are degenerate and are checked as such"""
    check_stage(engine, -1)


def test_infinite_d_is_refused(engine):
    from poolgen_amd import NativeError
    c = R.stage_cases()[0]
    d = c["d"].copy()
    d[2, 0] = math.inf
    with pytest.raises(NativeError, match="infinite"):
        engine.gudmc_from_tables(d, c["fst"], c["chrom"], c["ini"], c["fin"], c["thr"], c["rate"])
    with pytest.raises(NativeError, match="infinite"):
        engine.normal_fit(d)
    # the context is usable afterwards
    assert engine.gudmc_from_tables(c["d"], c["fst"], c["chrom"], c["ini"], c["fin"], c["thr"], c["rate"])["rows"].tolist() == \
        R.stage_reference(0)["rows"]


def test_gudmc_composes_tajima_d_fst_and_the_stage(engine):
    """Engine.gudmc on a 5-pool synthetic matrix == tajima_d + fst + gudmc_from_tables, bit for bit."""
    import torch
    rng = np.random.default_rng(12)
    n, L = 5, 240
    f = np.clip(rng.beta(0.8, 0.8, size=(L, 1)) + rng.normal(0.0, 0.15, size=(L, n)), 0.0, 1.0)
    f = np.round(f * 64.0) / 64.0                         # dyadic: f + (1 - f) is exactly 1, as fst's guard asks
    f[rng.random((L, n)) < 0.25] = 0.0                    # monomorphic pools: segregating sites differ between windows
    G = np.zeros((2 * L, n + (n & 1)))
    G[0::2, :n] = f
    G[1::2, :n] = 1.0 - f
    cov = np.zeros_like(G)
    cov[:, :n] = np.repeat(rng.integers(20, 60, size=(L, n)).astype(np.float64), 2, axis=0)
    locus_col = np.arange(0, 2 * L + 1, 2)
    chrom = np.array([0] * (L // 2) + [1] * (L - L // 2), dtype=np.int32)
    pos = np.concatenate([np.arange(1, L // 2 + 1) * 10, np.arange(1, L - L // 2 + 1) * 10]).astype(np.uint64)
    head, tail = engine.sliding_windows(chrom, pos, 100, 50, 5)
    assert len(head) >= 12
    Gd, cd = torch.from_numpy(G).cuda(), torch.from_numpy(cov).cuda()
    sizes = [42.0] * n
    args = (chrom[head], pos[head], pos[tail])
    whole = engine.gudmc(Gd, cd, locus_col, head, tail, *args, sizes, sigma_threshold=0.4, n=n)
    d_win = engine.tajima_d(Gd, cd, locus_col, head, tail, sizes, n=n)[0]
    fst_win = engine.fst(Gd, cd, locus_col, head, tail, n=n)[1]
    assert np.isfinite(d_win).any()
    parts = engine.gudmc_from_tables(d_win, fst_win, *args, sigma_threshold=0.4)
    assert whole["rows"].sum().item() > 0
    rows = whole["rows"].cpu().numpy()
    for name in whole:
        a, b = bits(whole[name]), bits(parts[name])
        if a.ndim == 2:                                    # per (pair, row): specified below rows[pair % n]
            keep = np.arange(a.shape[1])[None, :] < rows[np.arange(n * n) % n][:, None]
            a, b = a[keep], b[keep]
        assert np.array_equal(a, b), name
