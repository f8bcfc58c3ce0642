"""The restatement of gudmc (tests/gudmc_ref.py) against closed forms, and the measurement of the tolerance T the GPU tests use."""
import math

import numpy as np

import gudmc_ref as R


def test_fit_recovers_sample_mean_and_population_sd():
    rng = np.random.default_rng(3)
    for cnt, loc, scale in ((5, 0.0, 1.0), (12, -1.3, 0.4), (40, 0.2, 0.05), (30, 150.0, 80.0)):
        q = rng.normal(loc, scale, size=cnt).tolist()
        mu, sd, it = R.fit_normal(q)
        m = sum(q) / cnt
        s = math.sqrt(sum((v - m) ** 2 for v in q) / cnt)
        assert abs(mu - m) <= 1e-6 * s and abs(sd - s) <= 1e-6 * s, (cnt, mu - m, sd - s, it)
        mu2, sd2, _ = R.fit_normal(q, cost="moments")   # the closed form of the same cost lands at the same place
        assert abs(mu2 - m) <= 1e-6 * s and abs(sd2 - s) <= 1e-6 * s


def test_empty_column_stops_at_the_first_vertex():
    mu, sd, it = R.fit_normal([])
    assert (mu, it) == (1.5, 0) and sd == R.sigma_of(1.0)
    assert R.fit_column([math.nan, math.nan]) == (mu, sd, it)


def test_width_scan_hand_worked():
    """8 windows, mean 0, threshold 1: rows 0-2 a run of three on chr 0 (overlapping), row 3 insignificant, rows 4-5 significant
    across the chromosome change (no carry over it), row 6 significant after a gap (pos_ini beyond the previous pos_fin), row 7
    significant and overlapping row 6."""
    chrom = [0, 0, 0, 0, 0, 1, 1, 1]
    ini = [1, 51, 101, 151, 201, 1, 301, 351]
    fin = [100, 150, 200, 250, 300, 100, 400, 450]
    d = [1.5, -1.2, 2.0, 0.3, -1.0, 1.0, -3.0, 1.1]
    assert R.width_scan(d, 0.0, chrom, ini, fin, 1.0) == [99, 198, 297, 0, 99, 99, 99, 198]
    # row 4 follows an insignificant row that overlaps it: the carried width is that row's 0
    assert R.width_scan(d[:5], 0.0, chrom, ini, fin, 1.0)[4] == 99


def test_nan_windows_are_compacted_and_labels_stay():
    """A NaN window in the middle: the later values move one label up (the reference's defect, kept)."""
    d = np.array([[2.0], [math.nan], [-2.0], [2.5]])
    fst = np.full((4, 1), 0.25)
    fst[:, 0] = [0.1, 0.2, 0.3, 0.4]
    r = R.gudmc_stage(d, fst, [0, 0, 0, 0], [1, 51, 101, 151], [100, 150, 200, 250], sigma_threshold=0.5)
    assert r["rows"] == [3] and r["window"][0] == [0, 1, 2] and r["d"][0] == [2.0, -2.0, 2.5]
    fm = r["fst_mean"][0]
    assert r["fst_delta"][0] == [0.1 - fm, 0.2 - fm, 0.3 - fm]      # the Fst of windows 0, 1, 2: the labels' windows
    assert r["width"][0] == [99.0, 198.0, 297.0]


def test_round8_is_the_text_round_trip():
    assert R.round8(0.123456785) == 0.12345679 and R.round8(-0.123456785) == -0.12345679   # half away from zero
    assert R.round8(1.5) == 1.5 and math.isnan(R.round8(math.nan)) and R.round8(-math.inf) == -math.inf


def test_corpus_has_the_columns_the_gpu_tests_need():
    t, const = R.fit_table()
    counts = (~np.isnan(t)).sum(axis=0)
    assert counts[:6].tolist() == [0, 1, 2, 3, 12, 40] and sorted(const) == [1, 6]
    ref = R.fit_table_reference()
    assert any(r[2] == R.MAX_ITERS for r in ref) and any(0 < r[2] < R.MAX_ITERS for r in ref)
    assert [c for c, r in enumerate(ref) if r[1] <= R.DEGENERATE_SD] == [1, 6]
    for k, c in enumerate(R.stage_cases()):
        n = c["n"]
        res = R.stage_reference(k)
        deg = [i for i, f in enumerate(R.stage_fits(res)) if f[1] <= R.DEGENERATE_SD]
        assert deg == [n + a * n + a for a in range(n)], (k, deg)          # exactly the diagonal pairs' Fst
        assert res["rows"][n - 1] == 0 and res["rows"][1] == c["w"] - 1
        for p in res["pops"][:n - 1]:
            assert len({x for x in p["width"] if x > 0}) >= 2
    res = R.stage_reference(-1)
    assert all(x == 0 for p in res["pops"] for x in p["width"])


def test_tolerance_measured_forward_against_reverse():
    """T of gudmc_ref: 10 x the spread between two orders of the reference's own sum, over the whole corpus."""
    dm, ds = R.spread(R.fit_table_reference(False), R.fit_table_reference(True))
    for k in list(range(len(R.stage_cases()))) + [-1]:
        a, b = R.spread(R.stage_fits(R.stage_reference(k, False)), R.stage_fits(R.stage_reference(k, True)))
        dm, ds = max(dm, a), max(ds, b)
    print(f"forward against reverse: |d mu| / sigma {dm:.3g}, |d sigma| / sigma {ds:.3g}; 10 x the larger = {10 * max(dm, ds):.3g}")
    assert 0.0 < 10.0 * max(dm, ds) < 1e-5     # a sanity ceiling, not the bar
    assert R.T < 1e-5
