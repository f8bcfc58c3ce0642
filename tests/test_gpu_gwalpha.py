"""Engine.gwalpha / pg_gwalpha_batch[_dev] (gwas::gwalpha_ls, gwalpha_ml) against the restatement in tests/gwalpha_ref.py.

Inputs: gwalpha_ref.make_case -- coverage 20-59, frequencies linear in pool rank with a N(0, 0.3) slope clipped to
[0.03, 0.97]; a fifth of the loci with a third allele above the MAF, a fifth with a misread base below it, one locus with a pool
without reads (dropped by the filter), one with the same counts in every pool.  65 loci at n = 5 (a tail in every launch
geometry), 20 at n = 9 (16 interior points: whole rounds of a sub-group's lanes), 20 at n = 10 (one round more, partly filled),
12 at n = 3, 6 at n = 33; LS and ML.

What is asserted per case:
 (a) n_out, the allele of every row and the dropped (most frequent) allele bit-exact, the mean frequency within 1e-12;
 (b) the restatement's cost AT THE GPU'S RETURNED SHAPES equals the GPU's returned cost within 1e-9 max(1, |cost|): the device
     cost function and incomplete Beta, independent of the trajectory;
 (c) |(mu_A - mu_B)_GPU - (mu_A - mu_B)_ref| <= 1e-6 per row (5 x the 1.8e-7 two CPU trajectories that differ in the last bits
     showed on this recipe), alpha within the same bound scaled by 2 sqrt(p_a (1 - p_a)) / sig; at most 2 % of a case's rows
     may exceed it and none may exceed 1e-3 (a different basin);
 (d) 1 <= iters <= 1000.  Whether a fit meets the stop rule (the five costs within EPSILON of each other) before the cap is
     decided by the last bits of costs near 7 (ML) and is not a property two trajectories share: the count of rows where only
     one side ran into the cap is printed, not asserted.  A row that stopped early has iters < 1000 by construction of the
     solver's loop (the cap is the only other exit);
 (e) the reference's own locus gives its four literals within 1e-6 through pg_gwalpha_batch_dev, the host form and Engine.gwalpha.
Placement invariance (no restatement): 1001 loci at n = 5 and 257 at n = 10, run once, reversed, and as two calls split at an
odd locus with the second part in a buffer of its own: alpha, shapes, cost and iters bit-identical per locus."""
import ctypes as C
import functools
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import gwalpha_ref as G
import oracle_lib
from poolgen_amd import Filter
from poolgen_amd._native import PgFilter

pytestmark = pytest.mark.gpu
MAF = 0.03
CASES = {5: 65, 9: 20, 10: 20, 3: 12, 33: 6}
GOLD = Path(__file__).parent / "golden" / "gwalpha_literals.json"


@functools.lru_cache(maxsize=None)
def reference(n: int, method: str):
    """The restatement's rows for the case of n pools, computed once."""
    o = oracle_lib.load()
    counts, bins, q, sig, mn, mx = G.make_case(100 + n, CASES[n], n)
    flt = o.filt(True, 1, MAF, 0.0)
    rows = [G.gwalpha_locus(o, counts[l].astype(np.uint64), bins, q, sig, mn, mx, flt, method) for l in range(counts.shape[0])]
    return counts, bins, q, sig, mn, mx, rows


@pytest.mark.parametrize("method", ["LS", "ML"])
@pytest.mark.parametrize("n", sorted(CASES))
def test_gwalpha_matches_the_restatement(engine, oracle, n, method):
    counts, bins, q, sig, mn, mx, ref = reference(n, method)
    L = counts.shape[0]
    cd = torch.from_numpy(counts.astype(np.int32)).cuda()
    flt = Filter(True, 1, MAF, 0.0)
    n_out, ids, mf, alpha, shapes, cost, iters = [t.cpu().numpy() for t in engine.gwalpha(cd, bins, q, sig, mn, mx, flt, method)]
    kept_n, kept_ids, _, _ = [t.cpu().numpy() for t in engine.chisq(cd, bins, flt)]       # the survivors: kept rows + the dropped allele
    nrows = over = capdiff = 0
    worst_b = worst_c = worst_mf = 0.0
    for l in range(L):
        want = ref[l]
        assert n_out[l] == (0 if want is None else len(want)), (l, n_out[l])
        if want is None:
            continue
        survivors = set(int(v) for v in kept_ids[l, : kept_n[l]])
        assert survivors - set(int(v) for v in ids[l, : n_out[l]]) == {want[0]["dropped"]}, l
        for r, w in enumerate(want):
            assert ids[l, r] == w["allele"], (l, r)
            dmf = abs(mf[l, r] - w["mean_freq"])
            worst_mf = max(worst_mf, dmf)
            assert dmf <= 1e-12, (l, r, mf[l, r], w["mean_freq"])
            nrows += 1
            s = [float(v) for v in shapes[l, r]]
            assert all(G.EPS <= v <= 10.0 for v in s) and 1 <= iters[l, r] <= 1000, (l, r, s, iters[l, r])
            c_ref = G.cost_at(oracle, method, s, w["inputs"])                                   # (b)
            db = abs(c_ref - cost[l, r]) / max(1.0, abs(c_ref))
            worst_b = max(worst_b, db)
            assert db <= 1e-9, (l, r, c_ref, cost[l, r])
            dc = abs(G.mu_diff(s, mn, mx) - w["mu_diff"])                                       # (c)
            worst_c = max(worst_c, dc)
            assert dc <= 1e-3, (l, r, dc, s, w["shapes"])
            scale = 2.0 * math.sqrt(w["inputs"]["p_a"] * (1.0 - w["inputs"]["p_a"])) / sig
            assert abs(alpha[l, r] - G.alpha_of(s, w["inputs"]["p_a"], sig, mn, mx)) <= 1e-12 * max(1.0, abs(alpha[l, r]))
            if dc > 1e-6 or abs(alpha[l, r] - w["alpha"]) > 1e-6 * scale + 1e-12 * abs(w["alpha"]):
                over += 1
            capdiff += int((iters[l, r] == 1000) != (w["iters"] == 1000))                      # (d)
    print(f"gwalpha n={n} {method}: {nrows} rows of {L} loci; (a) mean freq {worst_mf:.3g}; (b) cost at the GPU's shapes "
          f"{worst_b:.3g} (relative to max(1, |cost|)); (c) max |d(mu_A - mu_B)| {worst_c:.3g}, {over} rows above 1e-6; "
          f"(d) {capdiff} rows where only one side met the cap")
    assert nrows >= L // 2
    assert over <= 0.02 * nrows


def _golden(oracle):
    g = json.loads(GOLD.read_text())
    counts = np.zeros((1, 5, 6), dtype=np.uint32)
    for j, a in enumerate(g["alleles"]):
        counts[0, :, G.ALLELES.index(a)] = np.array(g["counts"])[:, j]
    f = g["filter"]
    return g, counts, (bool(f["remove_ns"]), int(f["min_coverage_depth"]), float(f["min_allele_frequency"]), float(f["max_missingness_rate"]))


@pytest.mark.parametrize("method", ["LS", "ML"])
def test_reference_literals_through_every_entry_point(engine, native, oracle, method):
    g, counts, f = _golden(oracle)
    want = [ln.split(",") for ln in g["expected_ls" if method == "LS" else "expected_ml"].splitlines()]
    bins, q = np.array(g["bins"]), np.array(g["q"])
    got = {}
    # Engine.gwalpha = pg_gwalpha_batch_dev
    n_out, ids, mf, alpha, *_ = [t.cpu().numpy() for t in engine.gwalpha(torch.from_numpy(counts.astype(np.int32)).cuda(), bins, q,
                                                                         g["sig"], g["min"], g["max"], Filter(*f), method)]
    got["Engine.gwalpha"] = (n_out[0], ids[0], mf[0], alpha[0])
    # pg_gwalpha_batch_dev with the optional outputs left out
    cd = torch.from_numpy(counts.astype(np.int32)).cuda()
    o_n = torch.empty(1, dtype=torch.int32, device="cuda"); o_i = torch.empty(5, dtype=torch.int32, device="cuda")
    o_m = torch.empty(5, dtype=torch.float64, device="cuda"); o_a = torch.empty(5, dtype=torch.float64, device="cuda")
    pf = PgFilter(int(f[0]), 0, f[1], f[2], f[3])
    rc = native.pg_gwalpha_batch_dev(engine._ctx, cd.data_ptr(), 1, 5, bins.ctypes.data, q.ctypes.data, g["sig"], g["min"], g["max"],
                                     C.byref(pf), 0 if method == "LS" else 1, o_n.data_ptr(), o_i.data_ptr(), o_m.data_ptr(),
                                     o_a.data_ptr(), None, None, None)
    assert rc == 0, native.pg_last_error(engine._ctx)
    torch.cuda.synchronize()
    got["pg_gwalpha_batch_dev"] = (o_n.cpu().numpy()[0], o_i.cpu().numpy(), o_m.cpu().numpy(), o_a.cpu().numpy())
    # the host form
    h_n = np.zeros(1, dtype=np.int32); h_i = np.zeros(5, dtype=np.int32); h_m = np.zeros(5); h_a = np.zeros(5)
    h_s = np.zeros(20); h_c = np.zeros(5); h_it = np.zeros(5, dtype=np.int32)
    rc = native.pg_gwalpha_batch(engine._ctx, counts.ctypes.data, 1, 5, bins.ctypes.data, q.ctypes.data, g["sig"], g["min"], g["max"],
                                 C.byref(pf), 0 if method == "LS" else 1, h_n.ctypes.data, h_i.ctypes.data, h_m.ctypes.data,
                                 h_a.ctypes.data, h_s.ctypes.data, h_c.ctypes.data, h_it.ctypes.data)
    assert rc == 0, native.pg_last_error(engine._ctx)
    got["pg_gwalpha_batch"] = (h_n[0], h_i, h_m, h_a)
    for who, (no, ids_, mf_, al_) in got.items():
        assert no == 2, who
        for r, w in enumerate(want):
            print(f"{who} {method} {w[2]}: alpha {al_[r]!r}, reference prints {w[5]}")
            assert G.ALLELES[ids_[r]] == w[2] and oracle.round_own(mf_[r], 6) == w[3], (who, r)
            assert abs(al_[r] - float(w[5])) <= 1e-6, (who, r, al_[r], w[5])
    assert np.array_equal(got["pg_gwalpha_batch"][3][:2], got["pg_gwalpha_batch_dev"][3][:2])
    assert np.all((h_it[:2] >= 1) & (h_it[:2] <= 1000)) and np.all(np.isfinite(h_s[:8])) and np.all(np.isfinite(h_c[:2]))
    assert engine.last_listed()[0] == 1


def test_gwalpha_refuses_fewer_than_three_pools_and_bad_arguments(engine):
    from poolgen_amd import NativeError
    counts = torch.ones((4, 2, 6), dtype=torch.int32, device="cuda")
    with pytest.raises(NativeError):
        engine.gwalpha(counts, [0.5, 0.5], [0.0, 0.5], 0.1, 0.0, 1.0, Filter())
    with pytest.raises(ValueError):
        engine.gwalpha(torch.ones((4, 3, 6), dtype=torch.int32, device="cuda"), [0.5, 0.5], [0.0, 0.5, 0.7], 0.1, 0.0, 1.0, Filter())


@pytest.mark.parametrize("method", ["LS", "ML"])
@pytest.mark.parametrize("n,L", [(5, 1001), (10, 257)])
def test_gwalpha_does_not_depend_on_where_a_locus_sits(engine, n, L, method):
    counts, bins, q, sig, mn, mx = G.make_case(7 * n, L, n)
    flt = Filter(True, 1, MAF, 0.0)
    cd = torch.from_numpy(counts.astype(np.int32)).cuda()

    def run(t):
        return [v.cpu().numpy() for v in engine.gwalpha(t.contiguous(), bins, q, sig, mn, mx, flt, method)]

    base = run(cd)
    rev = run(torch.flip(cd, dims=[0]))
    cut = L // 3 | 1                                                  # an odd locus: the view behind it is not 16-byte aligned for odd n
    a, b = run(cd[:cut]), run(cd[cut:].clone())                       # ... so the second part is copied to a buffer of its own
    rows = int(base[0].sum())
    assert rows >= L // 2 and int((base[0] > 1).sum()) > 0
    for i, name in enumerate(["n_out", "ids", "mean_freq", "alpha", "shapes", "cost", "iters"]):
        assert np.array_equal(base[i], rev[i][::-1], equal_nan=(i in (2, 3, 4, 5))), f"{name}: reversed batch differs"
        assert np.array_equal(base[i], np.concatenate([a[i], b[i]]), equal_nan=(i in (2, 3, 4, 5))), f"{name}: split batch differs"
    print(f"placement n={n} {method}: {rows} rows, mean iterations {base[6][base[6] > 0].mean():.1f}")
