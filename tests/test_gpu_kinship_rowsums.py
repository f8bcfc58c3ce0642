"""The fused per-locus sums of the 13-tile kinship kernels (193 .. 208 pools, pg_kinship.hip) by DPP rows: a task is 4 consecutive
loci of a 32-locus stage, row r of the wave is locus r of the task, lane i of the row sums the pools i, i + 16, .., i + 192, and
only the last of these 13 slots can lie past the last pool (it then reads the shift, column 0, so that it adds exactly 0).  The 8
tasks of a stage go to the waves 0 .. 7 or 8 .. 15 by the stage's buffer, the 4 tasks of a half stage to the waves 0 .. 3.

What is held here, with the helpers and bounds of tests/test_gpu_kinship_stage_loop.py and tests/test_gpu_kinship_stage32.py:
  * every pool count 193 .. 208 (each has its own set of lanes past the last pool), k = 1 and 2, three row geometries with NaN in
    the padding columns: fused S bit for bit the plain S, fused fits against the oracle and against the two-pass path;
  * constant and near-fixed loci: the NaN pattern of the two-pass path and the same bounds on what is finite;
  * a locus has the same fits, bit for bit, wherever it sits in a slab (task row, wave half, whole stage, half stage, tail)."""
import numpy as np
import pytest
import torch

from test_gpu_kinship_stage_loop import close_fit, geometries
from test_gpu_kinship_stage32 import loci_of, wg_loci

pytestmark = pytest.mark.gpu

POOLS = tuple(range(193, 209))
GROUPS = ("small", "trip")
DROPS = (0, 1, 4, 16, 17)


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def loci_counts(group, cus):
    """{p: workgroup lengths it is there for}: the `small` group of test_gpu_kinship_stage32.py, and slabs of 64 loci (one trip of the
    two-stage loop) whose last workgroup holds 1 locus (a half-stage tail: task 0 cut after its first row) or 17 (a peeled whole
    stage: task 4 cut after its first row, the tasks 5 .. 7 past the slab's end)"""
    if group == "small":
        return loci_of("small", cus)
    return {(cus - 1) * 64 + r: {64, r} for r in (1, 17)}


def fused_fit(engine, G, Y, n, what):
    """(beta, var, pval) closed from the fused sums, and K"""
    engine.profile(True); engine.profile_reset()
    m, K, beta, var, pv = engine.ols_with_covariate(G, Y, 0.0, force_m=0, n=n)
    torch.cuda.synchronize()
    fin_n = engine.profile_get("sweep_finish")[1]
    sw_n = engine.profile_get("sweep")[1]
    engine.profile(False)
    assert m == 0 and fin_n == 1 and sw_n == 0, what + ": the fused path must have run"
    return tuple(x.cpu().numpy() for x in (beta, var, pv)), K


def two_pass_fit(engine, G, Y, n):
    engine.set_phenotypes(None)
    engine.covariates_set(n, None, Y)
    return tuple(x.cpu().numpy() for x in engine.ols_sweep(G, Y.shape[1], n))


def close_two_pass(fused, two, what):
    """the bounds of test_gpu_kinship_stage32.py: beta and var at rtol 1e-9 with a floor of 1e-10 of the largest value, p within 1e-10"""
    sb = float(np.nanmax(np.abs(two[0]), initial=0.0)); sv = float(np.nanmax(np.abs(two[1]), initial=0.0))
    assert np.allclose(fused[0], two[0], rtol=1e-9, atol=1e-10 * sb, equal_nan=True), what + " beta: fused vs two-pass"
    assert np.allclose(fused[1], two[1], rtol=1e-9, atol=1e-10 * sv, equal_nan=True), what + " var: fused vs two-pass"
    assert np.nanmax(np.abs(fused[2] - two[2]), initial=0.0) <= 1e-10, what + " pval: fused vs two-pass"


def test_loci_counts_reach_the_workgroup_lengths(cus):
    for group in GROUPS:
        for p, want in loci_counts(group, cus).items():
            assert set(wg_loci(p, cus)) == want, (group, p, cus, sorted(set(wg_loci(p, cus))))


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", POOLS)
def test_rowsums_points(engine, oracle, cus, n, group):
    from poolgen_amd import synth
    loci = sorted(loci_counts(group, cus))
    base = synth.genotype_matrix(max(loci) + 3, n, "cuda", seed=151, ld=n)
    Y2 = synth.phenotypes(base, n, k=2, seed=151)
    for p in loci:
        # the three geometries hold the same loci: one oracle run per (p, k) serves them all
        Gh = np.ascontiguousarray(base[3:3 + p].cpu().numpy())
        Kref = oracle.kinship(Gh, n)
        refs = {k: oracle.ols_with_covariate(Gh, Y2[:, :k], force_m=0) for k in (1, 2)}
        for label, G in geometries(base[:p + 3], n):
            assert np.array_equal(G.cpu().numpy()[:, :n], Gh)
            engine.set_phenotypes(None)
            S = engine.kinship_partial(G, n).cpu().numpy()
            for k in (1, 2):
                Y = Y2[:, :k]
                what = f"n={n} p={p} {label} k={k}"
                engine.set_phenotypes(Y, n)
                Sf = engine.kinship_partial(G, n).cpu().numpy()
                assert np.array_equal(Sf, S), what + " fused S vs plain S, bitwise"
                fused, K = fused_fit(engine, G, Y, n, what)
                assert np.allclose(K, Kref, rtol=1e-11, atol=0), what + " fused S vs oracle"
                close_fit(fused, refs[k], 1e-10, what + " fused vs oracle")
                close_two_pass(fused, two_pass_fit(engine, G, Y, n), what)


# (locus of the 64, what it holds): a constant locus, and three that differ from it in one pool by 1e-9 -- somewhere in the middle,
# in column 0 (the shift: every OTHER pool then has d = -1e-9) and in column n - 1 (next to the padding).  The loci sit in different
# tasks and task rows of the two stages of a 64-locus slab.
NEAR_FIXED = ((5, None), (22, "middle"), (39, "first"), (60, "last"))


@pytest.mark.parametrize("n", (200, 193))
def test_near_fixed_and_constant_loci(engine, n):
    from poolgen_amd import synth
    p = 64
    base = synth.genotype_matrix(p + 3, n, "cuda", seed=157, ld=n)
    Y2 = synth.phenotypes(base, n, k=2, seed=157)
    for row, where in NEAR_FIXED:
        base[3 + row, :] = 0.37
        if where is not None:
            base[3 + row, {"middle": n // 2, "first": 0, "last": n - 1}[where]] += 1e-9
    special = np.array([row for row, _ in NEAR_FIXED])
    plain = np.setdiff1d(np.arange(p), special)
    for label, G in geometries(base, n):
        for k in (1, 2):
            Y = Y2[:, :k]
            what = f"n={n} {label} k={k}"
            engine.set_phenotypes(Y, n)
            fused, _ = fused_fit(engine, G, Y, n, what)
            two = two_pass_fit(engine, G, Y, n)
            for a, b, name in zip(fused, two, ("beta", "var", "pval")):
                assert np.array_equal(np.isnan(a), np.isnan(b)), what + f" {name}: NaN pattern of the two-pass path"
            assert np.all(np.isnan(fused[0][special[0]])), what + ": a constant locus has no fit"
            close_two_pass(fused, two, what)
            # the ordinary loci again, on their own scale (a near-fixed locus's coefficient is ~1e9 times theirs)
            close_two_pass(tuple(x[plain] for x in fused), tuple(x[plain] for x in two), what + " ordinary loci")


@pytest.mark.parametrize("n", (193, 200, 208))
def test_same_bits_wherever_a_locus_sits(engine, cus, n):
    """Dropping 1, 4, 16 or 17 leading rows moves every locus to another task row, task, wave, stage buffer (and with it the other
    half of the waves) and in or out of the tails: whole stages of a trip in the long run, half stages alone in the short one."""
    from poolgen_amd import synth
    for total in ((cus - 1) * 64 + 17 + max(DROPS), 33 + max(DROPS)):
        base = synth.genotype_matrix(total, n, "cuda", seed=163, ld=n + (n & 1))
        Y2 = synth.phenotypes(base, n, k=2, seed=163)
        for k in (1, 2):
            Y = Y2[:, :k]
            fits = {}
            for drop in DROPS:
                G = base[drop:]
                assert G.is_contiguous() and G.data_ptr() % 16 == 0
                engine.set_phenotypes(Y, n)
                fits[drop], _ = fused_fit(engine, G, Y, n, f"n={n} p={total - drop} k={k}")
            for drop in DROPS[1:]:
                for a, b, name in zip(fits[0], fits[drop], ("beta", "var", "pval")):
                    assert np.array_equal(a[drop:], b, equal_nan=True), f"n={n} total={total} k={k} drop={drop} {name}"
