"""The 32-locus stage of the 13-tile kinship kernels (193 .. 208 pools, pg_kinship.hip).  A stage is 32 loci, staged as two halves
of 16; the launcher's slab rule stays in units of 16 loci, so a workgroup runs whole stages two per trip, a peeled whole stage for an
odd count of them, and a peeled half stage when its slab is an odd number of halves.  In a whole stage every wave forms the fused
per-locus sums of two loci at once (w and w + 16), in a half stage of one.

Checked per point, on the plain AND the fused kernel, with the helpers and bounds of tests/test_gpu_kinship_stage_loop.py: plain S
symmetric and against the oracle, fused S bit for bit the plain S, the fits closed from the fused sums against the oracle and the
two-pass path, all in three row geometries with NaN in the padding columns."""
import numpy as np
import pytest
import torch

from test_gpu_kinship_stage_loop import POOLS, close_fit, geometries

pytestmark = pytest.mark.gpu

# slab (loci per workgroup) -> (trips of the two-stage loop, peeled whole stages, half stages): what a full workgroup runs
SLAB_PATH = {
    16: (0, 0, 1),    # half stage only
    32: (0, 1, 0),    # one whole stage
    48: (0, 1, 1),    # whole stage plus half
    64: (1, 0, 0),    # one trip
    80: (1, 0, 1),    # one trip plus half
    96: (1, 1, 0),    # one trip plus a peeled whole stage
    128: (2, 0, 0),   # two trips: the run-time "one more stage" branch of a trip's second stage both ways
}
# loci of the LAST workgroup of a launch: a partial half stage (1, 15), a whole half (16), a whole half and a partial second half (17, 31)
TAILS = (1, 15, 16, 17, 31)
# one workgroup or two, no full grid: 1, 15 (partial half), 16 (half), 17 = 16 + 1, 31 = 16 + 15, 32 = 16 + 16, 33 = 16 + 16 + 1
SMALL = {1: {1}, 15: {15}, 16: {16}, 17: {16, 1}, 31: {16, 15}, 32: {16}, 33: {16, 1}}
GROUPS = ("small",) + tuple(SLAB_PATH)


def wg_loci(p, cus):
    """loci per workgroup, by the launcher's slab rule (pg_launch_kinship, one pool block; see test_gpu_kinship_stage_loop.py)"""
    nslab = max(1, min(cus, (p + 15) // 16))
    slab = ((p + nslab - 1) // nslab + 15) // 16 * 16
    nslab = (p + slab - 1) // slab
    return [min(p, (w + 1) * slab) - w * slab for w in range(nslab)]


def path_of(loci):
    """(trips, peeled whole stages, half stages) of a workgroup of `loci` loci, as the kernel's loop takes them"""
    halves = (loci + 15) // 16
    whole = halves // 2
    return whole // 2, whole % 2, halves % 2


def loci_of(group, cus):
    """{p: workgroup lengths it is there for}.  Slab s: p = (cus - 1) s + r fills cus - 1 workgroups with s loci and the last with r
    (r <= s: a larger remainder would lengthen the slab, so 17 and 31 do not go with s = 16)."""
    if group == "small":
        return dict(SMALL)
    return {(cus - 1) * group + r: {group, r} for r in TAILS if r <= group}


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_loci_counts_reach_the_workgroup_lengths(cus):
    """The model of the slab rule, on the device the tests run on: every p gives the workgroup lengths it is there for, and the
    slabs give the paths through the stage loop the table above names."""
    for group in GROUPS:
        for p, want in loci_of(group, cus).items():
            assert set(wg_loci(p, cus)) == want, (group, p, cus, sorted(set(wg_loci(p, cus))))
    for slab, want in SLAB_PATH.items():
        assert path_of(slab) == want, (slab, path_of(slab))
    assert {path_of(r) for r in TAILS} == {(0, 0, 1), (0, 1, 0)}
    assert max(max(loci_of(g, cus)) for g in GROUPS) <= (cus - 1) * 128 + 31


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", POOLS)
def test_stage32_points(engine, oracle, cus, n, group):
    from poolgen_amd import synth
    loci = sorted(loci_of(group, cus))
    base = synth.genotype_matrix(max(loci) + 3, n, "cuda", seed=131, ld=n)
    Y2 = synth.phenotypes(base, n, k=2, seed=131)
    for p in loci:
        # the three geometries hold the same loci: one oracle run per (p, k) serves them all
        Gh = np.ascontiguousarray(base[3:3 + p].cpu().numpy())
        Kref = oracle.kinship(Gh, n)
        refs = {k: oracle.ols_with_covariate(Gh, Y2[:, :k], force_m=0) for k in (1, 2)}
        for label, G in geometries(base[:p + 3], n):
            assert np.array_equal(G.cpu().numpy()[:, :n], Gh)
            # plain kernel (no phenotypes announced)
            engine.set_phenotypes(None)
            S = engine.kinship_partial(G, n).cpu().numpy()
            what = f"n={n} p={p} {label}"
            assert np.array_equal(S, S.T), what + " plain S symmetric"
            assert np.allclose(S / p, Kref, rtol=1e-11, atol=0), what + " plain S vs oracle"
            for k in (1, 2):
                Y = Y2[:, :k]
                what = f"n={n} p={p} {label} k={k}"
                ref = refs[k]
                # fused kernel alone: the same S, bit for bit
                engine.set_phenotypes(Y, n)
                Sf = engine.kinship_partial(G, n).cpu().numpy()
                assert np.array_equal(Sf, S), what + " fused S vs plain S, bitwise"
                # fused kernel + k_sweep_finish (force_m = 0: the fused path whatever K says)
                engine.profile(True); engine.profile_reset()
                m, K, beta, var, pv = engine.ols_with_covariate(G, Y, 0.0, force_m=0, n=n)
                torch.cuda.synchronize()
                fin_n = engine.profile_get("sweep_finish")[1]
                sw_n = engine.profile_get("sweep")[1]
                engine.profile(False)
                assert m == 0 and fin_n == 1 and sw_n == 0, what + ": the fused path must have run"
                fused = tuple(x.cpu().numpy() for x in (beta, var, pv))
                assert np.array_equal(K, K.T), what + " fused S symmetric"
                assert np.allclose(K, Kref, rtol=1e-11, atol=0), what + " fused S vs oracle"
                close_fit(fused, ref, 1e-10, what + " fused vs oracle")
                # the two-pass path on the same inputs
                engine.set_phenotypes(None)
                engine.covariates_set(n, None, Y)
                two = tuple(x.cpu().numpy() for x in engine.ols_sweep(G, k, n))
                sb = float(np.nanmax(np.abs(two[0]), initial=0.0)); sv = float(np.nanmax(np.abs(two[1]), initial=0.0))
                assert np.allclose(fused[0], two[0], rtol=1e-9, atol=1e-10 * sb, equal_nan=True), what + " beta: fused vs two-pass"
                assert np.allclose(fused[1], two[1], rtol=1e-9, atol=1e-10 * sv, equal_nan=True), what + " var: fused vs two-pass"
                assert np.nanmax(np.abs(fused[2] - two[2]), initial=0.0) <= 1e-10, what + " pval: fused vs two-pass"
