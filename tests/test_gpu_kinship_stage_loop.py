"""The stage loop of the 13-tile kinship kernels (193 .. 208 pools, pg_kinship.hip): two stages per trip with compile-time buffer
offsets, a peeled last stage for odd stage counts, staging pieces that exist per wave, and the fused per-locus sums written through
a buffer descriptor.  Every point is checked on the plain AND the fused kernel: S symmetric and against the oracle, fused S against
plain S, and the fits closed from the fused sums against the two-pass path and against the oracle."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# 193: one pool in the last tile column; 199: odd n (the odd-n kernel instance: tail zeroing of a row's last piece, and lanes of the
# fourth 64-pool group past the last pool); 200: the headline, narrow last column; 201: first without it; 208: full
POOLS = (193, 199, 200, 201, 208)

# Slab rule of pg_launch_kinship with one pool block: nslab = min(CUs, ceil(p / 16)), a slab is ceil(p / nslab) loci rounded up to a
# multiple of 16, and nslab is then recomputed as ceil(p / slab) -- so every workgroup holds at least one locus and a workgroup with
# 0 stages cannot occur in a launch (the kernel's nstages = 0 guards stay unreachable from here).  With 256 CUs:
#   p = 1, 15   one workgroup, one partial stage (1 and 15 loci): the peeled stage alone
#   p = 16      one workgroup, one whole stage
#   p = 17      two workgroups: a whole stage, and one locus
#   p = 33      three workgroups: whole, whole, one locus
#   p = 4805    slabs of 32 loci: 150 workgroups with 2 stages (one trip of the loop, no peeled stage), the last with 5 loci (1 partial)
#   p = 9620    slabs of 48 loci: 200 workgroups with 3 stages (one trip + the peeled stage: odd), the last with 20 loci = 2 stages (even),
#               its second one partial -- both parities of the stage count in one launch
#   p = 12840   slabs of 64 loci: 4 stages (two trips: the runtime "one more stage" branch of the second half both ways), the last
#               workgroup 40 loci = 3 stages, the third partial
LOCI = (1, 15, 16, 17, 33, 4805, 9620, 12840)
WANT_STAGES = {1: {1}, 15: {1}, 16: {1}, 17: {1}, 33: {1}, 4805: {2, 1}, 9620: {3, 2}, 12840: {4, 3}}


def stage_counts(p, cus):
    """stages per workgroup, by the launcher's slab rule (pg_launch_kinship, one pool block)"""
    nslab = max(1, min(cus, (p + 15) // 16))
    slab = ((p + nslab - 1) // nslab + 15) // 16 * 16
    nslab = (p + slab - 1) // slab
    return [(min(p, (w + 1) * slab) - w * slab + 15) // 16 for w in range(nslab)]


def geometries(base, n):
    """(label, G) for the three row geometries; the columns between n and the row pitch hold NaN (never data)"""
    tight = n + (n & 1)            # the library wants an even pitch: an odd n carries one padding column even when "tight"
    p = base.shape[0] - 3
    out = []
    for label, ld, off in (("ld=n", tight, 0), ("ld=n+2", tight + 2, 0), ("row offset 3", tight, 3)):
        full = torch.full((p + off, ld), float("nan"), dtype=torch.float64, device=base.device)
        full[:, :n] = base[3 - off:3 + p]          # the same p loci in every geometry
        G = full[off:]
        assert G.is_contiguous() and G.data_ptr() % 16 == 0
        out.append((label, G))
    return out


def close_fit(got, ref, rtol, what):
    """tests/test_gpu_kinship_path.py::cmp_fit at a given relative bound (the floor is that fraction of the largest value; p absolute)"""
    beta, var, pv = got
    ok = np.isfinite(ref["beta"])
    assert np.array_equal(np.isnan(beta), ~ok), what + " NaN pattern"
    assert np.allclose(beta[ok], ref["beta"][ok], rtol=rtol, atol=rtol * float(np.max(np.abs(ref["beta"][ok]), initial=0.0))), what + " beta"
    assert np.allclose(var[ok], ref["var"][ok], rtol=rtol, atol=rtol * float(np.max(np.abs(ref["var"][ok]), initial=0.0))), what + " var"
    assert np.max(np.abs(pv[ok] - ref["pval"][ok]), initial=0.0) <= 1e-10, what + " pval"


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_loci_counts_reach_the_stage_cases(cus):
    """The comment above, checked against the device the tests run on: each p gives the stage counts it is there for."""
    for p in LOCI:
        assert set(stage_counts(p, cus)) == WANT_STAGES[p], (p, cus, sorted(set(stage_counts(p, cus))))


@pytest.mark.parametrize("n", POOLS)
def test_stage_loop_points(engine, oracle, n):
    from poolgen_amd import synth
    pmax = max(LOCI)
    base = synth.genotype_matrix(pmax + 3, n, "cuda", seed=97, ld=n)
    Y2 = synth.phenotypes(base, n, k=2, seed=97)
    for p in LOCI:
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
                assert np.allclose(K, S / p, rtol=1e-12, atol=0), what + " fused S vs plain S"
                close_fit(fused, ref, 1e-10, what + " fused vs oracle")
                # the two-pass path on the same inputs
                engine.set_phenotypes(None)
                engine.covariates_set(n, None, Y)
                two = tuple(x.cpu().numpy() for x in engine.ols_sweep(G, k, n))
                sb = float(np.nanmax(np.abs(two[0]), initial=0.0)); sv = float(np.nanmax(np.abs(two[1]), initial=0.0))
                assert np.allclose(fused[0], two[0], rtol=1e-9, atol=1e-10 * sb, equal_nan=True), what + " beta: fused vs two-pass"
                assert np.allclose(fused[1], two[1], rtol=1e-9, atol=1e-10 * sv, equal_nan=True), what + " var: fused vs two-pass"
                assert np.nanmax(np.abs(fused[2] - two[2]), initial=0.0) <= 1e-10, what + " pval: fused vs two-pass"
