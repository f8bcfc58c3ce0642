"""Both sides of the dispatch rules the host code applies by pool count n, trait count k, covariate count m and locus count p,
against the CPU oracle.  Every shape names the rule it sits on and the source line of that rule: when a rule moves, its points move
with it.  Tolerances are the suite's own: index work and emitted alleles bit-exact, mean frequency bit-exact (1e-12 for the
order-free rows kernel), statistics and fits 1e-10."""
import subprocess

import numpy as np
import pytest
import torch

from test_gpu_cli import CLI
from test_gpu_kinship_path import cmp_fit, make
from test_gpu_locus_ops import check_stat_op, flt_pair, ols_kernel  # noqa: F401  (ols_kernel: the rows / stream fixture)

pytestmark = pytest.mark.gpu

PG_ERR_INVALID, PG_ERR_UNSUPPORTED = -1, -5


def stream_period(n):
    """loci per lane of the streaming pass (pg_locus_ops.hip:2394-2398): the smallest M with n * 24 * M a multiple of 128"""
    M = 1
    while (n * 24 * M) % 128:
        M *= 2
    return M


def fit_m0(oracle, G, Y, n):
    """the oracle's intercept-only fits (an n x 0 covariate: no kinship, no eigen-solve)"""
    return oracle.ols_with_covariate(np.ascontiguousarray(G.cpu().numpy()[:, :n]), Y, covariate=np.zeros((n, 0)))


def check_chisq(res, rows, ps, fo, oracle):
    n_out, ids, chi2, pv = (x.cpu().numpy() for x in res)
    for l in range(len(rows)):
        a, rid, rc, rp = oracle.chisq_locus(rows[l], ps, fo)
        assert n_out[l] == a, f"chisq locus {l}"
        if a:
            assert ids[l, :min(a, 5)].tolist() == rid.tolist()[:5]
            if np.isnan(rc):
                assert np.isnan(chi2[l]) and np.isnan(pv[l]) and np.isnan(rp)
                continue
            assert abs(chi2[l] - rc) <= 1e-10 * max(1.0, abs(rc)) and abs(pv[l] - rp) <= 1e-10, f"chisq locus {l}"


# ---- A. count operators ------------------------------------------------------------------------------------------------------
# Rows kernel (pg_locus_ops.hip:2450-2453): 16 lanes per locus for 32 <= n <= 112, 32 for n <= 224, 64 for n <= 448 and even n;
# everything else (n < 32, odd n above 224, n > 448) runs the streaming pass.  Streaming period M (:2394-2398) from the 2-adic part of
# n: 1 for n = 0 mod 16 ... 8 for n = 2 mod 4, 16 for odd n.  Second pass (:2513-2521): 16-byte pieces for even n, 8-byte for odd.
COUNT_POINTS = [
    31,    # below the rows kernel (n >= 32, :2450): streaming pass only; odd: M = 16, 8-byte second-pass pieces
    32,    # first rows-kernel count, 16 lanes; M = 1
    50,    # n = 2 mod 4: M = 8; rows kernel, 16 lanes
    112,   # last 16-lane count (n <= 112)
    113,   # first 32-lane count; odd
    224,   # last 32-lane count (n <= 224)
    225,   # odd above 224: no 64-lane rows kernel (n & 1, :2453), streaming pass
    226,   # first 64-lane count; n = 2 mod 4 (M = 8)
    448,   # last 64-lane count (n <= 448)
    449,   # above 448: streaming pass only; odd
    450,   # above 448, even, n = 2 mod 4
]
TRAITS = [1, 2, 3, 5]   # one trait group, two, an odd trait left over at t0 > 0 (ols_iter launches traits in pairs)


@pytest.mark.parametrize("dirty", [False, True], ids=["clean", "errors"])
@pytest.mark.parametrize("n", COUNT_POINTS)
def test_count_operators_across_pool_count_rules(engine, oracle, n, dirty, ols_kernel):
    from poolgen_amd import synth
    i = COUNT_POINTS.index(n)
    k = TRAITS[(i + 2 * dirty) % 4]
    L = max(64 * stream_period(n) + 37, 437)          # never a whole number of 64 * M units (nor of 64-locus rows units)
    counts = synth.sync_counts(L, n, "cuda", seed=300 + n, error_rate=0.005 if dirty else 0.0)
    counts[3::89, : max(1, n // 5), :] = 0                     # uncovered pools
    if dirty:
        counts[7::113, :, 1] = 0                               # only error alleles beside the major one
    Y = synth.phenotypes(synth.genotype_matrix(64, n, "cuda", seed=n), n, k=k, seed=n)
    ps = np.linspace(10, 30, n)
    kw = dict(maf=0.01, remove_ns=(i % 2 == 0)) if dirty else dict()   # both allele-column counts of the second pass (:2513-2521)
    f, fo = flt_pair(oracle, **kw)
    rows = counts.cpu().numpy().astype(np.uint64)
    check_stat_op(engine.ols_iterate(counts, ps, f, Y), oracle.ols_iterate_locus, rows, Y, ps, fo, oracle=oracle)
    check_stat_op(engine.correlation(counts, ps, f, Y), oracle.correlation_locus, rows, Y, ps, fo,
                  stat_rtol=0, stat_atol=1.0000001e-7)
    check_chisq(engine.chisq(counts, ps, f), rows, ps, fo, oracle)


def check_loader(engine, oracle, counts, host, ps, f, fo, keep_p_minus_1=False):
    """load_frequencies against filter_locus / to_frequencies (/ sort_by_allele_freq, the major allele dropped): the set of columns,
    their loci and alleles and every frequency bit-exact.  Returns (columns, col_locus, col_allele)."""
    n = host.shape[1]
    G, col_locus, col_allele = (x.cpu().numpy() for x in engine.load_frequencies(counts, ps, f, keep_p_minus_1=keep_p_minus_1))
    want_cols, want_loc, want_al = [], [], []
    for l in range(host.shape[0]):
        res = oracle.filter_locus(host[l], ps, fo)
        if res is None:
            continue
        ids, fc = res
        fr = oracle.to_frequencies(fc)
        if keep_p_minus_1:
            fr, ids = oracle.sort_by_allele_freq(fr, ids, True)
            fr, ids = fr[:, 1:], ids[1:]
        for j, a in enumerate(ids):
            want_cols.append(fr[:, j]); want_loc.append(l); want_al.append(int(a))
    assert len(want_cols) == G.shape[0]
    assert col_locus.tolist() == want_loc and col_allele.tolist() == want_al
    assert np.array_equal(G[:, :n], np.stack(want_cols), equal_nan=True)
    return len(want_cols), col_locus, col_allele


@pytest.mark.parametrize("n", [31, 50, 113, 226, 449, 450])
def test_loader_across_pool_count_rules(engine, oracle, n):
    """load_frequencies shares launch_passes (streaming period, staging, second pass) with the count operators."""
    from poolgen_amd import synth
    L = 64 * stream_period(n) + 37
    counts = synth.sync_counts(L, n, "cuda", seed=500 + n, error_rate=0.005)
    counts[3::101, 0, :] = 0
    ps = np.linspace(10, 30, n)
    f, fo = flt_pair(oracle, maf=0.01)
    host = counts.cpu().numpy().astype(np.uint64)
    assert check_loader(engine, oracle, counts, host, ps, f, fo)[0] > L


def test_pool_table_top_edge(engine, oracle):
    """The pool table of the streaming pass lives in LDS (pg_locus_ops.hip:2424-2425): ols_iter with two traits holds 3 doubles per
    pool, so n = 4096 is its largest pool count.  4096 runs and matches the oracle; 4097 is refused with PG_ERR_INVALID."""
    from poolgen_amd import NativeError, synth
    n, L = 4096, 300
    counts = synth.sync_counts(L, n, "cuda", seed=4096, error_rate=0.002)
    Y = synth.phenotypes(synth.genotype_matrix(64, n, "cuda", seed=1), n, k=2, seed=1)
    ps = np.full(n, 20.0)
    f, fo = flt_pair(oracle, maf=0.01)
    rows = counts.cpu().numpy().astype(np.uint64)
    check_stat_op(engine.ols_iterate(counts, ps, f, Y), oracle.ols_iterate_locus, rows, Y, ps, fo, oracle=oracle)
    n = 4097
    counts = synth.sync_counts(L, n, "cuda", seed=4097)
    Y = synth.phenotypes(synth.genotype_matrix(64, n, "cuda", seed=1), n, k=2, seed=1)
    with pytest.raises(NativeError, match=rf"failed \({PG_ERR_INVALID}\)"):
        engine.ols_iterate(counts, np.full(n, 20.0), f, Y)
    engine.synchronize()


# ---- B. sweep ----------------------------------------------------------------------------------------------------------------
# Matrix-core sweep while ms_fits(n, cu = m + 1 + k, 0) (pg_sweep.hip:967-972, :1308): U = 5..8 chunks per load group, 1 / 2 / 3
# column groups for cu <= 16 / 32 / 48; above its last pool count the vector-ALU k_ols_sweep<C> with C = round_cols(cu)
# (:1048-1053: 2, 3, 4, 6, 8, 12, 16, 24, 34).  Last matrix-core pool count: cu = 2 -> 1176, 3 -> 1120, 16 -> 728, 17 -> 336,
# 32 -> 112, 33 and 34 -> 240.
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [
    285,    # 36 chunks of 8 pools: U = 6 (ms_pick_u, pg_sweep.hip:958-965: the U of 8 .. 5 that pads least, the larger on a tie)
    301,    # 38 chunks: U = 8 (40)
    513,    # 65 chunks: U = 5
    777,    # 98 chunks: U = 7
    1000,   # 125 chunks: U = 5
    1176,   # 147 chunks: U = 7; cu = 2: last matrix-core count; cu = 3 (k = 2): vector-ALU C = 3
    1177,   # vector-ALU: C = 2 (k = 1), C = 3 (k = 2)
    1400,   # vector-ALU
])
def test_sweep_without_covariates_across_ms_fits(engine, oracle, n, k):
    G, Y = make(700, n, 31)
    Y = Y[:, :k]
    engine.covariates_set(n, None, Y)
    cmp_fit(engine.ols_sweep(G, k, n), fit_m0(oracle, G, Y, n), f"n={n} k={k}")


# (n, m, k, ld, off): cu = m + 1 + k
COV_POINTS = [
    (728, 14, 1, None, 0),    # cu = 16: one column group, last matrix-core count
    (729, 14, 1, 734, 1),     # cu = 16 above it: vector-ALU C = 16; odd ld / 2 and a slab offset
    (336, 14, 2, None, 0),    # cu = 17: two column groups, last matrix-core count
    (337, 14, 2, None, 0),    # cu = 17 above it: vector-ALU C = 24
    (112, 30, 1, None, 0),    # cu = 32: two column groups, last matrix-core count
    (113, 30, 1, None, 0),    # cu = 32 above it: vector-ALU C = 34
    (240, 31, 1, None, 0),    # cu = 33: three column groups, last matrix-core count
    (241, 31, 1, None, 0),    # cu = 33 above it: vector-ALU C = 34
    (240, 31, 2, 242, 3),     # cu = 34: three column groups, last matrix-core count; slab offset
    (241, 31, 2, None, 0),    # cu = 34 above it: vector-ALU C = 34
    (1121, 2, 1, None, 0),    # cu = 4 (last matrix-core count 1120): vector-ALU C = 4
    (1057, 3, 2, None, 0),    # cu = 6 (last 1056): vector-ALU C = 6
    (961, 6, 1, None, 0),     # cu = 8 (last 960): vector-ALU C = 8
    (900, 9, 2, 902, 0),      # cu = 12 (last 864): vector-ALU C = 12
]


@pytest.mark.parametrize("n,m,k,ld,off", COV_POINTS)
def test_sweep_with_covariates_across_column_groups(engine, oracle, n, m, k, ld, off):
    from poolgen_amd import synth
    p = 500
    Gfull = synth.genotype_matrix(p + off, n, "cuda", seed=n + m, ld=ld)
    if ld is not None and ld > n:
        Gfull[:, n:] = float("nan")                # padding between n and ld is never data
    G = Gfull[off:]
    assert G.is_contiguous()
    Y = synth.phenotypes(Gfull, n, k=k, seed=m)
    C = np.random.default_rng(n * m).standard_normal((n, m))
    engine.covariates_set(n, C, Y)
    got = engine.ols_sweep(G, k, n)
    ref = oracle.ols_with_covariate(np.ascontiguousarray(G.cpu().numpy()[:, :n]), Y, covariate=C)
    cmp_fit(got, ref, f"n={n} m={m} k={k} ld={ld} off={off}")


def test_sweep_column_limit_is_refused(engine):
    """cu = m + 1 + k = 35 is more than one sweep launch carries (pg_sweep.hip:1067-1070): PG_ERR_UNSUPPORTED, not a launch."""
    from poolgen_amd import NativeError
    n = 200
    G, Y = make(100, n, 5)
    C = np.random.default_rng(1).standard_normal((n, 33))
    with pytest.raises(NativeError, match=rf"failed \({PG_ERR_UNSUPPORTED}\)"):
        engine.covariates_set(n, C, Y[:, :1])
    engine.covariates_set(n, C[:, :32], Y[:, :1])            # cu = 34 is accepted
    engine.synchronize()


# ---- C. lazy kinship route ---------------------------------------------------------------------------------------------------
# pg_ols_kinship_dev without K (pg_sweep.hip:1330-1331, ms_pitch :967): a MODE-2 matrix-core pass when ms_fits(n, 1 + k, 2), whose closing stage has
# row pitch (cu + 2) | 1.  Last MODE-2 pool count: k = 1 -> 1120, k = 3 -> 1056, k = 15 -> 672; above it the full route.  (Checked
# with the MODE-0 pitch instead, the route used to launch up to 1176 / 1120 / 728 pools and fail for want of LDS.)
LAZY_POINTS = [
    (1120, 1),   # k = 1: last MODE-2 count
    (1121, 1),   # k = 1: first count past it (was: the launch asked for more than 160 KiB)
    (1150, 1),
    (1176, 1),   # k = 1: last MODE-0 count
    (1177, 1),   # past both
    (1056, 3),   # k = 3: last MODE-2 count
    (1057, 3),
    (1120, 3),   # k = 3: last MODE-0 count
    (672, 15),   # k = 15: last MODE-2 count
    (673, 15),
    (728, 15),   # k = 15: last MODE-0 count
]


def lazy_inputs(n, k):
    from poolgen_amd import synth
    G = synth.genotype_matrix(600, n, "cuda", seed=n + k)
    return G, synth.phenotypes(G, n, k=k, seed=k)


@pytest.mark.parametrize("n,k", LAZY_POINTS)
def test_lazy_kinship_route_across_its_lds_edge(engine, oracle, monkeypatch, n, k):
    G, Y = lazy_inputs(n, k)
    m, K, beta, var, pv = engine.ols_with_covariate(G, Y, 0.75, n=n, want_K=False)
    got = tuple(x.clone() for x in (beta, var, pv))
    assert m == 0 and K is None
    cmp_fit(got, fit_m0(oracle, G, Y, n), f"lazy n={n} k={k}")
    monkeypatch.setenv("POOLGEN_NO_LAZY_KINSHIP", "1")
    m2, _, beta2, var2, pv2 = engine.ols_with_covariate(G, Y, 0.75, n=n, want_K=False)
    assert m2 == 0
    assert torch.allclose(beta2, got[0], rtol=1e-10, atol=1e-10 * float(got[0].abs().max()))
    assert torch.allclose(var2, got[1], rtol=1e-10, atol=1e-10 * float(got[1].abs().max()))
    assert float((pv2 - got[2]).abs().max()) <= 1e-10


def test_lazy_route_grid_multiplier(engine, oracle, monkeypatch):
    """POOLGEN_SWEEP_GRID_MULT raises the MODE-2 grid above what the occupancy API gives; the lazy route's per-wave partials hold
    MS_LZ_PER_CU workgroups per CU, and the grid is clamped to them: same decision and the same bits."""
    n, k = 1000, 1
    G, Y = lazy_inputs(n, k)
    m, _, beta, var, pv = engine.ols_with_covariate(G, Y, 0.75, n=n, want_K=False)
    want = tuple(x.clone() for x in (beta, var, pv))
    monkeypatch.setenv("POOLGEN_SWEEP_GRID_MULT", "6")
    m2, _, beta2, var2, pv2 = engine.ols_with_covariate(G, Y, 0.75, n=n, want_K=False)
    assert m == m2 == 0
    for a, b in zip(want, (beta2, var2, pv2)):
        assert torch.equal(a, b)
    cmp_fit(want, fit_m0(oracle, G, Y, n), "grid multiplier")


# ---- E. the CLI's whole-file ols_iter_with_kinship (K_out = NULL: the lazy route) at a pool count of the old LDS gap -----------
def test_cli_kinship_at_a_pool_count_past_the_lazy_edge(oracle, tmp_path):
    from poolgen_amd import synth
    n, L = 1150, 1000
    counts = synth.sync_counts(L, n, "cpu", seed=1150).numpy().astype(np.uint64)
    Y = synth.phenotypes(synth.genotype_matrix(64, n, "cpu", seed=1150), n, k=1, seed=3)
    ps = [20.0] * n
    sync = tmp_path / "wide.sync"
    with open(sync, "w") as fh:
        fh.write("#chr\tpos\tref\t" + "\t".join(f"p{i}" for i in range(n)) + "\n")
        for l in range(L):
            fh.write(f"chr1\t{1000 + 13 * l}\tN\t" + "\t".join(":".join(map(str, counts[l, i])) for i in range(n)) + "\n")
    phen = tmp_path / "wide.csv"
    with open(phen, "w") as fh:
        fh.write("#name,size,t1\n")
        for i in range(n):
            fh.write(f"P{i},20,{float(Y[i, 0])!r}\n")
    r = subprocess.run([str(CLI), "ols_iter_with_kinship", "-f", str(sync), "-p", str(phen), "--phen-delim", ",", "--phen-name-col", "0",
                        "--phen-pool-size-col", "1", "--phen-value-col", "2", "--n-threads", "4", "--stream-chunk-mb", "0"],
                       capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr
    out = r.stdout.strip().splitlines()[-1]
    assert "-ols_iterative_xxt_1_eigens-" in out, out            # m = 0: one "eigenvector" (the intercept), gwas/ols.rs:393-398
    f = oracle.filt()
    lab, cols = [("intercept", 0, "intercept")], []
    for l in range(L):
        res = oracle.filter_locus(counts[l], ps, f)
        if res is None:
            continue
        ids, fc = res
        fr = oracle.to_frequencies(fc)
        for j, a in enumerate(ids):
            lab.append(("chr1", 1000 + 13 * l, "ATCGND"[a])); cols.append(fr[:, j])
    lines = open(out).read().splitlines()
    assert lines[0] == "#chr,pos,alleles,phenotype,statistic,pvalue" and len(lines) == 1 + len(cols)
    sl = list(range(0, len(cols), 7))
    G = np.array([cols[i] for i in sl])
    ref = oracle.ols_with_covariate(G, Y, covariate=np.zeros((n, 0)))
    for r_, i in enumerate(sl):
        fa = lines[1 + i].split(",")
        assert (fa[0], int(fa[1]), fa[2], fa[3]) == (lab[i][0], lab[i][1], lab[i][2], "Pheno_0")   # label shift, gwas/ols.rs:421-425
        b, p = float(fa[4]), float(fa[5])
        rb, rp = ref["beta"][r_, 0], ref["pval"][r_, 0]
        assert abs(b - rb) <= 1e-10 + 1e-10 * abs(rb) and abs(p - rp) <= 1e-10, (lines[1 + i], rb, rp)
