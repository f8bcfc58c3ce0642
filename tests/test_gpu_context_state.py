"""What a pg_ctx carries from one call to the next (struct pg_ctx, poolgen_amd/csrc/pg_common.h; the table is in
tests/DISPATCH_COVERAGE.md, "Carried state") must never change a result.

THE RULE every test here applies: an operation B that runs after a history A on one context returns, bit for bit, what B returns as
the first call on a fresh context under the same environment switches -- and that first-call result agrees with the CPU oracle at
the suite's existing tolerance for the operator (cmp_fit / 1e-10 for fits, binary128 for covariate fits, bit-exact index work,
1e-12 mean frequency for the rows kernel, exact for the parsers, assert_path for the GP paths).  Bit equality with an
oracle-checked result is the stronger statement, so the oracle runs once per operation, on the first-call result.

Every B is first run on TWO fresh contexts (reference()): an operator whose two first calls differ is no subject for a bit-for-bit
comparison; it is named in FALLBACK with the reason and compared with the oracle alone.  The list is printed by the last test of
the file and may hold two operators at most.

Contexts come from fresh() below: Engine(0), closed in `finally`.  At most two of them live at a time beside the session's engine
(which only prepares inputs here).  POOLGEN_OLS_ITER_KERNEL is pinned for the whole file: the adaptive choice (rows_next) depends
on history by design and has its own test, test_gpu_locus_ops.py::test_kernel_choice_follows_the_data."""
import contextlib
import ctypes as C
import gc
import random
import time

import numpy as np
import pytest
import torch

import dispatch_rules as R
import pileup_corpus
import sync_corpus
import vcf_corpus
from test_gpu_kinship_path import cmp_fit, make

pytestmark = pytest.mark.gpu

PG_ERR_INVALID, PG_ERR_STATE, PG_ERR_UNSUPPORTED = -1, -4, -5
FALLBACK = []      # (operation, reason): failed the determinism probe, compared with the oracle only.  Expected empty; at most two.
_REF = {}          # operation name -> its first-call result (host copies), probed and oracle-checked once
_T0 = [None]    # when the first case of this file started (set by the module fixture)


@pytest.fixture(autouse=True)
def pinned_dispatch(monkeypatch):
    monkeypatch.setenv("POOLGEN_OLS_ITER_KERNEL", "rows")
    for name in ("POOLGEN_TWO_PASS", "POOLGEN_NO_LAZY_KINSHIP", "POOLGEN_SWEEP_V1", "POOLGEN_SWEEP_V2", "POOLGEN_LOCUS_GROUPED"):
        monkeypatch.delenv(name, raising=False)


@pytest.fixture(scope="module", autouse=True)
def release_what_the_file_shares():
    """the inputs and first-call results are shared among the cases above and go with the file: nothing of them, and no block
    the allocator cached for them, stays behind in a session whose later tests start processes of their own on the same GPU"""
    _T0[0] = time.time()
    yield
    _INPUT.clear()
    _REF.clear()
    gc.collect()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


@contextlib.contextmanager
def fresh():
    from poolgen_amd import Engine
    e = Engine(0)
    try:
        yield e
    finally:
        torch.cuda.synchronize()
        e.close()


# ---- results as host values, compared bit for bit ---------------------------------------------------------------------------
def freeze(x):
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().numpy().copy()
    if isinstance(x, np.ndarray):
        return x.copy()
    if isinstance(x, dict):
        return {k: freeze(v) for k, v in x.items()}
    if isinstance(x, (tuple, list)):
        return tuple(freeze(v) for v in x)
    return x


def first_difference(a, b, path="result"):
    """None when a and b hold the same bits, else where they first differ and by how much"""
    if isinstance(a, dict):
        if not isinstance(b, dict) or sorted(a) != sorted(b):
            return f"{path}: keys differ"
        return next((d for k in sorted(a) for d in [first_difference(a[k], b[k], f"{path}[{k!r}]")] if d), None)
    if isinstance(a, tuple):
        if not isinstance(b, tuple) or len(a) != len(b):
            return f"{path}: lengths differ"
        return next((d for i, (x, y) in enumerate(zip(a, b)) for d in [first_difference(x, y, f"{path}[{i}]")] if d), None)
    if isinstance(a, np.ndarray):
        if not isinstance(b, np.ndarray) or a.dtype != b.dtype or a.shape != b.shape:
            return f"{path}: dtype / shape differ"
        if a.tobytes() == b.tobytes():
            return None
        ua, ub = (np.ascontiguousarray(v).reshape(-1).view(np.uint8).reshape(a.size, -1) for v in (a, b))
        bad = np.flatnonzero((ua != ub).any(axis=1))
        detail = ""
        if a.dtype.kind == "f":
            fa, fb = a.reshape(-1)[bad], b.reshape(-1)[bad]
            with np.errstate(all="ignore"):
                rel = np.abs(fa - fb) / np.maximum(np.abs(fb), 1e-300)
            detail = f", max |diff| {np.nanmax(np.abs(fa - fb)):.3e}, max relative {np.nanmax(rel):.3e}, {int((rel > 1e-6).sum())} above 1e-6"
        return f"{path}: {len(bad)} of {a.size} elements differ, first at flat index {int(bad[0])}{detail}"
    return None if a == b else f"{path}: {a!r} != {b!r}"


class Op:
    """name; run(engine) -> result; check(frozen result): the oracle at the suite's tolerance for this operator"""

    def __init__(self, name, run, check):
        self.name, self.run, self.check = name, run, check


def reference(op):
    if op.name not in _REF:
        with fresh() as a:
            ra = freeze(op.run(a))
        with fresh() as b:
            rb = freeze(op.run(b))
        op.check(ra)
        d = first_difference(ra, rb)
        if d:
            FALLBACK.append((op.name, "two fresh contexts disagree: " + d))
        _REF[op.name] = ra
    return _REF[op.name]


def must_equal_fresh(op, got, what):
    ref = reference(op)
    got = freeze(got)
    if any(name == op.name for name, _ in FALLBACK):
        op.check(got)
        return
    d = first_difference(got, ref)
    assert d is None, f"{op.name} {what}: differs from the first call on a fresh context -- {d}"


def launches(e, name="sweep_finish"):
    return e.profile_get(name)[1]


def state_error(call, code, text=None):
    from poolgen_amd import NativeError
    with pytest.raises(NativeError) as err:
        call()
    assert f"({code})" in str(err.value), str(err.value)
    if text:
        assert text in str(err.value), str(err.value)
    return err.value


# ---- the operations -----------------------------------------------------------------------------------------------------------
_INPUT = {}


def cached(key, builder):
    if key not in _INPUT:
        _INPUT[key] = builder()
    return _INPUT[key]


def freq_matrix(p, n, seed):
    """frequencies in (0.2, 0.8): what a large call leaves behind in a buffer is never a zero"""
    rng = np.random.default_rng(seed)
    G = np.zeros((p, n + (n & 1)))
    G[:, :n] = rng.uniform(0.2, 0.8, size=(p, n))
    return torch.from_numpy(G).cuda()


def big_phenotypes(n, k, seed):
    return np.random.default_rng(seed).normal(size=(n, k)) * 1e3


def deep_counts(L, n, seed):
    """every count of a present allele is 50 or more and every frequency of one lies in (0.2, 0.8), also in the matrix the loader
    makes of them; a third allele (a quarter of the reads) at ~30 % of the loci"""
    rng = np.random.default_rng(seed)
    depth = rng.integers(220, 400, size=(L, n))
    pr = np.clip(rng.uniform(0.4, 0.6, size=(L, 1)) + 0.05 * rng.normal(size=(L, n)), 0.32, 0.68)
    third = (rng.random(L) < 0.3)[:, None]
    c = np.zeros((L, n, 6), dtype=np.int64)
    c[:, :, 2] = np.where(third, depth // 4, 0)
    rest = depth - c[:, :, 2]
    c[:, :, 0] = np.rint(rest * pr)
    c[:, :, 1] = rest - c[:, :, 0]
    f = c[:, :, :3] / depth[:, :, None]
    assert c[:, :, :3][c[:, :, :3] > 0].min() >= 50 and f[f > 0].min() > 0.2 and f.max() < 0.8
    return torch.from_numpy(c.astype(np.int32)).cuda()


def suite_counts(L, n, seed):
    """the counts of test_gpu_locus_ops.py::test_synthetic_batches: third alleles, Ns, deletions, degenerate loci"""
    from poolgen_amd import synth
    counts = synth.sync_counts(L, n, "cuda", seed=seed)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    counts[:, :, 2] = (torch.rand(L, n, generator=g, device="cuda") < 0.15).int() * torch.randint(0, 9, (L, n), generator=g, device="cuda", dtype=torch.int32)
    counts[:, :, 4] = (torch.rand(L, n, generator=g, device="cuda") < 0.05).int()
    counts[::97, :, 5] = 3
    counts[5::211, :, 1] = 0; counts[5::211, :, 2] = 0
    counts[11::307, 0, :] = 0
    return counts


def sweep_op(p, n, k, seed, G=None, Y=None, tag=""):
    """B = covariates_set(n, None, Y) + ols_sweep(G): the two-pass intercept-only fits"""
    if G is None:
        G, Y2 = cached(("make", p, n, seed), lambda: make(p, n, seed))
        Y = np.ascontiguousarray(Y2[:, :k])

    def run(e):
        e.covariates_set(n, None, Y)
        return e.ols_sweep(G, k, n)

    def check(res, oracle=None):
        import oracle_lib
        cmp_fit(tuple(torch.from_numpy(x) for x in res), oracle_lib.load().ols_with_covariate(G.cpu().numpy(), Y, force_m=0, n=n), f"sweep p={p} n={n} k={k}")
    return Op(f"sweep{tag} p={p} n={n} k={k} seed={seed}", run, check)


def kinship_op(p, n, k, seed, force_m=-1, G=None, Y=None, tag=""):
    """B = ols_with_covariate(G, Y, want_K=True): kinship (fused sums where they ride), eigen rule, fits"""
    if G is None:
        G, Y2 = cached(("make", p, n, seed), lambda: make(p, n, seed))
        Y = np.ascontiguousarray(Y2[:, :k])

    def run(e):
        return e.ols_with_covariate(G, Y, 0.75, force_m=force_m, n=n)

    def check(res):
        import oracle_lib
        from test_gpu_exact import assert_close, errs, formula_p
        oracle, exact = oracle_lib.load(), oracle_lib.load_exact()
        m, K, beta, var, pv = res
        Gh = G.cpu().numpy()
        ref = oracle.ols_with_covariate(Gh, Y, 0.75, force_m=force_m, n=n)
        assert m == ref["m"] and np.allclose(K, ref["K"], rtol=1e-11, atol=0), f"kinship n={n}: m / K"
        if m == 0:
            cmp_fit(tuple(torch.from_numpy(x) for x in (beta, var, pv)), ref, f"kinship path p={p} n={n} k={k}")
            return
        # covariate fits: the literal oracle loses cond(X'X) eps digits there, so the suite's reference point for them is the binary128
        # chain (tests/test_gpu_exact.py; big_rtol = 1e-7 is its bound for the whole chain with the product's own eigenvectors);
        # the p-values are the reference's formula with df = n - 1 of THIS call
        ex = exact.ols_with_covariate(Gh, Y, 0.75, force_m=force_m, n=n)
        assert ex["m"] == m
        pf = formula_p(oracle, ex, n)
        print(f"[kinship path n={n} m={m}] |GPU - exact| {errs((beta, var, pv), ex, pf)}  |oracle - exact| {errs((ref['beta'], ref['var'], ref['pval']), ex, pf)}")
        assert_close((beta, var, pv), ex, pf, f"kinship path p={p} n={n} m={m}", big_rtol=1e-7)
        assert np.allclose(ref["beta"], ex["beta"], rtol=1e-6, atol=1e-10)      # the literal oracle within its own error of it
        assert np.nanmax(np.abs(pv - ref["pval"])) <= 1e-6                          # ... and its p-values (df = n - 1) next to the product's
    return Op(f"kinship{tag} p={p} n={n} k={k} seed={seed} force_m={force_m}", run, check)


def count_Y(n):
    from poolgen_amd import synth
    return cached(("count_Y", n), lambda: synth.phenotypes(synth.genotype_matrix(64, n, "cuda", seed=99), n, k=2, seed=4))


def count_ops(L, n, seed, counts=None, Y=None, tag=""):
    """ols_iterate, correlation, chisq on one counts batch"""
    from poolgen_amd import Filter
    if counts is None:
        counts = cached(("suite_counts", L, n, seed), lambda: suite_counts(L, n, seed))
    if Y is None:
        Y = count_Y(n)
    ps = np.linspace(10, 30, n)
    f = Filter()

    def check_stat(ref_name, **kw):
        def check(res):
            import oracle_lib
            from test_gpu_locus_ops import check_stat_op
            oracle = oracle_lib.load()
            rows = counts.cpu().numpy().astype(np.uint64)
            check_stat_op(tuple(torch.from_numpy(x) for x in res), getattr(oracle, ref_name), rows, Y, ps, oracle.filt(), oracle=oracle, **kw)
        return check

    def check_chisq(res):
        import oracle_lib
        oracle = oracle_lib.load()
        n_out, ids, chi2, pv = res
        rows = counts.cpu().numpy().astype(np.uint64)
        for l in range(L):
            a, rid, rc, rp = oracle.chisq_locus(rows[l], ps, oracle.filt())
            assert n_out[l] == a, l
            if a:
                assert ids[l, :min(a, 5)].tolist() == rid.tolist()[:5], l
                if np.isnan(rc):
                    assert np.isnan(chi2[l]) and np.isnan(pv[l]) and np.isnan(rp), l
                else:
                    assert abs(chi2[l] - rc) <= 1e-10 * max(1.0, abs(rc)) and abs(pv[l] - rp) <= 1e-10, l
    key = f"{tag} L={L} n={n} seed={seed}"
    return {"ols_iterate": Op("ols_iterate" + key, lambda e: e.ols_iterate(counts, ps, f, Y), check_stat("ols_iterate_locus")),
            "correlation": Op("correlation" + key, lambda e: e.correlation(counts, ps, f, Y), check_stat("correlation_locus", stat_rtol=0, stat_atol=1.0000001e-7)),
            "chisq": Op("chisq" + key, lambda e: e.chisq(counts, ps, f), check_chisq)}


def diversity_sizes(n):
    return (2 + (np.arange(n) * 7) % 41).astype(np.float64)      # whole numbers >= 2, differing between pools (tajima_d)


def loader_op(L, n, seed, counts=None, tag=""):
    """B = load_frequencies(counts, coverages=True): plan + emit with the coverages"""
    from poolgen_amd import Filter
    if counts is None:
        counts = cached(("suite_counts", L, n, seed), lambda: suite_counts(L, n, seed))
    ps = diversity_sizes(n)

    def check(res):
        import oracle_lib
        oracle = oracle_lib.load()
        G, col_locus, col_allele, cov = res
        host = counts.cpu().numpy().astype(np.uint64)
        cols, covs, loc, al = [], [], [], []
        for l in range(L):
            r = oracle.filter_locus(host[l], ps, oracle.filt())
            if r is None:
                continue
            ids, fc = r
            fr = oracle.to_frequencies(fc)
            for j, a in enumerate(ids):
                cols.append(fr[:, j]); covs.append(fc.sum(axis=1).astype(np.float64)); loc.append(l); al.append(int(a))
        assert len(cols) == G.shape[0] > 0 and col_locus.tolist() == loc and col_allele.tolist() == al
        assert np.array_equal(G[:, :n], np.stack(cols), equal_nan=True) and np.all(G[:, n:] == 0.0)
        assert np.array_equal(cov[:, :n], np.stack(covs), equal_nan=True)
    return Op(f"loader{tag} L={L} n={n} seed={seed}", lambda e: e.load_frequencies(counts, ps, Filter(), coverages=True), check)


def popgen_inputs(engine, L, n, seed, win, slide, minl, counts=None):
    """the loaded matrix of a counts batch (prepared on the session's engine) with its windows"""
    from poolgen_amd import Filter
    if counts is None:
        counts = cached(("suite_counts", L, n, seed), lambda: suite_counts(L, n, seed))
    ps = diversity_sizes(n)
    G, col_locus, col_allele, cov = engine.load_frequencies(counts, ps, Filter(), coverages=True)
    cl = col_locus.cpu().numpy()
    starts = [0] + [i for i in range(1, len(cl)) if cl[i] != cl[i - 1]] + [len(cl)]
    loci = cl[starts[:-1]]
    rng = np.random.default_rng(2)
    chrom = np.sort(rng.integers(0, 3, size=L))
    pos = np.concatenate([np.sort(rng.choice(np.arange(1, 40 * L), size=int((chrom == c).sum()), replace=False)) for c in range(3)])
    wh, wt = engine.sliding_windows(chrom[loci], pos[loci], win, slide, minl)
    assert len(wh) > 3
    return dict(G=G, cov=cov, col_locus=col_locus, col_allele=col_allele, starts=starts, wh=wh, wt=wt, ps=ps, n=n, chrom=chrom, pos=pos)


def popgen_ops(I, tag):
    G, cov, starts, wh, wt, ps, n = (I[k] for k in ("G", "cov", "starts", "wh", "wt", "ps", "n"))

    def oracle_inputs():
        Gh, ch = G.cpu().numpy(), cov.cpu().numpy()
        return np.vstack([np.ones(n), Gh[:, :n]]), [s + 1 for s in starts], ch[starts[:-1], :n].copy()

    def check_fst(res):
        import oracle_lib
        Xt, loci_idx, covs = oracle_inputs()
        rc, rmean, rwin = oracle_lib.load().fst(Xt, loci_idx, covs, wh, wt)
        assert rc == 0 and np.array_equal(res[1], rwin) and np.allclose(res[0], rmean, rtol=1e-12, atol=1e-15)

    def check_pi(res):
        import oracle_lib
        Xt, loci_idx, covs = oracle_inputs()
        rpw, rpm = oracle_lib.load().theta_pi(Xt, loci_idx, covs, wh, wt)
        assert np.array_equal(res[0], rpw) and np.array_equal(res[1], rpm)

    def check_tajima(res):
        import oracle_lib
        from test_gpu_popgen_diversity import restate, same
        Xt, loci_idx, covs = oracle_inputs()
        S, theta, tm, pi, d, dm = restate(oracle_lib.load(), Xt, loci_idx, covs, wh, wt, ps, None)
        gd, gdm, gtheta, gpi = res
        assert np.array_equal(gtheta, theta) and np.array_equal(gpi, pi) and same(gd, d) and same(gdm, dm)
    return {"fst": Op("fst " + tag, lambda e: e.fst(G, cov, starts, wh, wt, n=n), check_fst),
            "theta_pi": Op("theta_pi " + tag, lambda e: e.theta_pi(G, cov, starts, wh, wt, n=n), check_pi),
            "tajima_d": Op("tajima_d " + tag, lambda e: e.tajima_d(G, cov, starts, wh, wt, ps, n=n), check_tajima)}


def csv_op(I, tag):
    """B = freq_csv of the loaded matrix: the text, byte for byte the host formatter's"""
    names = ("chr1", "scaffold_12.1", "X")
    G, cl, ca, n = I["G"], I["col_locus"], I["col_allele"], I["n"]

    def check(res):
        from poolgen_amd.engine import freq_csv_host
        want = freq_csv_host(G.cpu().numpy(), cl.cpu().numpy(), ca.cpu().numpy(), I["chrom"], I["pos"], names, n=n, n_threads=4)
        assert res.tobytes() == want
    return Op("freq_csv " + tag, lambda e: e.freq_csv(G, cl, ca, I["chrom"], I["pos"], names, n=n), check)


BLOCK = 500     # a long text is a block of this many generated lines, repeated (the parsers do not care that positions repeat)


def sync_text(n, lines, seed):
    block = sync_corpus.random_text(np.random.default_rng(seed), n, min(lines, BLOCK), comment_every=9)[0]
    assert lines <= BLOCK or lines % BLOCK == 0
    return block * max(1, lines // BLOCK)


def vcf_text(n, lines, seed):
    rng = np.random.default_rng(seed)
    block = "".join(vcf_corpus.data_line(rng, n, short_ad=i % 5 == 4) for i in range(min(lines, BLOCK)))
    assert lines <= BLOCK or lines % BLOCK == 0
    return (vcf_corpus.HEADER + vcf_corpus.chrom_line(n) + block * max(1, lines // BLOCK)).encode("latin-1")


def pileup_text(n, lines, seed):
    rng = random.Random(seed)
    block = b"".join(pileup_corpus.good_line(rng, n) + b"\n" for _ in range(min(lines, BLOCK)))   # short read strings: 1 to 12 reads a pool
    assert lines <= BLOCK or lines % BLOCK == 0
    return block * max(1, lines // BLOCK)


def sync_op(n, lines, seed):
    text = cached(("sync", n, lines, seed), lambda: sync_text(n, lines, seed))

    def check(res):
        from poolgen_amd import sync_parse_host
        from test_gpu_sync_parse import same
        got = dict(res); got["counts"] = got["counts"].view(np.uint32); got["pos"] = got["pos"].view(np.uint64)
        want = sync_parse_host(text, 0, n_threads=16)
        same(got, want, f"sync {lines} lines")
        assert got["data_lines"] == lines and len(want["pos"]) == lines
    return Op(f"sync_parse n={n} lines={lines}", lambda e: e.sync_parse(text), check)


def vcf_op(n, lines, seed):
    text = cached(("vcf", n, lines, seed), lambda: vcf_text(n, lines, seed))
    sizes = (np.random.default_rng(seed).integers(5, 60, size=n) * 1.0).tolist()

    def check(res):
        from poolgen_amd import vcf_parse_host
        from test_gpu_vcf import same
        got = dict(res); got["counts"] = got["counts"].view(np.uint32); got["pos"] = got["pos"].view(np.uint64)
        want = vcf_parse_host(text, sizes, 30, 0.75, 0.1, n_threads=16)
        same(got, want, f"vcf {lines} lines")
        assert got["data_lines"] == lines and 0 < len(want["pos"]) < lines, (got["data_lines"], len(want["pos"]))
    return Op(f"vcf_parse n={n} lines={lines}", lambda e: e.vcf_parse(text, sizes, 30, 0.75, 0.1), check)


def pileup_op(n, lines, seed):
    text = cached(("pileup", n, lines, seed), lambda: pileup_text(n, lines, seed))
    sizes = [1.0 / n] * n
    rule = dict(pileup_corpus.BASE)

    def check(res):
        from poolgen_amd import pileup_parse_host
        from test_gpu_pileup_parse import same
        got = dict(res); got["counts"] = got["counts"].view(np.uint32); got["pos"] = got["pos"].view(np.uint64)
        want = pileup_parse_host(text, sizes, **rule, n_threads=16)
        same(got, want, f"pileup {lines} lines")
        assert got["lines"] == lines and 0 < len(want["pos"]) <= lines, (got["lines"], len(want["pos"]))
    return Op(f"pileup_parse n={n} lines={lines}", lambda e: e.pileup_parse(text, sizes, **rule), check)


def ridge_op(n, p, seed, n_folds=3, G=None, Y=None, tag=""):
    from test_gpu_dispatch_edges_gp import assert_path, design, host_xt, make_folds, spread_rows
    if G is None:
        G, Y = cached(("design", n, p, seed), lambda: design(n, p, 1, seed))
    rows = spread_rows(n)
    folds = make_folds(len(rows), n_folds, 1, seed=n)

    def check(res):
        import oracle_lib
        got = (torch.from_numpy(res[0]),) + tuple(res[1:])
        assert_path(got, oracle_lib.load().penalised_lambda_path(host_xt(G, n), Y, rows, folds, n_folds, alpha=0.0, n=n), f"ridge n={n} p={p}")
    return Op(f"gp_ridge{tag} n={n} p={p} seed={seed}", lambda e: e.gp_ridge(G, Y, rows, folds, n_folds, alpha=0.0, n=n), check)


# =============================================================================================================================
# a. the fused intercept-only sums must never describe another matrix
# =============================================================================================================================
FUSED_CASES = [(1501, 100, 1), (1501, 100, 2), (1501, 40, 1)]      # the odd locus count: the `half` rounding of k_sweep_finish_x2
for _p, _n, _k in FUSED_CASES:
    assert R.kin_fuses(_n, _k) and R.ms_fits(_n, 1 + _k, 0), (_n, _k)


def fused_inputs(oracle, p, n, k):
    """G1, G2 (two seeds), the phenotypes of the first; from the oracle alone: m = 0 for both, and fits that differ at >= 99 % of the
    loci by more than 1e-6 -- a stale answer cannot pass for the right one"""
    def build():
        G1, Y2 = make(p, n, 7)
        G2, _ = make(p, n, 8)
        Y = np.ascontiguousarray(Y2[:, :k])
        r1, r2 = (oracle.ols_with_covariate(G.cpu().numpy(), Y, 0.75, n=n) for G in (G1, G2))
        assert r1["m"] == 0 and r2["m"] == 0
        rel = np.abs(r1["beta"] - r2["beta"]) / np.maximum(np.abs(r2["beta"]), 1e-300)
        assert (rel > 1e-6).all(axis=1).mean() >= 0.99
        return G1, G2, Y
    return cached(("fused", p, n, k), build)


def after_composed_call(e, G1, G2, Y, n, k, history, bare):
    """history on G (= G1's values), G overwritten with G2's, then B: the sums of the history must not answer for the new matrix"""
    p = G1.shape[0]
    B = sweep_op(p, n, k, 8, G=G2, Y=Y, tag=" after another matrix")
    reference(B)
    G = G1.clone()
    e.profile(True)
    c0 = launches(e)
    if history == "composed":
        m = e.ols_with_covariate(G, Y, 0.75, n=n)[0]
    else:
        m = e.ols_with_covariate_sharded(G, p, Y, 0.75, n=n, want_K=True)[0]
    assert m == 0 and launches(e) == c0 + 1, "the history must have taken the fused route (k_sweep_finish)"
    return G, B, c0 + 1


@pytest.mark.parametrize("bare", [False, True], ids=["set+sweep", "sweep-alone"])
@pytest.mark.parametrize("history", ["composed", "sharded"])
@pytest.mark.parametrize("p,n,k", FUSED_CASES)
def test_fused_sums_do_not_outlive_a_composed_call(oracle, p, n, k, history, bare):
    """pg_ols_kinship_dev / pg_ols_kinship_sharded_dev announce the phenotypes themselves and used to return with the sums armed:
    the next pg_ols_sweep_dev on the same pointer and shape -- after the caller overwrote the matrix -- closed the OLD matrix's
    fits from them, return code 0.  (pg_covariates_set with the same Y takes its steady-state return and changes nothing.)"""
    G1, G2, Y = fused_inputs(oracle, p, n, k)
    with fresh() as e:
        G, B, c1 = after_composed_call(e, G1, G2, Y, n, k, history, bare)
        G.copy_(G2)
        if not bare:
            e.covariates_set(n, None, Y)
        got = e.ols_sweep(G, k, n)
        must_equal_fresh(B, got, f"after {history} + copy_")
        assert launches(e) == c1, "the sweep after the composed call closed its fits from that call's sums"


@pytest.mark.parametrize("p,n,k", FUSED_CASES[:1])
def test_fused_sums_do_not_outlive_a_freed_matrix(oracle, p, n, k):
    """the same with G freed and another tensor of its shape allocated: runs when the allocator hands the address out again"""
    G1, G2, Y = fused_inputs(oracle, p, n, k)
    with fresh() as e:
        G, B, c1 = after_composed_call(e, G1, G2, Y, n, k, "composed", False)
        ptr = G.data_ptr()
        del G
        Gn = torch.empty_like(G2)
        if Gn.data_ptr() != ptr:
            pytest.skip("the allocator returned another address for the new matrix (the copy_ variant covers the rule)")
        Gn.copy_(G2)
        e.covariates_set(n, None, Y)
        got = e.ols_sweep(Gn, k, n)
        must_equal_fresh(B, got, "after composed + free + allocate")
        assert launches(e) == c1


@pytest.mark.parametrize("writer", ["impute_mean", "set_missing_by_depth", "load_emit"])
def test_library_writes_into_the_matrix_drop_the_fused_sums(oracle, writer):
    """explicit opt-in and kinship pass, then a LIBRARY call writes into the matrix of the sums: the sweep reads G again.  (The
    loader really replaces the values.  The two imputation calls find nothing to change in a complete matrix, so the matrix is
    overwritten after them to make an answer from the old sums visible: the library dropped them at its own call.)"""
    from poolgen_amd import Filter
    p, n, k = FUSED_CASES[0]
    G1, G2, Y = fused_inputs(oracle, p, n, k)
    with fresh() as e:
        e.profile(True)
        e.set_phenotypes(Y)
        if writer == "load_emit":
            counts = cached(("suite_counts", 900, n, 99), lambda: suite_counts(900, n, 99))
            ps = np.linspace(10, 30, n)
            f = Filter().to_c()
            pp = C.c_int64()
            plan = lambda: e._lib.pg_load_plan_dev(e._ctx, counts.data_ptr(), 900, n, ps.ctypes.data, C.byref(f), 0, None, C.byref(pp))
            assert plan() == 0 and pp.value >= 900
            G = freq_matrix(pp.value, n, 3)
            cl = torch.empty(pp.value, dtype=torch.int64, device="cuda"); ca = torch.empty(pp.value, dtype=torch.int32, device="cuda")
            e.kinship_partial(G, n)                      # the sums of the random matrix; (the pass also ends the plan above)
            assert plan() == 0
            assert e._lib.pg_load_emit_dev(e._ctx, None, n, G.data_ptr(), G.shape[1], cl.data_ptr(), ca.data_ptr()) == 0
            after = G.clone()
        else:
            G = G1.clone()
            e.kinship_partial(G, n)
            if writer == "impute_mean":
                e.impute_mean(G, np.arange(p + 1), n=n)
            else:
                e.set_missing_by_depth(G, torch.full_like(G, 100.0), np.arange(p + 1), 5.0, n=n)
            assert torch.equal(G, G1)
            G.copy_(G2)
            after = G2
        B = sweep_op(after.shape[0], n, k, 0, G=after, Y=Y, tag=f" after {writer}")
        c0 = launches(e)
        e.covariates_set(n, None, Y)
        got = e.ols_sweep(G, k, n)
        must_equal_fresh(B, got, f"after {writer}")
        assert launches(e) == c0, f"the fused sums survived {writer}"


@pytest.mark.parametrize("p,n,k", FUSED_CASES)
def test_explicit_fused_sums_serve_one_sweep(oracle, p, n, k):
    """the legitimate use: set_phenotypes, kinship_partial, kinship_set, ols_sweep with G untouched takes k_sweep_finish and agrees
    with the two-pass route at the tolerance of test_fused_and_two_pass_paths_agree_with_oracle; a second sweep reads G again"""
    G1, _, Y = fused_inputs(oracle, p, n, k)
    B = sweep_op(p, n, k, 7, G=G1, Y=Y, tag=" two-pass")
    two = reference(B)
    with fresh() as e:
        e.profile(True)
        e.set_phenotypes(Y)
        S = e.kinship_partial(G1, n)
        m, _, _ = e.kinship_set(S, p, Y, 0.75)
        c0 = launches(e)
        b, v, pv = (x.cpu().numpy() for x in e.ols_sweep(G1, k, n))
        assert m == 0 and launches(e) == c0 + 1, "the opted-in sweep must take k_sweep_finish"
        cmp_fit(tuple(torch.from_numpy(x) for x in (b, v, pv)), oracle.ols_with_covariate(G1.cpu().numpy(), Y, force_m=0, n=n), "fused")
        assert np.allclose(b, two[0], rtol=1e-9, atol=1e-12, equal_nan=True) and float(np.nanmax(np.abs(pv - two[2]))) < 1e-11
        again = e.ols_sweep(G1, k, n)
        assert launches(e) == c0 + 1, "one sweep uses the sums"
        must_equal_fresh(B, again, "second sweep after the opt-in")


@pytest.mark.parametrize("field", ["pointer", "p", "ld", "k", "Y"])
def test_explicit_fused_sums_belong_to_one_matrix_and_one_phenotype(oracle, field):
    """opt-in and kinship pass, then a sweep that differs in ONE of pointer, p, ld, k, Y: k_sweep_finish is not taken and the bits are
    the two-pass route's"""
    p, n, _ = FUSED_CASES[0]
    k = 2
    G1, _, Y = fused_inputs(oracle, p, n, k)
    ld = G1.shape[1]
    flat = torch.empty(p * (ld + 2), dtype=torch.float64, device="cuda")
    flat.copy_(freq_matrix(p + 40, n, 5).reshape(-1)[:flat.numel()])
    Ga = flat[:p * ld].view(p, ld)                    # the matrix of the kinship pass for "ld": the same memory, pitch ld
    Y_other = np.ascontiguousarray(Y[::-1])
    with fresh() as e:
        e.profile(True)
        e.set_phenotypes(Y)
        Gk = Ga if field == "ld" else G1
        e.kinship_partial(Gk, n)
        if field == "pointer":
            Gs, Ys = G1.clone(), Y
        elif field == "p":
            Gs, Ys = G1[:p - 1], Y
        elif field == "ld":
            Gs, Ys = flat.view(p, ld + 2), Y
            assert Gs.data_ptr() == Gk.data_ptr()
        elif field == "k":
            Gs, Ys = G1, np.ascontiguousarray(Y[:, :1])
        else:
            Gs, Ys = G1, Y_other
        B = sweep_op(Gs.shape[0], n, Ys.shape[1], 0, G=Gs, Y=Ys, tag=f" other {field}")
        c0 = launches(e)
        e.covariates_set(n, None, Ys)
        got = e.ols_sweep(Gs, Ys.shape[1], n)
        assert launches(e) == c0, f"sums of another {field} were used"
        must_equal_fresh(B, got, f"other {field}")


def explicit_three_calls(e, G, Y, n, p):
    """B = kinship_partial + kinship_set + ols_sweep WITHOUT pg_set_phenotypes: on a fresh context the two-pass route"""
    S = e.kinship_partial(G, n)
    m, _, _ = e.kinship_set(S, p, Y, 0.75)
    assert m == 0
    return e.ols_sweep(G, Y.shape[1], n)


@pytest.mark.parametrize("history", ["composed", "sharded"])
@pytest.mark.parametrize("p,n,k", FUSED_CASES[:2])
def test_a_composed_call_opts_nobody_in(oracle, p, n, k, history):
    """pg_ols_kinship_dev / the sharded call announce their Y for their own length.  A caller who never called pg_set_phenotypes
    then runs his own kinship pass: it must not fuse (it did: the call's announcement stayed behind), so (1) kinship_partial +
    kinship_set + ols_sweep gives the two-pass bits of a fresh context, and (2) with the matrix overwritten between his kinship pass
    and the sweep he gets the new matrix's fits, not the old one's with rc 0"""
    G1, G2, Y = fused_inputs(oracle, p, n, k)
    B1 = sweep_op(p, n, k, 7, G=G1, Y=Y, tag=" two-pass")                 # (the three calls end in the same sweep of the same state)
    with fresh() as a, fresh() as b:
        three = freeze(explicit_three_calls(a, G1, Y, n, p))
        assert first_difference(three, freeze(B1.run(b))) is None, "fresh context: three calls without opt-in = covariates_set + sweep"
    with fresh() as e:
        G, B2, c1 = after_composed_call(e, G1, G2, Y, n, k, history, False)
        must_equal_fresh(B1, explicit_three_calls(e, G, Y, n, p), f"three calls after {history}")
        assert launches(e) == c1, "the caller's kinship pass fused although he never announced phenotypes"
        e.kinship_partial(G, n)
        G.copy_(G2)
        e.covariates_set(n, None, Y)
        got = e.ols_sweep(G, k, n)
        must_equal_fresh(B2, got, f"{history}, kinship_partial, copy_, covariates_set + sweep")
        assert launches(e) == c1


def test_the_callers_announcement_across_a_composed_call(oracle):
    """the caller's own pg_set_phenotypes stays in force across a composed call for the same phenotypes (his next kinship pass
    fuses, as it would without that call) and ends when the call replaced it with other phenotypes (two-pass bits)"""
    p, n, k = FUSED_CASES[1]
    G1, _, Y = fused_inputs(oracle, p, n, k)
    Y_other = np.ascontiguousarray(Y[::-1])
    B = sweep_op(p, n, k, 7, G=G1, Y=Y, tag=" two-pass")
    two = reference(B)
    for Yc, fuses in ((Y, True), (Y_other, False)):
        with fresh() as e:
            e.profile(True)
            e.set_phenotypes(Y)
            assert e.ols_with_covariate(G1, Yc, 0.75, n=n)[0] == 0
            c0 = launches(e)
            got = freeze(explicit_three_calls(e, G1, Y, n, p))
            assert launches(e) == c0 + (1 if fuses else 0), f"same phenotypes: {fuses}"
            if fuses:
                assert np.allclose(got[0], two[0], rtol=1e-9, atol=1e-12, equal_nan=True) and float(np.nanmax(np.abs(got[2] - two[2]))) < 1e-11
            else:
                must_equal_fresh(B, got, "after a composed call with other phenotypes")


def test_a_failed_composed_call_leaves_no_sums(oracle):
    """a NaN frequency: the fused kinship pass of pg_ols_kinship_dev has run when pg_kinship_set refuses.  The caller repairs the
    matrix in place and fits it with pg_covariates_set + pg_ols_sweep_dev: the sweep reads the repaired matrix"""
    p, n, k = 130, 33, 2
    assert R.kin_fuses(n, k)
    G, Y2 = cached(("make", p, n, 81), lambda: make(p, n, 81))
    Y = np.ascontiguousarray(Y2[:, :k])
    B = sweep_op(p, n, k, 81)
    reference(B)
    with fresh() as e:
        e.profile(True)
        Gbad = G.clone(); Gbad[17, 5] = float("nan")
        state_error(lambda: e.ols_with_covariate(Gbad, Y, 0.75, n=n), PG_ERR_INVALID, "contains NaN")
        c0 = launches(e)
        Gbad.copy_(G)
        e.covariates_set(n, None, Y)
        got = e.ols_sweep(Gbad, k, n)
        must_equal_fresh(B, got, "after a failed composed call and a repair in place")
        assert launches(e) == c0, "the sums of the failed call were used"


def test_the_composed_call_fuses_on_every_step(oracle):
    """the headline use: pg_ols_kinship_dev step after step on one context re-arms on each call and keeps taking k_sweep_finish"""
    p, n, k = 2000, 100, 2                                # (a shape of test_fused_and_two_pass_paths_agree_with_oracle)
    B = kinship_op(p, n, k, 53)
    reference(B)
    with fresh() as e:
        e.profile(True)
        for step in range(3):
            c0, s0 = launches(e), launches(e, "sweep")
            got = B.run(e)
            assert launches(e) == c0 + 1 and launches(e, "sweep") == s0, f"step {step}: not the fused route"
            must_equal_fresh(B, got, f"step {step}")


# =============================================================================================================================
# b. the regression state after other users of W_dev, and interleaved analyses
# =============================================================================================================================
def gp_histories():
    from test_gpu_dispatch_edges_gp import make_folds
    n, p = 40, 600
    G, Y2 = cached(("make", p, n, 61), lambda: make(p, n, 61))
    Y = np.ascontiguousarray(Y2[:, :1])
    rows = np.arange(n)
    folds = make_folds(n, 4, 1, seed=3)
    return n, p, G, Y, {
        "gp_ols": lambda e: e.gp_ols(G, Y, rows, n=n),
        "gp_ridge": lambda e: e.gp_ridge(G, Y, rows, folds, 4, alpha=0.0, n=n),
        "gp_penalised": lambda e: e.gp_penalised(G, Y, rows, folds, 4, 0.5, n=n),
        "gp_penalised_iterative_proxy": lambda e: e.gp_penalised(G, Y, rows, folds, 4, 0.5, iterative_proxy=True, n=n),
        "gp_proxy": lambda e: e.gp_proxy(G, Y, rows, n=n),
        "mle_with_covariate": lambda e: e.mle_with_covariate(G, Y, n=n),
    }


@pytest.mark.parametrize("user", ["gp_ols", "gp_ridge", "gp_penalised", "gp_penalised_iterative_proxy", "gp_proxy", "mle_with_covariate"])
def test_other_users_of_the_coefficient_table_leave_no_regression_state(user):
    """W_dev also carries the Z of the GP coefficient passes and the MLE's sums: after them a bare sweep is a call-order error
    (PG_ERR_STATE), never a fit against a coefficient table, and pg_covariates_set with the SAME n and Y (m = 0) uploads again -- its
    steady-state return must not fire on an overwritten W_dev.  The proxy models (include/poolgen_hip.h: they overwrite the context's
    covariates) leave none either: [1 | PC1] of the training pools is their own design."""
    n, p, G, Y, calls = gp_histories()
    B = sweep_op(p, n, 1, 61, G=G, Y=Y, tag=" b")
    reference(B)
    with fresh() as e:
        must_equal_fresh(B, B.run(e), "before")
        calls[user](e)
        out = torch.full((3, p, 1), -7.25, dtype=torch.float64, device="cuda")
        state_error(lambda: e.ols_sweep(G, 1, n, out), PG_ERR_STATE)
        torch.cuda.synchronize()
        assert bool((out == -7.25).all()), "a refused sweep wrote results"
        must_equal_fresh(B, B.run(e), f"after {user}")


@pytest.mark.parametrize("m", [0, 2])
@pytest.mark.parametrize("between", ["sweep", "ols_iterate", "correlation", "mle_with_covariate"])
def test_interleaved_analyses_with_other_pool_counts(between, m):
    """40 pools, 33, 40 again with the same Y on one context: the t coefficients (tcoef_dev, df = n - 1), W and syy are those of the
    current call every time -- also with a count operator or the MLE (which shares tcoef_dev) in between"""
    fit = (lambda p, n, seed: sweep_op(p, n, 2, seed)) if m == 0 else (lambda p, n, seed: kinship_op(p, n, 2, seed, force_m=2))
    A, A33 = fit(600, 40, 71), fit(600, 33, 72)
    reference(A); reference(A33)
    with fresh() as e:
        must_equal_fresh(A, A.run(e), "40 pools")
        if between == "sweep":
            must_equal_fresh(A33, A33.run(e), "33 pools after 40")
        elif between == "mle_with_covariate":
            G, Y2 = cached(("make", 600, 33, 72), lambda: make(600, 33, 72))
            e.mle_with_covariate(G, Y2[:, :1], n=33)
        else:
            op = count_ops(437, 33, 9)[between]
            must_equal_fresh(op, op.run(e), "33 pools after a sweep of 40")
        must_equal_fresh(A, A.run(e), f"40 pools again after {between}")
        must_equal_fresh(A33, A33.run(e), "33 pools at the end")


# =============================================================================================================================
# c. large first, small after: buffers that only ever grow (ws, W_dev, spec_dev, pin, lz_dev, S_dev)
# =============================================================================================================================
assert R.ms_fits(226, 3, 0) and R.ms_fits(33, 3, 0) and not R.kin_fuses(226, 1) and R.kin_fuses(33, 2) and R.kin_layout(226)["nb"] == 2


def large_then_small(small, large):
    """small after large, and small after small + large, against small as a first call"""
    reference(small)
    with fresh() as e:
        large.run(e)
        must_equal_fresh(small, small.run(e), "after the large call")
    with fresh() as e:
        must_equal_fresh(small, small.run(e), "as the first call of this context")
        large.run(e)
        must_equal_fresh(small, small.run(e), "after small, large")


def test_large_then_small_sweep_and_kinship():
    Gl, Yl = freq_matrix(3000, 226, 1), big_phenotypes(226, 2, 2)
    large_then_small(sweep_op(130, 33, 2, 81), sweep_op(3000, 226, 2, 0, G=Gl, Y=Yl, tag=" large"))
    large_then_small(kinship_op(130, 33, 2, 81), kinship_op(3000, 226, 2, 0, G=Gl, Y=Yl, tag=" large"))
    # the fused kinship pass large (one pool block, 200 pools), then small: spec_dev keeps the larger call's sums
    Gf, Yf = freq_matrix(3000, 200, 3), big_phenotypes(200, 2, 4)
    large_then_small(kinship_op(130, 33, 2, 81), kinship_op(3000, 200, 2, 0, G=Gf, Y=Yf, tag=" large fused"))
    # the lazy route (K_out = NULL): lz_dev and pin
    lazy = lambda G, Y, n, name: Op(name, lambda e: e.ols_with_covariate(G, Y, 0.75, n=n, want_K=False), kinship_lazy_check(G, Y, n))
    Gs, Ys2 = cached(("make", 130, 33, 81), lambda: make(130, 33, 81))
    large_then_small(lazy(Gs, Ys2, 33, "lazy kinship p=130 n=33"), lazy(Gl, Yl, 226, "lazy kinship large"))


def kinship_lazy_check(G, Y, n):
    def check(res):
        import oracle_lib
        m, K, beta, var, pv = res
        ref = oracle_lib.load().ols_with_covariate(G.cpu().numpy(), Y, 0.75, n=n)
        assert m == ref["m"] == 0 and K is None
        cmp_fit(tuple(torch.from_numpy(x) for x in (beta, var, pv)), ref, "lazy route")
    return check


@pytest.mark.parametrize("name", ["ols_iterate", "correlation", "chisq", "loader"])
def test_large_then_small_count_operators_and_loader(name):
    big = cached(("deep_counts", 4000, 226), lambda: deep_counts(4000, 226, 11))
    if name == "loader":
        small, large = loader_op(437, 31, 9), loader_op(4000, 226, 0, counts=big, tag=" large")
    else:
        small, large = count_ops(437, 31, 9)[name], count_ops(4000, 226, 0, counts=big, Y=big_phenotypes(226, 2, 12), tag=" large")[name]
    large_then_small(small, large)


@pytest.mark.parametrize("name", ["fst", "theta_pi", "tajima_d", "freq_csv"])
def test_large_then_small_popgen_and_csv(engine, name):
    Is = cached("popgen small", lambda: popgen_inputs(engine, 437, 31, 9, 400, 200, 2))
    Il = cached("popgen large", lambda: popgen_inputs(engine, 4000, 226, 0, 20000, 10000, 10,
                                                      counts=cached(("deep_counts", 4000, 226), lambda: deep_counts(4000, 226, 11))))
    if name == "freq_csv":
        small, large = csv_op(Is, "L=437 n=31"), csv_op(Il, "large")
    else:
        small, large = popgen_ops(Is, "L=437 n=31")[name], popgen_ops(Il, "large")[name]
    large_then_small(small, large)


@pytest.mark.parametrize("parser", ["sync_parse", "vcf_parse", "pileup_parse"])
def test_large_then_small_parsers(parser):
    """a text of a few hundred lines against one of 20 000: the second reservation of the large call replaces the workspace the
    first one filled (PgLineIndex of pg_text_steps.h rebuilds the front part whenever that happened), and the small call after it parses
    inside a workspace full of the large one's line tables"""
    mk = {"sync_parse": sync_op, "vcf_parse": vcf_op, "pileup_parse": pileup_op}[parser]
    small, large = mk(5, 300, 21), mk(5, 20000, 22)
    reference(large)
    large_then_small(small, large)
    with fresh() as e:                                  # the large text on a context whose workspace holds the small call's
        small.run(e)
        must_equal_fresh(large, large.run(e), "large after small")


def test_large_then_small_gp_ridge():
    Gl, Yl = freq_matrix(3000, 226, 5), big_phenotypes(226, 1, 6)
    large_then_small(ridge_op(33, 130, 91), ridge_op(226, 3000, 0, G=Gl, Y=Yl, tag=" large"))


# =============================================================================================================================
# d. the loader plan lives in the workspace: every other workspace user invalidates it
# =============================================================================================================================
CANARY = -7.25


class LoaderCall:
    """pg_load_plan_dev / pg_load_emit_dev through ctypes, the outputs embedded in canary-filled buffers"""

    def __init__(self, native, e, counts, ps, pad=64):
        from poolgen_amd import Filter
        self.native, self.e, self.counts, self.ps, self.pad = native, e, counts, ps, pad
        self.f = Filter().to_c()
        self.n = counts.shape[1]
        self.ld = self.n + (self.n & 1)

    def plan(self):
        p = C.c_int64(-1)
        c = self.counts
        rc = self.native.pg_load_plan_dev(self.e._ctx, c.data_ptr(), c.shape[0], self.n, self.ps.ctypes.data, C.byref(self.f), 0, None, C.byref(p))
        assert rc == 0, self.native.pg_last_error(self.e._ctx)
        self.p = p.value
        pad = self.pad
        self.G = torch.full(((self.p + 2 * pad) * self.ld,), CANARY, dtype=torch.float64, device="cuda")
        self.cl = torch.full((self.p + 2 * pad,), -77, dtype=torch.int64, device="cuda")
        self.ca = torch.full((self.p + 2 * pad,), -77, dtype=torch.int32, device="cuda")
        return self.p

    def emit(self):
        pad = self.pad
        rc = self.native.pg_load_emit_dev(self.e._ctx, None, self.n, self.G[pad * self.ld:].data_ptr(), self.ld, self.cl[pad:].data_ptr(),
                                          self.ca[pad:].data_ptr())
        torch.cuda.synchronize()
        return rc

    def untouched(self):
        return bool((self.G == CANARY).all()) and bool((self.cl == -77).all()) and bool((self.ca == -77).all())

    def result(self):
        pad, p, ld = self.pad, self.p, self.ld
        assert bool((self.G[:pad * ld] == CANARY).all()) and bool((self.G[(pad + p) * ld:] == CANARY).all()), "emit wrote outside G"
        assert bool((self.cl[:pad] == -77).all()) and bool((self.cl[pad + p:] == -77).all()) and bool((self.ca[:pad] == -77).all()) and \
            bool((self.ca[pad + p:] == -77).all()), "emit wrote outside the labels"
        return freeze((self.G[pad * ld:(pad + p) * ld].view(p, ld), self.cl[pad:pad + p], self.ca[pad:pad + p]))


def loader_reference(native):
    def build():
        counts = cached(("suite_counts", 437, 31, 9), lambda: suite_counts(437, 31, 9))
        ps = diversity_sizes(31)
        op = loader_op(437, 31, 9)
        ref = reference(op)
        with fresh() as e:
            lc = LoaderCall(native, e, counts, ps)
            lc.plan()
            assert lc.emit() == 0
            got = lc.result()
        assert first_difference(got, tuple(ref[:3])) is None, "ctypes plan + emit against Engine.load_frequencies"
        return counts, ps, got
    return cached("loader reference", build)


WS_USERS = ["kinship_partial", "chisq", "freq_csv", "sync_parse", "vcf_parse", "gp_predict"]


def workspace_user(engine, name):
    """one call of each user of the context's workspace, as a function of the engine that runs it"""
    if name == "kinship_partial":
        G, _ = cached(("make", 130, 33, 81), lambda: make(130, 33, 81))
        return lambda e: e.kinship_partial(G, 33)
    if name == "chisq":
        return count_ops(437, 31, 9)["chisq"].run
    if name == "freq_csv":
        return csv_op(cached("popgen small", lambda: popgen_inputs(engine, 437, 31, 9, 400, 200, 2)), "L=437 n=31").run
    if name == "sync_parse":
        return sync_op(5, 300, 21).run
    if name == "vcf_parse":
        return vcf_op(5, 300, 21).run
    G, _ = cached(("make", 130, 33, 81), lambda: make(130, 33, 81))
    beta = torch.ones((131, 1), dtype=torch.float64, device="cuda")
    return lambda e: e.gp_predict(G, beta, n=33)                       # the GP pass that reserves the workspace (pg_gp_predict_dev)


@pytest.mark.parametrize("user", WS_USERS)
def test_a_workspace_user_between_plan_and_emit(engine, native, user):
    """after pg_load_plan_dev, one call of another workspace user: pg_load_emit_dev answers PG_ERR_STATE and writes nothing; plan and
    emit again give the bytes of a fresh context"""
    counts, ps, want = loader_reference(native)
    call = workspace_user(engine, user)
    with fresh() as e:
        lc = LoaderCall(native, e, counts, ps)
        lc.plan()
        call(e)
        assert lc.emit() == PG_ERR_STATE, f"emit after {user}"
        assert b"pg_load_plan_dev" in native.pg_last_error(e._ctx)
        assert lc.untouched(), f"the refused emit after {user} wrote into its outputs"
        lc.plan()
        assert lc.emit() == 0, native.pg_last_error(e._ctx)
        assert first_difference(lc.result(), want) is None, f"plan, {user}, failed emit, plan, emit"


def test_plan_then_emit_twice(native):
    counts, ps, want = loader_reference(native)
    with fresh() as e:
        lc = LoaderCall(native, e, counts, ps)
        lc.plan()
        assert lc.emit() == 0
        one = lc.result()
        lc.G.fill_(CANARY); lc.cl.fill_(-77); lc.ca.fill_(-77)
        assert lc.emit() == 0
        assert first_difference(lc.result(), one) is None and first_difference(one, want) is None


# =============================================================================================================================
# e. after an error return
# =============================================================================================================================
def error_cases(engine):
    """name -> (the failing call, return code, what pg_last_error names, the next call of the same family, one of another family)"""
    from poolgen_amd import Filter
    G, Y2 = cached(("make", 130, 33, 81), lambda: make(130, 33, 81))
    Y = np.ascontiguousarray(Y2[:, :2])
    Ynan = Y.copy(); Ynan[3, 0] = np.nan
    Gnan = G.clone(); Gnan[17, 5] = float("nan")
    sweep, kin = sweep_op(130, 33, 2, 81), kinship_op(130, 33, 2, 81)
    counts = count_ops(437, 31, 9)
    Is = cached("popgen small", lambda: popgen_inputs(engine, 437, 31, 9, 400, 200, 2))
    pop = popgen_ops(Is, "L=437 n=31")
    text, n_exp, off, reason = sync_corpus.error_texts()["five_counts"]
    vtext, vsizes, vd, vb, vf, voff, vreason = vcf_corpus.error_texts()["no_ad"]
    Gbad = Is["G"].clone(); Gbad[1, 0] = 0.9
    big = cached(("suite_counts", 437, 31, 9), lambda: suite_counts(437, 31, 9)).clone()
    big[17, 2, 0] = 1 << 29
    ps = np.linspace(10, 30, 31)
    return {
        "nan_phenotype": (lambda e: e.covariates_set(33, None, Ynan), PG_ERR_INVALID, "NaN", sweep, sync_op(5, 300, 21)),
        "nan_frequency": (lambda e: e.ols_with_covariate(Gnan, Y, 0.75, n=33), PG_ERR_INVALID, "contains NaN", kin, counts["chisq"]),
        "no_residual_df": (lambda e: e.ols_with_covariate(G, Y, 0.75, force_m=31, n=33), PG_ERR_UNSUPPORTED, "no residual degrees of freedom", kin,
                           csv_op(Is, "L=437 n=31")),
        "broken_sync_line": (lambda e: e.sync_parse(text, n_exp), PG_ERR_INVALID, f"byte {off} ", sync_op(5, 300, 21), sweep),
        "vcf_line_without_ad": (lambda e: e.vcf_parse(vtext, vsizes, vd, vb, vf), PG_ERR_INVALID, f"byte {voff} ", vcf_op(5, 300, 21), loader_op(437, 31, 9)),
        "fst_not_summing_to_one": (lambda e: e.fst(Gbad, Is["cov"], Is["starts"], Is["wh"], Is["wt"], n=31), PG_ERR_INVALID, "do not sum up to one",
                                   pop["fst"], kin),
        "count_of_2_to_the_29": (lambda e: e.ols_iterate(big, ps, Filter(), count_Y(31)), PG_ERR_INVALID, "2^29",
                                 counts["ols_iterate"], sync_op(5, 300, 21)),
    }


@pytest.mark.parametrize("case", ["nan_phenotype", "nan_frequency", "no_residual_df", "broken_sync_line", "vcf_line_without_ad",
                                  "fst_not_summing_to_one", "count_of_2_to_the_29"])
def test_after_an_error_return(engine, case):
    """an argument or data check that the library answers with a return code (none of them reaches a fault): pg_last_error names the
    failure, and the next valid call of the same family and of another one give the bits of a fresh context"""
    fail, code, text, same_family, other = error_cases(engine)[case]
    reference(same_family); reference(other)
    with fresh() as e:
        with pytest.raises(Exception) as err:
            fail(e)
        msg = e._lib.pg_last_error(e._ctx).decode()
        assert text in msg, (case, msg)
        assert f"({code})" in str(err.value) or type(err.value).__name__ in ("SyncError", "VcfError"), str(err.value)
        must_equal_fresh(same_family, same_family.run(e), f"after {case}")
        must_equal_fresh(other, other.run(e), f"after {case}, another family")
    with fresh() as e:                                  # and with state from a valid call before the failure
        same_family.run(e)
        with pytest.raises(Exception):
            fail(e)
        must_equal_fresh(other, other.run(e), f"after valid, {case}: another family")
        must_equal_fresh(same_family, same_family.run(e), f"after valid, {case}")


# =============================================================================================================================
def test_zz_determinism_fallback_list():
    """printed by every run of this file: the operators that could not be compared bit for bit, with the reason"""
    print(f"\n[context state] determinism-probe fallback list ({len(FALLBACK)} operators): {FALLBACK}")
    print(f"[context state] {len(_REF)} operations probed on two fresh contexts each; wall time of the file so far {time.time() - _T0[0]:.1f} s")
    assert len(FALLBACK) <= 2, FALLBACK
