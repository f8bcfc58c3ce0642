"""The count operators on every pair of allele columns.  From 31 pools up every other test feeds them synth.sync_counts, whose
alleles sit in columns A and T; the kernels choose code by exactly that (pg_locus_ops.hip: the wave-uniform NAC = 2 branch of the
streaming pass and its re-used quotients, `pair_at` of the rows kernel, the speculated pair, the tie rules).  Here the loci come from
tests/count_corpus.py: all 30 ordered pairs, triples, ties, late and stray alleles, uncovered heads, shuffled so that one wave holds
many pairs.  tests/test_count_corpus.py proves on the CPU that no locus of the corpus has a rank-deficient design, so check_stat_op
must excuse none.  Tolerances are the suite's: emission and ids bit-exact, statistics 1e-10, Pearson r one unit of 7 decimals."""
import numpy as np
import pytest
import torch

import count_corpus as cc
import fisher_ref
import test_gpu_fisher
from test_count_corpus import FILTERS, POOL_COUNTS, corpus
from test_gpu_dispatch_edges import COUNT_POINTS, check_chisq, check_loader
from test_gpu_locus_ops import check_stat_op, flt_pair, ols_kernel  # noqa: F401  (ols_kernel: the rows / stream fixture)

pytestmark = pytest.mark.gpu
FILTER_IDS = ["ns-maf01", "keepns-maf001", "miss50"]
assert set(POOL_COUNTS) <= set(COUNT_POINTS)    # 31 streaming pass, odd; 32 first rows count; 113 32-lane rows, odd; 226 64-lane; 449 above
_dev = {}


def batch(n):
    """the corpus at n pools, once: host counts (read-only), tags, the device copy, pool sizes, two traits"""
    if n not in _dev:
        counts, tags = corpus(n)
        _dev[n] = (counts, tags, torch.from_numpy(counts.astype(np.int32)).cuda(), cc.pool_sizes(n), cc.phenotypes(n, 2))
    return _dev[n]


def tie_sums_report(n_out, ids, counts, tags, higher):
    """every emitted tie-sums locus reports one allele: the higher of its two slots (ols_iter) or the lower (pearson_corr)"""
    seen = 0
    for l in np.flatnonzero(tags == "tie-sums"):
        if n_out[l]:
            lo, hi = cc.read_slots(counts[l])
            assert n_out[l] == 1 and ids[l, 0] == (hi if higher else lo), f"tie-sums locus {l}: slots {lo}, {hi}, reported {ids[l, 0]}"
            seen += 1
    return seen


@pytest.mark.parametrize("fi", range(3), ids=FILTER_IDS)
@pytest.mark.parametrize("n", POOL_COUNTS)
def test_statistics_on_every_allele_pair(engine, oracle, monkeypatch, n, fi, ols_kernel):
    counts, tags, dev, ps, Y = batch(n)
    L = len(tags)
    f, fo = flt_pair(oracle, **FILTERS[fi])
    rows = counts.astype(np.uint64)
    res = engine.ols_iterate(dev, ps, f, Y)
    if ols_kernel == "stream":
        loci, listed = engine.last_listed()
        assert loci == L and 0 < listed < L, f"{listed} of {loci} loci listed: both the in-place closing and the second pass must run"
    assert check_stat_op(res, oracle.ols_iterate_locus, rows, Y, ps, fo, oracle=oracle) == 0
    assert tie_sums_report(res[0].cpu().numpy(), res[1].cpu().numpy(), counts, tags, True) >= 20
    res = engine.correlation(dev, ps, f, Y)
    assert check_stat_op(res, oracle.correlation_locus, rows, Y, ps, fo, stat_rtol=0, stat_atol=1.0000001e-7) == 0
    assert tie_sums_report(res[0].cpu().numpy(), res[1].cpu().numpy(), counts, tags, False) >= 20
    chi = engine.chisq(dev, ps, f)
    check_chisq(chi, rows, ps, fo, oracle)
    if n in (113, 226):                          # the rows kernel's register and buffered variants (as test_chisq_register_and_buffer_variants_agree)
        monkeypatch.setenv("POOLGEN_ROWS_DIRECT", "0")
        for x, y in zip(chi, engine.chisq(dev, ps, f)):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy(), equal_nan=True)


def deepened(counts, tags):
    """a few pools of every third locus sequenced 40 times deeper (as test_gpu_fisher.test_synthetic_counts): with many equally deep
    pools the table scaled to 34 reads is all zero"""
    out = counts.copy()
    rng = np.random.default_rng(len(tags))
    n = counts.shape[1]
    for l in range(0, len(tags), 3):
        if tags[l] != "deep":
            out[l, rng.choice(n, size=int(rng.integers(1, 6)), replace=False), :] *= 40
    return out


@pytest.mark.parametrize("deep_pools", [False, True], ids=["corpus", "deepened"])
@pytest.mark.parametrize("fi", range(3), ids=FILTER_IDS)
@pytest.mark.parametrize("n", [32, 113])
def test_fisher_on_every_allele_pair(engine, oracle, n, fi, deep_pools):
    counts, tags, _, ps, _ = batch(n)
    if deep_pools:
        counts = deepened(counts, tags)
    f, fo = flt_pair(oracle, **FILTERS[fi])
    got = test_gpu_fisher.run_gpu(engine, counts, ps, f)
    # numbers: one locus per family through the literal restatement (quadratic in n p), every other locus through the compacted one
    emitted = np.flatnonzero(got[0] > 0)
    lit = [int(emitted[tags[emitted] == t][0]) for t in cc.TAGS if (tags[emitted] == t).any()][:: 1 if n == 32 else 3]
    comp = [int(l) for l in emitted if l not in set(lit)]
    n_emitted, compared, worst = test_gpu_fisher.check(oracle, counts, ps, fo, got, literal=lit, compact=comp)
    tables = sum(1 for l in comp if fisher_ref.scaled(oracle.filter_locus(counts[l].astype(np.uint64), ps, fo)[1]).any())
    print(f"fisher n={n} {FILTER_IDS[fi]} deepened={deep_pools}: {n_emitted} loci emit a row, {len(lit)} literal + {len(comp)} compacted "
          f"comparisons, {tables} scaled tables with a non-zero cell, worst relative deviation {worst:.3g}")
    assert compared == n_emitted > len(tags) // 2
    assert not deep_pools or tables > 50


@pytest.mark.parametrize("kpm1", [False, True], ids=["all-alleles", "p-minus-1"])
@pytest.mark.parametrize("fi", range(3), ids=FILTER_IDS)
@pytest.mark.parametrize("n", [31, 113, 449])
def test_loader_on_every_allele_pair(engine, oracle, n, fi, kpm1):
    counts, tags, dev, ps, _ = batch(n)
    f, fo = flt_pair(oracle, **FILTERS[fi])
    ncol, col_locus, col_allele = check_loader(engine, oracle, dev, counts.astype(np.uint64), ps, f, fo, keep_p_minus_1=kpm1)
    assert ncol > len(tags) // 2
    ties = 0
    for l in np.flatnonzero(tags == "tie-sums"):     # the stable sort keeps the lower slot first = major: --keep-p-minus-1 drops it
        al = col_allele[col_locus == l].tolist()
        if al:
            lo, hi = cc.read_slots(counts[l])
            assert al == ([hi] if kpm1 else [lo, hi]), f"tie-sums locus {l}"
            ties += 1
    assert ties >= 20


def live_equal(a, b):
    """two raw results (slot-major): the same bits in every specified element"""
    n_out = a[0]
    assert torch.equal(n_out, b[0])
    for x, y in zip(a[1:], b[1:]):
        if x.dim() == 1:
            live = n_out > 0
        else:
            live = torch.arange(x.shape[0], device=x.device)[:, None] < n_out[None, :]
            if x.dim() == 3:
                live = live[:, :, None].expand_as(x)
        same = (x == y) | (torch.isnan(x) & torch.isnan(y)) if x.is_floating_point() else (x == y)
        assert bool(same[live].all())


def test_second_pass_routes_on_every_allele_pair(engine, oracle, monkeypatch, ols_kernel):
    """the second pass with its list taken as it is and grouped by survivor count (as test_second_pass_routes_agree): the same bits"""
    n = 113
    counts, tags, dev, ps, Y = batch(n)
    f, fo = flt_pair(oracle, **FILTERS[1])          # N kept, maf 0.001: two to six survivors
    outs = {}
    for route in ("0", "1"):
        monkeypatch.setenv("POOLGEN_LOCUS_GROUPED", route)
        outs[route] = [tuple(x.clone() for x in engine.chisq(dev, ps, f, raw=True)),
                       tuple(x.clone() for x in engine.ols_iterate(dev, ps, f, Y, raw=True)),
                       tuple(x.clone() for x in engine.correlation(dev, ps, f, Y, raw=True))]
        loci, listed = engine.last_listed()
        assert loci == len(tags) and listed > 0
    for a, b in zip(outs["0"], outs["1"]):
        live_equal(a, b)
    rows = counts.astype(np.uint64)
    for route in ("0", "1"):
        monkeypatch.setenv("POOLGEN_LOCUS_GROUPED", route)
        assert check_stat_op(engine.ols_iterate(dev, ps, f, Y), oracle.ols_iterate_locus, rows, Y, ps, fo, oracle=oracle) == 0


@pytest.mark.parametrize("n", POOL_COUNTS)
def test_relabelled_columns_give_the_same_bits(engine, oracle, n, ols_kernel):
    """pg_locus_ops.hip says of its A/T fast paths "Same sums either way" / "the same bits".  The `clean` loci with their two alleles
    in A and T (the four the corpus has there, and the other 56 with their lower slot moved to A and their higher one to T, so that
    a wave is full of them) run the fast paths; the same counts moved to every other slot pair a' < b' run the general ones.  n_out,
    mean frequency, statistic and p-value must not change by a bit, and the ids must be the moved ones."""
    counts, tags, _, ps, Y = batch(n)
    clean = counts[tags == "clean"]
    base = np.zeros_like(clean)
    for i, c in enumerate(clean):
        lo, hi = cc.read_slots(c)
        base[i, :, 0], base[i, :, 1] = c[:, lo], c[:, hi]
    f, fo = flt_pair(oracle, remove_ns=False, maf=0.001)

    def run(c):
        d = torch.from_numpy(c.astype(np.int32)).cuda()
        return [engine.ols_iterate(d, ps, f, Y), engine.correlation(d, ps, f, Y), engine.chisq(d, ps, f), engine.fisher(d, ps, f)]

    def host(op):
        return [x.cpu().numpy() for x in op]

    want = run(base)
    assert check_stat_op(want[0], oracle.ols_iterate_locus, base.astype(np.uint64), Y, ps, fo, oracle=oracle) == 0
    want = [host(op) for op in want]
    assert all((w[0] > 0).all() for w in want)
    pairs = [p for p in cc.UNORDERED if p != (0, 1)]
    assert len(pairs) == 14
    for a, b in pairs:
        moved = np.zeros_like(base)
        moved[:, :, a], moved[:, :, b] = base[:, :, 0], base[:, :, 1]
        for name, w, g in zip(("ols_iter", "pearson_corr", "chisq_test", "fisher_exact_test"), want, run(moved)):
            what = f"{name}, A/T moved to {'ATCGND'[a]}/{'ATCGND'[b]}"
            g = host(g)
            assert np.array_equal(w[0], g[0]), what
            live = np.arange(w[1].shape[1])[None, :] < w[0][:, None]                # L x 5: the slots below n_out
            assert np.array_equal(np.where(w[1][live] == 0, a, b), g[1][live]), what
            for x, y in zip(w[2:], g[2:]):                                           # per slot (x trait), or per locus
                if x.ndim > 1:
                    x, y = x[live], y[live]
                assert np.array_equal(x, y, equal_nan=True), what


def into_a_t_c(c):
    """one biallelic locus of the corpus with its lower slot moved to A and its higher one to T; the single stray read of a
    stray-first locus goes to C"""
    slots = cc.read_slots(c)
    rare = [j for j in slots if c[:, j].sum() == 1] if len(slots) == 3 else []
    lo, hi = [j for j in slots if j not in rare]
    out = np.zeros_like(c)
    out[:, 0], out[:, 1] = c[:, lo], c[:, hi]
    if rare:
        out[:, 2] = c[:, rare[0]]
    return out


@pytest.mark.parametrize("n", [31, 113])
def test_a_t_batch_that_switches_code_inside_a_locus(engine, oracle, n, ols_kernel):
    """Which of the streaming pass' two variants a pool runs is decided per pool for the whole wave.  A batch whose alleles all sit in
    A and T, with a single C read in a few pools of a few loci, runs most pools through NAC = 2 and the pools with a C read through the
    general code, so every locus of the wave changes variant between two of its pools; a stray-first locus among them has speculated
    (A, C) when the NAC = 2 pools come, which is where `__all(rs2 == rsi)` is false inside NAC = 2."""
    counts, tags, _, ps, Y = batch(n)
    loci = [into_a_t_c(c) for t in ("clean", "late", "tie-pool0", "stray-first") for c in counts[tags == t]]
    small = np.flatnonzero(ps < 100)
    for i in range(0, 60, 3):                                  # one C read in one small pool of every third clean locus
        loci[i][small[(5 * i) % len(small)], 2] += 1
    mixed = np.stack(loci)
    order = np.random.default_rng(n).permutation(len(mixed))
    mixed = np.ascontiguousarray(mixed[order])
    assert not mixed[:, :, 3:].any() and 0 < (mixed[:, :, 2] > 0).any(axis=0).sum() < n    # pools with and without a C read
    dev = torch.from_numpy(mixed.astype(np.int32)).cuda()
    rows = mixed.astype(np.uint64)
    for kw in (dict(remove_ns=False, maf=0.001), dict(remove_ns=True, maf=0.01)):
        f, fo = flt_pair(oracle, **kw)
        assert check_stat_op(engine.ols_iterate(dev, ps, f, Y), oracle.ols_iterate_locus, rows, Y, ps, fo, oracle=oracle) == 0
        assert check_stat_op(engine.correlation(dev, ps, f, Y), oracle.correlation_locus, rows, Y, ps, fo,
                             stat_rtol=0, stat_atol=1.0000001e-7) == 0
        check_chisq(engine.chisq(dev, ps, f), rows, ps, fo, oracle)
        check_loader(engine, oracle, dev, rows, ps, f, fo, keep_p_minus_1=True)
