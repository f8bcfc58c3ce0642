"""The claims of tests/count_corpus.py, checked against the oracle alone (no GPU): what each family of loci is, that the oracle
emits what the family is meant to make it emit, and that NO emitted locus has a rank-deficient design -- so the GPU test
(test_gpu_allele_slots.py) may demand that check_stat_op excuses nothing."""
import numpy as np
import pytest

import count_corpus as cc

POOL_COUNTS = [31, 32, 113, 226, 449]
FILTERS = [dict(remove_ns=True, maf=0.01), dict(remove_ns=False, maf=0.001), dict(min_cov=0, miss=0.5, remove_ns=True, maf=0.01)]
SEED = 7
N_SLOT = 4
_memo = {}


def flt(oracle, kw):
    return oracle.filt(kw.get("remove_ns", True), kw.get("min_cov", 1), kw.get("maf", 0.001), kw.get("miss", 0.0))


def corpus(n):
    if n not in _memo:
        counts, tags = cc.corpus(n, SEED)
        counts.setflags(write=False)
        _memo[n] = (counts, tags)
    return _memo[n]


def design_cond(oracle, counts, ps, fo):
    """cond_2 of the reference's design matrix [1 | sorted frequencies without the major allele] (as test_gpu_locus_ops.design_cond)"""
    ids, fc = oracle.filter_locus(counts, ps, fo)
    fr, ids = oracle.sort_by_allele_freq(oracle.to_frequencies(fc), ids, True)
    X = np.ones_like(fr); X[:, 1:] = fr[:, 1:]
    return np.linalg.cond(X[~np.isnan(X).any(axis=1)])


@pytest.mark.parametrize("n", POOL_COUNTS)
def test_corpus_is_what_it_says(n):
    counts, tags = corpus(n)
    again, tags2 = cc.corpus(n, SEED)
    assert np.array_equal(counts, again) and tags.tolist() == tags2.tolist()          # deterministic
    L = len(tags)
    assert counts.shape == (L, n, 6) and counts.dtype == np.int64 and 300 <= L <= 420
    want = {"clean": 60, "err": 60, "late": 30, "stray-first": 30, "tie-pool0": 30, "tie-sums": 30, "order-flip": 30, "deep": 30,
            "tri": 20, "uncovered-head": 15}
    assert {t: int((tags == t).sum()) for t in cc.TAGS} == want
    # interleaved: every run of 64 neighbouring loci holds most of the families and many different slot sets
    for lo in range(0, L - 63, 32):
        assert len(set(tags[lo:lo + 64])) >= 7
        assert len({tuple(cc.read_slots(c)) for c in counts[lo:lo + 64]}) >= 12
    for tag, k in (("clean", 2), ("late", 2), ("tie-pool0", 2), ("tie-sums", 2), ("order-flip", 2), ("deep", 2), ("uncovered-head", 2),
                   ("stray-first", 3), ("tri", 3)):
        sets = [tuple(cc.read_slots(c)) for c in counts[tags == tag]]
        assert all(len(s) == k for s in sets), tag
        if k == 2:
            assert set(sets) == set(cc.UNORDERED), tag                                 # every pair of columns
    assert {tuple(cc.read_slots(c)) for c in counts[tags == "tri"]} == set(cc.TRIPLES)
    late_at = set()
    for c in counts[tags == "late"]:
        a, b = cc.read_slots(c)
        minor = a if c[:, a].sum() < c[:, b].sum() else b
        late_at.add(int(np.flatnonzero(c[:, minor])[0]))
    assert late_at == {1, 15, 16, 17, n - 1}
    for c in counts[tags == "stray-first"]:
        rare = [j for j in cc.read_slots(c) if c[:, j].sum() == 1]
        assert len(rare) == 1 and c[0, rare[0]] == 1
        assert sum(bool(c[:3, j].any()) for j in range(6) if j != rare[0]) == 1         # pools 0..2: the major allele only
    for c in counts[tags == "tie-pool0"]:
        a, b = cc.read_slots(c)
        assert c[0, a] == c[0, b] > 0
    heads = set()
    for c in counts[tags == "uncovered-head"]:
        covered = c.sum(axis=1) > 0
        u = int(np.argmax(covered))
        assert not covered[:u].any() and covered[u:].all()
        heads.add(u)
    assert heads == {1, 15, 16, 17}
    # deep: below the library's 2^29 limit, and deep enough that a 32-bit product or a float would show
    for c in counts[tags == "deep"]:
        assert c.max() < (1 << 29) and c.max() > (1 << 26) and not (c & ((1 << 20) - 1)).any()
    # order-flip: the pool-size-weighted q and the plain column sums order the two alleles differently
    ps = cc.pool_sizes(n)
    assert ps.max() / ps.min() >= 30
    w = ps / ps.sum()
    for c in counts[tags == "order-flip"]:
        a, b = cc.read_slots(c)
        fr = c[:, [a, b]] / c[:, [a, b]].sum(axis=1, keepdims=True)
        q, cs = w @ fr, fr.sum(axis=0)
        assert (q[0] - q[1]) * (cs[0] - cs[1]) < 0 and abs(q[0] - q[1]) > 0.1 and abs(cs[0] - cs[1]) > 0.1 * n


@pytest.mark.parametrize("kw", FILTERS, ids=["ns-maf01", "keepns-maf001", "miss50"])
@pytest.mark.parametrize("n", POOL_COUNTS)
def test_no_emitted_locus_is_rank_deficient(oracle, n, kw):
    """cond(X) <= 1e7 is the line check_stat_op draws; the GPU test relies on no locus of the corpus crossing it."""
    counts, tags = corpus(n)
    ps, fo = cc.pool_sizes(n), flt(oracle, kw)
    worst, emitted = 0.0, 0
    for l, c in enumerate(counts):
        if oracle.filter_locus(c, ps, fo) is None:
            continue
        emitted += 1
        cond = design_cond(oracle, c, ps, fo)
        assert cond <= 1e7, f"locus {l} ({tags[l]}): design condition {cond:.3g}"
        worst = max(worst, cond)
    print(f"n={n} {kw}: {emitted} of {len(tags)} loci emitted, largest design condition {worst:.3g}")
    assert emitted > len(tags) // 2
    if kw.get("miss"):                          # the family that counts only here
        kept = [oracle.filter_locus(c, ps, fo) is not None for c in counts[tags == "uncovered-head"]]
        assert any(kept)


@pytest.mark.parametrize("n", POOL_COUNTS)
def test_rows_emitted_per_family(oracle, n):
    counts, tags = corpus(n)
    ps, Y = cc.pool_sizes(n), cc.phenotypes(n, 2)
    keep_ns = flt(oracle, dict(remove_ns=False, maf=0.001))
    for l, c in enumerate(counts):
        if tags[l] in ("clean", "tri"):
            na, ids, _, _, _ = oracle.ols_iterate_locus(c, Y, ps, keep_ns)
            assert na == (1 if tags[l] == "clean" else 2), f"locus {l} ({tags[l]})"
            assert set(ids) < set(cc.read_slots(c))
    # remove_ns=True against remove_ns=False under one maf: a locus without a read in N is untouched; one whose alleles include N
    # is dropped or loses exactly that allele
    for maf in (0.01, 0.001):
        with_ns, without = flt(oracle, dict(remove_ns=False, maf=maf)), flt(oracle, dict(remove_ns=True, maf=maf))
        touched = 0
        for l, c in enumerate(counts):
            a, b = oracle.filter_locus(c, ps, with_ns), oracle.filter_locus(c, ps, without)
            if not c[:, N_SLOT].any():
                assert (a is None) == (b is None), f"locus {l} ({tags[l]})"
                if a is not None:
                    assert a[0].tolist() == b[0].tolist() and np.array_equal(a[1], b[1])
                    ra, rb = oracle.ols_iterate_locus(c, Y, ps, with_ns), oracle.ols_iterate_locus(c, Y, ps, without)
                    assert ra[:3] == rb[:3] and np.array_equal(ra[3], rb[3], equal_nan=True) and np.array_equal(ra[4], rb[4], equal_nan=True)
                continue
            if b is not None:
                assert N_SLOT not in b[0].tolist()
            if tags[l] in ("clean", "deep", "tie-sums", "tie-pool0", "order-flip"):      # two alleles, one of them N: nothing is left
                assert a is not None and N_SLOT in a[0].tolist() and b is None, f"locus {l} ({tags[l]})"
                touched += 1
            if tags[l] == "tri" and N_SLOT in cc.read_slots(c):                          # three alleles: the other two stay
                assert a is not None and b is not None and b[0].tolist() == [j for j in a[0].tolist() if j != N_SLOT]
                touched += 1
        assert touched >= 50


@pytest.mark.parametrize("n", POOL_COUNTS)
def test_tie_sums_follow_the_stable_sort(oracle, n):
    """Both column sums are n / 2 to the bit.  sort_by_allele_freq is stable (sync.rs:477-506): the lower slot stays first = major,
    ols_iter reports the HIGHER slot; pearson_corr drops the last column unsorted and reports the LOWER slot."""
    counts, tags = corpus(n)
    ps, Y = cc.pool_sizes(n), cc.phenotypes(n, 2)
    fo = flt(oracle, dict(remove_ns=False, maf=0.001))
    seen = set()
    for c in counts[tags == "tie-sums"]:
        lo, hi = cc.read_slots(c)
        na, ids, mf, _, _ = oracle.ols_iterate_locus(c, Y, ps, fo)
        assert na == 1 and ids == [hi] and mf == [0.5]
        na, ids, mf, _, _ = oracle.correlation_locus(c, Y, ps, fo)
        assert na == 1 and ids == [lo] and mf == [0.5]
        fr = oracle.to_frequencies(oracle.filter_locus(c, ps, fo)[1])
        assert fr.sum(axis=0).tolist() == [n / 2, n / 2]
        seen.add((lo, hi, bool(c[0, lo] < c[0, hi])))
    assert len(seen) == 30
