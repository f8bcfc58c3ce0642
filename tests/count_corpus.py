"""A deterministic corpus of loci for the count operators (ols_iter, pearson_corr, chisq_test, fisher_exact_test, the loader) whose
alleles sit in EVERY pair of sync columns, not only in A and T as synth.sync_counts puts them.  numpy only, generated on the host, so
the CPU test (test_count_corpus.py) and the GPU test (test_gpu_allele_slots.py) see the same loci.

Sync columns ("slots"): 0 A, 1 T, 2 C, 3 G, 4 N, 5 D.  Depths are Poisson(60) + 10 unless stated.  Families (tag -> content):

  clean           each of the 30 ordered (major slot, minor slot) pairs, two loci, reads in those two columns only
  err             the same pairs, two loci; every read moves with probability 0.005 to one of the other four columns
  late            per ordered pair: the minor allele has no read before pool j, j cycling through 1, 15, 16, 17, n - 1
  stray-first     per ordered pair: pools 0..2 show the major allele only, pool 0 also ONE read in a third slot
  tie-pool0       per ordered pair: equal counts of both alleles in pool 0 (the first covered pool)
  tie-sums        per ordered pair (x, y): depth 16 everywhere, pools alternating (4, 12) / (12, 4) in (x, y), and (8, 8) in the last
                  pool of an odd n: both column sums are exactly n / 2
  order-flip      per ordered pair (x, y): x is rare in the small pools and frequent in the few large ones of pool_sizes(n), so the
                  pool-size-weighted q says x > y and the plain column sums say x < y
  deep            per ordered pair: a clean locus of depth Poisson(60) + 40 with every count multiplied by 2^20: the largest count of
                  every locus lies between 2^26 and 2^29
  tri             each of the 20 slot triples: three alleles, all far above any filter used
  uncovered-head  per unordered pair: the first u pools have no reads, u cycling through 1, 15, 16, 17

The loci are shuffled, not grouped by tag: any 64 neighbouring loci hold many different pairs."""
import itertools

import numpy as np

TAGS = ("clean", "err", "late", "stray-first", "tie-pool0", "tie-sums", "order-flip", "deep", "tri", "uncovered-head")
ORDERED = [(a, b) for a in range(6) for b in range(6) if a != b]            # (major slot, minor slot): 30
UNORDERED = list(itertools.combinations(range(6), 2))                       # 15
TRIPLES = list(itertools.combinations(range(6), 3))                         # 20
LARGE_EVERY, LARGE_AT, LARGE_SIZE = 8, 3, 400.0


def pool_sizes(n):
    """Pool sizes that go with the corpus: one pool in eight is large (400), the others small (10 .. 16) -- the range `order-flip`
    needs for the weighted and the unweighted order of two alleles to differ."""
    i = np.arange(n)
    return np.where(i % LARGE_EVERY == LARGE_AT, LARGE_SIZE, 10.0 + (i % 7))


def phenotypes(n, k, seed=0):
    """k traits without structure (standard normal), n x k"""
    return np.random.default_rng([seed, n, k, 77]).standard_normal((n, k))


def _depth(rng, n):
    return rng.poisson(60.0, n) + 10


def _minor_prob(rng, n, lo=0.1, hi=0.4):
    """per-pool probability of the minor allele: a base frequency in [lo, hi] and pool noise"""
    b = rng.uniform(lo, hi)
    return np.clip(b + 0.08 * rng.standard_normal(n), 0.03, 0.47)


def _biallelic(rng, n, major, minor, pm=None, extra_depth=0):
    c = np.zeros((n, 6), dtype=np.int64)
    d = _depth(rng, n) + extra_depth
    m = rng.binomial(d, _minor_prob(rng, n) if pm is None else pm)
    c[:, minor] = m
    c[:, major] = d - m
    return c


def _others(*slots):
    return [j for j in range(6) if j not in slots]


def corpus(n, seed):
    """-> (counts[L, n, 6] int64, tags[L] of str)"""
    assert n >= 20
    rng = np.random.default_rng([seed, n])
    loci, tags = [], []

    def add(tag, c):
        loci.append(c); tags.append(tag)

    for a, b in ORDERED:
        for _ in range(2):
            add("clean", _biallelic(rng, n, a, b))
    for a, b in ORDERED:
        for _ in range(2):
            c = _biallelic(rng, n, a, b)
            oth = _others(a, b)
            for s in (a, b):
                moved = rng.binomial(c[:, s], 0.005)
                c[:, s] -= moved
                c[:, oth] += rng.multinomial(moved, [0.25] * 4)
            add("err", c)
    for i, (a, b) in enumerate(ORDERED):
        j = (1, 15, 16, 17, n - 1)[i % 5]
        pm = _minor_prob(rng, n, 0.25, 0.4)
        pm[:j] = 0.0
        c = _biallelic(rng, n, a, b, pm)
        c[j, b] = max(c[j, b], 1); c[j, a] = max(c[j, a], 1)       # pool j does show the minor allele
        add("late", c)
    for i, (a, b) in enumerate(ORDERED):
        pm = _minor_prob(rng, n)
        pm[:3] = 0.0
        c = _biallelic(rng, n, a, b, pm)
        c[0, _others(a, b)[i % 4]] = 1
        add("stray-first", c)
    for a, b in ORDERED:
        c = _biallelic(rng, n, a, b)
        half = int(_depth(rng, 1)[0]) // 2
        c[0, a] = c[0, b] = half
        add("tie-pool0", c)
    for x, y in ORDERED:
        c = np.zeros((n, 6), dtype=np.int64)
        c[0::2, x], c[0::2, y] = 4, 12
        c[1::2, x], c[1::2, y] = 12, 4
        if n & 1:
            c[n - 1, x] = c[n - 1, y] = 8
        add("tie-sums", c)
    large = pool_sizes(n) == LARGE_SIZE
    for x, y in ORDERED:
        px = np.where(large, 0.9, 0.2) + 0.03 * rng.standard_normal(n)
        c = _biallelic(rng, n, y, x, np.clip(px, 0.05, 0.95))      # "minor" column of the helper: x
        add("order-flip", c)
    for a, b in ORDERED:
        add("deep", _biallelic(rng, n, a, b, extra_depth=30) << 20)
    for i, tr in enumerate(TRIPLES):
        base = np.roll(np.array([0.5, 0.3, 0.2]), i % 3)
        c = np.zeros((n, 6), dtype=np.int64)
        d = _depth(rng, n)
        for p in range(n):
            pr = np.clip(base + 0.06 * rng.standard_normal(3), 0.05, None)
            c[p, list(tr)] = rng.multinomial(d[p], pr / pr.sum())
        add("tri", c)
    for i, (a, b) in enumerate(UNORDERED):
        c = _biallelic(rng, n, *((a, b) if i % 2 == 0 else (b, a)))
        c[: (1, 15, 16, 17)[i % 4]] = 0
        add("uncovered-head", c)

    order = rng.permutation(len(loci))
    counts = np.stack(loci)[order]
    assert counts.min() >= 0 and counts.max() < (1 << 29)
    return np.ascontiguousarray(counts), np.array(tags)[order]


def read_slots(locus):
    """the slots of one locus (n x 6) that hold at least one read, ascending"""
    return [j for j in range(6) if locus[:, j].any()]
