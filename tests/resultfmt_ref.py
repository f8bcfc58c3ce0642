"""The rows of the result writer, restated plainly over tests/rustfmt.py (test-side only): what pg_result_rows_dev /
pg_host_result_rows and pg_kinship_rows_dev / pg_host_kinship_rows must print, and generated inputs for them.

D = rustfmt.display, R(x, n) = rustfmt.roundup_own, a letter indexes "ATCGND"; arrays are slot-major as the batch operators leave
them: ids / freq element (slot r, locus l) at r * L + l, stat / pval at (r * L + l) * k + trait."""
import numpy as np

import f64_corpus
import rustfmt

ALLELES = "ATCGND"
MAX_OUT = 5
OPS = ("fisher_exact_test", "chisq_test", "gwalpha", "pearson_corr", "ols_iter")
UNIT_MAX = 1 << 22
D = rustfmt.display
R = f64_corpus.roundup_own       # rustfmt.roundup_own with its one wrong product put right (f64_corpus.sensible_round)


def result_rows(op, n_out, ids, freq, stat, pval, chrom, pos, names, k=1) -> bytes:
    L = len(n_out)
    out = []
    for l in range(L):
        n = min(int(n_out[l]), MAX_OUT)
        if n <= 0:
            continue
        head = "%s,%d," % (names[int(chrom[l])], int(pos[l]))
        if op in ("fisher_exact_test", "chisq_test"):
            letters = "".join(ALLELES[int(ids[r * L + l])] for r in range(n))
            s = D(float(stat[l])) if op == "fisher_exact_test" else R(float(stat[l]), 6)
            out.append("%s%s,%s,%s\n" % (head, letters, s, D(float(pval[l]))))
            continue
        for r in range(n):
            e = r * L + l
            letter = ALLELES[int(ids[e])]
            if op == "gwalpha":
                out.append("%s%s,%s,Pheno_0,%s,Unknown\n" % (head, letter, R(float(freq[e]), 6), R(float(stat[e]), 6)))
                continue
            for j in range(k):
                if op == "ols_iter":
                    out.append("%s%s,%s,Pheno_%d,%s,%s\n" % (head, letter, R(float(freq[e]), 8), j, R(float(stat[e * k + j]), 6), R(float(pval[e * k + j]), 12)))
                else:
                    out.append("%s%s,%s,Pheno_%d,%s,%s\n" % (head, letter, D(float(freq[e])), j, R(float(stat[e * k + j]), 6), D(float(pval[e * k + j]))))
    return "".join(out).encode()


def kinship_rows(beta, pval, col_chrom, col_pos, col_allele, names, row0=0, rows=None) -> bytes:
    beta = np.asarray(beta, dtype=np.float64); pval = np.asarray(pval, dtype=np.float64)
    beta = beta.reshape(beta.shape[0], -1); pval = pval.reshape(beta.shape)
    p, k = beta.shape
    rows = p * k - row0 if rows is None else rows
    out = []
    for r in range(row0, row0 + rows):
        j, i = divmod(r, p)
        label = "intercept,0,intercept" if i == 0 else "%s,%d,%s" % (names[int(col_chrom[i - 1])], int(col_pos[i - 1]), ALLELES[int(col_allele[i - 1])])
        out.append("%s,Pheno_%d,%s,%s\n" % (label, j, D(float(beta[i, j])), D(float(pval[i, j]))))
    return "".join(out).encode()


def chrom_names(n, rng, longest=40):
    """n <= 10 distinct names of 1 to `longest` bytes (the first of one byte, the second of `longest`): rows start at every alignment"""
    lengths = [1, longest] + [int(v) for v in rng.integers(1, longest + 1, size=max(0, n - 2))]
    return [(str(i) + "_chromosome_name" * (longest // 16 + 1))[:ln] for i, ln in zip(range(n), lengths)]


def positions(L, rng):
    """positions of 1 to 20 digits"""
    digits = rng.integers(1, 21, size=L)
    pos = np.array([int(rng.integers(10 ** (int(d) - 1), min(10 ** int(d), 2 ** 64) - 1, dtype=np.uint64, endpoint=True)) if d > 1 else int(rng.integers(0, 10)) for d in digits], dtype=np.uint64)
    pos[:3] = [0, 2 ** 64 - 1, 10 ** 19][:min(3, L)]
    return pos


def generated(op, L, k, seed, names=None, realistic=False):
    """inputs of L loci for `op`: n_out from 0 to 5 with runs of dropped loci, statistics from the corpus (cells of 1 to 327 bytes)
    or, with `realistic`, frequencies / statistics / p-values of ordinary size; arrays of dropped loci hold junk ids"""
    rng = np.random.default_rng(seed)
    if op in ("fisher_exact_test", "chisq_test", "gwalpha"):
        k = 1
    names = chrom_names(7, rng) if names is None else names
    n_out = rng.integers(0, MAX_OUT + 1, size=L).astype(np.int32)
    if not realistic:
        n_out[rng.integers(0, L, size=max(1, L // 50))] = 7                     # above PG_MAX_OUT: clipped
        n_out[rng.integers(0, L, size=max(1, L // 50))] = -2
    for start in rng.integers(0, L, size=max(1, L // 400)):                      # runs of dropped loci (longer than a tile holds)
        n_out[start:start + int(rng.integers(1, 700))] = 0
    ids = rng.integers(0, 6, size=MAX_OUT * L).astype(np.int32)
    for l in np.nonzero(n_out <= 0)[0][:50]:
        ids[l] = 99                                                              # never read
    per_locus = op in ("fisher_exact_test", "chisq_test")
    size = L if per_locus else MAX_OUT * L * k
    if realistic:
        freq = np.round(rng.random(MAX_OUT * L), 9)
        stat = rng.normal(size=size) * rng.choice([1e-3, 1.0, 50.0], size=size)
        pval = rng.random(size) ** rng.choice([1, 4, 30], size=size)
    else:
        freq = f64_corpus.sample(MAX_OUT * L, seed + 1)
        stat = f64_corpus.sample(size, seed + 2)
        pval = f64_corpus.sample(size, seed + 3)
    chrom = np.sort(rng.integers(0, len(names), size=L)).astype(np.int32)
    return dict(op=op, k=k, n_out=n_out, ids=ids, freq=None if per_locus else freq, stat=stat, pval=None if op == "gwalpha" else pval, chrom=chrom,
                pos=positions(L, rng), names=names)


def args_of(g):
    return g["op"], g["n_out"], g["ids"], g["freq"], g["stat"], g["pval"], g["chrom"], g["pos"], g["names"], g["k"]


def generated_kinship(p, k, seed, names=None):
    rng = np.random.default_rng(seed)
    names = chrom_names(5, rng) if names is None else names
    beta = f64_corpus.sample(p * k, seed + 1).reshape(p, k).copy()
    pval = f64_corpus.sample(p * k, seed + 2)[::-1].reshape(p, k).copy()
    m = p                                    # a label per column of the matrix: the last one is never printed
    return dict(beta=beta, pval=pval, col_chrom=np.sort(rng.integers(0, len(names), size=m)).astype(np.int32), col_pos=positions(m, rng),
                col_allele=rng.integers(0, 6, size=m).astype(np.int32), names=names)


def kinship_args_of(g):
    return g["beta"], g["pval"], g["col_chrom"], g["col_pos"], g["col_allele"], g["names"]
