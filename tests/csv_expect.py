"""What sync2csv's file must hold, built without the code under test: the cell text from rustfmt.roundup_own
(parse_f64_roundup_and_own, base/helpers.rs:103-117), the rows from the oracle's loader steps (test-side only)."""
from pathlib import Path

import numpy as np

import rustfmt

GOLD = Path(__file__).parent / "golden"
AL = "ATCGND"
GOLDEN_ROWS = {False: 15892, True: 9336}   # data rows of tests/golden/test.sync under the CLI's default filter


def cell(x: float) -> str:
    return rustfmt.roundup_own(float(x), 6)


def rows_text(G, n, col_locus, col_allele, chrom_ids, pos, chrom_names, row0=0, rows=None) -> bytes:
    """The text of rows [row0, row0 + rows) of a p x ld matrix (only its first n columns are pools)."""
    G = np.asarray(G)
    rows = G.shape[0] - row0 if rows is None else rows
    memo = {}
    out = []
    for r in range(row0, row0 + rows):
        l = int(col_locus[r])
        cells = []
        for x in G[r, :n].tolist():
            key = "NaN" if x != x else x
            t = memo.get(key)
            if t is None:
                t = memo[key] = cell(x)
            cells.append(t)
        out.append(f"{chrom_names[int(chrom_ids[l])]},{int(pos[l])},{AL[int(col_allele[r])]}," + ",".join(cells) + "\n")
    return "".join(out).encode()


def labels(p, seed=0, n_loci=None, names=("chr1", "scaffold_12.1", "X")):
    """Random but valid labels for p rows: (col_locus, col_allele, chrom_ids, pos, chrom_names)."""
    rng = np.random.default_rng(seed)
    n_loci = max(1, p // 2) if n_loci is None else n_loci
    col_locus = np.sort(rng.integers(0, n_loci, size=p)).astype(np.int64)
    col_allele = rng.integers(0, 6, size=p).astype(np.int32)
    chrom_ids = np.sort(rng.integers(0, len(names), size=n_loci)).astype(np.int32)
    pos = rng.integers(0, 3_000_000_000, size=n_loci).astype(np.uint64)
    return col_locus, col_allele, chrom_ids, pos, list(names)


SPECIAL = [float("nan"), 0.0, 1.0, 0.9999996, 4e-7, 0.5e-6, 1e-6, 0.333333, 0.2, 0.0625, 1.0 / 3.0, 0.1234565, 0.9999995,
           0.99999949999, 0.123456, 0.5, 2.0 / 7.0, 0.000001, 0.00001, 0.0001]


def count_frequencies(rows, n, seed):
    """c / d from small integer counts, NaN where d = 0, and the special values sprinkled in."""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 40, size=(rows, n)).astype(np.float64)
    d = c + rng.integers(0, 40, size=(rows, n))
    with np.errstate(invalid="ignore", divide="ignore"):
        G = c / d
    m = rng.random((rows, n)) < 0.1
    G[m] = rng.choice(np.array(SPECIAL), size=int(m.sum()))
    return G


def golden_fixture(oracle):
    """tests/golden/test.sync parsed by the oracle: (counts [L x 5 x 6] uint64 list, chrom_ids, pos, chrom_names, order) with
    `order` the stable (chromosome, position) sort the loader applies (base/sync.rs:1092-1101)."""
    rows = []
    for line in (GOLD / "test.sync").read_text().splitlines():
        n, chrom, pos, counts = oracle.parse_sync_line(line)
        if n > 0:
            rows.append((chrom, pos, counts))
    names = []
    for r in rows:
        if r[0] not in names:
            names.append(r[0])
    chrom_ids = np.array([names.index(r[0]) for r in rows], dtype=np.int32)
    pos = np.array([r[1] for r in rows], dtype=np.uint64)
    order = sorted(range(len(rows)), key=lambda i: (rows[i][0], rows[i][1]))
    return [r[2] for r in rows], chrom_ids, pos, names, np.array(order, dtype=np.int64)


def golden_pool_names():
    return [line.split(",")[0] for line in (GOLD / "test.csv").read_text().splitlines() if line and not line.startswith("#")]


_golden_memo = {}


def golden_text(oracle, keep_p_minus_1: bool, header: bool = True) -> bytes:
    """The oracle composition: filter_locus -> to_frequencies -> (sort_by_allele_freq, drop the first) per locus in sorted
    order, one line per surviving allele, cells by rustfmt.  Computed once per variant and shared."""
    key = bool(keep_p_minus_1)
    if key not in _golden_memo:
        counts, chrom_ids, pos, names, order = golden_fixture(oracle)
        ps = np.full(5, 20.0)
        fo = oracle.filt(True, 1, 0.001, 0.0)
        memo = {}
        lines = []
        for l in order:
            res = oracle.filter_locus(counts[l], ps, fo)
            if res is None:
                continue
            ids, fc = res
            fr = oracle.to_frequencies(fc)
            if key:
                fr, ids = oracle.sort_by_allele_freq(fr, ids, True)
                fr, ids = fr[:, 1:], ids[1:]
            for j, a in enumerate(ids):
                cells = []
                for x in fr[:, j].tolist():
                    k = "NaN" if x != x else x
                    if k not in memo:
                        memo[k] = cell(x)
                    cells.append(memo[k])
                lines.append(f"{names[chrom_ids[l]]},{int(pos[l])},{AL[int(a)]}," + ",".join(cells) + "\n")
        assert len(lines) == GOLDEN_ROWS[key], len(lines)   # a guard against an empty comparison
        _golden_memo[key] = "".join(lines).encode()
    body = _golden_memo[key]
    return (("#chr,pos,allele," + ",".join(golden_pool_names()) + "\n").encode() if header else b"") + body
