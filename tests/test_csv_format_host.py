"""pg_host_csv_freq_rows: the host form of sync2csv's row formatter (the checker of the device form) against
rustfmt.roundup_own (parse_f64_roundup_and_own(x, 6), base/helpers.rs:103-117) and a plain restatement of the row."""
import ctypes as C

import numpy as np
import pytest

import csv_expect as E
import rustfmt

PG_ERR_INVALID = -1
PAD = 7.0          # what the padding columns (ld > n) hold: no frequency, so a formatter that read one would refuse the call


def call(native, G, n, col_locus, col_allele, chrom_ids, pos, names, row0=0, rows=None, cap=None, guard=64, threads=3):
    """-> (rc, bytes needed, buffer incl. `guard` bytes of 0xAA behind cap); cap=None: the size the query returns."""
    from poolgen_amd.engine import _chrom_table
    G = np.ascontiguousarray(G, dtype=np.float64)
    p, ld = G.shape
    rows = p - row0 if rows is None else rows
    text, off = _chrom_table(names)
    keep = [np.ascontiguousarray(col_locus, dtype=np.int64), np.ascontiguousarray(col_allele, dtype=np.int32),
            np.ascontiguousarray(chrom_ids, dtype=np.int32), np.ascontiguousarray(pos, dtype=np.uint64)]
    args = [G.ctypes.data, ld, n, row0, rows] + [a.ctypes.data for a in keep] + [text.ctypes.data, off.ctypes.data, len(off) - 1]
    need = C.c_int64(-7)
    if cap is None:
        rc = native.pg_host_csv_freq_rows(*args, None, 0, C.byref(need), threads)
        if need.value <= 0:
            return rc, need.value, np.empty(0, dtype=np.uint8)
        assert rc == PG_ERR_INVALID            # a size query: 0 bytes of room are not enough
        cap = need.value
    buf = np.full(cap + guard, 0xAA, dtype=np.uint8)
    rc = native.pg_host_csv_freq_rows(*args, buf.ctypes.data, cap, C.byref(need), threads)
    return rc, need.value, buf


def format_cells(native, values, n=1000):
    """Every value as one cell of an n-pool table with a fixed one-locus label; the cells' texts in order."""
    v = np.asarray(values, dtype=np.float64)
    rows = (len(v) + n - 1) // n
    G = np.zeros((rows, n + 2))                                   # ld > n: two padding columns that must never be read:
    G[:, n:] = PAD                                                # as a cell this value would fail the call
    cells = np.zeros(rows * n)
    cells[:len(v)] = v
    G[:, :n] = cells.reshape(rows, n)
    rc, need, buf = call(native, G, n, np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int32), [0], [7], ["c"])
    assert rc == 0
    out = []
    for line in buf[:need].tobytes().decode().splitlines():
        assert line.startswith("c,7,A,")
        cells = line[6:].split(",")
        assert len(cells) == n
        out += cells
    return out[:len(v)]


def check_cells(native, values):
    got = format_cells(native, values)
    want = [rustfmt.roundup_own(float(x), 6) for x in values]
    bad = [(float(x), g, w) for x, g, w in zip(values, got, want) if g != w]
    assert not bad, (len(bad), bad[:10])


def test_cell_rule_every_millionth(native):
    check_cells(native, np.arange(1_000_001) / 1e6)


def test_cell_rule_ties(native):
    check_cells(native, (2 * np.arange(1_000_000) + 1) / 2e6)


def test_cell_rule_small_fractions(native):
    vals = [a / b for b in range(1, 401) for a in range(0, b + 1)]
    check_cells(native, np.array(vals))


def test_cell_rule_special_values(native):
    assert format_cells(native, [0.9999996, 4e-7, float("nan"), 0.0, 1.0, 1.0 / 3.0, 0.2, 0.0625, 1e-6], n=9) == \
        ["1", "0", "NaN", "0", "1", "0.333333", "0.2", "0.0625", "0.000001"]


def test_prefix_names_positions_alleles(native):
    names = ["c", "ab", "Chromosome1", "scaffold_12.1", "x" * 39 + "_", "9.8_7" * 8, "Z" * 17]
    assert sorted(len(s) for s in names)[0] == 1 and max(len(s) for s in names) == 40
    positions = [0, 9, 10, 2 ** 32, 2 ** 63, 2 ** 64 - 1, 99, 100, 10 ** 19, 10 ** 19 - 1]
    chrom_ids = [i % len(names) for i in range(len(positions))]
    p = len(positions) * 6
    col_locus = np.repeat(np.arange(len(positions)), 6)
    col_allele = np.tile(np.arange(6), len(positions))
    G = E.count_frequencies(p, 3, seed=1)
    rc, need, buf = call(native, G, 3, col_locus, col_allele, chrom_ids, positions, names)
    want = E.rows_text(G, 3, col_locus, col_allele, chrom_ids, positions, names)
    assert rc == 0 and need == len(want)
    assert buf[:need].tobytes() == want
    assert (names[5] + ",18446744073709551615,D,").encode() in want and b"c,0,A," in want      # the cases are really in there


@pytest.mark.parametrize("threads", [1, 4, 64])
def test_padding_row0_and_threads(native, threads):
    p, n, ld = 37, 5, 8
    G = np.full((p, ld), PAD)
    G[:, :n] = E.count_frequencies(p, n, seed=2)
    lab = E.labels(p, seed=3)
    whole = E.rows_text(G, n, *lab)
    for row0, rows in [(0, p), (1, p - 1), (11, 5), (36, 1), (5, 0)]:
        rc, need, buf = call(native, G, n, *lab, row0=row0, rows=rows, threads=threads)
        want = E.rows_text(G, n, *lab, row0=row0, rows=rows)
        assert rc == 0 and need == len(want) and buf[:need].tobytes() == want    # (a padding column read as a cell: rc != 0)
    assert whole == b"".join(E.rows_text(G, n, *lab, row0=r, rows=1) for r in range(p))


def test_capacity_protocol(native):
    p, n = 23, 6
    G = E.count_frequencies(p, n, seed=4)
    lab = E.labels(p, seed=5)
    want = E.rows_text(G, n, *lab)
    rc, need, _ = call(native, G, n, *lab, cap=0, guard=8)
    assert rc == PG_ERR_INVALID and need == len(want)                        # the size query
    rc, need, buf = call(native, G, n, *lab, cap=len(want) - 1)
    assert rc == PG_ERR_INVALID and need == len(want) and np.all(buf == 0xAA)  # one byte short: nothing is written
    rc, need, buf = call(native, G, n, *lab, cap=len(want))
    assert rc == 0 and need == len(want) and buf[:need].tobytes() == want and np.all(buf[need:] == 0xAA)


@pytest.mark.parametrize("value", [-0.1, 1.5, float("inf"), float("-inf"), 1.0000000000000002, -1e-300])
def test_out_of_domain_cells_are_rejected(native, value):
    p, n = 9, 4
    G = E.count_frequencies(p, n, seed=6)
    lab = E.labels(p, seed=7)
    assert call(native, G, n, *lab)[0] == 0
    G[5, 2] = value
    size_without = call(native, np.where(G == value, 0.5, G), n, *lab)[1]
    rc, need, buf = call(native, G, n, *lab, cap=4096)
    assert rc == PG_ERR_INVALID and np.all(buf == 0xAA)
    assert need == size_without - 2                  # the size is still reported: the cell counts as the "0" it would print as, not "0.5"
    assert call(native, G, n, *lab, row0=0, rows=5, cap=4096)[0] == 0         # ... but only where the cell is


def test_python_wrapper_matches(native):
    from poolgen_amd.engine import freq_csv_host
    p, n = 31, 7
    G = np.zeros((p, 8)); G[:, :n] = E.count_frequencies(p, n, seed=8)
    lab = E.labels(p, seed=9)
    assert freq_csv_host(G, *lab, n=n, n_threads=2) == E.rows_text(G, n, *lab)
    assert freq_csv_host(G, *lab, n=n, row0=4, rows=9) == E.rows_text(G, n, *lab, row0=4, rows=9)
    # out=: one call into the caller's buffer, the filled part comes back; a buffer that is too small is an error
    want = E.rows_text(G, n, *lab)
    buf = np.full(len(want) + 10, 0xAA, dtype=np.uint8)
    got = freq_csv_host(G, *lab, n=n, out=buf)
    assert got.tobytes() == want and got.base is buf and np.all(buf[len(want):] == 0xAA)
    from poolgen_amd import NativeError
    with pytest.raises(NativeError):
        freq_csv_host(G, *lab, n=n, out=np.empty(len(want) - 1, dtype=np.uint8))
    G[3, 1] = 1.5
    with pytest.raises(NativeError, match="no allele frequency"):
        freq_csv_host(G, *lab, n=n)
