"""pg_csv_freq_rows_dev (pg_csv.hip): the text the GPU formats equals the host form's (pg_host_csv_freq_rows, itself checked
against rustfmt in test_csv_format_host.py) byte for byte, on both sides of every dispatch rule; and from the golden counts it
equals the oracle composition."""
import ctypes as C

import numpy as np
import pytest
import torch

import csv_expect as E

pytestmark = pytest.mark.gpu
PG_ERR_INVALID = -1
TILE = 16384          # CSV_TILE of pg_csv.hip: the bytes of text a workgroup stages in LDS


def dev_args(engine, G, n, col_locus, col_allele, chrom_ids, pos, names):
    from poolgen_amd.engine import _chrom_table
    text, off = _chrom_table(names)
    t = [torch.from_numpy(np.ascontiguousarray(G, dtype=np.float64)).cuda(),
         torch.from_numpy(np.ascontiguousarray(col_locus, dtype=np.int64)).cuda(),
         torch.from_numpy(np.ascontiguousarray(col_allele, dtype=np.int32)).cuda(),
         torch.from_numpy(np.ascontiguousarray(chrom_ids, dtype=np.int32)).cuda(),
         torch.from_numpy(np.ascontiguousarray(pos, dtype=np.uint64).view(np.int64)).cuda(),
         torch.from_numpy(text).cuda(), torch.from_numpy(off).cuda()]
    return t, len(off) - 1


def raw_call(engine, t, n_chrom, n, row0, rows, buf, cap):
    """the C entry point itself, with the caller's buffer and capacity -> (rc, bytes)"""
    G = t[0]
    need = C.c_int64(-7)
    rc = engine._lib.pg_csv_freq_rows_dev(engine._ctx, G.data_ptr(), G.shape[1], n, row0, rows, t[1].data_ptr(), t[2].data_ptr(),
                                          t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), n_chrom,
                                          buf.data_ptr() if buf is not None else None, cap, C.byref(need))
    torch.cuda.synchronize()
    return rc, need.value


def dev_text(engine, G, n, lab, row0=0, rows=None) -> bytes:
    col_locus, col_allele, chrom_ids, pos, names = lab
    out = engine.freq_csv(torch.from_numpy(np.ascontiguousarray(G, dtype=np.float64)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(col_locus, dtype=np.int64)).cuda(),
                          torch.from_numpy(np.ascontiguousarray(col_allele, dtype=np.int32)).cuda(), chrom_ids, pos, names, n=n,
                          row0=row0, rows=rows)
    assert out.dtype == torch.uint8 and out.is_cuda
    return out.cpu().numpy().tobytes()


def host_text(G, n, lab, row0=0, rows=None) -> bytes:
    from poolgen_amd.engine import freq_csv_host
    return freq_csv_host(G, *lab, n=n, row0=row0, rows=rows, n_threads=4)


def matrix(rows, n, seed):
    """count frequencies with specials; row 3 all "0" (the shortest text), row 5 all 8-byte cells (the longest)"""
    ld = n + (n & 1) + 2
    G = np.full((rows, ld), 7.0)             # the padding columns hold no frequency: a kernel that read one would refuse the call
    G[:, :n] = E.count_frequencies(rows, n, seed)
    if rows > 3:
        G[3, :n] = 0.0
    if rows > 5:
        G[5, :n] = 0.123457
    return G


# Pool counts.  The rule of pg_csv.hip (csv_lpr_shift): a row is formatted by the smallest power of two of lanes that holds n,
# at most a wave of 64 -- so 1|2, 2|3, 4|5, 8|9, 16|17, 32|33 are its boundaries, and from 65 pools on a wave takes a row in
# several turns (64|65, 128|129).  63 / 64 / 65 / 200 are the issue's.
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 128, 129, 200])
def test_pool_and_row_counts(engine, n):
    for rows in (1, 255, 256, 257):          # the scan's first level: 256 rows per workgroup
        G = matrix(rows, n, seed=n * 1000 + rows)
        lab = E.labels(rows, seed=rows + n)
        want = host_text(G, n, lab)
        if rows == 257 and n in (5, 200):     # the host form is itself the checked one; once more against the restatement
            assert want == E.rows_text(G, n, *lab)
        assert dev_text(engine, G, n, lab) == want, (n, rows)


def test_second_level_of_the_scan(engine):
    """n = 1 and 262 145 rows: one row past 256 rows x 1 024 workgroup sums, the scan kernel's round.  (The longest row is
    "c,4999,A,0.333333" + newline = 18 bytes, so the emit kernel takes 910 rows per workgroup.)"""
    rows = 262_145
    G = np.zeros((rows, 2))
    G[:, 0] = E.count_frequencies(rows, 1, seed=12)[:, 0]
    col_locus = np.arange(rows, dtype=np.int64) % 5000
    lab = (col_locus, np.zeros(rows, dtype=np.int32), np.zeros(5000, dtype=np.int32), np.arange(5000, dtype=np.uint64), ["c"])
    assert dev_text(engine, G, 1, lab) == host_text(G, 1, lab)


def test_the_shortest_rows_fill_a_tile(engine):
    """Rows per workgroup = 16 384 / the longest row, without a cap: n = 1 with the label "c,<digit>,A," gives rows of 8 to 15
    bytes, 1 092 rows per workgroup (every lane takes more than four rows in turn), and 5 000 rows span five workgroups; with
    all-"0" cells the rows are 8 bytes and one workgroup takes 2 048."""
    rows = 5000
    G = np.zeros((rows, 2)); G[:, 1] = 7.0
    G[:, 0] = E.count_frequencies(rows, 1, seed=13)[:, 0]
    lab = (np.arange(rows, dtype=np.int64) % 10, np.zeros(rows, dtype=np.int32), np.zeros(10, dtype=np.int32), np.arange(10, dtype=np.uint64), ["c"])
    want = host_text(G, 1, lab)
    assert max(len(x) + 1 for x in want.split(b"\n")[:-1]) == 15 and want == E.rows_text(G, 1, *lab)
    assert dev_text(engine, G, 1, lab) == want
    G[:, 0] = 0.0
    want = host_text(G, 1, lab)
    assert len(want) == 8 * rows
    assert dev_text(engine, G, 1, lab) == want


def test_out_buffer_and_unvalidated_call(engine):
    """Engine.freq_csv(out=...): one call into the caller's buffer, the filled part returned, nothing behind it touched; with
    validate=False and a second table of names."""
    n, rows = 9, 300
    G = matrix(rows, n, seed=51)
    lab = E.labels(rows, seed=52)
    want = host_text(G, n, lab)
    t, _ = dev_args(engine, G, n, *lab)
    buf = torch.full((len(want) + 32,), 0xAA, dtype=torch.uint8, device="cuda")
    for validate in (True, False):
        buf.fill_(0xAA)
        got = engine.freq_csv(t[0], t[1], t[2], t[3], t[4], lab[4], n=n, out=buf, validate=validate)
        assert got.data_ptr() == buf.data_ptr() and got.cpu().numpy().tobytes() == want and bool((buf[len(want):] == 0xAA).all())
    from poolgen_amd import NativeError
    with pytest.raises(NativeError):
        engine.freq_csv(t[0], t[1], t[2], t[3], t[4], lab[4], n=n, out=buf[:len(want) - 1])
    other = ["A", "bb", "ccc"]                                   # the cached name table follows the names
    lab2 = lab[:4] + (other,)
    assert engine.freq_csv(t[0], t[1], t[2], t[3], t[4], other, n=n).cpu().numpy().tobytes() == host_text(G, n, lab2)
    with pytest.raises(ValueError):
        engine.freq_csv(t[0], t[1] + 10 ** 6, t[2], t[3], t[4], other, n=n)


# The long-row rule: a tile holds 16 384 / longest row rows; with fewer than the 4 waves of a workgroup (a longest row above
# 4 096 bytes) the whole workgroup formats row after row together instead of a wave a row.  With the label "c,1,A," a row of
# 8-byte cells is 6 + 9 n bytes: 4 092 at n = 454 (4 rows per tile, a wave each), 4 101 at n = 455 (3 rows, workgroup per row);
# 700 pools: 2 rows per tile, 1 000 pools: 1 row, 2 turns and 4 turns of 256 cells.
@pytest.mark.parametrize("n,rpb", [(454, 4), (455, 3), (700, 2), (1000, 1)])
def test_rows_of_more_than_a_quarter_tile(engine, n, rpb):
    rows = 11
    G = np.full((rows, n + 2), 7.0)
    G[:, :n] = E.count_frequencies(rows, n, seed=n)
    G[4, :n] = 0.123457
    G[7, :n] = 0.0
    lab = (np.zeros(rows, dtype=np.int64), np.arange(rows, dtype=np.int32) % 6, [0], [1], ["c"])
    want = host_text(G, n, lab)
    longest = max(len(x) + 1 for x in want.split(b"\n")[:-1])
    assert longest == 6 + 9 * n and TILE // longest == rpb
    assert dev_text(engine, G, n, lab) == want
    if n == 455:
        assert want == E.rows_text(G, n, *lab)


# The tile rule: the emit kernel stages rows in LDS while the LONGEST row of the call fits CSV_TILE = 16 384 bytes, and takes the
# direct path (a wave per row, byte stores to the output) otherwise.  With the label "c,1,A," (6 bytes) a row of 8-byte cells
# is 6 + 9 n bytes: 16 377 at n = 1 819 (staged, one row per workgroup), 16 386 at n = 1 820 (direct).
@pytest.mark.parametrize("n,long_rows,direct", [(1819, True, False), (1820, True, True), (1820, False, False)])
def test_rows_longer_than_the_tile(engine, n, long_rows, direct):
    rows = 7
    G = np.zeros((rows, n + 2))
    G[:, :n] = E.count_frequencies(rows, n, seed=n)
    if long_rows:
        G[2, :n] = 0.123457
    lab = (np.zeros(rows, dtype=np.int64), np.zeros(rows, dtype=np.int32), [0], [1], ["c"])
    want = host_text(G, n, lab)
    longest = max(len(x) + 1 for x in want.split(b"\n")[:-1])
    assert (longest > TILE) == direct and (not long_rows or longest == 6 + 9 * n)
    assert dev_text(engine, G, n, lab) == want


def test_special_values_in_every_lane(engine):
    """NaN, 0, 1, the ties and the other special values in every column, hence every lane position modulo 64."""
    S = np.array(E.SPECIAL)
    n, rows = 130, 2 * len(S)
    G = np.zeros((rows, n))
    G[:, :] = S[(np.arange(rows)[:, None] + np.arange(n)[None, :]) % len(S)]
    lab = E.labels(rows, seed=1)
    want = host_text(G, n, lab)
    assert want == E.rows_text(G, n, *lab)
    assert dev_text(engine, G, n, lab) == want
    for n2 in (5, 64):
        assert dev_text(engine, np.ascontiguousarray(G[:, :n2 + 1]), n2, lab) == host_text(np.ascontiguousarray(G[:, :n2 + 1]), n2, lab)


@pytest.mark.parametrize("n", [5, 200])
def test_slab_invariance(engine, n):
    rows = 700
    G = matrix(rows, n, seed=21)
    lab = E.labels(rows, seed=22)
    whole = dev_text(engine, G, n, lab)
    assert whole == host_text(G, n, lab)
    for r in (1, 7, 300):
        assert dev_text(engine, G, n, lab, 0, r) + dev_text(engine, G, n, lab, r, rows - r) == whole


@pytest.mark.parametrize("n,rows,shift", [(5, 300, 0), (5, 300, 3), (200, 40, 9), (700, 9, 5), (1820, 3, 1)])
def test_guard_region_and_capacity(engine, n, rows, shift):
    """Nothing at or behind `bytes` is written, whatever the buffer's alignment; one byte short, nothing is written at all."""
    G = matrix(rows, n, seed=31)
    if n == 1820:
        G[1, :n] = 0.123457                                      # the direct path (at 700 pools row 5 is that long: workgroup per row)
    lab = E.labels(rows, seed=32)
    want = host_text(G, n, lab)
    t, n_chrom = dev_args(engine, G, n, *lab)
    rc, need = raw_call(engine, t, n_chrom, n, 0, rows, None, 0)
    assert rc == PG_ERR_INVALID and need == len(want)            # the size query
    store = torch.full((shift + need + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    buf = store[shift:]                                          # a buffer that starts `shift` bytes into a 16-byte word
    rc, got = raw_call(engine, t, n_chrom, n, 0, rows, buf, need - 1)
    assert rc == PG_ERR_INVALID and got == need and bool((store == 0xAA).all())
    rc, got = raw_call(engine, t, n_chrom, n, 0, rows, buf, need)
    assert rc == 0 and got == need
    host = store.cpu().numpy()
    assert host[shift:shift + need].tobytes() == want
    assert np.all(host[:shift] == 0xAA) and np.all(host[shift + need:] == 0xAA)


@pytest.mark.parametrize("value", [-0.1, 1.5, float("inf")])
def test_out_of_domain_cell(engine, value):
    n, rows = 65, 300
    G = matrix(rows, n, seed=41)
    lab = E.labels(rows, seed=42)
    G[211, 64] = value
    t, n_chrom = dev_args(engine, G, n, *lab)
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
    rc, need = raw_call(engine, t, n_chrom, n, 0, rows, buf, buf.numel())
    assert rc == PG_ERR_INVALID and b"no allele frequency" in engine._lib.pg_last_error(engine._ctx)
    good = G.copy(); good[211, 64] = 0.0
    assert need == len(host_text(good, n, lab))                 # the size is still reported (the cell counted as "0"), as the host form does
    assert raw_call(engine, t, n_chrom, n, 0, 211, buf, buf.numel())[0] == 0      # the rows in front of it are fine
    from poolgen_amd import NativeError
    with pytest.raises(NativeError):
        dev_text(engine, G, n, lab)


@pytest.mark.parametrize("kpm1", [False, True])
def test_from_counts_equals_the_oracle_composition(engine, oracle, kpm1):
    """tests/golden/test.sync -> Engine.load_frequencies -> Engine.freq_csv under the CLI's default filter."""
    from poolgen_amd import Filter
    counts, chrom_ids, pos, names, order = E.golden_fixture(oracle)
    dev = torch.from_numpy(np.stack(counts).astype(np.int32)).cuda()
    G, col_locus, col_allele = engine.load_frequencies(dev, np.full(5, 20.0), Filter(min_allele_frequency=0.001), keep_p_minus_1=kpm1,
                                                       order=torch.from_numpy(order))
    assert G.shape[0] == E.GOLDEN_ROWS[kpm1]
    text = engine.freq_csv(G, col_locus, col_allele, chrom_ids, pos, names, n=5).cpu().numpy().tobytes()
    assert text == E.golden_text(oracle, kpm1, header=False)
    if not kpm1:
        assert text.startswith(b"Chromosome1,456527,T,0,0.333333,0.333333,0.2,0.142857\n")
