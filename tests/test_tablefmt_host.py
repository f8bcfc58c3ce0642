"""pg_host_f64_table and pg_host_gudmc_rows, the plain C++ twins of the popgen writer's device formatters (pg_f64_table_dev,
pg_gudmc_rows_dev): against the restatement (tests/tablefmt_ref.py over tests/rustfmt.py) and against hand-written bytes, their
buffer contract, their refusals, thread-count independence; the restatement of gudmc's rows against gudmc_ref.csv_rows.  Runs
without a GPU."""
import ctypes as C

import numpy as np
import pytest

import f64_corpus as FC
import gudmc_ref as GR
import tablefmt_ref as TR

PG_OK, PG_ERR_INVALID = 0, -1
NAN, INF = float("nan"), float("inf")


def host_table(x, labels=None, **kw):
    from poolgen_amd import f64_table_host
    return f64_table_host(x, labels, **kw)


def test_hand_written_bytes(native):
    one = np.array([[0.5]])
    assert host_table(one) == b"0.5\n" == TR.table(one)                                             # a 1 x 1 table
    assert host_table(one, ["x,"]) == b"x,0.5\n"
    x = np.array([[1.0, 0.123456789, NAN], [-0.0, INF, -INF]])
    assert host_table(x, ["a,", "bb,"], n_digits=8) == b"a,1,0.12345679,NaN\nbb,-0,inf,-inf\n"
    assert host_table(x, ["", ""], n_digits=-1) == b"1,0.123456789,NaN\n-0,inf,-inf\n"            # empty labels
    assert host_table(x, None, n_digits=-1) == b"1,0.123456789,NaN\n-0,inf,-inf\n"                # no labels
    assert host_table(x, ["a", "b"], n_digits=-1) == b"a1,0.123456789,NaN\nb-0,inf,-inf\n"         # no separator is added
    # a transposed view (row_stride = 1): printed column by column, no copy
    assert host_table(x.T, ["p,", "q,", "r,"], n_digits=8) == b"p,1,-0\nq,0.12345679,inf\nr,NaN,-inf\n"
    assert x.T.strides == (8, 24)
    # first_col_digits different from n_digits: name,D(mean),R(w_0,8),...
    y = np.array([[0.123456789012, 0.123456789012, 2.0 / 3.0]])
    assert host_table(y, ["pool,"], n_digits=8, first_col_digits=-1) == b"pool,0.123456789012,0.12345679,0.66666667\n"
    assert host_table(y, ["pool,"], n_digits=-1, first_col_digits=2) == b"pool,0.12,0.123456789012,0.6666666666666666\n"
    # the smallest denormal: a cell of 327 bytes with its sign
    tiny = np.array([[5e-324, -5e-324]])
    want = b"0." + b"0" * 323 + b"5,-0." + b"0" * 323 + b"5\n"
    assert host_table(tiny) == want == TR.table(tiny) and len(want) == 326 + 1 + 327 + 1


def test_restatement_of_gudmc_rows_equals_gudmc_ref(native):
    c = GR.stage_cases()[2]
    ref = GR.stage_reference(2)
    n, w = c["n"], c["w"]
    assert (n, w) == (3, 40) and 0 in ref["rows"] and len(set(ref["rows"])) > 1      # a population without rows, NaN windows
    pools = ["alpha", "b", "pool_c"]
    names = ["chrI", "chromosome_2"]
    per_window = [names[k] for k in c["chrom"]]
    want = "".join(",".join(f) + "\n" for f in GR.csv_rows(ref, pools, per_window, c["ini"], c["fin"])).encode()
    arrays = TR.padded(ref, n, w)
    assert TR.gudmc_rows(arrays, c["chrom"], c["ini"], c["fin"], pools, names) == want and want.count(b"\n") == n * sum(ref["rows"])
    from poolgen_amd import gudmc_rows_host
    for threads in (1, 3):
        assert gudmc_rows_host(arrays, c["chrom"], c["ini"], c["fin"], pools, names, n_threads=threads) == want
    lines = want.splitlines(True)
    first = np.concatenate([[0], np.cumsum([ref["rows"][i % n] for i in range(n * n)])])
    cuts = sorted({0, 1, int(first[1]), int(first[1]) + 1, int(first[4]) - 1, int(first[4]), len(lines) - 1, len(lines)})
    for lo in cuts:                                                                      # inside a pair and on a pair boundary
        for hi in cuts:
            if hi >= lo:
                assert gudmc_rows_host(arrays, c["chrom"], c["ini"], c["fin"], pools, names, row0=lo, rows=hi - lo, n_threads=2) == b"".join(lines[lo:hi])
    from poolgen_amd import NativeError
    bad = c["chrom"].copy(); bad[0] = 2                                                  # a chromosome id outside the name table
    with pytest.raises(NativeError):
        gudmc_rows_host(arrays, bad, c["ini"], c["fin"], pools, names)
    for row0, rows in ((0, len(lines) + 1), (len(lines), 1), (-1, 1), (0, -1)):
        with pytest.raises(NativeError):
            gudmc_rows_host(arrays, c["chrom"], c["ini"], c["fin"], pools, names, row0=row0, rows=rows)
    assert gudmc_rows_host(arrays, c["chrom"], c["ini"], c["fin"], pools, names, row0=len(lines), rows=0) == b""


@pytest.fixture(scope="module")
def sample():
    """the f64_corpus sample as a 37-column table with labels, and the restatement's text for three digit settings: once"""
    x = FC.sample(37 * 60, seed=11).reshape(60, 37)
    labels = [f"row{r}," if r % 7 else "" for r in range(60)]
    return x, labels, {nd: TR.table(x, labels, *nd) for nd in ((-1, None), (8, None), (8, -1), (0, 22))}


def test_host_twin_equals_restatement_on_any_number_of_threads(native, sample):
    x, labels, want = sample
    for (nd, nd0), text in want.items():
        assert len(text) > 20_000
        for threads in (1, 3):
            assert host_table(x, labels, n_digits=nd, first_col_digits=nd0, n_threads=threads) == text, (nd, nd0, threads)
    whole = want[(8, -1)]
    lines = whole.splitlines(True)
    assert host_table(x.T, None, n_digits=8, n_threads=3) == TR.table(x.T, None, 8)
    for row0, n_rows in ((0, 0), (0, 1), (59, 1), (60, 0), (13, 29)):
        assert host_table(x, labels, n_digits=8, first_col_digits=-1, row0=row0, n_rows=n_rows, n_threads=3) == b"".join(lines[row0:row0 + n_rows])


def raw_table(native, x, labels, buf, cap, threads=2, **change):
    """the C entry point itself -> (rc, bytes); `change` replaces arguments by name"""
    from poolgen_amd.engine import label_table
    text, off = (None, None) if labels is None else label_table(labels)
    a = dict(data=x, rows=x.shape[0], cols=x.shape[1], rs=x.strides[0] // 8, cs=x.strides[1] // 8, row0=0, n_rows=x.shape[0], nd=8, nd0=-1, text=text, off=off)
    a.update(change)
    ptr = lambda v: None if v is None else v.ctypes.data
    need = C.c_int64(-7)
    rc = native.pg_host_f64_table(ptr(a["data"]), a["rows"], a["cols"], a["rs"], a["cs"], a["row0"], a["n_rows"], a["nd"], a["nd0"], ptr(a["text"]), ptr(a["off"]),
                                  ptr(buf), cap, C.byref(need), threads)
    return rc, need.value


def test_cap_rules_and_alignment(native, sample):
    x, labels, texts = sample
    want = texts[(8, -1)]
    assert raw_table(native, x, labels, None, 0) == (PG_ERR_INVALID, len(want))                 # the size query
    buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
    assert raw_table(native, x, labels, buf, len(want) - 1) == (PG_ERR_INVALID, len(want)) and (buf == 0xAA).all()
    for cap in (len(want), len(want) + 64):
        buf[:] = 0xAA
        assert raw_table(native, x, labels, buf, cap) == (PG_OK, len(want))
        assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()             # nothing at or behind text[bytes]
    for off in range(16):
        b = np.full(len(want) + 32, 0xAA, dtype=np.uint8)
        v = b[off:]
        assert raw_table(native, x, labels, v, len(want)) == (PG_OK, len(want))
        assert v[:len(want)].tobytes() == want and (b[:off] == 0xAA).all() and (v[len(want):] == 0xAA).all()


def test_refused_inputs(native, sample):
    x, labels, texts = sample
    from poolgen_amd.engine import label_table
    buf = np.full(len(texts[(8, -1)]) + 8, 0xAA, dtype=np.uint8)

    def refused(**change):
        buf[:] = 0xAA
        assert raw_table(native, x, labels, buf, buf.size, **change) == (PG_ERR_INVALID, 0) and (buf == 0xAA).all(), change

    assert raw_table(native, x, labels, buf, buf.size)[0] == PG_OK
    off = label_table(labels)[1].copy(); off[5] = off[4] - 1                                      # offsets that decrease
    refused(off=off)
    off = label_table(labels)[1].copy(); off[0] = -1
    refused(off=off)
    off = label_table(labels)[1].copy(); off[60] = off[59] + (1 << 22) + 1                       # a label above 2^22 bytes
    refused(off=off)
    for change in (dict(row0=-1), dict(n_rows=-1), dict(row0=61, n_rows=0), dict(row0=1, n_rows=60), dict(rows=-1), dict(cols=0), dict(rs=-1), dict(cs=-1),
                   dict(nd=23), dict(nd0=23), dict(data=None), dict(text=None)):
        refused(**change)
    assert raw_table(native, x, labels, buf, -1) == (PG_ERR_INVALID, 0)
    assert raw_table(native, x, labels, None, 5) == (PG_ERR_INVALID, 0)                            # a capacity without a buffer
    buf[:] = 0xAA
    assert raw_table(native, x, labels, buf, buf.size, n_rows=0) == (PG_OK, 0) and (buf == 0xAA).all()
    assert raw_table(native, x, labels, buf, buf.size, row0=60, n_rows=0) == (PG_OK, 0)
    # a bad offset among rows that are not formatted is not read
    off = label_table(labels)[1].copy(); off[50:] = 0
    assert raw_table(native, x, labels, buf, buf.size, off=off, n_rows=10)[0] == PG_OK
