"""pg_f64_table_dev and pg_gudmc_rows_dev, the popgen writer's device formatters: device == host twin == restatement
(tests/tablefmt_ref.py) on the shapes where a cell-parallel scan and a tile flush can go wrong.  The formatter's constants: 256
cells per workgroup (one workgroup of the scan's first level), 1024 workgroup sums per round of its second level, a tile of
16 384 bytes."""
import numpy as np
import pytest
import torch

import f64_corpus as FC
import gudmc_ref as GR
import tablefmt_ref as TR

pytestmark = pytest.mark.gpu
TILE = 16384
LONG = -5e-324                                                                           # a cell of 327 bytes


def dev_table(engine, x, labels=None, transposed=False, **kw):
    t = torch.from_numpy(np.ascontiguousarray(x.T if transposed else x)).to(torch.device("cuda", engine.device))
    return engine.f64_table(t.T if transposed else t, labels, **kw).cpu().numpy().tobytes()


def all_three(engine, x, labels=None, **kw):
    """the device's text, once it equals the host twin's and the restatement's"""
    from poolgen_amd import f64_table_host
    want = TR.table(x, labels, kw.get("n_digits", -1), kw.get("first_col_digits"), kw.get("row0", 0), kw.get("n_rows"))
    assert f64_table_host(x, labels, n_threads=3, **kw) == want
    got = dev_table(engine, x, labels, **kw)
    assert got == want, (x.shape, kw, len(got), len(want))
    return got


@pytest.mark.parametrize("cols", [1, 255, 256, 257])
def test_columns_around_a_workgroup(engine, cols):
    x = FC.sample(cols * 5, seed=cols).reshape(5, cols)                                   # cells of 1 to 327 bytes, NaN, inf, -0 among them
    labels = [f"r{r}," for r in range(5)]
    assert len(all_three(engine, x, labels, n_digits=8, first_col_digits=-1)) > 10 * cols
    all_three(engine, x, None)
    from poolgen_amd import f64_table_host
    assert dev_table(engine, x.T, None, transposed=True, n_digits=8) == f64_table_host(x.T, None, n_digits=8) == TR.table(x.T, None, 8)


def test_one_cell_more_than_a_round_of_the_second_scan_level(engine):
    rows, cols = 5, 52429
    assert rows * cols == 256 * 1024 + 1
    x = (np.arange(rows * cols, dtype=np.float64) * 0.001 - 100.0).reshape(rows, cols)
    x[3, 77] = LONG
    text = all_three(engine, x, [f"{r}:" for r in range(rows)])
    assert text.count(b"\n") == rows and text.count(b",") == rows * (cols - 1)


@pytest.mark.parametrize("nbytes", [TILE - 1, TILE, TILE + 1])
def test_a_row_either_side_of_the_tile(engine, nbytes):
    for cols in (100, (TILE - 2) // 2):                                                   # a long label and few cells; hardly a label and many cells
        x = np.ones((3, cols))
        lab = "L" * (nbytes - 2 * cols)
        text = all_three(engine, x, [lab, "", lab])
        assert [len(l) for l in text.splitlines(True)] == [nbytes, 2 * cols, nbytes]


def test_long_cells_span_tiles_and_straddle_their_edges(engine):
    rng = np.random.default_rng(5)
    x = (rng.integers(1, 1 << 40, size=(1, 3000)).astype(np.float64) * 5e-324) * rng.choice([-1.0, 1.0], size=(1, 3000))
    text = all_three(engine, x, ["one row,"])
    assert len(text) > 3000 * 318 > 50 * TILE
    for before in (TILE - 330, TILE - 327, TILE - 100, TILE - 1, TILE, 2 * TILE - 50):     # the 327-byte cell begins `before` bytes into the text
        cols = before // 2
        x = np.ones((1, cols + 3))
        x[0, cols] = LONG
        all_three(engine, x, ["x" * (before - 2 * cols)])


@pytest.mark.parametrize("label_bytes", [TILE - 1, TILE + 1, 3 * TILE + 5, 1 << 22])
def test_a_label_longer_than_a_tile(engine, label_bytes):
    x = np.array([[0.5, LONG], [1.0, 2.0], [3.0, 4.0]])
    rng = np.random.default_rng(label_bytes)
    long_label = bytes(rng.integers(97, 123, size=label_bytes, dtype=np.uint8))
    text = all_three(engine, x, [b"a,", long_label, b"z,"])
    assert len(text) == (2 + 4 + 328) + (label_bytes + 4) + (2 + 4)
    from poolgen_amd import NativeError
    with pytest.raises(NativeError):                                                      # one byte above the label limit
        dev_table(engine, x, [b"a,", bytes((1 << 22) + 1), b"z,"])


def test_alignments_guard_bytes_and_row_cuts(engine):
    from poolgen_amd import NativeError
    dev = torch.device("cuda", engine.device)
    x = FC.sample(5 * 300, seed=9).reshape(5, 300)
    labels = [f"row{r}," for r in range(5)]
    want = TR.table(x, labels, 8, -1)
    t = torch.from_numpy(x).to(dev)
    for off in range(16):                                                                 # every alignment of text_dev
        buf = torch.full((len(want) + 64,), 0xAA, dtype=torch.uint8, device=dev)
        got = engine.f64_table(t, labels, n_digits=8, first_col_digits=-1, out=buf[off:off + len(want)])
        whole = buf.cpu().numpy()
        assert got.numel() == len(want) and whole[off:off + len(want)].tobytes() == want
        assert (whole[:off] == 0xAA).all() and (whole[off + len(want):] == 0xAA).all()    # the bytes around the text left untouched
    buf = torch.full((len(want) + 64,), 0xAA, dtype=torch.uint8, device=dev)
    with pytest.raises(NativeError, match="the buffer holds"):                            # one byte short: nothing written
        engine.f64_table(t, labels, n_digits=8, first_col_digits=-1, out=buf[:len(want) - 1])
    assert (buf.cpu().numpy() == 0xAA).all()
    lines = want.splitlines(True)
    for row0 in range(6):                                                                 # every cut of the 5 rows
        for n_rows in range(6 - row0):
            got = engine.f64_table(t, labels, n_digits=8, first_col_digits=-1, row0=row0, n_rows=n_rows).cpu().numpy().tobytes()
            assert got == b"".join(lines[row0:row0 + n_rows]), (row0, n_rows)
    for row0, n_rows in ((0, 6), (5, 1), (6, 0), (-1, 1), (0, -1)):
        with pytest.raises(NativeError):
            engine.f64_table(t, labels, row0=row0, n_rows=n_rows)
    from poolgen_amd.engine import label_table
    text, off = label_table(labels)
    off[3] = off[2] - 1                                                                   # offsets that decrease
    with pytest.raises(NativeError, match="label"):
        engine.f64_table(t, (torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)))
    assert engine.f64_table(t, (torch.from_numpy(text).to(dev), torch.from_numpy(off).to(dev)), n_rows=2).numel() > 0   # not among the rows asked for
    with pytest.raises(NativeError):
        engine.f64_table(t, labels, n_digits=23)


# ---- gudmc's rows -------------------------------------------------------------------------------------------------------------
POOLS = ["alpha", "b", "pool_c"]
CHROMS = ["chrI", "chromosome_2"]


@pytest.fixture(scope="module")
def stage(engine):
    """pg_gudmc_dev's outputs for n = 3, w = 40 (NaN windows, population 2 without rows), on the device and as arrays, and the
    restatement's text of them: once"""
    c = GR.stage_cases()[2]
    out = engine.gudmc_from_tables(c["d"], c["fst"], c["chrom"], c["ini"], c["fin"], c["thr"], c["rate"])
    host = {k: v.cpu().numpy() for k, v in out.items()}
    rows = host["rows"].tolist()
    assert (c["n"], c["w"]) == (3, 40) and rows[2] == 0 and 0 < rows[1] < rows[0] == 40
    return c, out, host, TR.gudmc_rows(host, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS)


def test_gudmc_rows_device_host_restatement(engine, stage):
    from poolgen_amd import gudmc_rows_host
    c, out, host, want = stage
    assert want.count(b"\n") == 3 * int(host["rows"].sum()) and all(l.count(b",") == 14 for l in want.splitlines())
    assert gudmc_rows_host(host, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS, n_threads=3) == want
    assert engine.gudmc_rows(out, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS).cpu().numpy().tobytes() == want


def test_gudmc_rows_in_slabs_and_refusals(engine, stage):
    from poolgen_amd import NativeError
    c, out, host, want = stage
    lines = want.splitlines(True)
    rows = host["rows"].tolist()
    first = np.concatenate([[0], np.cumsum([rows[i % 3] for i in range(9)])]).tolist()
    assert first[-1] == len(lines)
    cuts = sorted({0, 1, first[1] - 1, first[1], first[1] + 1, first[2], first[3], first[4] + 5, first[8], len(lines) - 1, len(lines)})
    for lo, hi in zip(cuts[:-1], cuts[1:]):                                               # cuts inside a pair and on pair boundaries
        got = engine.gudmc_rows(out, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS, row0=lo, rows=hi - lo).cpu().numpy().tobytes()
        assert got == b"".join(lines[lo:hi]), (lo, hi)
    for step in (1, 7):
        parts = [engine.gudmc_rows(out, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS, row0=r, rows=min(step, len(lines) - r)).cpu().numpy().tobytes()
                 for r in range(0, len(lines), step)]
        assert b"".join(parts) == want
    assert engine.gudmc_rows(out, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS, row0=len(lines), rows=0).numel() == 0
    bad = c["chrom"].copy(); bad[0] = 2                                                   # a chromosome id outside the name table
    with pytest.raises(NativeError):
        engine.gudmc_rows(out, bad, c["ini"], c["fin"], POOLS, CHROMS)
    for row0, n_rows in ((0, len(lines) + 1), (len(lines), 1), (-1, 1), (0, -1)):
        with pytest.raises(NativeError):
            engine.gudmc_rows(out, c["chrom"], c["ini"], c["fin"], POOLS, CHROMS, row0=row0, rows=n_rows)
