"""pg_result_rows_dev and pg_kinship_rows_dev: the CSV rows of the GWAS analyses formatted on the GPU (pg_resultfmt.hip).  Device
equals host twin equals restatement (tests/resultfmt_ref.py) for every row kind, with dropped loci in runs across tile boundaries,
chromosome names of 1 to 40 bytes, positions of 1 to 20 digits, cells of 1 to 327 bytes, units on both sides of the tile limit
(the direct path forced by a name longer than the tile), every split of a small kinship case, and errors that leave the context
usable."""
import ctypes as C

import numpy as np
import pytest
import torch

import resultfmt_ref as RR

pytestmark = pytest.mark.gpu
PG_OK, PG_ERR_INVALID = 0, -1
TILE = 16384                         # RF_TILE of pg_resultfmt.hip
L = 3000


def host_rows(g, n_threads=8):
    from poolgen_amd import result_rows_host
    op, n_out, ids, freq, stat, pval, chrom, pos, names, k = RR.args_of(g)
    return result_rows_host(op, n_out, ids, freq, stat, pval, chrom, pos, names, k=k, n_threads=n_threads)


def dev(a, dtype=None):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a.copy()).cuda()


def dev_rows(engine, g, **kw):
    op, n_out, ids, freq, stat, pval, chrom, pos, names, k = RR.args_of(g)
    return engine.result_rows(op, dev(n_out), dev(ids), dev(freq), dev(stat), dev(pval), dev(chrom), dev(pos), names, k=k, **kw).cpu().numpy().tobytes()


def dev_kinship(engine, g, row0=0, rows=None):
    beta, pval, cc, cp, ca, names = RR.kinship_args_of(g)
    return engine.kinship_rows(dev(beta), dev(pval), dev(cc), dev(cp), dev(ca), names, row0=row0, rows=rows).cpu().numpy().tobytes()


def first_difference(got, want):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "line %d: device %r, host %r" % (i, a[:120], b[:120])
    return "lines %d / %d, bytes %d / %d" % (len(g), len(w), len(got), len(want))


CASES = [(op, k) for op in RR.OPS for k in ((1, 2, 3) if op in ("pearson_corr", "ols_iter") else (1,))]


@pytest.mark.parametrize("op,k", CASES)
def test_rows_equal_host_twin_and_restatement(engine, op, k):
    """corpus statistics: cells of 1 to 327 bytes, so that a workgroup's tile holds few loci and every tile boundary is ragged"""
    g = RR.generated(op, L, k, seed=1000 + 10 * RR.OPS.index(op) + k)
    got, want = dev_rows(engine, g), host_rows(g)
    assert got == want, first_difference(got, want)
    part = dict(g); part["n_out"] = g["n_out"].copy(); part["n_out"][400:] = 0       # the restatement on the first loci (it is slow), all else dropped
    assert dev_rows(engine, part) == RR.result_rows(*RR.args_of(part))
    lens = [len(l) for l in want.split(b"\n")]
    assert min(lens[:-1]) < 60 and max(lens) > 300                                    # short rows and rows with long cells


@pytest.mark.parametrize("op,k", [("ols_iter", 1), ("ols_iter", 3), ("fisher_exact_test", 1), ("gwalpha", 1)])
def test_realistic_rows_fill_whole_tiles(engine, op, k):
    """ordinary statistics: rows of some 50 bytes, hundreds of loci per workgroup, 256 lanes looping over a tile"""
    g = RR.generated(op, L, k, seed=77 + k, realistic=True)
    got, want = dev_rows(engine, g), host_rows(g)
    assert got == want, first_difference(got, want)
    part = dict(g); part["n_out"] = g["n_out"].copy(); part["n_out"][300:] = 0
    assert dev_rows(engine, part) == RR.result_rows(*RR.args_of(part))


def test_units_on_both_sides_of_the_tile_limit_and_the_direct_path(engine):
    """a locus' text just below, at and above the tile (the name's length sets it), then one far above it"""
    base = RR.generated("pearson_corr", 300, 2, seed=5, realistic=True)
    base["n_out"][:] = np.minimum(base["n_out"], 1); base["n_out"][10] = 1; base["ids"] = np.minimum(base["ids"], 5)
    base["chrom"][:] = 1; base["chrom"][10] = 0                                       # locus 10 carries the long name, twice (k = 2)
    short = host_rows(dict(base, names=["c", "d"]))
    unit10 = lambda name_len: 2 * (name_len - 1)                                      # bytes locus 10 gains over the one-byte name
    rows10 = [l for l in short.splitlines(True) if l.startswith(b"c,")]
    assert len(rows10) == 2
    at_tile = (TILE - sum(map(len, rows10))) // 2 + 1                                 # the name length at which locus 10 has TILE bytes (or TILE - 1)
    for name_len in (at_tile - 1, at_tile, at_tile + 1, at_tile + 2, 3 * TILE):
        g = dict(base, names=["c" * name_len, "d"])
        got, want = dev_rows(engine, g), host_rows(g)
        assert len(want) == len(short) + unit10(name_len)
        assert got == want, (name_len, first_difference(got, want))
    sizes = [sum(map(len, rows10)) + unit10(n) for n in (at_tile - 1, at_tile, at_tile + 1, at_tile + 2)]
    assert min(sizes) <= TILE < max(sizes)                                            # both sides of the limit were met


def test_alignment_capacity_and_canary(engine):
    g = RR.generated("ols_iter", 500, 2, seed=12, realistic=True)
    want = host_rows(g)
    for off in (0, 1, 7, 8, 15):
        buf = torch.full((len(want) + 48,), 0xAA, dtype=torch.uint8, device="cuda")
        out = dev_rows(engine, g, out=buf[off:off + len(want)])
        b = buf.cpu().numpy()
        assert out == want and b[off:off + len(want)].tobytes() == want and (b[:off] == 0xAA).all() and (b[off + len(want):] == 0xAA).all(), off


def test_kinship_rows(engine):
    from test_resultfmt_host import KIN_LITERAL
    g, want = KIN_LITERAL
    assert dev_kinship(engine, g) == want                                             # the intercept label, the shift, the unprinted last label
    for p, k in ((1, 1), (1, 3), (2, 1), (2, 2), (1000, 1), (1000, 3)):
        g = RR.generated_kinship(p, k, seed=50 + p + k)
        from poolgen_amd import kinship_rows_host
        host = kinship_rows_host(*RR.kinship_args_of(g), n_threads=8)
        got = dev_kinship(engine, g)
        assert got == host, (p, k, first_difference(got, host))
        if p <= 2 or k == 1:
            assert got == RR.kinship_rows(*RR.kinship_args_of(g))
    g = RR.generated_kinship(4, 3, seed=9)
    lines = dev_kinship(engine, g).splitlines(True)
    assert len(lines) == 12
    for row0 in range(13):
        for rows in range(13 - row0):
            assert dev_kinship(engine, g, row0, rows) == b"".join(lines[row0:row0 + rows]), (row0, rows)   # the parts concatenate to the whole


def test_errors_leave_the_context_usable(engine):
    from poolgen_amd import NativeError
    g = RR.generated("ols_iter", 600, 2, seed=4, realistic=True)
    g["n_out"] = np.maximum(g["n_out"], 1); g["ids"] = np.minimum(g["ids"], 5)
    want = host_rows(g)
    assert dev_rows(engine, g) == want

    def altered(key, index, value):
        a = g[key].copy(); a[index] = value
        return dict(g, **{key: a})

    for bad in (altered("chrom", 300, -1), altered("chrom", 300, len(g["names"])), altered("ids", 300, 6), altered("ids", 300, -1),
                dict(g, names=["n" * RR.UNIT_MAX] + g["names"][1:]), dict(g, k=0), dict(g, k=4097)):
        with pytest.raises(NativeError):
            dev_rows(engine, bad)
        assert dev_rows(engine, g) == want                                            # the next call gives the same bytes
    need = C.c_int64(-7)
    assert engine._lib.pg_result_rows_dev(engine._ctx, 9, 5, 1, None, None, None, None, None, None, None, None, None, 0, None, 0, C.byref(need)) == PG_ERR_INVALID
    assert need.value == 0
    assert engine._lib.pg_result_rows_dev(engine._ctx, 4, 0, 1, None, None, None, None, None, None, None, None, None, 0, None, 0, C.byref(need)) == PG_OK
    assert need.value == 0                                                            # L = 0
    dropped = dict(g, n_out=np.zeros_like(g["n_out"]))
    assert dev_rows(engine, dropped) == b""                                           # every locus dropped: no text, no launch of the emit step
    small = torch.empty(len(want) - 1, dtype=torch.uint8, device="cuda")
    with pytest.raises(NativeError):
        dev_rows(engine, g, out=small)
    kg = RR.generated_kinship(5, 2, seed=1)
    for row0, rows in ((0, 11), (10, 1), (-1, 2)):
        with pytest.raises(NativeError):
            dev_kinship(engine, kg, row0, rows)
    bad = dict(kg); a = kg["col_allele"].copy(); a[0] = 6; bad["col_allele"] = a
    with pytest.raises(NativeError):
        dev_kinship(engine, bad)
    assert dev_kinship(engine, kg) == RR.kinship_rows(*RR.kinship_args_of(kg)) and dev_rows(engine, g) == want
