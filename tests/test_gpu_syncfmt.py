"""pg_sync_format_rows_dev (pg_syncfmt.hip): the sync lines the GPU formats equal the host twin's (pg_host_sync_format_rows, itself
checked against the restatement and hand-written bytes in test_syncfmt_host.py) and the restatement's (tests/syncfmt_ref.py)
byte for byte, on both sides of every dispatch rule of the kernels; the buffer contract; the refusals; and the compositions with
the three parsers, rows never leaving the device."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import syncfmt_corpus as SC
import syncfmt_ref as SR

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
PG_OK, PG_ERR_INVALID = 0, -1


def kernel_constant(name):
    """a `constexpr int NAME = <number or 1 << number>` of pg_syncfmt.hip"""
    src = (ROOT / "poolgen_amd" / "csrc" / "pg_syncfmt.hip").read_text()
    m = re.search(r"\b%s = (\d+)( << (\d+|[A-Z_]+))?[;,]" % name, src)
    assert m, name
    if m.group(2) is None:
        return int(m.group(1))
    shift = m.group(3)
    return int(m.group(1)) << (int(shift) if shift.isdigit() else kernel_constant(shift))


TILE = kernel_constant("SF_TILE")                  # bytes of text a workgroup stages in LDS
COUNT_ROWS = kernel_constant("SF_COUNT_ROWS")      # rows per workgroup of the scan's first level
SCAN_WIDTH = kernel_constant("SF_SCAN_WIDTH")      # workgroup sums per round of its second level


def to_dev(rows):
    """the rows as Engine.sync_format takes them: tensors on the device (the uint32 / uint64 bits as int32 / int64)"""
    return [torch.from_numpy(np.ascontiguousarray(rows["counts"], dtype=np.uint32).view(np.int32)).cuda(),
            torch.from_numpy(np.ascontiguousarray(rows["pos"], dtype=np.uint64).view(np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(rows["ref"], dtype=np.uint8)).cuda(),
            torch.from_numpy(np.ascontiguousarray(rows["line_off"], dtype=np.int64)).cuda(),
            torch.from_numpy(np.ascontiguousarray(rows["chrom_len"], dtype=np.int32)).cuda(),
            torch.from_numpy(np.frombuffer(rows["slab"] or b"\0", dtype=np.uint8).copy()).cuda()[:len(rows["slab"])]]


def dev_text(engine, rows) -> bytes:
    out = engine.sync_format(*to_dev(rows))
    assert out.dtype == torch.uint8 and out.is_cuda
    return out.cpu().numpy().tobytes()


def host_text(rows, n_threads=4) -> bytes:
    from poolgen_amd import sync_format_host
    return sync_format_host(*SC.args_of(rows), n_threads=n_threads)


def raw_call(engine, t, buf, cap, n_pools=None, n_rows=None, slab_bytes=None):
    """the C entry point itself, with the caller's buffer and capacity -> (rc, bytes)"""
    need = C.c_int64(-7)
    rc = engine._lib.pg_sync_format_rows_dev(engine._ctx, t[5].data_ptr() if t[5].numel() else None, t[5].numel() if slab_bytes is None else slab_bytes,
                                             t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), t[4].data_ptr(),
                                             t[0].shape[1] if n_pools is None else n_pools, t[0].shape[0] if n_rows is None else n_rows,
                                             buf.data_ptr() if buf is not None else None, cap, C.byref(need))
    torch.cuda.synchronize()
    return rc, need.value


def host_raw_call(engine, rows, cap, n_pools=None, n_rows=None, slab_bytes=None):
    """the host twin on the same arguments -> (rc, bytes)"""
    slab = np.frombuffer(rows["slab"], dtype=np.uint8)
    c = np.ascontiguousarray(rows["counts"], dtype=np.uint32)
    buf = np.empty(max(cap, 1), dtype=np.uint8)
    need = C.c_int64(-7)
    rc = engine._lib.pg_host_sync_format_rows(slab.ctypes.data if slab.size else None, slab.size if slab_bytes is None else slab_bytes, c.ctypes.data,
                                              rows["pos"].ctypes.data, rows["ref"].ctypes.data, rows["line_off"].ctypes.data,
                                              rows["chrom_len"].ctypes.data, c.shape[1] if n_pools is None else n_pools,
                                              c.shape[0] if n_rows is None else n_rows, buf.ctypes.data, cap, C.byref(need), 2)
    return rc, need.value


def test_literals(engine):
    for name, rows, want in SC.LITERALS:
        assert dev_text(engine, rows) == want, name


# Pool counts.  The rule of pg_syncfmt.hip (sf_lpr_shift): a row is formatted by the smallest power of two of lanes that holds
# n_pools, at most a wave of 64: 1 -> 1, 2 -> 2, 5 and 8 -> 8, 9 -> 16, 63 and 64 -> 64; from 65 pools on a lane takes several
# pools in turn (65: two turns, the second with one pool; 200: four).  Counts of every digit count are mixed inside every pool, so
# the text lengths differ from lane to lane; rows 0.. carry the position edges, every reference byte and every name place.
@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 63, 64, 65, 200])
def test_pool_counts(engine, n):
    k = 300 if n <= 9 else 41
    rows = SC.generated(n, k, seed=n)
    want = host_text(rows)
    assert want == SR.rows_text(*SC.args_of(rows))
    assert dev_text(engine, rows) == want


# Row counts around the scan's boundaries: its first level takes COUNT_ROWS rows per workgroup, its second SCAN_WIDTH sums per
# round.  n = 1 and no names keep the rows short (at most "\t" + 20 + "\t" + 1 + 66 + 1 bytes).
@pytest.mark.parametrize("k", [1, COUNT_ROWS - 1, COUNT_ROWS, COUNT_ROWS + 1, COUNT_ROWS * SCAN_WIDTH + 1])
def test_row_counts_around_the_scan_boundaries(engine, k):
    rows = SC.generated(1, k, seed=7, names=False)
    want = host_text(rows, 16)
    if k <= COUNT_ROWS + 1:
        assert want == SR.rows_text(*SC.args_of(rows))
    else:                                                                 # (the restatement on the first and the last rows)
        first, last = ({key: (v[sl] if key != "slab" else v) for key, v in rows.items()} for sl in (slice(0, 300), slice(k - 300, k)))
        assert want.startswith(SR.rows_text(*SC.args_of(first))) and want.endswith(SR.rows_text(*SC.args_of(last)))
    assert dev_text(engine, rows) == want


def test_the_shortest_rows_fill_a_tile(engine):
    """Rows per workgroup = TILE / the longest row, without a cap: "\\t0\\tA\\t0:0:0:0:0:0\\n" is 17 bytes, so a workgroup takes
    963 rows (its 256 one-lane groups take several each) and 5 000 rows span six workgroups."""
    k = 5000
    rows = SC.rows_of(b"", [(0, 0, 0, ord("A"), [[0] * 6])] * k)
    want = b"\t0\tA\t0:0:0:0:0:0\n" * k
    assert TILE // 17 > 256 and host_text(rows) == want
    assert dev_text(engine, rows) == want


def long_rows(n, name_len, k=3):
    """k rows of n pools of ten-digit counts under a name of name_len bytes: row 1 is name_len + 4 + 66 n + 1 bytes long (its
    position is one digit), the others have a 20-digit position and shorter counts"""
    r = SC.generated(n, k, seed=n + name_len, digits=10, names=False)
    r["slab"] = bytes(97 + i % 26 for i in range(name_len))
    r["chrom_len"] = np.full(k, name_len, dtype=np.int32)
    r["pos"] = np.array([2 ** 64 - 1, 7, 10 ** 19][:k], dtype=np.uint64)
    r["counts"][0] //= 1000
    r["counts"][2:] //= 10
    return r


# The tile rule: the emit kernel stages rows in LDS while the LONGEST row of the call fits TILE bytes, and takes the direct path (a
# wave per row, byte stores to the output) otherwise.  248 pools of ten-digit counts are 66 x 248 + 5 = 16 373 bytes with an
# empty name; the name's length moves the longest row to TILE - 1, TILE (staged, one row per workgroup) and TILE + 1 (direct).
@pytest.mark.parametrize("over", [-1, 0, 1])
def test_rows_around_the_tile(engine, over):
    n = (TILE - 5) // 66
    name_len = TILE + over - (66 * n + 5)
    assert 0 <= name_len < 66
    rows = long_rows(n, name_len)
    want = host_text(rows)
    assert max(len(l) + 1 for l in want.split(b"\n")[:-1]) == TILE + over
    assert want == SR.rows_text(*SC.args_of(rows))
    assert dev_text(engine, rows) == want


def test_the_longest_rows_take_the_direct_path(engine):
    """4096 pools of ten-digit counts, 3 rows of about 270 KB"""
    rows = long_rows(SR.MAX_POOLS, 300)
    want = host_text(rows)
    assert max(len(l) + 1 for l in want.split(b"\n")[:-1]) == 300 + 5 + 66 * SR.MAX_POOLS > TILE
    assert want == SR.rows_text(*SC.args_of(rows))
    assert dev_text(engine, rows) == want


@pytest.mark.parametrize("n,k,direct", [(5, 300, False), (200, 40, False), (260, 3, True)])
def test_alignment_capacity_and_canaries(engine, n, k, direct):
    """text_dev at every misalignment 0 .. 15: the size query, one byte short (nothing written at all), the exact size; 64 bytes in
    front of and behind the text stay as they were."""
    rows = long_rows(n, 40, k) if direct else SC.generated(n, k, seed=31 + n)
    want = host_text(rows)
    assert (max(len(l) + 1 for l in want.split(b"\n")[:-1]) > TILE) == direct
    t = to_dev(rows)
    rc, need = raw_call(engine, t, None, 0)
    assert rc == PG_ERR_INVALID and need == len(want)                    # the size query
    for shift in range(16):
        store = torch.full((64 + shift + need + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        buf = store[64 + shift:]                                         # (torch's blocks start on a multiple of 16)
        assert buf.data_ptr() % 16 == shift
        rc, got = raw_call(engine, t, buf, need - 1)
        assert rc == PG_ERR_INVALID and got == need and bool((store == 0xAA).all()), shift
        rc, got = raw_call(engine, t, buf, need)
        assert rc == PG_OK and got == need, shift
        host = store.cpu().numpy()
        assert host[64 + shift:64 + shift + need].tobytes() == want, shift
        assert np.all(host[:64 + shift] == 0xAA) and np.all(host[64 + shift + need:] == 0xAA), shift


def test_refusals_match_the_host_twin(engine):
    rows = SC.generated(4, 300, seed=9)
    want = host_text(rows)
    buf = torch.full((len(want) + 64,), 0xAA, dtype=torch.uint8, device="cuda")

    def both(change, **kw):
        r = dict(rows)
        for key, v in change.items():
            a = r[key].copy(); a[277] = v; r[key] = a                    # a row of the second workgroup of the measure step
        buf.fill_(0xAA)
        rc, got = raw_call(engine, to_dev(r), buf, buf.numel(), **kw)
        assert (rc, got) == host_raw_call(engine, r, buf.numel(), **kw), (change, kw)
        assert rc == PG_ERR_INVALID and got == 0 and bool((buf == 0xAA).all()), (change, kw)

    both({"line_off": -1})
    both({"chrom_len": -1})
    both({"line_off": len(rows["slab"]), "chrom_len": 1})
    both({"line_off": len(rows["slab"]) - 3, "chrom_len": 4})
    both({"line_off": 2 ** 62, "chrom_len": 2 ** 31 - 1})
    both({}, slab_bytes=int(rows["line_off"].max()) - 1)
    both({}, slab_bytes=-1)
    both({}, n_pools=0)
    both({}, n_pools=SR.MAX_POOLS + 1)                                   # refused before anything is launched
    both({}, n_rows=-1)
    assert b"lies outside the slab" not in engine._lib.pg_last_error(engine._ctx)
    both({"chrom_len": -5})
    assert b"lies outside the slab" in engine._lib.pg_last_error(engine._ctx)
    t = to_dev(rows)
    rc, got = raw_call(engine, t, None, 5)                               # a capacity without a buffer
    assert rc == PG_ERR_INVALID and got == 0
    buf.fill_(0xAA)
    rc, got = raw_call(engine, t, buf, buf.numel(), n_rows=0)            # rows = 0: PG_OK, bytes = 0
    assert (rc, got) == (PG_OK, 0) == host_raw_call(engine, rows, buf.numel(), n_rows=0) and bool((buf == 0xAA).all())
    from poolgen_amd import NativeError
    bad = dict(rows); a = rows["line_off"].copy(); a[0] = -1; bad["line_off"] = a
    with pytest.raises(NativeError):
        dev_text(engine, bad)
    # a name that ends exactly at the slab's end, and the empty name behind its last byte, are fine
    ok = dict(rows); a = rows["line_off"].copy(); a[277] = len(rows["slab"]); ok["line_off"] = a
    b = rows["chrom_len"].copy(); b[277] = 0; ok["chrom_len"] = b
    assert dev_text(engine, ok) == host_text(ok)


def test_out_buffer(engine):
    """Engine.sync_format(out=...): one call into the caller's buffer, the filled part returned, nothing behind it touched"""
    rows = SC.generated(9, 100, seed=51)
    want = host_text(rows)
    t = to_dev(rows)
    buf = torch.full((len(want) + 32,), 0xAA, dtype=torch.uint8, device="cuda")
    got = engine.sync_format(*t, out=buf)
    assert got.data_ptr() == buf.data_ptr() and got.cpu().numpy().tobytes() == want and bool((buf[len(want):] == 0xAA).all())
    from poolgen_amd import NativeError
    with pytest.raises(NativeError):
        engine.sync_format(*t, out=buf[:len(want) - 1])


# ---- compositions: parse on the device, format on the device, nothing brought to the host in between -------------------------
@pytest.mark.parametrize("depth,breadth,maf", [(1, 1.0, 0.001), (1, 1.0, 0.0), (10, 1.0, 0.0), (5, 0.5, 0.05)])
def test_vcf_parse_then_format(engine, depth, breadth, maf):
    from poolgen_amd import sync_format_host, vcf_parse_host
    text = (GOLDEN / "test.vcf").read_bytes()
    sizes = [0.1] * 10
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    p = engine.vcf_parse(slab, sizes, depth, breadth, maf)
    got = engine.sync_format(p["counts"], p["pos"], p["ref"], p["line_off"], p["chrom_len"], slab).cpu().numpy().tobytes()
    h = vcf_parse_host(text, sizes, depth, breadth, maf, n_threads=4)
    assert got == sync_format_host(h["counts"], h["pos"], h["ref"], h["line_off"], h["chrom_len"], text, n_threads=4)
    if (depth, maf) == (1, 0.0):
        import vcf_ref
        want = vcf_ref.vcf2sync_bytes(text, sizes, depth, breadth, maf)
        assert got == want[want.index(b"\n") + 1:] and len(got) > 0


@pytest.mark.parametrize("k", [0, 1])
def test_pileup_parse_then_format(engine, k):
    import pileup_corpus
    from poolgen_amd import pileup_parse_host, sync_format_host
    sizes, rule, _, _, text, _ = pileup_corpus.generated(k)
    text = b"".join(text.splitlines(keepends=True)[:400])
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    p = engine.pileup_parse(slab, sizes, **rule)
    got = engine.sync_format(p["counts"], p["pos"], p["ref"], p["line_off"], p["chrom_len"], slab).cpu().numpy().tobytes()
    h = pileup_parse_host(text, sizes, n_threads=4, **rule)
    assert h["counts"].shape[0] > 100
    assert got == sync_format_host(h["counts"], h["pos"], h["ref"], h["line_off"], h["chrom_len"], text, n_threads=4)


@pytest.mark.parametrize("n", [3, 70])
def test_sync_parse_then_format_is_the_identity(engine, n):
    import sync_corpus
    text, counts = sync_corpus.random_text(np.random.default_rng(n), n, 300)
    slab = torch.from_numpy(np.frombuffer(text, dtype=np.uint8).copy()).cuda()
    p = engine.sync_parse(slab, expect_n=n)
    assert p["counts"].shape[0] == 300
    ref = torch.full((300,), ord("A"), dtype=torch.uint8, device="cuda")  # the sync parser returns no reference bytes: sync_corpus writes "A"
    got = engine.sync_format(p["counts"], p["pos"], ref, p["line_off"], p["chrom_len"], slab).cpu().numpy().tobytes()
    assert got == text


def test_nothing_is_carried_between_calls(engine):
    """Two calls on one context, a large one and then a small one: the second gives the bytes a fresh context gives."""
    from poolgen_amd import Engine
    large = SC.generated(200, 600, seed=61)
    small = SC.generated(5, 3, seed=62)
    assert dev_text(engine, large) == host_text(large)
    second = dev_text(engine, small)
    e = Engine(0)
    try:
        first = dev_text(e, small)
    finally:
        torch.cuda.synchronize()
        e.close()
    assert second == first == host_text(small)
