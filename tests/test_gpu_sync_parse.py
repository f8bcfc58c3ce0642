"""pg_sync_parse_dev, the sync parser on the GPU: device = host twin = literal restatement (tests/sync_ref.py), exactly, on the
fixture, the corpus, and the shapes at which the kernels take another path."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import sync_corpus
import sync_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
ARRAYS = ("counts", "pos", "line_off", "chrom_len")
SCALARS = ("data_lines", "n_pools")


def as_numpy(r):
    """Engine.sync_parse's dictionary as the host twin's: counts and pos are the unsigned bits"""
    out = dict(r)
    for k in ARRAYS:
        out[k] = r[k].cpu().numpy()
    out["counts"] = out["counts"].view(np.uint32)
    out["pos"] = out["pos"].view(np.uint64)
    return out


def same(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (what, k)


@pytest.fixture(scope="module")
def fixture_text():
    return (GOLDEN / "test.sync").read_bytes()


@pytest.fixture(scope="module")
def fixture_want(fixture_text):
    return R.parse_ref(fixture_text)


def test_fixture_and_corpus(engine, fixture_text, fixture_want):
    from poolgen_amd import sync_parse_host
    cases = [("fixture", fixture_text, 0, fixture_want), ("fixture_expect_5", fixture_text, 5, fixture_want)]
    cases += [(k, t, n, R.parse_ref(t, n)) for k, (t, n) in sync_corpus.corpus().items()]
    for name, text, n, want in cases:
        same(sync_parse_host(text, n, n_threads=16), want, name)
        same(as_numpy(engine.sync_parse(text, n)), want, name)
    assert fixture_want["counts"].shape == (6674, 5, 6)
    assert engine.sync_parse(b"")["data_lines"] == 0 and engine.sync_parse(b"")["counts"].shape == (0, 0, 6)


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 63, 64, 65, 200, 1024, 1025, 4096])
def test_pool_counts_at_the_lane_group_steps(engine, n):
    """8, 16, 32 and 64 lanes per line; more pools than a wave has lanes; one line per workgroup above 1024 pools"""
    from poolgen_amd import sync_parse_host
    rng = np.random.default_rng(100 + n)
    lines = 37 if n <= 200 else 3
    text, counts = sync_corpus.random_text(rng, n, lines, comment_every=5)
    skipped = sync_corpus.line("chrZ", "x", [sync_corpus.GOOD] * n).encode()
    text = text + skipped + text[text.rfind(b"\n", 0, len(text) - 1) + 1:]          # a skipped line, then the last line again
    counts = np.concatenate([counts, counts[-1:]])
    want = sync_parse_host(text, 0, n_threads=16)
    assert np.array_equal(want["counts"], counts) and want["n_pools"] == n and want["data_lines"] == lines + 2
    if n <= 200:
        same(want, R.parse_ref(text), n)
    same(as_numpy(engine.sync_parse(text)), want, n)
    same(as_numpy(engine.sync_parse(text, n)), want, (n, "expect_n"))


def test_more_than_4096_pools_are_refused(engine, fixture_text, fixture_want):
    from poolgen_amd import NativeError
    from poolgen_amd.engine import SyncError
    with pytest.raises(NativeError):
        engine.sync_parse(fixture_text, 4097)                                          # before anything is launched
    text = sync_corpus.line("c", 1, ["1:2:3:4:5:6"] * 4097).encode()
    with pytest.raises(SyncError) as e:
        engine.sync_parse(text)
    assert (e.value.offset, e.value.reason) == (0, R.E_POOLS)
    same(as_numpy(engine.sync_parse(fixture_text)), fixture_want, "the context stays usable")


def one_pool_text(lines):
    """`lines` data lines of one pool whose answer is known by construction; every seventh position is no number (skipped)"""
    i = np.arange(lines)
    keep = i % 7 != 3
    text = "".join(f"c{k % 3}\t{k + 1 if kp else 'x'}\tN\t{k % 11}:{k % 5}:0:{k}:0:3\n" for k, kp in zip(i.tolist(), keep.tolist()))
    counts = np.zeros((int(keep.sum()), 1, 6), dtype=np.uint32)
    counts[:, 0, 0] = (i % 11)[keep]
    counts[:, 0, 1] = (i % 5)[keep]
    counts[:, 0, 3] = i[keep]
    counts[:, 0, 5] = 3
    return text.encode(), counts, (i[keep] + 1).astype(np.uint64)


@pytest.mark.parametrize("lines", [1, 255, 256, 257, 256 * 1024 + 1])
def test_line_counts_at_the_scan_levels(engine, lines):
    """one workgroup of the keep scan, its edge, and more than 1024 workgroups (the second round of the 64-bit scan)"""
    from poolgen_amd import sync_parse_host
    text, counts, pos = one_pool_text(lines)
    want = sync_parse_host(text, 0, n_threads=16)
    assert np.array_equal(want["counts"], counts) and np.array_equal(want["pos"], pos) and want["data_lines"] == lines
    if lines <= 257:
        same(want, R.parse_ref(text), lines)
    same(as_numpy(engine.sync_parse(text)), want, lines)
    same(as_numpy(engine.sync_parse(text[:-1])), want, (lines, "no final newline"))


def test_every_alignment_of_the_text(engine):
    """slices of one device tensor that start at each of 16 consecutive bytes"""
    rng = np.random.default_rng(5)
    text, counts = sync_corpus.random_text(rng, 5, 41, comment_every=8)
    dev = torch.frombuffer(bytearray(b"#" * 31 + b"\n" + text), dtype=torch.uint8).cuda()
    seen = set()
    for a in range(16):
        t = dev[a:]                                         # a comment line of 32 - a bytes in front
        seen.add(t.data_ptr() % 16)
        r = as_numpy(engine.sync_parse(t))
        assert np.array_equal(r["counts"], counts) and r["data_lines"] == 41, a
    assert len(seen) == 16


def test_result_does_not_depend_on_the_slab_cut(engine, fixture_text, fixture_want):
    """one slab; slabs of 1 line, of 7 lines and of 4 KB cut at line starts (slices of one device tensor, so of every alignment)"""
    whole = as_numpy(engine.sync_parse(fixture_text))
    same(whole, fixture_want, "whole")
    dev = torch.frombuffer(bytearray(fixture_text), dtype=torch.uint8).cuda()
    starts = [o for o, _ in R.text_lines(fixture_text)] + [len(fixture_text)]
    by_4k, last = [0], 0
    for s in starts:
        if s - by_4k[-1] > 4096:
            by_4k.append(last)
        last = s
    for cuts in (starts[:60] + [len(fixture_text)], starts[::7] + [len(fixture_text)], by_4k + [len(fixture_text)]):
        parts = [(a, as_numpy(engine.sync_parse(dev[a:z], 5))) for a, z in zip(cuts[:-1], cuts[1:]) if z > a]
        assert {p["n_pools"] for _, p in parts} <= {0, 5}
        got = {k: np.concatenate([p[k] + (a if k == "line_off" else 0) for a, p in parts if p["n_pools"]]) for k in ARRAYS}
        for k in ARRAYS:
            assert np.array_equal(got[k], whole[k]), (k, len(cuts))
        assert sum(p["data_lines"] for _, p in parts) == whole["data_lines"]


def test_nothing_is_written_behind_the_capacities(engine, fixture_text, fixture_want):
    from poolgen_amd._native import PgSyncInfo
    lib, ctx = engine._lib, engine._ctx
    want = fixture_want
    k, n = len(want["pos"]), 5
    text = torch.frombuffer(bytearray(b"abc" + fixture_text), dtype=torch.uint8).cuda()[3:]   # not 16-byte aligned
    info = PgSyncInfo()
    pad = 64
    bufs = [torch.full((k * n * 6 + pad,), 0x2B2B2B2B, dtype=torch.int32, device="cuda"), torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int64, device="cuda"),
            torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int64, device="cuda"), torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")]
    clean = [x.clone() for x in bufs]

    def call(cap_loci, cap_counts):
        rc = lib.pg_sync_parse_dev(ctx, text.data_ptr(), text.numel(), 0, *[x.data_ptr() for x in bufs], cap_loci, cap_counts, C.byref(info))
        engine.synchronize()
        return rc
    assert call(0, 0) == -1 and (info.kept, info.n_pools) == (k, n)             # the size query
    assert call(k - 1, k * n * 6) == -1 and call(k, k * n * 6 - 1) == -1
    assert all(torch.equal(x, c) for x, c in zip(bufs, clean))                    # too small: nothing written
    assert call(k, k * n * 6) == 0
    assert np.array_equal(bufs[0][:k * n * 6].cpu().numpy().view(np.uint32).reshape(k, n, 6), want["counts"])
    assert np.array_equal(bufs[1][:k].cpu().numpy().view(np.uint64), want["pos"])
    assert np.array_equal(bufs[2][:k].cpu().numpy(), want["line_off"])
    assert np.array_equal(bufs[3][:k].cpu().numpy(), want["chrom_len"])
    assert torch.equal(bufs[0][k * n * 6:], clean[0][k * n * 6:]) and all(torch.equal(x[k:], c[k:]) for x, c in zip(bufs[1:], clean[1:]))


def test_error_texts_fail_with_the_first_bad_line_and_leave_the_context_usable(engine, fixture_text, fixture_want):
    from poolgen_amd.engine import SyncError
    for name, (text, n, off, reason) in sync_corpus.error_texts().items():
        with pytest.raises(SyncError) as e:
            engine.sync_parse(text, n)
        assert (e.value.offset, e.value.reason) == (off, reason), name
        assert f"byte {off} " in str(e.value), name
        assert f"byte {off} " in engine._lib.pg_last_error(engine._ctx).decode(), name     # the message names the line
        same(as_numpy(engine.sync_parse(fixture_text)), fixture_want, ("after", name))
