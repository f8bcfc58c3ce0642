"""pg_vcf_parse_dev, the VCF parser on the GPU: device = host twin = literal restatement (tests/vcf_ref.py), exactly, on the
reference's fixture, the corpus, and the shapes at which the kernels take another path."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

import vcf_corpus
import vcf_ref as R

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
ARRAYS = ("counts", "pos", "ref", "line_off", "chrom_len")
SCALARS = ("data_lines", "n_pools", "chrom_line_off")


def as_numpy(r):
    """Engine.vcf_parse's dictionary as the host twin's: counts and pos are the unsigned bits"""
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
    return (GOLDEN / "test.vcf").read_bytes()


def test_fixture_and_corpus(engine, fixture_text):
    from poolgen_amd import vcf_parse_host
    cases = [(f"fixture_{d}_{b}_{f}", fixture_text, [0.1] * 10, d, b, f) for d, b, f in [(1, 1.0, 0.001), (1, 1.0, 0.0), (10, 1.0, 0.0), (5, 0.5, 0.05)]]
    cases += vcf_corpus.corpus()
    kept = []
    for name, text, sizes, d, b, f in cases:
        want = R.parse_ref(text, sizes, d, b, f)
        same(vcf_parse_host(text, sizes, d, b, f, n_threads=16), want, name)
        same(as_numpy(engine.vcf_parse(text, sizes, d, b, f)), want, name)
        kept.append(len(want["pos"]))
    assert kept[:4] == [380, 400, 61, 210]


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 63, 64, 65, 200])
def test_pool_counts_at_the_lane_group_steps(engine, n):
    """8, 16, 32 and 64 lanes per line; more pools than a wave has lanes"""
    from poolgen_amd import vcf_parse_host
    rng = np.random.default_rng(100 + n)
    text = (vcf_corpus.HEADER + vcf_corpus.chrom_line(n) + "".join(vcf_corpus.data_line(rng, n, short_ad=i % 5 == 4) for i in range(37))).encode("latin-1")   # every fifth line has one column: dropped
    sizes = (rng.integers(5, 60, size=n) * 1.0).tolist()
    want = R.parse_ref(text, sizes, 30, 0.75, 0.1)
    assert 0 < len(want["pos"]) < 37
    same(vcf_parse_host(text, sizes, 30, 0.75, 0.1, n_threads=16), want, n)
    same(as_numpy(engine.vcf_parse(text, sizes, 30, 0.75, 0.1)), want, n)


def test_every_alignment_of_the_text(engine):
    """slices of one device tensor that start at each of 16 consecutive bytes, the last line with and without its newline"""
    from poolgen_amd import vcf_parse_host
    rng = np.random.default_rng(5)
    sizes = [10.0, 20.0, 30.0, 40.0, 50.0]
    body = (vcf_corpus.chrom_line(5) + "".join(vcf_corpus.data_line(rng, 5, short_ad=i % 4 == 3) for i in range(11))).encode("latin-1")
    for text in (body, body[:-1]):
        dev = torch.frombuffer(bytearray(b"#" * 31 + b"\n" + text), dtype=torch.uint8).cuda()
        seen = set()
        for a in range(16):
            t = dev[a:]                                         # a comment line of 32 - a bytes in front
            seen.add(t.data_ptr() % 16)
            want = vcf_parse_host(b"#" * (31 - a) + b"\n" + text, sizes, 1, 0.5, 0.0, n_threads=1)
            assert 0 < len(want["pos"]) < 11
            same(as_numpy(engine.vcf_parse(t, sizes, 1, 0.5, 0.0)), want, (a, len(text)))
        assert len(seen) == 16


def one_pool_text(lines):
    """`lines` data lines of one pool whose answer is known by construction: AD = i % 7, i % 5"""
    i = np.arange(lines)
    a, b = i % 7, i % 5
    text = "".join(f"c{k % 3}\t{k + 1}\t.\tA\tT\t.\t.\tPADDING=xxxxxxx\tAD\t{x},{y}\n" for k, x, y in zip(i.tolist(), a.tolist(), b.tolist()))
    keep = (a + b) >= 1
    counts = np.zeros((int(keep.sum()), 1, 6), dtype=np.uint32)
    counts[:, 0, 0] = a[keep]
    counts[:, 0, 1] = b[keep]
    return text.encode(), counts, (i[keep] + 1).astype(np.uint64)


@pytest.mark.parametrize("lines", [1, 255, 256, 257, 256 * 1024 + 1])
def test_line_counts_at_the_scan_levels(engine, lines):
    """one workgroup of the keep scan, its edge, and more than 1024 workgroups (the second round of the 64-bit scan)"""
    from poolgen_amd import vcf_parse_host
    text, counts, pos = one_pool_text(lines)
    want = vcf_parse_host(text, [1.0], 1, 1.0, 0.0, n_threads=16)
    assert np.array_equal(want["counts"], counts) and np.array_equal(want["pos"], pos) and want["data_lines"] == lines
    if lines <= 257:
        same(want, R.parse_ref(text, [1.0], 1, 1.0, 0.0), lines)
    same(as_numpy(engine.vcf_parse(text, [1.0], 1, 1.0, 0.0)), want, lines)
    same(as_numpy(engine.vcf_parse(text[:-1], [1.0], 1, 1.0, 0.0)), want, (lines, "no final newline"))


def test_result_does_not_depend_on_the_slab_cut(engine, fixture_text):
    """one slab; slabs of 1 line, of 7 lines and of 4 KB cut at line starts (slices of one device tensor, so of every alignment)"""
    sizes = [0.1] * 10
    whole = as_numpy(engine.vcf_parse(fixture_text, sizes))
    dev = torch.frombuffer(bytearray(fixture_text), dtype=torch.uint8).cuda()
    starts = [o for o, _ in R.text_lines(fixture_text)] + [len(fixture_text)]
    by_4k, last = [0], 0
    for s in starts:
        if s - by_4k[-1] > 4096:
            by_4k.append(last)
        last = s
    for cuts in (starts[:60] + [len(fixture_text)], starts[::7] + [len(fixture_text)], by_4k + [len(fixture_text)]):
        parts = [(a, as_numpy(engine.vcf_parse(dev[a:z], sizes))) for a, z in zip(cuts[:-1], cuts[1:]) if z > a]
        assert {p["n_pools"] for _, p in parts} <= {0, 10}
        got = {k: np.concatenate([p[k] + (a if k == "line_off" else 0) for a, p in parts if p["n_pools"]]) for k in ARRAYS}
        for k in ARRAYS:
            assert np.array_equal(got[k], whole[k]), (k, len(cuts))
        assert sum(p["data_lines"] for _, p in parts) == whole["data_lines"]
        assert max(a + p["chrom_line_off"] for a, p in parts if p["chrom_line_off"] >= 0) == whole["chrom_line_off"]


def test_nothing_is_written_behind_the_capacities(engine, fixture_text):
    from poolgen_amd._native import PgVcfInfo
    lib, ctx = engine._lib, engine._ctx
    want = R.parse_ref(fixture_text, [0.1] * 10)
    k, n = len(want["pos"]), 10
    text = torch.frombuffer(bytearray(b"abc" + fixture_text), dtype=torch.uint8).cuda()[3:]   # not 16-byte aligned
    ps = np.full(10, 0.1)
    info = PgVcfInfo()
    pad = 64
    bufs = [torch.full((k * n * 6 + pad,), 0x2B2B2B2B, dtype=torch.int32, device="cuda"), torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int64, device="cuda"),
            torch.full((k + pad,), 0x2B, dtype=torch.uint8, device="cuda"), torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int64, device="cuda"),
            torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")]
    clean = [x.clone() for x in bufs]

    def call(cap_loci, cap_counts):
        rc = lib.pg_vcf_parse_dev(ctx, text.data_ptr(), text.numel(), ps.ctypes.data, 10, 1, 1.0, 0.001, *[x.data_ptr() for x in bufs], cap_loci, cap_counts,
                                  C.byref(info))
        engine.synchronize()
        return rc
    assert call(0, 0) == -1 and (info.kept, info.n_pools) == (k, n)             # the size query
    assert call(k - 1, k * n * 6) == -1 and call(k, k * n * 6 - 1) == -1
    assert all(torch.equal(x, c) for x, c in zip(bufs, clean))                    # too small: nothing written
    assert call(k, k * n * 6) == 0
    assert np.array_equal(bufs[0][:k * n * 6].cpu().numpy().view(np.uint32).reshape(k, n, 6), want["counts"])
    assert np.array_equal(bufs[1][:k].cpu().numpy().view(np.uint64), want["pos"])
    assert np.array_equal(bufs[3][:k].cpu().numpy(), want["line_off"])
    assert torch.equal(bufs[0][k * n * 6:], clean[0][k * n * 6:]) and all(torch.equal(x[k:], c[k:]) for x, c in zip(bufs[1:], clean[1:]))


def test_error_texts_fail_with_the_first_bad_line_and_leave_the_context_usable(engine, fixture_text):
    from poolgen_amd.engine import VcfError
    for name, (text, sizes, d, b, f, off, reason) in vcf_corpus.error_texts().items():
        with pytest.raises(VcfError) as e:
            engine.vcf_parse(text, sizes, d, b, f)
        assert (e.value.offset, e.value.reason) == (off, reason), name
        assert f"byte {off} " in engine._lib.pg_last_error(engine._ctx).decode(), name     # the message names the line
    text, sizes, d, b, f = vcf_corpus.dropped_not_errors()
    same(as_numpy(engine.vcf_parse(text, sizes, d, b, f)), R.parse_ref(text, sizes, d, b, f), "dropped_not_errors")
    assert len(engine.vcf_parse(fixture_text, [0.1] * 10)["pos"]) == 380
    assert engine.vcf_parse(b"", [1.0])["data_lines"] == 0
