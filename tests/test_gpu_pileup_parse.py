"""pg_pileup_parse_dev, the mpileup parser on the GPU: device = host twin = literal restatement (tests/pileup_ref.py), exactly,
on the corpus, the generated lines, and the shapes at which the kernels take another path."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import pileup_corpus
import pileup_ref as R

pytestmark = pytest.mark.gpu
ARRAYS = ("counts", "pos", "ref", "line_off", "chrom_len")
SCALARS = ("lines", "n_pools")


def as_numpy(r):
    """Engine.pileup_parse's dictionary as the host twin's: counts and pos are the unsigned bits"""
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
        g = np.asarray(got[k])
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (what, k)


def test_corpus(engine):
    from poolgen_amd import pileup_parse_host
    for name, text, sizes, rule in pileup_corpus.texts():
        want = R.parse_ref(text, sizes, **rule)
        same(pileup_parse_host(text, sizes, **rule, n_threads=8), want, name)
        same(as_numpy(engine.pileup_parse(text, sizes, **rule)), want, name)


@pytest.mark.parametrize("k", range(len(pileup_corpus.FILTER_SETS)))
def test_generated_lines(engine, k):
    """the lines that are no error as one text; the first twenty fatal ones each behind sound lines"""
    from poolgen_amd import pileup_parse_host
    from poolgen_amd.engine import PileupError
    sizes, rule, lines, outcomes, text, want = pileup_corpus.generated(k)
    same(pileup_parse_host(text, sizes, **rule, n_threads=8), want, k)
    same(as_numpy(engine.pileup_parse(text, sizes, **rule)), want, k)
    head = text[:R.text_lines(text)[5][0]]
    for line, o in [(l, o) for l, o in zip(lines, outcomes) if o[0] == "E"][:20]:
        with pytest.raises(PileupError) as e:
            engine.pileup_parse(head + line + b"\n" + head, sizes, **rule)
        assert (e.value.offset, e.value.reason) == (len(head), o[1]), line


@pytest.mark.parametrize("n", [1, 2, 5, 8, 9, 63, 64, 65, 200])
def test_pool_counts_at_the_lane_group_steps(engine, n):
    """8, 16, 32 and 64 lanes per line; more pools than a wave has lanes; every seventh line a pool short or long (dropped)"""
    from poolgen_amd import pileup_parse_host
    from test_pileup import _random_line
    rng = random.Random(100 + n)
    lines = [_random_line(rng, n + (0 if i % 7 else rng.choice([-1, 1, 70])), False) for i in range(41)]
    text = ("\n".join(lines) + "\n").encode("latin-1")
    sizes = [rng.randint(5, 60) for _ in range(n)]
    sizes = [s / sum(sizes) for s in sizes]
    rule = dict(remove_ns=True, keep_lowercase_reference=False, max_base_error_rate=0.01, min_coverage_depth=1, min_coverage_breadth=0.75,
                min_allele_frequency=0.02)
    want = R.parse_ref(text, sizes, **rule)
    assert want["error"] is None and 0 < len(want["pos"]) < 41
    same(pileup_parse_host(text, sizes, **rule, n_threads=8), want, n)
    same(as_numpy(engine.pileup_parse(text, sizes, **rule)), want, n)


def test_more_than_4096_pool_sizes_are_refused(engine):
    from poolgen_amd import NativeError
    with pytest.raises(NativeError, match="4096"):
        engine.pileup_parse(b"c1\t5\tA\t1\t.\tI\n", [1.0 / 4097] * 4097)
    text = b"c1\t5\tA" + b"\t1\tT\tI\t1\t.\tI" * 2048 + b"\n"                 # 4096 pools: one line per workgroup
    want = R.parse_ref(text, [1.0 / 4096] * 4096)
    assert len(want["pos"]) == 1
    same(as_numpy(engine.pileup_parse(text, [1.0 / 4096] * 4096)), want, 4096)


def short_pool_text(lines):
    """`lines` lines of one short pool whose answer is known by construction: i % 4 reads of T among i % 3 + i % 4 reads"""
    i = np.arange(lines)
    a, t = i % 3, i % 4
    text = "".join(f"c{k % 3}\t{k + 1}\tA\t{x + y}\t{'.' * x + 'T' * y}\t{'I' * (x + y)}\n" if x + y else f"c{k % 3}\t{k + 1}\tA\t0\t*\t*\n"
                   for k, x, y in zip(i.tolist(), a.tolist(), t.tolist()))
    keep = (a + t) >= 1
    counts = np.zeros((int(keep.sum()), 1, 6), dtype=np.uint32)
    counts[:, 0, 0] = a[keep]
    counts[:, 0, 1] = t[keep]
    return text.encode(), counts, (i[keep] + 1).astype(np.uint64)


@pytest.mark.parametrize("lines", [1, 255, 256, 257, 256 * 1024 + 1])
def test_line_counts_at_the_scan_levels(engine, lines):
    """one workgroup of the keep scan, its edge, and more than 1024 workgroups (the second round of the 64-bit scan)"""
    from poolgen_amd import pileup_parse_host
    text, counts, pos = short_pool_text(lines if lines > 1 else 2)
    if lines == 1:
        text, counts, pos = text[text.index(b"\n") + 1:], counts[:1], pos[:1]
    rule = dict(pileup_corpus.BASE)
    want = pileup_parse_host(text, [1.0], **rule, n_threads=8)
    assert np.array_equal(want["counts"], counts) and np.array_equal(want["pos"], pos) and want["lines"] == lines
    if lines <= 257:
        same(want, R.parse_ref(text, [1.0], **rule), lines)
    same(as_numpy(engine.pileup_parse(text, [1.0], **rule)), want, lines)
    same(as_numpy(engine.pileup_parse(text[:-1], [1.0], **rule)), want, (lines, "no final newline"))


@pytest.mark.parametrize("reads", [1, 63, 64, 65, 4096, 70000])
def test_one_pool_with_many_reads(engine, reads):
    """a count above 65 535; indels, read starts and low qualities in between"""
    from poolgen_amd import pileup_parse_host
    rng = random.Random(reads)
    codes, quals = ["T"], ["I"]
    for _ in range(reads - 1):
        codes.append("." if rng.random() < 0.97 else rng.choice(["T", ",", "c", "^].", "G$", "a+2GG", "*", ".-11ACGTACGTACG", "N", "t"]))
        quals.append("I" if rng.random() < 0.97 else rng.choice("5J#"))
    rule = dict(pileup_corpus.BASE)
    text = b"".join(f"chrX\t{7 + k}\t{ref}\t{reads}\t{''.join(codes)}\t{''.join(quals)}\n".encode() for k, ref in enumerate("TAg"))
    want = R.parse_ref(text, [1.0], **rule)
    assert want["error"] is None and len(want["pos"]) == 3 and (reads < 70000 or want["counts"].max() > 65535)
    same(pileup_parse_host(text, [1.0], **rule, n_threads=3), want, reads)
    same(as_numpy(engine.pileup_parse(text, [1.0], **rule)), want, reads)


def test_all_16_alignments_of_the_text(engine):
    sizes, rule, _, _, text, want = pileup_corpus.generated(1)
    text = text[:R.text_lines(text)[200][0]]
    want = R.parse_ref(text, sizes, **rule)
    for a in range(16):
        dev = torch.frombuffer(bytearray(b"\n" * (16 + a) + text), dtype=torch.uint8).cuda()[16 + a:]
        assert dev.data_ptr() % 16 == a
        same(as_numpy(engine.pileup_parse(dev, sizes, **rule)), want, a)
        same(as_numpy(engine.pileup_parse(dev[:-1], sizes, **rule)), want, (a, "no final newline"))


def test_result_does_not_depend_on_the_slab_cut(engine):
    """one slab; slabs of 1 line, of 7 lines and of 4 KB cut at line starts (slices of one device tensor, so of every alignment)"""
    sizes, rule, _, _, text, want = pileup_corpus.generated(2)
    whole = as_numpy(engine.pileup_parse(text, sizes, **rule))
    same(whole, want, "whole")
    dev = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    starts = [o for o, _ in R.text_lines(text)] + [len(text)]
    by_4k, last = [0], 0
    for s in starts:
        if s - by_4k[-1] > 4096:
            by_4k.append(last)
        last = s
    for cuts in (starts[:60] + [len(text)], starts[::7] + [len(text)], by_4k + [len(text)]):
        parts = [(a, as_numpy(engine.pileup_parse(dev[a:z], sizes, **rule))) for a, z in zip(cuts[:-1], cuts[1:]) if z > a]
        got = {k: np.concatenate([p[k] + (a if k == "line_off" else 0) for a, p in parts]) for k in ARRAYS}
        for k in ARRAYS:
            assert np.array_equal(got[k], whole[k]), (k, len(cuts))
        assert sum(p["lines"] for _, p in parts) == whole["lines"]


def test_nothing_is_written_behind_the_capacities(engine):
    from poolgen_amd._native import PgPileupInfo
    lib, ctx = engine._lib, engine._ctx
    sizes, rule, _, _, text, want = pileup_corpus.generated(0)
    k, n = len(want["pos"]), len(sizes)
    dev = torch.frombuffer(bytearray(b"abc" + text), dtype=torch.uint8).cuda()[3:]   # not 16-byte aligned
    ps = np.asarray(sizes, dtype=np.float64)
    info = PgPileupInfo()
    pad = 64
    bufs = [torch.full((k * n * 6 + pad,), 0x2B2B2B2B, dtype=torch.int32, device="cuda"), torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int64, device="cuda"),
            torch.full((k + pad,), 0x2B, dtype=torch.uint8, device="cuda"), torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int64, device="cuda"),
            torch.full((k + pad,), 0x2B2B2B2B, dtype=torch.int32, device="cuda")]
    clean = [x.clone() for x in bufs]

    def call(cap_loci, cap_counts):
        rc = lib.pg_pileup_parse_dev(ctx, dev.data_ptr(), dev.numel(), ps.ctypes.data, n, int(rule["remove_ns"]), int(rule["keep_lowercase_reference"]),
                                     rule["max_base_error_rate"], rule["min_coverage_depth"], rule["min_coverage_breadth"], rule["min_allele_frequency"],
                                     *[x.data_ptr() for x in bufs], cap_loci, cap_counts, C.byref(info))
        engine.synchronize()
        return rc
    assert call(0, 0) == -1 and (info.kept, info.lines, info.err_reason) == (k, want["lines"], 0)     # the size query
    assert call(k - 1, k * n * 6) == -1 and call(k, k * n * 6 - 1) == -1
    assert all(torch.equal(x, c) for x, c in zip(bufs, clean))                    # too small: nothing written
    assert call(k, k * n * 6) == 0
    assert np.array_equal(bufs[0][:k * n * 6].cpu().numpy().view(np.uint32).reshape(k, n, 6), want["counts"])
    assert np.array_equal(bufs[1][:k].cpu().numpy().view(np.uint64), want["pos"])
    assert np.array_equal(bufs[2][:k].cpu().numpy(), want["ref"])
    assert np.array_equal(bufs[3][:k].cpu().numpy(), want["line_off"]) and np.array_equal(bufs[4][:k].cpu().numpy(), want["chrom_len"])
    assert torch.equal(bufs[0][k * n * 6:], clean[0][k * n * 6:]) and all(torch.equal(x[k:], c[k:]) for x, c in zip(bufs[1:], clean[1:]))


def test_error_texts_fail_with_the_first_bad_line_and_leave_the_engine_usable(engine):
    from poolgen_amd.engine import PileupError
    sizes, rule, _, _, text, want = pileup_corpus.generated(0)
    for name, (etext, esizes, erule, off, reason) in pileup_corpus.error_texts().items():
        with pytest.raises(PileupError) as e:
            engine.pileup_parse(etext, esizes, **erule)
        assert (e.value.offset, e.value.reason) == (off, reason), name
        assert f"byte {off} " in engine._lib.pg_last_error(engine._ctx).decode(), name     # the message names the line
    same(as_numpy(engine.pileup_parse(text, sizes, **rule)), want, "after the errors")
    assert engine.pileup_parse(b"", [1.0])["lines"] == 0
