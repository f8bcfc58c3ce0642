"""pg_f64_text_dev: the number text of the result writer formatted on the GPU (pg_resultfmt.hip over pg_f64_text.h).  The bytes
equal the host twin's -- the same source compiled for the host, itself checked against Rust's rule in tests/test_f64_text_host.py --
on the whole corpus, at counts around a wave and a workgroup's tile, at every alignment of the output; for roundup_own the device's
multiply, round and divide must give the host's bits, which the half-way members of the corpus decide."""
import ctypes as C

import numpy as np
import pytest
import torch

import f64_corpus as FC

pytestmark = pytest.mark.gpu
PG_OK, PG_ERR_INVALID = 0, -1
TILE = 16384                         # RF_TILE of pg_resultfmt.hip: the bytes a workgroup stages


def host_text(x, nd=-1):
    from poolgen_amd import f64_text_host
    return f64_text_host(x, nd, 8)


def dev_text(engine, x, nd=-1, **kw):
    t = torch.from_numpy(np.array(x, dtype=np.float64)).cuda()
    return engine.f64_text(t, nd, **kw).cpu().numpy().tobytes()


def first_difference(got: bytes, want: bytes, x):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "value %r (bits %016x): device %r, host %r" % (float(x[i]), FC.to_bits(float(x[i])), a, b)
    return "lengths %d / %d" % (len(g), len(w))


@pytest.mark.parametrize("nd", (-1,) + FC.NDS)
def test_corpus_equals_host_twin(engine, nd):
    x = FC.corpus()
    got, want = dev_text(engine, x, nd), host_text(x, nd)
    assert got == want, first_difference(got, want, x)
    if nd in (-1, 6):
        assert want == FC.expected(nd)                                  # (and the host twin is Rust's text: checked here once more, cheaply)


def test_halves_round_like_the_host(engine):
    """x * 10^nd, the rounding and the division on the device give the host's bits: every half-way member and its neighbours"""
    rng = np.random.default_rng(8)
    for nd in FC.NDS:
        x = np.array(FC.halfway(nd, rng))
        assert dev_text(engine, x, nd) == host_text(x, nd) == ("\n".join(FC.roundup_own(v, nd) for v in x.tolist()) + "\n").encode(), nd


def test_counts_around_a_wave_and_a_tile(engine):
    x = FC.sample(4000, 3)
    x[::7] = 1e-300                                                      # long cells: fewer values per tile, a ragged last workgroup
    lens = np.array([len(l) + 1 for l in host_text(x).split(b"\n")[:-1]])
    upb = TILE // int(lens.max())                                        # values a workgroup takes when the longest one is in the call
    assert upb < 64
    short = np.round(np.random.default_rng(4).random(5000), 3)           # at most 6 bytes a line: 16384 // 6 values per workgroup, 256 lanes looping
    for vals, counts in ((x, [1, 63, 64, 65, upb - 1, upb, upb + 1, 2 * upb, 255, 256, 257, 4000]), (short, [1, 64, 2729, 2730, 2731, 2732, 5000])):
        for count in counts:
            got, want = dev_text(engine, vals[:count]), host_text(vals[:count])
            assert got == want, (count, first_difference(got, want, vals))


def test_every_alignment_exact_capacity_and_canary(engine):
    x = FC.sample(1500, 6)
    want = host_text(x, 8)
    xd = torch.from_numpy(x).cuda()
    for off in range(16):
        buf = torch.full((len(want) + 48,), 0xAA, dtype=torch.uint8, device="cuda")
        view = buf[off:off + len(want)]                                  # exactly the capacity the text needs
        out = engine.f64_text(xd, 8, out=view)
        assert out.numel() == len(want)
        b = buf.cpu().numpy()
        assert b[off:off + len(want)].tobytes() == want and (b[:off] == 0xAA).all() and (b[off + len(want):] == 0xAA).all(), off


def test_size_query_refusals_and_a_usable_context_afterwards(engine):
    from poolgen_amd import NativeError
    lib, ctx = engine._lib, engine._ctx
    x = FC.sample(700, 7)
    want = host_text(x, 6)
    xd = torch.from_numpy(x).cuda()
    need = C.c_int64(-7)
    assert lib.pg_f64_text_dev(ctx, xd.data_ptr(), xd.numel(), 6, None, 0, C.byref(need)) == PG_ERR_INVALID and need.value == len(want)
    buf = torch.full((len(want) + 16,), 0xAA, dtype=torch.uint8, device="cuda")
    assert lib.pg_f64_text_dev(ctx, xd.data_ptr(), xd.numel(), 6, buf.data_ptr(), len(want) - 1, C.byref(need)) == PG_ERR_INVALID
    assert need.value == len(want) and bool((buf == 0xAA).all())          # one short: the size, nothing written
    assert lib.pg_f64_text_dev(ctx, xd.data_ptr(), 0, 6, buf.data_ptr(), buf.numel(), C.byref(need)) == PG_OK and need.value == 0
    for count, nd, cap, ptr in ((-1, 6, 8, buf.data_ptr()), (5, 23, 8, buf.data_ptr()), (5, 6, -1, buf.data_ptr()), (5, 6, 8, None)):
        assert lib.pg_f64_text_dev(ctx, xd.data_ptr(), count, nd, ptr, cap, C.byref(need)) == PG_ERR_INVALID and need.value == 0
    assert lib.pg_f64_text_dev(ctx, None, 5, 6, buf.data_ptr(), buf.numel(), C.byref(need)) == PG_ERR_INVALID and need.value == 0
    assert bool((buf == 0xAA).all())
    with pytest.raises(NativeError):
        engine.f64_text(xd, 23)
    assert dev_text(engine, x, 6) == want                                # the next call gives the same bytes
