"""pg_host_vcf_parse, the plain C++ twin of the device VCF parser, against the literal restatement (tests/vcf_ref.py): every
array exactly.  Runs without a GPU."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

import vcf_corpus
import vcf_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden"
ARRAYS = ("counts", "pos", "ref", "line_off", "chrom_len")
SCALARS = ("data_lines", "n_pools", "chrom_line_off")


def same(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        g = np.asarray(got[k])
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (what, k)


@pytest.fixture(scope="module")
def cases():
    """(name, text, sizes, depth, breadth, maf, the restatement's result), computed once"""
    fx = (GOLDEN / "test.vcf").read_bytes()
    out = [(f"fixture_{d}_{b}_{f}", fx, [0.1] * 10, d, b, f) for d, b, f in [(1, 1.0, 0.001), (1, 1.0, 0.0), (10, 1.0, 0.0), (5, 0.5, 0.05)]]
    out += vcf_corpus.corpus()
    return [c + (R.parse_ref(*c[1:]),) for c in out]


@pytest.mark.parametrize("threads", [1, 16])
def test_host_twin_equals_restatement(native, cases, threads):
    from poolgen_amd import vcf_parse_host
    for name, text, sizes, d, b, f, want in cases:
        same(vcf_parse_host(text, sizes, d, b, f, n_threads=threads), want, name)


def test_host_twin_takes_numpy_and_unaligned_text(native, cases):
    from poolgen_amd import vcf_parse_host
    name, text, sizes, d, b, f, want = cases[0]
    buf = np.frombuffer(b"xyz" + text, dtype=np.uint8)[3:]
    same(vcf_parse_host(buf, sizes, d, b, f, n_threads=4), want, name)


def test_error_texts_fail_with_the_first_bad_line(native):
    from poolgen_amd import vcf_parse_host
    from poolgen_amd.engine import VcfError
    for name, (text, sizes, d, b, f, off, reason) in vcf_corpus.error_texts().items():
        for threads in (1, 16):
            with pytest.raises(VcfError) as e:
                vcf_parse_host(text, sizes, d, b, f, n_threads=threads)
            assert (e.value.offset, e.value.reason) == (off, reason), (name, threads)
    text, sizes, d, b, f = vcf_corpus.dropped_not_errors()
    same(vcf_parse_host(text, sizes, d, b, f), R.parse_ref(text, sizes, d, b, f), "dropped_not_errors")   # the breadth rule comes first


def test_status_code_and_deviations(native):
    """the C ABI itself: PG_ERR_INVALID, the info block, and nothing written"""
    from poolgen_amd._native import PgVcfInfo
    errs = vcf_corpus.error_texts()
    for name in ("count_above_u32", "high_byte_ref", "high_byte_alt", "pos_letters"):
        text, sizes, d, b, f, off, reason = errs[name]
        t = np.frombuffer(text, dtype=np.uint8)
        ps = np.asarray(sizes, dtype=np.float64)
        info = PgVcfInfo()
        pos = np.full(8, 77, dtype=np.uint64)
        rc = native.pg_host_vcf_parse(t.ctypes.data, t.size, ps.ctypes.data, len(ps), d, b, f, None, pos.ctypes.data, None, None, None, 8, 0, C.byref(info), 2)
        assert rc == -1 and (info.err_line_off, info.err_reason, info.kept, info.n_pools) == (off, reason, 0, 0), name
        assert (pos == 77).all()


def test_capacities_are_respected(native, cases):
    """a size query first; a buffer one row short fails and writes nothing; the exact size succeeds and leaves the bytes behind it alone"""
    from poolgen_amd._native import PgVcfInfo
    name, text, sizes, d, b, f, want = cases[0]
    t = np.frombuffer(text, dtype=np.uint8); ps = np.asarray(sizes, dtype=np.float64)
    k, n = len(want["pos"]), want["n_pools"]
    info = PgVcfInfo()

    def call(cap_loci, cap_counts, bufs):
        return native.pg_host_vcf_parse(t.ctypes.data, t.size, ps.ctypes.data, len(ps), d, b, f, *[x.ctypes.data for x in bufs], cap_loci, cap_counts,
                                        C.byref(info), 3)
    pad = 5
    bufs = [np.full(k * n * 6 + pad, 0xAB, dtype=np.uint32), np.full(k + pad, 0xAB, dtype=np.uint64), np.full(k + pad, 0xAB, dtype=np.uint8),
            np.full(k + pad, 0xAB, dtype=np.int64), np.full(k + pad, 0xAB, dtype=np.int32)]
    assert call(0, 0, bufs) == -1 and (info.kept, info.n_pools) == (k, n)
    assert call(k - 1, k * n * 6, bufs) == -1 and call(k, k * n * 6 - 1, bufs) == -1
    assert all((x == 0xAB).all() for x in bufs)
    assert call(k, k * n * 6, bufs) == 0
    assert np.array_equal(bufs[0][:k * n * 6].reshape(k, n, 6), want["counts"]) and np.array_equal(bufs[1][:k], want["pos"])
    assert (bufs[0][k * n * 6:] == 0xAB).all() and all((x[k:] == 0xAB).all() for x in bufs[1:])


def test_result_does_not_depend_on_the_slab_cut(native, cases):
    from poolgen_amd import vcf_parse_host
    name, text, sizes, d, b, f, want = cases[0]
    starts = [o for o, _ in R.text_lines(text)] + [len(text)]
    cuts = starts[::7] + [len(text)]
    parts = [vcf_parse_host(text[a:z], sizes, d, b, f, n_threads=2) for a, z in zip(cuts[:-1], cuts[1:]) if z > a]
    assert np.array_equal(np.concatenate([p["counts"] for p in parts if p["n_pools"]]), want["counts"])
    assert np.array_equal(np.concatenate([p["line_off"] + a for p, a in zip(parts, cuts)]), want["line_off"])
    assert sum(p["data_lines"] for p in parts) == want["data_lines"]
