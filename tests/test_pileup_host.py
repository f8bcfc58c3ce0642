"""pg_host_pileup_parse, the plain C++ twin of the device pileup parser, against the literal restatement (tests/pileup_ref.py):
every array and the info block exactly.  Runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

import pileup_corpus
import pileup_ref as R

ARRAYS = ("counts", "pos", "ref", "line_off", "chrom_len")
SCALARS = ("lines", "n_pools")
THREADS = (1, 3, 8)


def same(got, want, what):
    for k in SCALARS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in ARRAYS:
        g = np.asarray(got[k])
        assert g.dtype == want[k].dtype and g.shape == want[k].shape, (what, k, g.dtype, g.shape, want[k].shape)
        assert np.array_equal(g, want[k]), (what, k)


@pytest.fixture(scope="module")
def cases():
    """(name, text, sizes, rule, the restatement's result), computed once"""
    return [c + (R.parse_ref(c[1], c[2], **c[3]),) for c in pileup_corpus.texts()]


@pytest.mark.parametrize("threads", THREADS)
def test_host_twin_equals_restatement_on_the_corpus(native, cases, threads):
    from poolgen_amd import pileup_parse_host
    for name, text, sizes, rule, want in cases:
        same(pileup_parse_host(text, sizes, **rule, n_threads=threads), want, name)


@pytest.mark.parametrize("k", range(len(pileup_corpus.FILTER_SETS)))
def test_host_twin_equals_restatement_on_generated_lines(native, k):
    """1 500 lines of test_pileup's generator per filter set: the lines that are no error as one text, every fatal line on its own
    behind sound ones"""
    from poolgen_amd import pileup_parse_host
    from poolgen_amd.engine import PileupError
    sizes, rule, lines, outcomes, text, want = pileup_corpus.generated(k)
    assert want["error"] is None and 20 < len(want["pos"]) < want["lines"]
    for threads in THREADS:
        same(pileup_parse_host(text, sizes, **rule, n_threads=threads), want, (k, threads))
    head = text[:R.text_lines(text)[5][0]]
    for line, o in zip(lines, outcomes):
        if o[0] == "E":
            with pytest.raises(PileupError) as e:
                pileup_parse_host(head + line + b"\n" + head, sizes, **rule, n_threads=2)
            assert (e.value.offset, e.value.reason) == (len(head), o[1]), line


def test_host_twin_takes_numpy_and_unaligned_text(native, cases):
    from poolgen_amd import pileup_parse_host
    name, text, sizes, rule, want = cases[0]
    buf = np.frombuffer(b"xyz" + text, dtype=np.uint8)[3:]
    same(pileup_parse_host(buf, sizes, **rule, n_threads=4), want, name)
    empty = pileup_parse_host(b"", sizes, **rule)
    assert empty["lines"] == 0 and empty["counts"].shape == (0, len(sizes), 6)


def test_error_texts_fail_with_the_first_bad_line(native):
    from poolgen_amd import pileup_parse_host
    from poolgen_amd.engine import PileupError
    for name, (text, sizes, rule, off, reason) in pileup_corpus.error_texts().items():
        for threads in THREADS:
            with pytest.raises(PileupError) as e:
                pileup_parse_host(text, sizes, **rule, n_threads=threads)
            assert (e.value.offset, e.value.reason) == (off, reason), (name, threads)


def raw_args(text, sizes, rule):
    t = np.frombuffer(text, dtype=np.uint8)
    ps = np.asarray(sizes, dtype=np.float64)
    return t, ps, [t.ctypes.data, t.size, ps.ctypes.data, len(ps), int(rule["remove_ns"]), int(rule["keep_lowercase_reference"]),
                   rule["max_base_error_rate"], rule["min_coverage_depth"], rule["min_coverage_breadth"], rule["min_allele_frequency"]]


def test_status_code_and_info_block(native):
    """the C ABI itself: PG_ERR_INVALID, the info block, nothing written; more than 4096 pool sizes refused"""
    from poolgen_amd._native import PgPileupInfo
    errs = pileup_corpus.error_texts()
    for name in ("e_position", "e_indel", "e2_mismatch_then_coverage", "e_empty_line"):
        text, sizes, rule, off, reason = errs[name]
        t, ps, args = raw_args(text, sizes, rule)
        info = PgPileupInfo()
        pos = np.full(8, 77, dtype=np.uint64)
        rc = native.pg_host_pileup_parse(*args, None, pos.ctypes.data, None, None, None, 8, 0, C.byref(info), 2)
        assert rc == -1 and (info.err_line_off, info.err_reason, info.kept, info.lines) == (off, reason, 0, len(R.text_lines(text))), name
        assert (pos == 77).all()
    text, sizes, rule, _, _ = errs["e_position"]
    t, ps, args = raw_args(text, [1.0 / 4097] * 4097, rule)
    info = PgPileupInfo()
    assert native.pg_host_pileup_parse(*args, None, None, None, None, None, 0, 0, C.byref(info), 1) == -1 and info.err_reason == 0


def test_capacities_are_respected(native, cases):
    """a size query first; a buffer one row short fails and writes nothing; the exact size succeeds and leaves the bytes behind it alone"""
    from poolgen_amd._native import PgPileupInfo
    name, text, sizes, rule, want = [c for c in cases if c[0] == "no_final_newline"][0]
    t, ps, args = raw_args(text, sizes, rule)
    k, n = len(want["pos"]), len(sizes)
    assert k > 1
    info = PgPileupInfo()

    def call(cap_loci, cap_counts, bufs):
        return native.pg_host_pileup_parse(*args, *[x.ctypes.data for x in bufs], cap_loci, cap_counts, C.byref(info), 3)
    pad = 5
    bufs = [np.full(k * n * 6 + pad, 0xAB, dtype=np.uint32), np.full(k + pad, 0xAB, dtype=np.uint64), np.full(k + pad, 0xAB, dtype=np.uint8),
            np.full(k + pad, 0xAB, dtype=np.int64), np.full(k + pad, 0xAB, dtype=np.int32)]
    assert call(0, 0, bufs) == -1 and (info.kept, info.lines, info.err_reason) == (k, want["lines"], 0)
    assert call(k - 1, k * n * 6, bufs) == -1 and call(k, k * n * 6 - 1, bufs) == -1
    assert all((x == 0xAB).all() for x in bufs)
    assert call(k, k * n * 6, bufs) == 0
    assert np.array_equal(bufs[0][:k * n * 6].reshape(k, n, 6), want["counts"]) and np.array_equal(bufs[1][:k], want["pos"])
    assert np.array_equal(bufs[2][:k], want["ref"]) and np.array_equal(bufs[3][:k], want["line_off"]) and np.array_equal(bufs[4][:k], want["chrom_len"])
    assert (bufs[0][k * n * 6:] == 0xAB).all() and all((x[k:] == 0xAB).all() for x in bufs[1:])


def test_result_does_not_depend_on_the_slab_cut(native):
    from poolgen_amd import pileup_parse_host
    sizes, rule, _, _, text, want = pileup_corpus.generated(0)
    starts = [o for o, _ in R.text_lines(text)] + [len(text)]
    cuts = starts[::7] + [len(text)]
    parts = [pileup_parse_host(text[a:z], sizes, **rule, n_threads=2) for a, z in zip(cuts[:-1], cuts[1:]) if z > a]
    assert np.array_equal(np.concatenate([p["counts"] for p in parts]), want["counts"])
    assert np.array_equal(np.concatenate([p["line_off"] + a for p, a in zip(parts, cuts)]), want["line_off"])
    assert sum(p["lines"] for p in parts) == want["lines"]
