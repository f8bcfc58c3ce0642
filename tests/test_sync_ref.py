"""pg_host_sync_parse, the plain C++ twin of the device sync parser, against the literal restatement (tests/sync_ref.py) and
against the CLI's own host parser as `hostcheck parse` prints it: the fixture, the corpus, the error texts, the capacities and
the slab cuts.  No GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import sync_corpus
import sync_ref as R

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden"
HOSTCHECK = ROOT / "poolgen_amd" / "csrc" / "hostcheck"
ARRAYS = ("counts", "pos", "line_off", "chrom_len")
SCALARS = ("data_lines", "n_pools")


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
def good(fixture_text):
    """(name, text, expect_n, restatement) of the fixture and every text of the corpus that parses"""
    cases = [("fixture", fixture_text, 0), ("fixture_expect_5", fixture_text, 5)] + [(k, t, n) for k, (t, n) in sync_corpus.corpus().items()]
    return [(name, text, n, R.parse_ref(text, n)) for name, text, n in cases]


def hostcheck_parse(tmp_path, text, threads):
    f = tmp_path / "t.sync"
    f.write_bytes(text)
    return subprocess.run([str(HOSTCHECK), "parse", str(f), str(threads)], capture_output=True)


def test_the_corpus_holds_what_it_says(good):
    by = {name: want for name, _, _, want in good}
    assert by["fixture"]["counts"].shape == (6674, 5, 6)
    assert by["bad_positions_are_skipped"]["pos"].tolist() == [1, 5, 9999999999999999999, 2]      # "+5" is a number, as in the CLI's parser
    assert by["first_line_bad_position_fixes_the_pools"]["pos"].tolist() == [6, 7]
    assert by["count_widths"]["counts"][0, 0].tolist() == [0, 9, 10, 65535, 65536, 4294967295]
    assert by["seven_and_eight_counts"]["counts"][:, 0].tolist() == [[1, 2, 3, 4, 5, 6]] * 2
    assert by["only_comments"]["n_pools"] == 0 and by["only_skipped_lines"]["n_pools"] == 2 and len(by["only_skipped_lines"]["pos"]) == 0
    for name, (text, n, off, reason) in sync_corpus.error_texts().items():
        with pytest.raises(R.SyncPanic) as e:
            R.parse_ref(text, n)
        assert (e.value.offset, e.value.reason) == (off, reason), name


@pytest.mark.parametrize("threads", [1, 16])
def test_host_twin_equals_the_restatement(native, good, threads):
    from poolgen_amd import sync_parse_host
    for name, text, n, want in good:
        same(sync_parse_host(text, n, n_threads=threads), want, name)
    same(sync_parse_host(bytearray(good[0][1]), 0, n_threads=threads), good[0][3], "bytearray")
    assert sync_parse_host(b"", 0, n_threads=threads)["data_lines"] == 0


@pytest.mark.parametrize("threads", [1, 16])
def test_host_twin_equals_the_cli_parser(native, good, tmp_path, threads):
    """what `hostcheck parse` prints (parse_sync_file: chromosome, position, counts) is what pg_host_sync_parse returns"""
    from poolgen_amd import sync_parse_host
    for name, text, n, _ in good:
        if n:
            continue                                                    # parse_sync_file takes the pool count from the file
        r = hostcheck_parse(tmp_path, text, threads)
        assert r.returncode == 0, (name, r.stderr)
        assert r.stdout == R.hostcheck_form(text, sync_parse_host(text, 0, n_threads=threads)).encode("latin-1"), name


@pytest.mark.parametrize("threads", [1, 16])
def test_error_texts_fail_where_the_cli_parser_fails(native, tmp_path, threads):
    from poolgen_amd import sync_parse_host
    from poolgen_amd.engine import SyncError
    for name, (text, n, off, reason) in sync_corpus.error_texts().items():
        with pytest.raises(SyncError) as e:
            sync_parse_host(text, n, n_threads=threads)
        assert (e.value.offset, e.value.reason) == (off, reason), name
        assert f"byte {off} " in str(e.value), name
        if n == 0:
            assert hostcheck_parse(tmp_path, text, threads).returncode != 0, name


def test_many_threads_on_a_larger_text(native):
    """shares that end inside lines, comment lines at share edges"""
    from poolgen_amd import sync_parse_host
    from poolgen_amd.engine import SyncError
    rng = np.random.default_rng(3)
    text, counts = sync_corpus.random_text(rng, 9, 700, comment_every=13)
    for threads in (1, 3, 16):
        r = sync_parse_host(text, 0, n_threads=threads)
        assert np.array_equal(r["counts"], counts) and r["data_lines"] == 700
        assert np.array_equal(r["pos"], 1000 + 7 * np.arange(700, dtype=np.uint64))
    bad = text + b"chr\t1\tA\t1:2:3\n"
    for threads in (1, 16):
        with pytest.raises(SyncError) as e:
            sync_parse_host(bad, 0, n_threads=threads)
        assert (e.value.offset, e.value.reason) == (len(text), R.E_COUNT)     # a line with another pool count and a bad count


def test_status_code_and_nothing_written(native):
    """the C ABI itself: PG_ERR_INVALID, the info block, and nothing written"""
    from poolgen_amd._native import PgSyncInfo
    for name in ("count_above_u32", "one_pool_more", "empty_line", "expect_n_wrong"):
        text, n, off, reason = sync_corpus.error_texts()[name]
        t = np.frombuffer(text, dtype=np.uint8)
        info = PgSyncInfo()
        pos = np.full(8, 77, dtype=np.uint64)
        rc = native.pg_host_sync_parse(t.ctypes.data, t.size, n, None, pos.ctypes.data, None, None, 8, 0, C.byref(info), 2)
        assert rc == -1 and (info.err_line_off, info.err_reason, info.kept, info.n_pools) == (off, reason, 0, 0), name
        assert (pos == 77).all()
    info = PgSyncInfo()
    assert native.pg_host_sync_parse(None, 0, 4097, None, None, None, None, 0, 0, C.byref(info), 1) == -1      # more than 4096 pools


def test_capacities_are_respected(native, good):
    """a size query first; a buffer one element short fails and writes nothing; the exact size succeeds and leaves the bytes behind it alone"""
    from poolgen_amd._native import PgSyncInfo
    name, text, n0, want = good[0]
    t = np.frombuffer(text, dtype=np.uint8)
    k, n = len(want["pos"]), want["n_pools"]
    info = PgSyncInfo()

    def call(cap_loci, cap_counts, bufs):
        return native.pg_host_sync_parse(t.ctypes.data, t.size, 0, *[x.ctypes.data for x in bufs], cap_loci, cap_counts, C.byref(info), 3)
    pad = 5
    bufs = [np.full(k * n * 6 + pad, 0xAB, dtype=np.uint32), np.full(k + pad, 0xAB, dtype=np.uint64), np.full(k + pad, 0xAB, dtype=np.int64),
            np.full(k + pad, 0xAB, dtype=np.int32)]
    assert call(0, 0, bufs) == -1 and (info.kept, info.n_pools) == (k, n)
    assert call(k - 1, k * n * 6, bufs) == -1 and call(k, k * n * 6 - 1, bufs) == -1
    assert all((x == 0xAB).all() for x in bufs)
    assert call(k, k * n * 6, bufs) == 0
    assert np.array_equal(bufs[0][:k * n * 6].reshape(k, n, 6), want["counts"]) and np.array_equal(bufs[1][:k], want["pos"])
    assert (bufs[0][k * n * 6:] == 0xAB).all() and all((x[k:] == 0xAB).all() for x in bufs[1:])


def test_result_does_not_depend_on_the_slab_cut(native, good):
    from poolgen_amd import sync_parse_host
    name, text, n0, want = good[0]
    starts = [o for o, _ in R.text_lines(text)] + [len(text)]
    for cuts in (starts[::7] + [len(text)], starts[:40] + [len(text)]):
        for expect in (0, 5):
            parts = [(a, sync_parse_host(text[a:z], expect, n_threads=2)) for a, z in zip(cuts[:-1], cuts[1:]) if z > a]
            assert {p["n_pools"] for _, p in parts} <= {0, 5}                  # 0: a slab of comment lines
            for k in ARRAYS:
                assert np.array_equal(np.concatenate([p[k] + (a if k == "line_off" else 0) for a, p in parts if p["n_pools"]]), want[k]), k
            assert sum(p["data_lines"] for _, p in parts) == want["data_lines"]
