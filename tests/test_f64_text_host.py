"""pg_host_f64_text, the host side of the number text of the result writer (pg_f64_text.h: the same source the device compiles):
against tests/rustfmt.py -- Rust's `{}` and parse_f64_roundup_and_own -- on the seeded corpus of tests/f64_corpus.py, against
hand-written literals, and against `hostcheck fmt`, today's host formatter (std::to_chars), with which it must agree below 2^53
and from which it is pinned to differ above.  Runs without a GPU."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

import f64_corpus as FC
import rustfmt

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "poolgen_amd" / "csrc"
PG_OK, PG_ERR_INVALID = 0, -1


def host_text(x, nd=-1, n_threads=4):
    from poolgen_amd import f64_text_host
    return f64_text_host(x, nd, n_threads)


def first_difference(got: bytes, want: bytes, x):
    g, w = got.split(b"\n"), want.split(b"\n")
    for i, (a, b) in enumerate(zip(g, w)):
        if a != b:
            return "value %r (bits %016x): got %r, want %r" % (float(x[i]), FC.to_bits(float(x[i])), a, b)
    return "lengths %d / %d" % (len(g), len(w))


def test_the_corpus_holds_what_it_promises():
    c = FC.corpus()
    assert len(c) >= 250_000
    lens = {len(s) for s in FC.displayed()}
    assert min(lens) == 1 and max(lens) == FC.MAX_LEN
    assert set(range(1, 60)) <= lens                                   # every short length, the boundary of every length rule
    assert np.isnan(c).any() and np.isinf(c).any() and (c == 0).any() and (np.abs(c) >= 2.0 ** 54).any()
    for nd in FC.NDS:
        for n in (nd - 1, nd, nd + 1):
            if n >= 1:
                assert any(len(rustfmt.display(v)) == n for v in FC.with_length(n, np.random.default_rng(1), tries=5)), (nd, n)
    for nd in FC.NDS:                                                  # the restatement's one flaw is met, and C's round() settles it
        hit = [v for v in FC.halfway(nd, np.random.default_rng(3)) if abs(v * float("1e%d" % nd)) == FC.HALF_BELOW]
        assert (hit or nd != 0) and all(round(v * float("1e%d" % nd)) == 0 and FC.sensible_round(v, nd) == 0 for v in hit), nd
    f = 1e6
    assert any((v * f) % 1.0 == 0.5 for v in FC.halfway(6, np.random.default_rng(2)))   # exact halves survive the rounded multiply


def test_display_equals_rust_on_the_corpus(native):
    got = host_text(FC.corpus())
    assert got == FC.expected(-1), first_difference(got, FC.expected(-1), FC.corpus())


@pytest.mark.parametrize("nd", FC.NDS)
def test_roundup_own_equals_the_restatement_on_the_corpus(native, nd):
    got = host_text(FC.corpus(), nd)
    assert got == FC.expected(nd), first_difference(got, FC.expected(nd), FC.corpus())


LITERALS = [
    (1e23, b"100000000000000000000000"), (0.5223146158470686, b"0.5223146158470686"), (0.7797774084757156, b"0.7797774084757156"),
    (0.0, b"0"), (-0.0, b"-0"), (float("nan"), b"NaN"), (float("inf"), b"inf"), (float("-inf"), b"-inf"), (1.0, b"1"), (-1.5, b"-1.5"),
    (0.1, b"0.1"), (0.3, b"0.3"), (2.0 / 3.0, b"0.6666666666666666"), (1e-7, b"0.0000001"), (123456.789, b"123456.789"),
    (5e-324, b"0." + b"0" * 323 + b"5"), (1.7976931348623157e308, b"17976931348623157" + b"0" * 292),
    (-2.2250738585072014e-308, b"-0." + b"0" * 307 + b"22250738585072014"), (9007199254740993.0, b"9007199254740992"),
    (9007199254740991.0, b"9007199254740991"), (1e21, b"1" + b"0" * 21), (1e22, b"1" + b"0" * 22), (4.35, b"4.35"), (1e15 + 0.5, b"1000000000000000.5"),
    (2.0 ** 63, b"9223372036854776000"), (2.0 ** 64, b"18446744073709552000"), (1.8e16, b"18000000000000000"),
]
ROUNDED = [  # (x, nd, text)
    (0.123456789, 6, b"0.123457"), (0.1234, 6, b"0.1234"), (0.12345, 7, b"0.12345"), (0.1234565, 6, b"0.123457"), (2.5, 0, b"3"), (-2.5, 0, b"-3"),
    (0.5, 0, b"1"), (-0.4, 0, b"-0"), (0.49999999999999994, 0, b"0"), (1e-9, 6, b"0"), (-1e-9, 6, b"-0"), (123456.7891234, 6, b"123456.789123"),
    (float("nan"), 6, b"NaN"), (float("nan"), 2, b"NaN"), (float("inf"), 2, b"inf"), (float("-inf"), 12, b"-inf"), (1e300, 22, b"inf"),
    (0.000123456789012345, 12, b"0.000123456789"), (0.99999999, 6, b"1"), (12345.0, 6, b"12345"), (123456.0, 6, b"123456"), (1234567.0, 6, b"1234567"),
    (0.3, 22, b"0.3"), (1.005, 2, b"1"), (1.0049999999999999, 2, b"1"), (8.345, 2, b"8.35"),
]


def test_literals(native):
    for x, want in LITERALS:
        assert rustfmt.display(x).encode() == want, x                   # the restatement against the hand-written bytes
        assert host_text([x]) == want + b"\n", x
    for x, nd, want in ROUNDED:
        assert FC.roundup_own(x, nd).encode() == want, (x, nd)
        if abs(x * float("1e%d" % nd)) != FC.HALF_BELOW:                  # (the one product rustfmt.sensible_round gets wrong: f64_corpus.py)
            assert rustfmt.roundup_own(x, nd).encode() == want, (x, nd)
        assert host_text([x], nd) == want + b"\n", (x, nd)
    longest = max(LITERALS, key=lambda t: len(t[1]))
    assert len(longest[1]) == FC.MAX_LEN == 327                          # PG_F64_TEXT_MAX of the public header
    assert "#define PG_F64_TEXT_MAX 327" in (ROOT / "include" / "poolgen_hip.h").read_text()


def hostcheck_fmt(values, nd):
    """today's host formatter: (display, roundup_own(x, nd)) per value"""
    text = "".join("%r %d\n" % (v, nd) for v in values)
    r = subprocess.run([str(CSRC / "hostcheck"), "fmt"], input=text, capture_output=True, text=True, check=True)
    return [tuple(line.split(" ")) for line in r.stdout.splitlines()]


def test_agrees_with_todays_host_formatter_below_2_53_and_differs_above(native):
    c = FC.corpus()
    small = c[~(np.abs(c) >= 2.0 ** 53)]                                 # NaN included
    assert len(small) > len(c) // 2                                        # half of all bit patterns lie below 1
    for nd in (6, 12):
        ours_d = host_text(small).split(b"\n")[:-1]
        ours_r = host_text(small, nd).split(b"\n")[:-1]
        theirs = hostcheck_fmt(small.tolist(), nd)
        assert len(theirs) == len(small)
        for x, a, b, (td, tr) in zip(small.tolist(), ours_d, ours_r, theirs):
            assert a.decode() == td and b.decode() == tr, (x, nd, a, td, b, tr)
    # the finding, kept visible: from about 2^54 on std::to_chars prints the exact integer, Rust (and this formatter) the shortest digits
    (td, _), = hostcheck_fmt([1e23], 6)
    assert td == "99999999999999991611392" and host_text([1e23]) == b"100000000000000000000000\n"
    big = c[np.isfinite(c) & (np.abs(c) >= 2.0 ** 54)][:2000]
    theirs = hostcheck_fmt(big.tolist(), 6)
    ours = host_text(big).split(b"\n")[:-1]
    assert sum(a.decode() != td for a, (td, _) in zip(ours, theirs)) > len(big) // 2
    assert all(float(a) == x for a, x in zip(ours, big.tolist()))         # ours still reads back as the same double


def test_buffer_contract_and_refusals(native):
    x = np.ascontiguousarray(FC.sample(300, 5))
    want = host_text(x, 6, 1)

    def call(buf, cap, count=None, nd=6, threads=2, xs=x):
        need = C.c_int64(-7)
        rc = native.pg_host_f64_text(xs.ctypes.data if xs is not None else None, len(x) if count is None else count, nd,
                                     buf.ctypes.data if buf is not None else None, cap, C.byref(need), threads)
        return rc, need.value

    assert call(None, 0) == (PG_ERR_INVALID, len(want))                  # the size query
    buf = np.full(len(want) + 64, 0xAA, dtype=np.uint8)
    assert call(buf, len(want) - 1) == (PG_ERR_INVALID, len(want)) and (buf == 0xAA).all()    # one short: nothing written
    for cap in (len(want), len(want) + 64):
        buf[:] = 0xAA
        assert call(buf, cap) == (PG_OK, len(want))
        assert buf[:len(want)].tobytes() == want and (buf[len(want):] == 0xAA).all()
    for off in range(16):                                                # any alignment of the text
        b = np.full(len(want) + 32, 0xAA, dtype=np.uint8)
        v = b[off:]
        assert call(v, len(want)) == (PG_OK, len(want)) and v[:len(want)].tobytes() == want and (b[:off] == 0xAA).all() and (v[len(want):] == 0xAA).all()
    for threads in (1, 3, 16):
        assert host_text(x, 6, threads) == want
    buf[:] = 0xAA
    assert call(buf, buf.size, count=0) == (PG_OK, 0) and (buf == 0xAA).all()
    assert call(buf, buf.size, count=-1) == (PG_ERR_INVALID, 0)
    assert call(buf, -1) == (PG_ERR_INVALID, 0)
    assert call(None, 5) == (PG_ERR_INVALID, 0)
    assert call(buf, buf.size, nd=23) == (PG_ERR_INVALID, 0) and (buf == 0xAA).all()
    assert call(buf, buf.size, xs=None) == (PG_ERR_INVALID, 0)
    assert native.pg_host_f64_text(x.ctypes.data, 3, 6, None, 0, None, 1) == PG_ERR_INVALID
    plain = host_text(x, -1)
    big = np.empty(len(plain), dtype=np.uint8)
    assert call(big, big.size, nd=-5) == (PG_OK, len(plain)) and big.tobytes() == plain   # any negative n_digits: display


def test_the_power_table_is_the_generators(native):
    """the committed pg_f64_pow10.h is what tools/gen_f64_pow10.py writes"""
    import sys
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "gen_f64_pow10.py"), "--check"])
    assert r.returncode == 0
