"""The seeded corpus of doubles the number text of the result writer is checked on (pg_f64_text.h: display and roundup_own), shared
by tests/test_f64_text_host.py, tests/test_resultfmt_host.py and the GPU tests.  Everything is built once per process; the expected
text comes from tests/rustfmt.py, the Python restatement of Rust's `{}` and of parse_f64_roundup_and_own."""
import functools
import math
import struct

import numpy as np

import rustfmt

NDS = (0, 6, 7, 8, 12, 22)            # the roundup_own digit counts that are checked
SPECIALS = [0.0, -0.0, 5e-324, -5e-324, 1.7976931348623157e308, -1.7976931348623157e308, 1e23, 9007199254740993.0, float("nan"),
            float("inf"), float("-inf"), 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 0.1, 0.5223146158470686,
            0.7797774084757156, 1e22, 1e21, 1e16, 9007199254740992.0, 18014398509481984.0, 1.8e16, 123456.789, 0.3, 2.5, 1e-7]
MAX_LEN = 327                          # len("-0." + "0" * 307 + 17 digits): the longest display()


def from_bits(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u & (2 ** 64 - 1)))[0]


def to_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def ulps(x: float, d: int) -> float:
    """x moved by d units in the last place (finite x; stays on x's side of zero)"""
    return from_bits(to_bits(x) + d)


def halfway(nd: int, rng) -> list:
    """exact halves of the rounding, (m + 0.5) / 10^nd, and their neighbours: what round-half-away and the two separately rounded
    operations of sensible_round decide"""
    out = []
    f = float("1e%d" % nd)
    for j in range(0, 15):
        for m in [0, 1, 2, 10 ** j, 10 ** j - 1] + [int(v) for v in rng.integers(0, 10 ** j + 1, size=12)]:
            x = (m + 0.5) / f
            for s in (x, -x):
                out += [s, ulps(s, 1), ulps(s, -1)] if s != 0 else [s]
    for d in range(-3, 4):                     # products next to and at the largest double below one half (see sensible_round below)
        y = ulps(0.49999999999999994 / f, d)
        out += [y, -y]
    return out


def with_length(n: int, rng, tries: int = 40) -> list:
    """values whose display() has exactly n characters (n >= 1): integers, fractions below 1, negative ones"""
    out = []
    for _ in range(tries):
        cands = []
        if 1 <= n <= 15:
            cands.append("".join([str(rng.integers(1, 10))] + [str(d) for d in rng.integers(0, 10, size=n - 1)]))
        if n >= 3:
            digits = int(rng.integers(1, min(17, n - 2) + 1))
            body = "".join(str(d) for d in rng.integers(0, 10, size=digits - 1)) + str(rng.integers(1, 10))
            cands.append("0." + "0" * (n - 2 - digits) + body)
        if n >= 4:
            digits = int(rng.integers(1, min(17, n - 3) + 1))
            body = "".join(str(d) for d in rng.integers(0, 10, size=digits - 1)) + str(rng.integers(1, 10))
            cands.append("-0." + "0" * (n - 3 - digits) + body)
        if 4 <= n <= 16:
            ip = int(rng.integers(1, n - 2))
            cands.append("".join([str(rng.integers(1, 10))] + [str(d) for d in rng.integers(0, 10, size=ip - 1)]) + "." +
                         "".join(str(d) for d in rng.integers(0, 10, size=n - ip - 2)) + str(rng.integers(1, 10)))
        for c in cands:
            x = float(c)
            if len(rustfmt.display(x)) == n:
                out.append(x)
    return out


@functools.lru_cache(maxsize=None)
def corpus() -> np.ndarray:
    rng = np.random.default_rng(20261020)
    parts = [rng.integers(0, 2 ** 64, size=200_000, dtype=np.uint64).view(np.float64),        # random bit patterns
             rng.random(20_000)]                                                             # [0, 1)
    logu = [float("%de%d" % (int(m), int(e) - 16)) for m, e in zip(rng.integers(10 ** 16, 10 ** 17, size=30_000), rng.integers(-324, 309, size=30_000))]
    parts.append(np.array(logu) * rng.choice([-1.0, 1.0], size=len(logu)))                   # log-uniform 17-digit values
    p10 = []
    for e in range(-323, 309):
        x = float("1e%d" % e)
        for d in (-2, -1, 0, 1, 2):
            y = ulps(x, d)
            if math.isfinite(y):
                p10 += [y, -y]
    parts.append(np.array(p10))
    edges = [from_bits((b << 52) | f) for b in range(0, 2047) for f in (0, 1, 2 ** 52 - 2, 2 ** 52 - 1)]
    parts.append(np.array(edges + [-x for x in edges]))
    ks = list(range(0, 1500)) + [int(v) for v in rng.integers(0, 2 ** 53, size=1500)]
    parts.append(np.array([k * 2.0 ** -53 for k in ks] + [1.0 - k * 2.0 ** -53 for k in ks]))    # what 2 (1 - cdf) produces
    for nd in NDS:
        parts.append(np.array(halfway(nd, rng)))
        for n in (nd - 1, nd, nd + 1):
            if n >= 1:
                parts.append(np.array(with_length(n, rng)))
    parts.append(np.array(SPECIALS))
    out = np.concatenate(parts)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def displayed() -> tuple:
    """rustfmt.display of every member"""
    return tuple(rustfmt.display(v) for v in corpus().tolist())


HALF_BELOW = 0.49999999999999994       # the largest double below one half


def sensible_round(x: float, nd: int) -> float:
    """rustfmt.sensible_round, except at the one product it gets wrong: for |x * 10^nd| = 0.49999999999999994 its floor(|v| + 0.5)
    is 1 (the sum rounds up to 1.0) and its guard `r - |v| > 0.5` compares a difference that itself rounded down to 0.5, so it
    returns 1 where f64::round returns 0 (as C's round() does, which today's host writer calls).  That value rounds to zero here."""
    f = float("1e%d" % nd)
    v = x * f
    if abs(v) == HALF_BELOW:
        return math.copysign(0.0, v) / f
    return rustfmt.sensible_round(x, nd)


def roundup_own(x: float, nd: int, s: str = None) -> str:
    s = rustfmt.display(x) if s is None else s
    return s if len(s) < nd else rustfmt.display(sensible_round(x, nd))


@functools.lru_cache(maxsize=None)
def expected(nd: int) -> bytes:
    """the text pg_host_f64_text / pg_f64_text_dev must give for the corpus: one line per value"""
    if nd < 0:
        return ("\n".join(displayed()) + "\n").encode()
    return ("\n".join(roundup_own(v, nd, s) for v, s in zip(corpus().tolist(), displayed())) + "\n").encode()


def sample(n: int, seed: int) -> np.ndarray:
    """n members drawn with a seed, the long and the special ones among them (cells of 1 to 327 bytes)"""
    c = corpus()
    rng = np.random.default_rng(seed)
    picks = c[rng.integers(0, len(c), size=n)]
    head = np.array([1e-300, -2.2250738585072014e-308, 5e-324, 1.7976931348623157e308, 0.0, float("nan"), 1.0, -0.0, float("inf"), 0.25])
    picks[:min(n, len(head))] = head[:n]
    return picks
