"""pg_host_watterson_windows = theta_watterson's own window loop (popgen/watterson_theta.rs:56-164) on the host: head / tail
against the two existing implementations of define_sliding_windows, cov / seed / slot against the line-for-line
restatement (tests/popgen_diversity_restated.py), and the restatement itself against the reference's two unit tests."""
import json
from pathlib import Path

import numpy as np

import popgen_diversity_restated as R

GOLD = Path(__file__).parent / "golden"
LIT = json.loads((GOLD / "popgen_diversity_literals.json").read_text())


def both(native, chrom, pos, w, s, m):
    ids = {}
    ch = np.array([ids.setdefault(c, len(ids)) for c in chrom], dtype=np.int32)
    po = np.ascontiguousarray(pos, dtype=np.uint64)
    l = len(ch)
    out = [np.full(l, -7, dtype=np.int64) for _ in range(5)]
    nw = native.pg_host_watterson_windows(ch.ctypes.data, po.ctypes.data, l, w, s, m, *[o.ctypes.data for o in out])
    h2 = np.empty(l, dtype=np.int64); t2 = np.empty(l, dtype=np.int64)
    nw2 = native.pg_host_sliding_windows(ch.ctypes.data, po.ctypes.data, l, w, s, m, h2.ctypes.data, t2.ctypes.data)
    return [o[:nw].tolist() for o in out], (h2[:nw2].tolist(), t2[:nw2].tolist())


def cases():
    """(chrom, pos, size, slide, min_loci): several chromosomes, gaps wider than the window, slide < size, min_loci of
    1, 3 and 10; L = 1; L = 2 on two chromosomes (the reference's own case)."""
    out = [([0], [5], 100, 50, m) for m in (1, 3, 10)]
    out += [(["X", "Y"], [123, 456], 100, 50, m) for m in (1, 3, 10)]
    rng = np.random.default_rng(17)
    for _ in range(120):
        l = int(rng.integers(2, 300))
        chrom = np.sort(rng.integers(0, int(rng.integers(1, 6)), size=l)).tolist()
        pos = []
        for c in sorted(set(chrom)):                       # dense runs separated by gaps of several windows
            k = chrom.count(c)
            step = rng.integers(1, 40, size=k)
            step[rng.random(k) < 0.08] += 2000
            pos += np.cumsum(step).tolist()
        for m in (1, 3, 10):
            out.append((chrom, pos, int(rng.integers(60, 500)), int(rng.integers(10, 60)), m))
    return out


def test_watterson_windows_match_sliding_windows_and_the_restated_loop(native, oracle):
    ditched = short = 0
    for chrom, pos, w, s, m in cases():
        assert s < w
        (head, tail, cov, seed, slot), (h2, t2) = both(native, chrom, pos, w, s, m)
        oh, ot = oracle.sliding_windows(chrom, pos, w, s, m)
        assert (head, tail) == (h2, t2) == (oh.tolist(), ot.tolist())
        rh, rt, rcov, rseed, rslot, _ = R.watterson_windows(chrom, pos, w, s, m)
        assert (head, tail, cov, seed, slot) == (rh.tolist(), rt.tolist(), rcov.tolist(), rseed.tolist(), rslot.tolist())
        ditched += sum(1 for h, sd, sl in zip(head, seed, slot) if sd == sl != h)
        short += sum(1 for h, t, c in zip(head, tail, cov) if c != t - h + 1)
    # without these the inputs would not show the reference's count for what it is
    assert ditched > 0, "no kept window went through the ditch-and-reuse branch"
    assert short > 0, "no kept window whose counted loci differ from tail - head + 1"


def test_watterson_windows_of_the_reference_unit_test(native):
    (head, tail, cov, seed, slot), _ = both(native, ["X", "Y"], [123, 456], 100, 50, 1)
    assert (head, tail, cov, seed, slot) == ([0, 1], [0, 1], [1, 1], [0, 1], [0, 1])
    # one locus: one window, nothing ditched
    assert both(native, [0], [9], 100, 50, 10)[0] == [[0], [0], [1], [0], [0]]
    # two chromosomes, too few loci on the first: the slot is re-used, its tail stays behind its new head
    assert both(native, ["X", "Y"], [123, 456], 100, 50, 3)[0] == [[1], [0], [1], [0], [0]]


def test_restatement_reproduces_the_reference_literals(native, oracle):
    """watterson_theta.rs:298-398 and tajima_d.rs:180-278 on the CPU, over the library's windows: the restatement the GPU
    tests compare against prints the reference's own expected roundings."""
    lab = LIT["labels"]
    idx, lc, lp = oracle.count_loci(lab["chromosome"], lab["position"])
    head, tail, cov, seed, slot, terms = R.watterson_windows(lc[:-1], lp[:-1], LIT["window_size_bp"], LIT["window_slide_size_bp"],
                                                             LIT["min_loci_per_window"])
    got, _ = both(native, lc[:-1], lp[:-1], LIT["window_size_bp"], LIT["window_slide_size_bp"], LIT["min_loci_per_window"])
    assert got == [head.tolist(), tail.tolist(), cov.tolist(), seed.tolist(), slot.tolist()]
    covs = np.array(LIT["coverages_pool_by_locus"]).T
    x = np.array(LIT["watterson"]["x_pool_by_column"]).T
    S, c = R.segregating_sites(R.poly_flags(x, idx), head, tail, terms)
    theta, _ = R.theta_watterson(S, c, LIT["pool_sizes"])
    e = LIT["watterson"]["expect_round4"]
    assert [oracle.round_own(theta[0, 1], 4), oracle.round_own(theta[1, 1], 4), oracle.round_own(theta[0, 2], 4), oracle.round_own(theta[1, 2], 4)] == \
        [e["pop2_window1"], e["pop2_window2"], e["pop3_window1"], e["pop3_window2"]]
    assert theta[0, 2] == 0.23239960609853114
    x = np.array(LIT["tajima_d"]["x_pool_by_column"]).T
    S, c = R.segregating_sites(R.poly_flags(x, idx), head, tail, terms)
    theta, _ = R.theta_watterson(S, c, LIT["pool_sizes"])
    pi, _ = oracle.theta_pi(x, idx, covs, head, tail)
    d, _ = R.tajima_d(theta, pi, LIT["pool_sizes"])
    e = LIT["tajima_d"]["expect_round4"]
    assert [oracle.round_own(d[0, 1], 4), oracle.round_own(d[1, 1], 4), oracle.round_own(d[0, 3], 4), oracle.round_own(d[1, 3], 4)] == \
        [e["pop2_window1"], e["pop2_window2"], e["pop4_window1"], e["pop4_window2"]]
    assert (d[0, 3], d[1, 3]) == (-5.395430943536947, 7.071957377676666)
