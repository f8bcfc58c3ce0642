"""fisher_exact_test on the GPU (Engine.fisher / pg_fisher_batch[_dev] / Operators::fisher) against the restatement of
tables::fisher in tests/fisher_ref.py, fed by the oracle's LocusCounts::filter.  Alleles kept, their ids and which loci emit a
row: exact.  p_observed and pval (= p_observed + p_extremes): relative 1e-10.  Every test prints the worst relative deviation."""
import ctypes as C
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest
import torch

import fisher_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = Path(__file__).parent / "golden"
LIT = json.loads((GOLD / "fisher_literals.json").read_text())
TOL = 1e-10
PG_ERR_INVALID = -1
COL = {a: i for i, a in enumerate("ATCGND")}


def flt_pair(oracle, remove_ns=True, min_cov=1, maf=0.001, miss=0.0):
    from poolgen_amd.engine import Filter
    return Filter(remove_ns, min_cov, maf, miss), oracle.filt(remove_ns, min_cov, maf, miss)


def run_gpu(engine, counts_np, ps, f):
    """counts_np: L x n x 6 -> host arrays n_out[L], ids[L, 5], p_observed[L], pval[L]"""
    t = torch.tensor(np.ascontiguousarray(counts_np, dtype=np.int32), device="cuda")
    no, ids, po, pv = engine.fisher(t, ps, f)
    torch.cuda.synchronize()
    return no.cpu().numpy(), ids.cpu().numpy(), po.cpu().numpy(), pv.cpu().numpy()


def check(oracle, counts_np, ps, fo, got, literal=None, compact=None):
    """Emission pattern of EVERY locus against the oracle's filter; the numbers of the loci in `literal` against the literal
    restatement, of those in `compact` against the compacted one (None = all loci through the literal one).
    Returns (rows emitted, loci compared numerically, worst relative deviation)."""
    no, ids, po, pv = got
    L = counts_np.shape[0]
    if literal is None and compact is None:
        literal = range(L)
    literal, compact = set(literal or ()), set(compact or ())
    worst, emitted, compared = 0.0, 0, 0
    for l in range(L):
        r = oracle.filter_locus(counts_np[l].astype(np.uint64), ps, fo)
        if r is None:
            assert no[l] == 0, f"locus {l}: the filter drops it, the GPU emits {no[l]} alleles"
            continue
        rid, m = r
        emitted += 1
        assert no[l] == len(rid), f"locus {l}: {no[l]} alleles kept, the filter keeps {len(rid)}"
        assert ids[l, :min(len(rid), 5)].tolist() == [int(x) for x in rid[:5]], f"locus {l}: allele ids"
        if l in literal:
            want = fisher_ref.fisher(m)
        elif l in compact:
            want = fisher_ref.fisher_compact(m)
        else:
            continue
        compared += 1
        d = max(fisher_ref.rel(po[l], want[0]), fisher_ref.rel(pv[l], want[1]))
        assert d <= TOL, f"locus {l}: p_observed {po[l]!r} pval {pv[l]!r}, restatement {want!r} (relative {d:.3g}); table {m.tolist()}"
        worst = max(worst, d)
    return emitted, compared, worst


def locus_from_table(n, alleles, table):
    c = np.zeros((n, 6), dtype=np.int64)
    for j, a in enumerate(alleles):
        c[:, COL[a]] = [row[j] for row in table]
    return c


def unit_locus():
    f = LIT["fisher"]
    return locus_from_table(3, f["alleles_vector"], f["matrix"])[None], f


def test_reference_unit_locus_through_every_interface(engine, oracle, native):
    counts, lit = unit_locus()
    fl = lit["filter"]
    f, fo = flt_pair(oracle, fl["remove_ns"], fl["min_coverage_depth"], fl["min_allele_frequency"], fl["max_missingness_rate"])
    ps = lit["pool_sizes"]
    worst = 0.0
    # Engine.fisher (pg_fisher_batch_dev)
    no, ids, po, pv = run_gpu(engine, counts, ps, f)
    assert no.tolist() == [2] and "".join("ATCGND"[i] for i in ids[0, :2]) == "TC"
    worst = max(worst, fisher_ref.rel(po[0], lit["p_observed"]), fisher_ref.rel(pv[0], lit["pvalue"]))
    # pg_fisher_batch, host buffers
    from poolgen_amd._native import PgFilter
    c32 = np.ascontiguousarray(counts, dtype=np.uint32)
    psd = np.ascontiguousarray(ps, dtype=np.float64)
    cf = PgFilter(1, 0, fl["min_coverage_depth"], fl["min_allele_frequency"], fl["max_missingness_rate"])
    hno = np.zeros(1, dtype=np.int32); hid = np.full(5, -1, dtype=np.int32); hpo = np.zeros(1); hpv = np.zeros(1)
    rc = native.pg_fisher_batch(engine._ctx, c32.ctypes.data, 1, 3, psd.ctypes.data, C.byref(cf), hno.ctypes.data, hid.ctypes.data,
                                hpo.ctypes.data, hpv.ctypes.data)
    assert rc == 0, native.pg_last_error(engine._ctx)
    assert hno.tolist() == [2] and hid[:2].tolist() == [COL["T"], COL["C"]]
    worst = max(worst, fisher_ref.rel(hpo[0], lit["p_observed"]), fisher_ref.rel(hpv[0], lit["pvalue"]))
    assert hpo[0] == po[0] and hpv[0] == pv[0]            # same kernel, same locus: same bits
    # Operators::fisher (apitest: the reference's unit test, transcribed)
    r = subprocess.run([str(ROOT / "poolgen_amd" / "csrc" / "apitest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    line = next(l for l in r.stdout.splitlines() if l.strip().startswith("fisher -> "))
    fields = line.split("-> ")[1].split(",")
    assert fields[:3] == ["Chromosome1", "12345", "TC"]
    worst = max(worst, fisher_ref.rel(float(fields[3]), lit["p_observed"]), fisher_ref.rel(float(fields[4]), lit["pvalue"]))
    assert "ok   fisher(locus_counts, filter_stats)" in r.stdout and "FAIL" not in r.stdout
    print(f"unit locus, three interfaces: worst relative deviation from the reference literals {worst:.3g}")
    assert worst <= TOL


@pytest.mark.parametrize("min_cov,maf", [(1, 0.001), (10, 0.01)])
def test_reference_fixture_every_locus(engine, oracle, min_cov, maf):
    """tests/golden/test.sync x test.csv pool sizes, every locus, under the two filter sets of the reference's CI."""
    rows = []
    for line in (GOLD / "test.sync").read_text().splitlines():
        n, chrom, pos, cnt = oracle.parse_sync_line(line)
        if n > 0:
            rows.append(cnt)
    counts = np.stack(rows).astype(np.int64)
    ps = np.loadtxt(GOLD / "test.csv", delimiter=",", comments="#", usecols=(1,))
    assert counts.shape[0] == 6674 and counts.shape[1] == len(ps) == 5
    f, fo = flt_pair(oracle, True, min_cov, maf, 0.0)
    emitted, compared, worst = check(oracle, counts, ps, fo, run_gpu(engine, counts, ps, f))
    print(f"test.sync min_cov={min_cov} maf={maf}: {emitted} of {counts.shape[0]} loci emit a row, all compared with the literal "
          f"restatement, worst relative deviation {worst:.3g}")
    assert compared == emitted > 500


@pytest.mark.parametrize("remove_ns", [True, False])
@pytest.mark.parametrize("error_rate", [0.0, 0.005])
@pytest.mark.parametrize("n", [3, 16, 17, 64, 100, 200])
def test_synthetic_counts(engine, oracle, n, error_rate, remove_ns):
    """synth.sync_counts; a third of the loci additionally get a few pools sequenced 40 times deeper, so that with many pools the
    scaled table does not come out all zero (34 reads over 100 equally deep pools leave no cell above zero)."""
    from poolgen_amd import synth
    L = 1000 + n + 37                                         # never a multiple of 64 for these n
    assert L % 64 != 0
    counts = synth.sync_counts(L, n, "cpu", seed=900 + n, error_rate=error_rate).numpy().astype(np.int64)
    rng = np.random.default_rng(n * 7 + int(remove_ns))
    for l in range(0, L, 3):
        deep = rng.choice(n, size=min(n, int(rng.integers(1, 6))), replace=False)
        counts[l, deep, :] *= 40
    ps = np.full(n, 20.0)
    f, fo = flt_pair(oracle, remove_ns)
    got = run_gpu(engine, counts, ps, f)
    # the sample: every locus with three or more surviving alleles first (up to the budget), then a seeded draw
    budget = 64
    multi = [l for l in range(L) if got[0][l] >= 3][:budget]
    rest = [l for l in rng.permutation(L).tolist() if got[0][l] > 0 and l not in set(multi)]
    sample = multi + rest[:max(0, budget - len(multi))]
    assert len(sample) >= 64
    if n <= 17:
        lit, comp = sample, []
    else:
        # eight through the literal restatement (quadratic in n p: the cheapest two with three or more alleles, the rest biallelic)
        by_cost = sorted(sample, key=lambda l: (got[0][l], l))
        pick = [l for l in by_cost if got[0][l] >= 3][:2]
        pick += [l for l in by_cost if l not in set(pick)][:8 - len(pick)]
        lit, comp = pick, [l for l in sample if l not in set(pick)]
        assert len(lit) >= 8
    emitted, compared, worst = check(oracle, counts, ps, fo, got, literal=lit, compact=comp)
    print(f"synthetic n={n} error_rate={error_rate} remove_ns={remove_ns}: L={L}, {emitted} emit a row (pattern of all loci compared), "
          f"{len(multi)} sampled loci keep >= 3 alleles, {len(lit)} literal + {len(comp)} compacted comparisons, worst relative deviation {worst:.3g}")
    assert compared == len(sample)


HAND = [  # (what, alleles, table pools x alleles)
    ("total 17 < 34", "TC", [[0, 3], [1, 5], [2, 6]]),
    ("total = 34", "AT", [[10, 7], [5, 4], [4, 4]]),
    ("total = 35", "AT", [[10, 7], [5, 4], [5, 4]]),
    ("total 833, cells 49 / 98 / 392 scale to 1 / 3 / 15", "AG", [[49, 98], [392, 0], [196, 98]]),
    ("last pool all zero after scaling", "AT", [[300, 200], [250, 250], [3, 2]]),
    ("last surviving allele all zero after scaling", "AT", [[99, 1], [99, 1], [98, 2]]),
    ("first pool all zero after scaling", "CG", [[3, 2], [300, 200], [250, 250]]),
    ("first surviving allele all zero after scaling", "AT", [[1, 99], [1, 99], [2, 98]]),
    ("five surviving alleles", "ATCGD", [[10, 8, 6, 5, 4], [7, 9, 5, 6, 3], [8, 8, 8, 8, 8]]),
    ("dropped by the filter (fixed)", "AT", [[10, 0], [10, 0], [10, 0]]),
]


def test_hand_made_tables(engine, oracle):
    n = 3
    ps = np.full(n, 0.2)
    f, fo = flt_pair(oracle, True, 1, 0.001, 0.0)
    loci = np.stack([locus_from_table(n, al, tb) for _, al, tb in HAND])
    # the tables are what their names say
    s = fisher_ref.scaled(np.array(HAND[3][2]))
    assert s.sum() <= 34 and s[0].tolist() == [1.0, 3.0] and s[1, 0] == 15.0
    assert fisher_ref.scaled(np.array(HAND[4][2]))[-1].sum() == 0 and fisher_ref.scaled(np.array(HAND[5][2]))[:, -1].sum() == 0
    assert fisher_ref.scaled(np.array(HAND[6][2]))[0].sum() == 0 and fisher_ref.scaled(np.array(HAND[7][2]))[:, 0].sum() == 0
    worst = 0.0
    singles = []
    for i, (what, al, tb) in enumerate(HAND):                 # L = 1 each
        got = run_gpu(engine, loci[i:i + 1], ps, f)
        emitted, compared, w = check(oracle, loci[i:i + 1], ps, fo, got)
        assert emitted == (0 if "dropped" in what else 1), what
        if emitted:
            assert "".join("ATCGND"[k] for k in got[1][0, :got[0][0]]) == al, what
        worst = max(worst, w)
        singles.append(got)
    got = run_gpu(engine, loci, ps, f)                        # and all in one batch
    emitted, compared, w = check(oracle, loci, ps, fo, got)
    assert emitted == compared == len(HAND) - 1
    for i, sg in enumerate(singles):                          # a locus' result does not depend on its batch
        assert sg[0][0] == got[0][i]
        if sg[0][0]:
            assert sg[2][0] == got[2][i] and sg[3][0] == got[3][i] and sg[1][0].tolist() == got[1][i].tolist()
    print(f"hand-made tables: {len(HAND)} loci alone and in one batch, worst relative deviation {max(worst, w):.3g}")


def test_result_is_a_function_of_the_locus_alone(engine):
    """The same 4 096 loci as one batch, as 7 uneven pieces, reversed, and after unrelated chisq / ols_iterate calls on
    error-bearing counts on the same engine: bit-identical on every emitted locus."""
    from poolgen_amd import synth
    from poolgen_amd.engine import Filter
    n, L = 17, 4096
    counts = synth.sync_counts(L, n, "cuda", seed=77, error_rate=0.005)
    counts[::3, :4, :] *= 7
    counts[5::11, -1, :] = (counts[5::11, -1, :].double() * 0.02).ceil().int()
    counts = counts.contiguous()
    ps = np.full(n, 20.0)
    f = Filter()

    def run(c):
        no, ids, po, pv = engine.fisher(c, ps, f)
        torch.cuda.synchronize()
        return no, ids, po, pv

    def same(a, b):
        live = a[0] > 0
        slot = torch.arange(5, device="cuda")[None, :] < a[0][:, None]
        return (torch.equal(a[0], b[0]) and torch.equal(a[1][slot], b[1][slot]) and torch.equal(a[2][live], b[2][live])
                and torch.equal(a[3][live], b[3][live]))

    base = run(counts)
    assert int((base[0] > 0).sum()) > L // 2 and int((base[0] >= 3).sum()) > 0
    cuts = [0, 1, 64, 777, 1500, 1501, 3333, L]
    pieces = [run(counts[a:b].clone()) for a, b in zip(cuts[:-1], cuts[1:])]   # fresh copies: 16-byte aligned whatever the cut
    glued = tuple(torch.cat([p[i] for p in pieces]) for i in range(4))
    assert same(base, glued), "pieces differ from the whole batch"
    rev = run(counts.flip(0).contiguous())
    assert same(base, tuple(x.flip(0) for x in rev)), "the reversed batch differs"
    noisy = synth.sync_counts(3000, 100, "cuda", seed=5, error_rate=0.01)
    Y = synth.phenotypes(synth.genotype_matrix(64, 100, "cuda", seed=1), 100, k=1, seed=1)
    engine.chisq(noisy, np.full(100, 20.0), f)
    engine.ols_iterate(noisy, np.full(100, 20.0), f, Y)
    assert same(base, run(counts)), "an unrelated chisq / ols_iterate call changed the result"
    clean = synth.sync_counts(3000, 100, "cuda", seed=6)
    engine.chisq(clean, np.full(100, 20.0), f)
    engine.ols_iterate(clean, np.full(100, 20.0), f, Y)
    assert same(base, run(counts)), "an unrelated chisq / ols_iterate call on clean counts changed the result"
    print(f"purity: {int((base[0] > 0).sum())} emitted loci of {L} bit-identical over 7 pieces, reversed order and foreign calls in between")


def test_argument_checks(engine, oracle, native):
    from poolgen_amd import NativeError, synth
    from poolgen_amd._native import PgFilter
    n, L = 5, 200                                             # odd n: a view that starts at an odd locus is 8 bytes off
    counts = synth.sync_counts(L, n, "cuda", seed=3)
    ps = np.full(n, 20.0)
    f, fo = flt_pair(oracle)
    cf = PgFilter(1, 0, 1, 0.001, 0.0)
    no = torch.empty(L, dtype=torch.int32, device="cuda"); ids = torch.empty((5, L), dtype=torch.int32, device="cuda")
    po = torch.empty(L, dtype=torch.float64, device="cuda"); pv = torch.empty(L, dtype=torch.float64, device="cuda")

    def call(cptr, l, no_ptr=None, pv_ptr=None):
        return native.pg_fisher_batch_dev(engine._ctx, cptr, l, n, ps.ctypes.data, C.byref(cf), no.data_ptr() if no_ptr is None else no_ptr,
                                          ids.data_ptr(), po.data_ptr(), pv.data_ptr() if pv_ptr is None else pv_ptr)

    assert counts.data_ptr() % 16 == 0 and (counts.data_ptr() + n * 24) % 16 == 8
    assert call(counts.data_ptr() + n * 24, L - 1) == PG_ERR_INVALID and b"16-byte aligned" in native.pg_last_error(engine._ctx)
    assert call(counts.data_ptr(), 0) == PG_ERR_INVALID
    assert call(counts.data_ptr(), L, pv_ptr=0) == PG_ERR_INVALID
    assert call(counts.data_ptr(), L, no_ptr=0) == PG_ERR_INVALID
    assert call(0, L) == PG_ERR_INVALID
    big = counts.clone()
    big[17, 2, 0] = 1 << 29
    with pytest.raises(NativeError, match=rf"failed \({PG_ERR_INVALID}\)"):
        engine.fisher(big, ps, f)
    hc = np.zeros((1, n, 6), dtype=np.uint32)
    hno = np.zeros(1, dtype=np.int32); hid = np.zeros(5, dtype=np.int32); hpo = np.zeros(1); hpv = np.zeros(1)
    assert native.pg_fisher_batch(engine._ctx, hc.ctypes.data, 0, n, ps.ctypes.data, C.byref(cf), hno.ctypes.data, hid.ctypes.data,
                                  hpo.ctypes.data, hpv.ctypes.data) == PG_ERR_INVALID
    assert native.pg_fisher_batch(engine._ctx, hc.ctypes.data, 1, n, ps.ctypes.data, C.byref(cf), hno.ctypes.data, hid.ctypes.data,
                                  None, hpv.ctypes.data) == PG_ERR_INVALID
    # the context still works
    host = counts.cpu().numpy().astype(np.int64)
    emitted, compared, worst = check(oracle, host, ps, fo, run_gpu(engine, host, ps, f))
    assert emitted == compared > 0
    print(f"after the refused calls: {emitted} loci, worst relative deviation {worst:.3g}")
