"""`poolgen gudmc` end to end on tests/golden/test.sync and test.csv with the reference's own test parameters (window 100, slide
50, min loci 20; gudmc.rs:500-510).  By default the file is the header alone (the reference hands tajima_d fractions for pool
sizes, every D is NaN); with --popgen-as-documented the rows are the restatement's (tests/gudmc_ref.py): the columns the reference
fixes exactly byte for byte, the fitted ones within the measured tolerance after parsing."""
import math
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gudmc_ref as R
import popgen_diversity_restated as D

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
WIN, SLIDE, MINL = 100, 50, 20
EXACT = (0, 1, 2, 3, 4, 9, 10, 11)      # pop_a, pop_b, chr, pos_ini, pos_fin, tajima_d_pop_b, the width and its deviation


def run_cli(*args, ok=True):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def expected(oracle):
    """the restatement on the fixture, pool sizes as written, every locus of a window counted"""
    from test_gpu_popgen_diversity import _fixture_matrix, restate
    chrom, pos, Xt, covs = _fixture_matrix(oracle)
    idx, lc, lp = oracle.count_loci(chrom, pos)
    rows = [l.split(",") for l in (GOLD / "test.csv").read_text().splitlines() if not l.startswith("#")]
    names, written = [r[0] for r in rows], [float(r[1]) for r in rows]
    head, tail = oracle.sliding_windows(lc[:-1], lp[:-1], WIN, SLIDE, MINL)
    assert len(head) >= 5
    d_win = restate(oracle, Xt, idx, covs, head, tail, written, None)[4]
    rc, _, fst_win = oracle.fst(Xt, idx, covs, head, tail)
    assert rc == 0
    # With these parameters the fixture's last window is the stale tail of a ditched slot (tail < head): an empty slice in the
    # reference, whose mean_axis is None -> NaN in both tables (pi.rs:87-90, fst.rs:194-197).  The oracle's loops divide an
    # empty sum by a negative length there, so the rows are set here.
    stale = [w for w in range(len(head)) if tail[w] < head[w]]
    assert stale == [len(head) - 1]
    d_win[stale, :] = np.nan
    fst_win[stale, :] = np.nan
    ids = {}
    wchr = [ids.setdefault(lc[h], len(ids)) for h in head]
    ini, fin = [lp[h] for h in head], [lp[t] for t in tail]
    res = R.gudmc_stage(d_win, fst_win, wchr, ini, fin, 2.0, 0.73)
    return res, R.csv_rows(res, names, [lc[h] for h in head], ini, fin), names


@pytest.fixture(scope="module")
def sync(tmp_path_factory):
    d = tmp_path_factory.mktemp("gudmc_cli")
    shutil.copy(GOLD / "test.sync", d / "test.sync")
    return d / "test.sync"


def common(sync):
    return ["-f", sync, "-p", GOLD / "test.csv", "--phen-value-col", "2,3", "--n-threads", 2, "--window-size-bp", WIN,
            "--window-slide-size-bp", SLIDE, "--min-loci-per-window", MINL]


def test_default_is_the_header_alone(sync):
    r = subprocess.run([str(CLI), "gudmc", *map(str, common(sync))], capture_output=True, text=True, cwd=sync.parent)
    assert r.returncode == 0, r.stderr
    assert "--popgen-as-documented" in r.stderr and "header alone" in r.stderr
    out = Path(r.stdout.strip().splitlines()[-1])
    assert re.fullmatch(re.escape(str(sync.parent / "test")) + r"-gudmc-[0-9.]+\.csv", str(out)), out
    assert out.read_text() == R.HEADER + "\n"
    assert not list(sync.parent.glob("gudmc_intermediate_file_*")) and not list(sync.parent.glob("*.tmp"))


def test_as_documented_matches_the_restatement(sync, expected):
    res, want, names = expected
    out = sync.parent / "documented.csv"
    r = run_cli("gudmc", *common(sync), "--popgen-as-documented", "-o", out)
    assert r.stdout.strip().endswith(str(out))
    got = out.read_text().splitlines()
    assert got[0] == R.HEADER
    assert len(got) - 1 == len(want) == len(names) * sum(res["rows"]) > 0
    n = len(names)
    degenerate = {a * n + a for a in range(n)}
    assert {i for i in range(n * n) if res["fst_sd"][i] <= R.DEGENERATE_SD} == degenerate
    assert all(p["width_sd"] > R.DEGENERATE_SD for p in res["pops"])
    worst = 0.0
    for line, w in zip(got[1:], want):
        f = line.split(",")
        assert len(f) == 15 and [f[c] for c in EXACT] == [w[c] for c in EXACT], (line, w)
        a, b = names.index(f[0]), names.index(f[1])
        i = a * n + b
        # 5 mean D, 6 mean Fst, 7 sd D, 8 sd Fst, 12 width p, 13 fst_delta, 14 fst p: printed at 7 decimals (half a unit of the
        # last digit on either side) on top of the tolerance
        half = 1.0000001e-7
        bounds = {5: R.T * res["d_sd"][b], 7: R.T * res["d_sd"][b], 12: R.T}
        if i in degenerate:
            assert abs(float(f[6])) <= 1e-12 and float(f[8]) <= R.DEGENERATE_SD
        else:
            bounds.update({6: R.T * res["fst_sd"][i], 8: R.T * res["fst_sd"][i], 13: R.T * res["fst_sd"][i], 14: R.T})
        for c, bound in bounds.items():
            g, e = float(f[c]), float(w[c])
            if math.isnan(e):
                assert math.isnan(g), (line, c)
                continue
            worst = max(worst, abs(g - e))
            assert abs(g - e) <= bound + half, (line, w, c)
    print(f"gudmc CSV: {len(want)} rows, rows per population {res['rows']}, worst |printed - restatement| {worst:.3g}")
    before = out.read_bytes()
    r = run_cli("gudmc", *common(sync), "--popgen-as-documented", "-o", out, ok=False)      # an existing target is refused
    assert "Unable to create file" in r.stderr and out.read_bytes() == before


def test_refusals(sync):
    d = sync.parent
    dashed = d / "dashed.sync"
    lines = (GOLD / "test.sync").read_text().splitlines()
    first = next(l for l in lines if not l.startswith("#")).split("\t")[0]
    assert sum(l.startswith(first + "\t") for l in lines) > 20
    dashed.write_text("\n".join(l.replace(first, first + "-b", 1) if l.startswith(first + "\t") else l for l in lines) + "\n")
    args = common(sync)
    args[1] = dashed
    r = run_cli("gudmc", *args, "--popgen-as-documented", "-o", d / "never.csv", ok=False)
    assert "contains `-`" in r.stderr and not (d / "never.csv").exists()
    r = run_cli("gudmc", *common(sync), "--recombination-rate-cm-per-mb", "1.5", ok=False)
    assert "between 0.0 and 1.0" in r.stderr
    assert "gudmc" in run_cli("--help").stdout
    r = run_cli("fst", *common(sync), "--popgen-as-documented", ok=False)
    assert "--popgen-as-documented applies to" in r.stderr
