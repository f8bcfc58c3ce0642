"""`poolgen gwalpha` end to end against the restatement's lines (tests/gwalpha_ref.py): chr, pos, allele, freq, Pheno_0 and
Unknown byte for byte, alpha parsed and within 2e-6 (one unit of the printed digit plus the trajectory bound of
tests/test_gpu_gwalpha.py); LS, ML and an unknown method name (= ML, main.rs:337-356); the refusals; pileup input; two GPUs."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gwalpha_ref as G

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
PHEN = G.gwalpha_fmt_text("trait", 0.3, 0.5, 6.5, [0.15, 0.4, 0.6, 0.85], [1.0, 2.5, 4.0, 6.0])
HEADER = "#chr,pos,alleles,freq,phenotype,statistic,pvalue"


def run_cli(*args, ok=True, env=None):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("gwalpha_cli")
    sync = d / "forty.sync"
    sync.write_text("\n".join((GOLD / "test.sync").read_text().splitlines()[:40]) + "\n")
    phen = d / "phen.py"
    phen.write_text(PHEN)
    return d, sync, phen


@pytest.fixture(scope="module")
def expected(inputs):
    """The restatement's rows per method: [(the six exact fields, alpha)]."""
    import oracle_lib
    o = oracle_lib.load()
    _, sync, _ = inputs
    bins, q, sig, mn, mx, _ = G.parse_gwalpha_fmt(PHEN)
    out = {}
    for method in ("LS", "ML"):
        rows = []
        for line in sync.read_text().splitlines():
            n, chrom, pos, cnt = o.parse_sync_line(line)
            if n <= 0:
                continue
            assert n == 5
            r = G.gwalpha_locus(o, cnt, bins, q, sig, mn, mx, o.filt(True, 1, 0.001, 0.0), method)
            for ln in (G.csv_lines(o, chrom, pos, r).splitlines() if r else []):
                f = ln.split(",")
                rows.append((f[:5] + f[6:], float(f[5])))
        out[method] = rows
    return out


@pytest.mark.parametrize("flag,method", [("LS", "LS"), ("ML", "ML"), ("simplex", "ML"), (None, "ML")])
def test_cli_gwalpha_matches_the_restatement(inputs, expected, flag, method):
    d, sync, phen = inputs
    out = d / f"out_{flag}.csv"
    extra = [] if flag is None else ["--gwalpha-method", flag]
    r = run_cli("gwalpha", "-f", sync, "-p", phen, "--phen-format", "gwalpha_fmt", "-o", out, "--n-threads", 2, *extra)
    assert r.stdout.strip().endswith(str(out))
    got = out.read_text().splitlines()
    want = expected[method]
    assert got[0] == HEADER and len(got) - 1 == len(want) >= 20
    worst = 0.0
    for a, (fields, alpha) in zip(got[1:], want):
        f = a.split(",")
        assert len(f) == 7 and f[:5] + f[6:] == fields, (a, fields)
        assert "e" not in f[5].lower()
        worst = max(worst, abs(float(f[5]) - alpha))
        assert abs(float(f[5]) - alpha) <= 2e-6, (a, alpha)
    print(f"gwalpha CSV --gwalpha-method {flag}: {len(want)} rows, worst |alpha - restatement| {worst:.3g}")
    run_cli("gwalpha", "-f", sync, "-p", phen, "--phen-format", "gwalpha_fmt", "-o", out, ok=False)   # an existing target is refused


def test_cli_gwalpha_refusals_and_default_name(inputs):
    d, sync, phen = inputs
    r = run_cli("gwalpha", "-f", sync, "-p", GOLD / "test.csv", "-o", d / "never.csv", ok=False)
    assert "--phen-format gwalpha_fmt" in r.stderr and not (d / "never.csv").exists()
    r = run_cli("gwalpha", "-f", sync, "-p", GOLD / "test.csv", "--phen-format", "default", "-o", d / "never.csv", ok=False)
    assert "--phen-format gwalpha_fmt" in r.stderr
    assert "Invalid phenotype format" in run_cli("gwalpha", "-f", sync, "-p", phen, "--phen-format", "csv", ok=False).stderr
    two = d / "two.py"
    two.write_text(G.gwalpha_fmt_text("t", 0.3, 0.0, 1.0, [0.5], [0.5]))
    assert "at least 3 pools" in run_cli("gwalpha", "-f", sync, "-p", two, "--phen-format", "gwalpha_fmt", ok=False).stderr
    assert "gwalpha" in run_cli("--help").stdout
    r = run_cli("gwalpha", "-f", sync, "-p", phen, "--phen-format=gwalpha_fmt")
    name = r.stdout.strip().splitlines()[-1]
    assert name.startswith(str(d / "forty-")) and name.endswith("-gwalpha.csv") and Path(name).read_text().startswith(HEADER)


def test_cli_gwalpha_pileup_input_equals_pileup2sync_then_gwalpha(inputs):
    import random
    from test_pileup import _random_line
    d, _, phen = inputs
    rng = random.Random(11)
    pile = d / "in.pileup"
    pile.write_text("\n".join(_random_line(rng, 5, False) for _ in range(400)) + "\n", encoding="latin-1")
    fmt = ["-p", phen, "--phen-format", "gwalpha_fmt"]
    sync = d / "conv.sync"
    run_cli("pileup2sync", "-f", pile, *fmt, "-o", sync, "--n-threads", 2)
    a, b = d / "from_sync.csv", d / "from_pileup.csv"
    run_cli("gwalpha", "-f", sync, *fmt, "-o", a, "--n-threads", 2)
    run_cli("gwalpha", "-f", pile, *fmt, "-o", b, "--n-threads", 2)
    assert a.read_bytes() == b.read_bytes() and a.read_text().count("\n") > 20


def test_cli_gwalpha_ranks_sharing_one_gpu_equal_one(inputs):
    """The rank machinery of the streamed path (one contiguous part per rank, concatenated in rank order) with the ranks on GPU 0."""
    d, sync, phen = inputs
    base = ["gwalpha", "-f", sync, "-p", phen, "--phen-format", "gwalpha_fmt", "--n-threads", 2]
    one, three = d / "rank1.csv", d / "rank3.csv"
    run_cli(*base, "-o", one)
    run_cli(*base, "-o", three, "--n-gpus", 3, "--gpu-ids", "0,0,0", env=dict(os.environ, PGH_COMM="host"))
    assert one.read_bytes() == three.read_bytes() and not list(d.glob("*.tmp"))


def test_cli_gwalpha_two_gpus_equal_one(inputs):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("--n-gpus 2 needs two visible devices; fewer than two are visible here")
    d, sync, phen = inputs
    base = ["gwalpha", "-f", sync, "-p", phen, "--phen-format", "gwalpha_fmt", "--n-threads", 2]
    one, two = d / "gpu1.csv", d / "gpu2.csv"
    run_cli(*base, "-o", one)
    run_cli(*base, "-o", two, "--n-gpus", 2)
    assert one.read_bytes() == two.read_bytes() and not list(d.glob("*.tmp"))
