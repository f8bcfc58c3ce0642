"""`poolgen fisher_exact_test` end to end (the reference's first CI invocations, .github/workflows/rust.yml:29-30) against the
restatement in tests/fisher_ref.py: header, row count, row order and the text of the label columns equal; the two numbers,
printed with the shortest round-trip formatter, parsed and within a relative 1e-10."""
import os
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

import fisher_ref

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
TOL = 1e-10


def run_cli(*args, ok=True, env=None):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.mark.parametrize("extra,min_cov,maf", [([], 1, 0.001),
                                               (["--min-coverage-depth", "10", "--min-allele-frequency", "0.01"], 10, 0.01)])
def test_cli_fisher_exact_test(oracle, tmp_path, extra, min_cov, maf):
    ps = np.loadtxt(GOLD / "test.csv", delimiter=",", comments="#", usecols=(1,))
    fo = oracle.filt(True, min_cov, maf, 0.0)
    want = []
    for line in (GOLD / "test.sync").read_text().splitlines():
        n, chrom, pos, cnt = oracle.parse_sync_line(line)
        if n <= 0:
            continue
        r = oracle.filter_locus(cnt, ps, fo)
        if r is None:
            continue
        ids, m = r
        want.append((chrom, str(pos), "".join("ATCGND"[i] for i in ids), fisher_ref.fisher(m)))
    out = tmp_path / "f.csv"
    r = run_cli("fisher_exact_test", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "--n-threads", 2, "-o", out, *extra)
    assert r.stdout.strip().endswith(str(out))
    got = out.read_text().splitlines()
    assert got[0] == "#chr,pos,alleles,statistic,pvalue"
    assert len(got) - 1 == len(want) > 500
    worst = 0.0
    for a, (chrom, pos, alleles, (po, pv)) in zip(got[1:], want):
        fa = a.split(",")
        assert len(fa) == 5 and fa[:3] == [chrom, pos, alleles], (a, chrom, pos, alleles)
        assert "e" not in fa[3].lower() and "e" not in fa[4].lower()           # Rust's Display never prints an exponent
        d = max(fisher_ref.rel(float(fa[3]), po), fisher_ref.rel(float(fa[4]), pv))
        assert d <= TOL, (a, po, pv, d)
        worst = max(worst, d)
    print(f"fisher_exact_test CSV {extra}: {len(want)} rows, worst relative deviation {worst:.3g}")
    run_cli("fisher_exact_test", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "-o", out, ok=False)   # create_new: an existing target is refused


def test_cli_fisher_default_output_name_and_help(tmp_path):
    shutil.copy(GOLD / "test.sync", tmp_path / "my.data.sync")
    r = run_cli("fisher_exact_test", "-f", tmp_path / "my.data.sync", "-p", GOLD / "test.csv")
    name = r.stdout.strip().splitlines()[-1]
    assert name.startswith(str(tmp_path / "my.data-")) and name.endswith("-fisher_exact_test.csv") and Path(name).exists()
    assert "fisher_exact_test" in run_cli("--help").stdout
    assert "fisher_exact_test" in run_cli("ridge_iter", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", ok=False).stderr   # the "available:" list


def test_cli_fisher_in_pieces_equals_one_piece(tmp_path):
    base = ["fisher_exact_test", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "--n-threads", 3, "--min-coverage-depth", 5]
    one, many = tmp_path / "one.csv", tmp_path / "many.csv"
    run_cli(*base, "-o", one)
    run_cli(*base, "-o", many, env={**os.environ, "PGH_STREAM_CHUNK_BYTES": "20000"})   # some 300 pieces for the fixture
    assert one.read_bytes() == many.read_bytes() and one.stat().st_size > 10000


def test_cli_fisher_pileup_input_equals_pileup2sync_then_analysis(tmp_path):
    import random
    from test_pileup import _random_line
    rng = random.Random(8)
    lines = [_random_line(rng, 5, False) for _ in range(3000)]
    pile = tmp_path / "in.pileup"
    pile.write_text("\n".join(lines) + "\n", encoding="latin-1")
    phen = GOLD / "test.csv"
    for tag, extra in (("", []), ("_ns", ["--keep-ns"])):
        sync = tmp_path / f"conv{tag}.sync"
        run_cli("pileup2sync", "-f", pile, "-p", phen, "-o", sync, "--n-threads", 3, *extra)
        a, b = tmp_path / f"sync{tag}.csv", tmp_path / f"pileup{tag}.csv"
        run_cli("fisher_exact_test", "-f", sync, "-p", phen, "-o", a, "--n-threads", 2, *extra)
        run_cli("fisher_exact_test", "-f", pile, "-p", phen, "-o", b, "--n-threads", 2, *extra)
        assert a.read_bytes() == b.read_bytes() and a.read_text().count("\n") > 100, tag


def test_cli_fisher_two_gpus_equal_one(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("--n-gpus 2 needs two visible devices; fewer than two are visible here")
    base = ["fisher_exact_test", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "--n-threads", 4]
    one, two = tmp_path / "one.csv", tmp_path / "two.csv"
    run_cli(*base, "-o", one)
    run_cli(*base, "-o", two, "--n-gpus", 2)
    assert one.read_bytes() == two.read_bytes() and one.stat().st_size > 10000
    assert not list(tmp_path.glob("*.tmp"))


def test_cli_fisher_ranks_sharing_one_gpu_equal_one(tmp_path):
    """The rank machinery (contiguous parts, one part file per rank, concatenated in rank order) with the ranks sharing GPU 0,
    as the sibling operators' multi-rank test runs it where one device is visible."""
    base = ["fisher_exact_test", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "--n-threads", 4]
    env = dict(os.environ, PGH_STREAM_CHUNK_BYTES="50000")
    one = tmp_path / "one.csv"
    run_cli(*base, "-o", one, env=env)
    for ranks, ids in ((2, "0,0"), (5, "0,0,0,0,0")):
        out = tmp_path / f"r{ranks}.csv"
        run_cli(*base, "-o", out, "--n-gpus", ranks, "--gpu-ids", ids, env=dict(env, PGH_COMM="host"))
        assert one.read_bytes() == out.read_bytes() and one.stat().st_size > 10000
        assert not list(tmp_path.glob("*.tmp"))
