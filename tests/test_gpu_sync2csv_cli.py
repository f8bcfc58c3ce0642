"""`poolgen sync2csv` (FileSyncPhen::write_csv, base/sync.rs:1182-1262): the reference's two CI invocations on the golden
fixture against the oracle composition, byte for byte; slab sizes, names and refusals, pileup input, a missing phenotype."""
import random
import re
import subprocess
from pathlib import Path

import pytest

import csv_expect as E

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden"
EXE = ROOT / "poolgen_amd" / "csrc" / "poolgen"
CI = ["--phen-delim", ",", "--phen-name-col", "0", "--phen-value-col", "2,3", "--n-threads", "2"]   # .github/workflows/rust.yml:41-42


def run(args, **kw):
    return subprocess.run([str(EXE)] + [str(a) for a in args], capture_output=True, text=True, **kw)


@pytest.mark.parametrize("kpm1", [False, True])
def test_ci_invocations_and_slab_sizes(oracle, tmp_path, kpm1):
    want = E.golden_text(oracle, kpm1)
    assert want.count(b"\n") == 1 + E.GOLDEN_ROWS[kpm1]
    assert want.startswith(b"#chr,pos,allele,G1,G2,G3,G4,G5\n")
    if not kpm1:
        assert want.split(b"\n")[1] == b"Chromosome1,456527,T,0,0.333333,0.333333,0.2,0.142857"
    for tag, extra in (("default", []), ("one", ["--csv-slab-rows", "1"] if kpm1 else ["--csv-slab-rows=1"]), ("odd", ["--csv-slab-rows", "97"])):
        out = tmp_path / f"{tag}.csv"
        r = run(["sync2csv", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "-o", out] + CI + (["--keep-p-minus-1"] if kpm1 else []) + extra)
        assert r.returncode == 0, r.stderr
        assert r.stdout.strip() == str(out)
        assert out.read_bytes() == want, tag


def test_names_and_refusals(tmp_path):
    sync = tmp_path / "my.data.sync"
    sync.write_bytes((GOLD / "test.sync").read_bytes()[:20000].rsplit(b"\n", 1)[0] + b"\n")
    r = run(["sync2csv", "-f", sync, "-p", GOLD / "test.csv"] + CI)
    assert r.returncode == 0, r.stderr
    name = r.stdout.strip()
    assert re.fullmatch(re.escape(str(tmp_path / "my.data")) + r"-\d+(\.\d+)?-allele_frequencies\.csv", name), name   # sync.rs:1191-1211
    assert Path(name).read_bytes().startswith(b"#chr,pos,allele,G1,G2,G3,G4,G5\nChromosome1,456527,T,")
    before = Path(name).read_bytes()
    r = run(["sync2csv", "-f", sync, "-p", GOLD / "test.csv", "-o", name] + CI)                        # an existing target is refused
    assert r.returncode == 1 and "must not exist" in r.stderr and Path(name).read_bytes() == before
    r = run(["sync2csv", "-f", sync, "-p", GOLD / "test.csv", "-o", tmp_path / "two.csv", "--n-gpus", "2"] + CI)
    assert r.returncode == 1 and "--n-gpus" in r.stderr and "sync2csv" in r.stderr and not (tmp_path / "two.csv").exists()
    r = run(["sync2csv", "-f", sync, "-p", GOLD / "test.csv", "-o", tmp_path / "one.csv", "--n-gpus", "1"] + CI)   # one GPU is what it runs on
    assert r.returncode == 0 and (tmp_path / "one.csv").read_bytes() == before, r.stderr
    assert "sync2csv" in run(["--help"]).stdout and "--csv-slab-rows" in run(["--help"]).stdout
    r = run(["no_such_tool", "-f", sync, "-p", GOLD / "test.csv"])
    assert r.returncode == 1 and "sync2csv" in r.stderr and "watterson_estimator, tajima_d" in r.stderr
    # a filter nothing passes: an error, and no file (sync.rs:1220)
    r = run(["sync2csv", "-f", sync, "-p", GOLD / "test.csv", "-o", tmp_path / "none.csv", "--min-coverage-depth", "100000"] + CI)
    assert r.returncode == 1 and "No data passed the filtering variables" in r.stderr and not (tmp_path / "none.csv").exists()


def test_pileup_input_equals_pileup2sync_then_sync2csv(tmp_path):
    from test_pileup import _random_line
    rng = random.Random(5)
    lines = [_random_line(rng, 5, False) for _ in range(3000)]
    pile = tmp_path / "in.pileup"; pile.write_text("\n".join(lines) + "\n", encoding="latin-1")
    phen = GOLD / "test.csv"
    sync = tmp_path / "conv.sync"
    assert run(["pileup2sync", "-f", pile, "-p", phen, "-o", sync, "--n-threads", "3"]).returncode == 0
    assert sync.read_text().count("\n") > 300
    a, b = tmp_path / "from_sync.csv", tmp_path / "from_pileup.csv"
    for src, dst in ((sync, a), (pile, b)):
        r = run(["sync2csv", "-f", src, "-p", phen, "-o", dst, "--n-threads", "3", "--csv-slab-rows", "500"])
        assert r.returncode == 0, r.stderr
    assert a.read_bytes() == b.read_bytes() and a.read_bytes().count(b"\n") > 300


def test_a_missing_phenotype_keeps_the_pool(oracle, tmp_path):
    """write_csv names self.pool_names (sync.rs:1222, :1236): a pool without phenotype stays in the table."""
    phen = tmp_path / "na.csv"
    text = (GOLD / "test.csv").read_text().replace("G3,20,0.5,49.8", "G3,20,NA,49.8")
    assert "NA" in text
    phen.write_text(text)
    out = tmp_path / "na_out.csv"
    r = run(["sync2csv", "-f", GOLD / "test.sync", "-p", phen, "-o", out] + CI)
    assert r.returncode == 0, r.stderr
    assert out.read_bytes() == E.golden_text(oracle, False)
