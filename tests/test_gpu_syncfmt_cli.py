"""The CLI with `--sync-writer gpu`: the sync lines of vcf2sync and of pileup2sync --pileup-parser gpu formatted on the GPU.  Every
file must be byte for byte the one `--sync-writer host` (the default) writes, whatever the slab size; an error on the way leaves
no file; the flag is refused where it means nothing."""
import os
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

import pileup_corpus

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"


def run(args, ok=True, env=None, cwd=None):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env, cwd=cwd)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def phen10(tmp_path_factory):
    """ten pools of equal size, two traits: the pools of tests/golden/test.vcf"""
    rng = np.random.default_rng(3)
    p = tmp_path_factory.mktemp("syncfmt_cli") / "phen10.csv"
    p.write_text("#pop,size,trait1,trait2\n" + "".join(f"Pool{i},10.0,{rng.random():.6f},{rng.random():.6f}\n" for i in range(10)))
    return p


@pytest.fixture(scope="module")
def pileup(tmp_path_factory):
    """600 sound lines of five pools (the fixture's phenotype file names five) from pileup_corpus' generator: about 90 KB"""
    rng = random.Random(17)
    p = tmp_path_factory.mktemp("syncfmt_cli_pileup") / "some.pileup"
    p.write_bytes(b"".join(pileup_corpus.good_line(rng, 5) + b"\n" for _ in range(600)))
    return p


def both_writers(tmp_path, args, env):
    """the conversion with --sync-writer host and with --sync-writer gpu -> (the host's file, the gpu's file, the gpu run)"""
    files = []
    for writer in ("host", "gpu"):
        out = tmp_path / f"{writer}.sync"
        r = run([*args, "-o", out, "--sync-writer", writer], env=env)
        assert r.stdout.strip() == str(out)
        files.append(out.read_bytes())
        loci = files[-1].count(b"\n") - 1
        assert f"\n{loci} loci written\n" in "\n" + r.stderr, r.stderr      # the loci count is still printed
    return files[0], files[1], r


@pytest.mark.parametrize("slab", [None, "5000"])                          # 5 000 bytes: some twenty slabs of the fixture
@pytest.mark.parametrize("extra", [[], ["--min-coverage-depth", "5", "--min-coverage-breadth", "0.5", "--min-allele-frequency", "0.05"]])
def test_vcf2sync(tmp_path, phen10, extra, slab):
    env = dict(os.environ, PGH_TIMING="1", **({"PGH_VCF_SLAB_BYTES": slab} if slab else {}))
    host, gpu, r = both_writers(tmp_path, ["vcf2sync", "-f", GOLD / "test.vcf", "-p", phen10, "--n-threads", "3", *extra], env)
    assert gpu == host and host.count(b"\n") > 100 and host.startswith(b"#chr\tpos\tref\t")
    assert "sync writer on the GPU" in r.stderr                           # the flag reaches the writer
    if not extra:
        import vcf_ref
        assert gpu == vcf_ref.vcf2sync_bytes((GOLD / "test.vcf").read_bytes(), [0.1] * 10)


def test_vcf2sync_pool_names_behind_the_first_lines(tmp_path, phen10):
    """The header takes the names of the LAST "#CHROM" line (vcf.rs:343-359), which may follow data lines that have been written by
    then: the file is still the host writer's."""
    text = (GOLD / "test.vcf").read_bytes()
    lines = text.splitlines(keepends=True)
    chrom = next(l for l in lines if l.startswith(b"#CHROM"))
    renamed = b"\t".join(chrom.rstrip(b"\n").split(b"\t")[:9] + [b"late%d" % i for i in range(10)]) + b"\n"
    vcf = tmp_path / "late.vcf"
    vcf.write_bytes(text + renamed)
    env = dict(os.environ, PGH_VCF_SLAB_BYTES="5000")
    host, gpu, _ = both_writers(tmp_path, ["vcf2sync", "-f", vcf, "-p", phen10], env)
    assert gpu == host and host.startswith(b"#chr\tpos\tref\tlate0\tlate1\t") and host.count(b"\n") > 100
    assert sorted(p.name for p in tmp_path.iterdir()) == ["gpu.sync", "host.sync", "late.vcf"]


@pytest.mark.parametrize("slab", [None, "20000"])                         # 20 000 bytes: five slabs
@pytest.mark.parametrize("extra", [[], ["--min-allele-frequency", "0.0", "--keep-ns"]])
def test_pileup2sync(tmp_path, pileup, extra, slab):
    env = dict(os.environ, **({"PGH_PILEUP_SLAB_BYTES": slab} if slab else {}))
    assert slab is None or pileup.stat().st_size > 3 * int(slab)
    args = ["pileup2sync", "-f", pileup, "-p", GOLD / "test.csv", "--pileup-parser", "gpu", "--n-threads", "3", *extra]
    host, gpu, _ = both_writers(tmp_path, args, env)
    assert gpu == host and host.count(b"\n") > 100 and host.startswith(b"#chr\tpos\tref\tG1\tG2\tG3\tG4\tG5\n")
    out = tmp_path / "default.sync"                                       # and both are the default's (the host parser, the host writer)
    run(["pileup2sync", "-f", pileup, "-p", GOLD / "test.csv", "-o", out, *extra])
    assert out.read_bytes() == host


def test_broken_line_gives_the_same_message_and_leaves_no_file(tmp_path, phen10, pileup):
    """The bad line lies in a late slab: sync lines have been written by then, and the file goes again."""
    text = (GOLD / "test.vcf").read_bytes()
    bad = tmp_path / "bad.vcf"
    bad.write_bytes(text + b"chrZ\t500\t.\tA\tT\t50\t.\tDP=9\tGT:AD" + b"\t0/1:3,." * 10 + b"\n")
    env = dict(os.environ, PGH_VCF_SLAB_BYTES="5000")
    msgs = []
    for writer in ("host", "gpu"):
        r = run(["vcf2sync", "-f", bad, "-p", phen10, "-o", tmp_path / "out.sync", "--sync-writer", writer], ok=False, env=env)
        line = text.count(b"\n") + 1
        assert "Input file error" in r.stderr and f"at line {line} " in r.stderr and "chrZ\t500" in r.stderr, r.stderr
        assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.vcf"], writer      # no output file, nothing else left
        msgs.append(r.stderr)
    assert msgs[0] == msgs[1]
    good = pileup.read_bytes()
    badp = tmp_path / "bad.pileup"
    badp.write_bytes(good + b"chr9\t77\tA" + b"\t2\t.+xA\tII" * 5 + b"\n")
    env = dict(os.environ, PGH_PILEUP_SLAB_BYTES="20000")
    msgs = []
    for writer in ("host", "gpu"):
        r = run(["pileup2sync", "-f", badp, "-p", GOLD / "test.csv", "-o", tmp_path / "out.sync", "--pileup-parser", "gpu", "--sync-writer", writer],
                ok=False, env=env)
        line = good.count(b"\n") + 1
        assert f"at line {line}," in r.stderr and "chr9\t77" in r.stderr, r.stderr
        assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.pileup", "bad.vcf"], writer
        msgs.append(r.stderr)
    assert msgs[0] == msgs[1]


def test_existing_output_is_refused_and_untouched(tmp_path, phen10, pileup):
    out = tmp_path / "there.sync"
    out.write_bytes(b"mine\n")
    r = run(["vcf2sync", "-f", GOLD / "test.vcf", "-p", phen10, "-o", out, "--sync-writer", "gpu"], ok=False)
    assert "Unable to create file" in r.stderr and out.read_bytes() == b"mine\n"
    r = run(["pileup2sync", "-f", pileup, "-p", GOLD / "test.csv", "-o", out, "--pileup-parser", "gpu", "--sync-writer", "gpu"], ok=False)
    assert "Unable to create file" in r.stderr and out.read_bytes() == b"mine\n"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["there.sync"]


def test_refusals_name_the_flag(tmp_path, phen10, pileup):
    out = tmp_path / "x.sync"
    r = run(["pileup2sync", "-f", pileup, "-p", GOLD / "test.csv", "-o", out, "--sync-writer", "gpu"], ok=False)
    assert "--sync-writer gpu" in r.stderr and "--pileup-parser gpu" in r.stderr                 # names the missing flag
    r = run(["pileup2sync", "-f", pileup, "-p", GOLD / "test.csv", "-o", out, "--pileup-parser", "host", "--sync-writer", "gpu"], ok=False)
    assert "--sync-writer gpu" in r.stderr and "--pileup-parser gpu" in r.stderr
    r = run(["ols_iter", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "-o", tmp_path / "x.csv", "--sync-writer", "gpu"], ok=False)
    assert "--sync-writer gpu" in r.stderr and "ols_iter" in r.stderr
    r = run(["vcf2sync", "-f", GOLD / "test.vcf", "-p", phen10, "-o", out, "--sync-writer", "nonsense"], ok=False)
    assert "`nonsense`" in r.stderr and "--sync-writer" in r.stderr
    r = run(["ols_iter", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "-o", tmp_path / "x.csv", "--sync-writer", "nonsense"], ok=False)
    assert "`nonsense`" in r.stderr and "--sync-writer" in r.stderr
    assert sorted(p.name for p in tmp_path.iterdir()) == []
    assert "--sync-writer <host|gpu>" in run(["--help"]).stdout
    run(["ols_iter", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "-o", tmp_path / "x.csv", "--sync-writer", "host"])   # the default, spelled out
    assert (tmp_path / "x.csv").stat().st_size > 100
