"""The CLI with `--pileup-parser gpu`: the mpileup text parsed on the GPU.  Every output file must be byte for byte the default's
(the host parser's), on inputs taken in several pieces and several slabs."""
import os
import random
import subprocess
from pathlib import Path

import pytest

from test_pileup import _random_line

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
PIECES = dict(os.environ, PGH_STREAM_CHUNK_BYTES="50000", PGH_PILEUP_SLAB_BYTES="20000")     # half a dozen pieces of two or three slabs


def run(args, ok=True, env=PIECES):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def pileup(tmp_path_factory):
    """3 000 lines of five pools (the fixture's phenotype file names five) in (chromosome, position) order, as the streamed
    kinship path needs it; one line in a hundred has a pool too many and is dropped"""
    rng = random.Random(5)
    lines = {}
    while len(lines) < 3000:
        l = _random_line(rng, 5 if rng.random() > 0.01 else 6, False)
        f = l.split("\t")
        lines[(f[0].encode(), int(f[1]))] = l
    p = tmp_path_factory.mktemp("pileup_cli") / "sorted.pileup"
    p.write_text("\n".join(lines[k] for k in sorted(lines)) + "\n", encoding="latin-1")
    assert p.stat().st_size > 250_000
    return p


def both_parsers(tmp_path, analysis, pileup, extra, suffix="csv"):
    """the analysis with the default parser and with --pileup-parser gpu: the files each run left, name -> bytes"""
    outs = []
    for tag, flag in (("host", []), ("gpu", ["--pileup-parser", "gpu"])):
        d = tmp_path / tag
        d.mkdir()
        run([analysis, "-f", pileup, "-p", GOLD / "test.csv", "-o", d / f"out.{suffix}", "--n-threads", "3", *extra, *flag])
        outs.append({p.name: p.read_bytes() for p in sorted(d.iterdir())})
    return outs


CASES = {
    "pileup2sync": ("pileup2sync", ["--min-allele-frequency", "0.0"], "sync"),
    "pileup2sync_keep_lowercase": ("pileup2sync", ["--keep-lowercase-reference", "--keep-ns", "--max-base-error-rate", "0.005"], "sync"),
    "chisq_test": ("chisq_test", [], "csv"),
    "ols_iter": ("ols_iter", ["--phen-value-col", "2,3"], "csv"),
    "sync2csv": ("sync2csv", ["--phen-value-col", "2,3"], "csv"),
    "ols_iter_with_kinship_streamed": ("ols_iter_with_kinship", ["--phen-value-col", "2,3", "-x", "0.5"], "csv"),
    "chisq_test_two_ranks": ("chisq_test", ["--n-gpus", "2", "--gpu-ids", "0,0"], "csv"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_parser_gives_the_same_bytes(tmp_path, pileup, case):
    analysis, extra, suffix = CASES[case]
    host, gpu = both_parsers(tmp_path, analysis, pileup, extra, suffix)
    assert sorted(host) == sorted(gpu) and len(host) >= 1
    for name in host:
        assert host[name] == gpu[name], name
        assert host[name].count(b"\n") > 100, name


def test_pileup2sync_header_default_name_and_overwrite(tmp_path, pileup):
    r = subprocess.run([str(CLI), "pileup2sync", "-f", str(pileup), "-p", str(GOLD / "test.csv"), "--pileup-parser", "gpu"], capture_output=True, text=True,
                       cwd=tmp_path, env=PIECES)
    assert r.returncode == 0, r.stderr
    out = Path(r.stdout.strip())
    assert out.name.startswith("sorted-") and out.suffix == ".sync"
    lines = out.read_text(encoding="latin-1").splitlines()
    assert lines[0] == "#chr\tpos\tref\tG1\tG2\tG3\tG4\tG5" and r.stderr.strip().endswith(f"{len(lines) - 1} loci written")
    before = out.read_bytes()
    r = run(["pileup2sync", "-f", pileup, "-p", GOLD / "test.csv", "-o", out, "--pileup-parser", "gpu"], ok=False)
    assert "Unable to create file" in r.stderr and out.read_bytes() == before            # refused before any work, nothing touched


def test_broken_line_names_the_line_and_leaves_nothing(tmp_path, pileup):
    good = pileup.read_bytes()
    cut = good.index(b"\n", 200_000) + 1                              # in a later piece
    bad = good[:cut] + b"chr9\t77\tA" + b"\t2\t.+xA\tII" * 5 + b"\n" + good[cut:]
    p = tmp_path / "bad.pileup"
    p.write_bytes(bad)
    line = bad[:cut].count(b"\n") + 1
    for analysis, extra in (("chisq_test", []), ("sync2csv", ["--phen-value-col", "2,3"]), ("chisq_test", ["--n-gpus", "2", "--gpu-ids", "0,0"]),
                            ("pileup2sync", [])):
        r = run([analysis, "-f", p, "-p", GOLD / "test.csv", "-o", tmp_path / "out.csv", "--pileup-parser", "gpu", *extra], ok=False)
        assert f"at line {line}," in r.stderr and "chr9\t77" in r.stderr and "insertions and deletion" in r.stderr, r.stderr
        assert sorted(x.name for x in tmp_path.iterdir()) == ["bad.pileup"], analysis       # no output file, no *.tmp


def test_refusals(tmp_path, pileup):
    base = ["-p", GOLD / "test.csv", "-o", tmp_path / "x.csv"]
    r = run(["chisq_test", "-f", GOLD / "test.sync", *base, "--pileup-parser", "gpu"], ok=False)
    assert "--pileup-parser gpu" in r.stderr and "*.pileup" in r.stderr
    r = run(["vcf2sync", "-f", GOLD / "test.vcf", *base, "--pileup-parser", "gpu"], ok=False)
    assert "--pileup-parser gpu" in r.stderr
    r = run(["chisq_test", "-f", pileup, *base, "--pileup-parser", "fast"], ok=False)
    assert "`fast`" in r.stderr and "--pileup-parser" in r.stderr
    r = run(["chisq_test", "-f", pileup, *base, "--sync-parser", "gpu"], ok=False)             # stays refused
    assert "--sync-parser gpu" in r.stderr and "*.sync" in r.stderr
    assert not (tmp_path / "x.csv").exists()
    assert "--pileup-parser <host|gpu>" in run(["--help"]).stdout
    r = run(["chisq_test", "-f", pileup, *base, "--pileup-parser", "host"], env=dict(PIECES, PGH_TIMING="1"))
    assert (tmp_path / "x.csv").stat().st_size > 1000 and "pileup reader on GPU" not in r.stderr
    r = run(["chisq_test", "-f", pileup, "-p", GOLD / "test.csv", "-o", tmp_path / "y.csv", "--pileup-parser", "gpu"], env=dict(PIECES, PGH_TIMING="1"))
    assert "pileup reader on GPU 0" in r.stderr                                               # the flag reaches the reader
