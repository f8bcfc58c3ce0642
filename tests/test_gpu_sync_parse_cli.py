"""The CLI with `--sync-parser gpu`: the sync text parsed on the GPU, the counts kept there for the operators.  Every output
file must be byte for byte the default's (the host parser's), on inputs taken in several pieces."""
import os
import subprocess
from pathlib import Path

import pytest

import sync_corpus

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
PIECES = dict(os.environ, PGH_STREAM_CHUNK_BYTES="50000", PGH_SYNC_SLAB_BYTES="70000")     # a dozen pieces, nine slabs of the fixture


def run(args, ok=True, env=PIECES):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def sorted_sync(tmp_path_factory):
    """the fixture in (chromosome, position) order, as the streamed kinship path needs it"""
    lines = [l for l in (GOLD / "test.sync").read_text().splitlines() if not l.startswith("#")]
    lines.sort(key=lambda l: (l.split("\t")[0].encode(), int(l.split("\t")[1])))
    p = tmp_path_factory.mktemp("sync_cli") / "sorted.sync"
    p.write_text("\n".join(lines) + "\n")
    return p


@pytest.fixture(scope="module")
def phen_missing(tmp_path_factory):
    """the fixture's phenotypes with one value missing: ols_iter drops that pool on the host"""
    rows = (GOLD / "test.csv").read_text().splitlines()
    cells = rows[2].split(",")
    cells[2] = "NA"
    rows[2] = ",".join(cells)
    p = tmp_path_factory.mktemp("sync_cli_phen") / "missing.csv"
    p.write_text("\n".join(rows) + "\n")
    return p


def both_parsers(tmp_path, analysis, sync, phen, extra):
    """the analysis with the default parser and with --sync-parser gpu: the files each run left, name -> bytes"""
    outs = []
    for tag, flag in (("host", []), ("gpu", ["--sync-parser", "gpu"])):
        d = tmp_path / tag
        d.mkdir()
        run([analysis, "-f", sync, "-p", phen, "-o", d / "out.csv", "--n-threads", "3", *extra, *flag])
        outs.append({p.name: p.read_bytes() for p in sorted(d.iterdir())})
    return outs


WINDOWS = ["--window-size-bp", "1000000", "--min-loci-per-window", "1"]
CASES = {
    "chisq_test": ("chisq_test", ["--min-coverage-depth", "5"], False, False),
    "fisher_exact_test": ("fisher_exact_test", [], False, False),
    "pearson_corr": ("pearson_corr", ["--phen-value-col", "2,3"], False, False),
    "ols_iter": ("ols_iter", ["--phen-value-col", "2,3"], False, False),
    "ols_iter_missing_phenotype": ("ols_iter", ["--phen-value-col", "2,3"], False, True),
    "ols_iter_with_kinship_streamed": ("ols_iter_with_kinship", ["--phen-value-col", "2,3", "-x", "0.5"], True, False),
    "ols_iter_with_kinship_whole_file": ("ols_iter_with_kinship", ["--phen-value-col", "2,3", "-x", "0.5", "--stream-chunk-mb", "0"], True, False),
    "sync2csv": ("sync2csv", ["--phen-value-col", "2,3"], False, False),
    "fst": ("fst", WINDOWS + ["--min-coverage-depth", "5", "--min-allele-frequency", "0.1", "--keep-ns"], False, False),
    "chisq_test_two_ranks": ("chisq_test", ["--n-gpus", "2", "--gpu-ids", "0,0"], False, False),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_gpu_parser_gives_the_same_bytes(tmp_path, sorted_sync, phen_missing, case):
    analysis, extra, needs_sorted, missing = CASES[case]
    host, gpu = both_parsers(tmp_path, analysis, sorted_sync if needs_sorted else GOLD / "test.sync", phen_missing if missing else GOLD / "test.csv", extra)
    assert sorted(host) == sorted(gpu) and len(host) >= 1
    for name in host:
        assert host[name] == gpu[name], name
        assert host[name].count(b"\n") > 3, name


def test_broken_sync_names_the_line_and_leaves_nothing(tmp_path):
    good = (GOLD / "test.sync").read_bytes()
    cut = good.index(b"\n", 200_000) + 1                              # in a later piece
    bad = good[:cut] + b"Chromosome1\t77\tC\t0:0:4:0:0:0\t0:1:2:0:0:0\t0:2:x:0:0:0\t0:1:4:0:0:0\t0:1:6:0:0:0\n" + good[cut:]
    sync = tmp_path / "bad.sync"
    sync.write_bytes(bad)
    line = bad[:cut].count(b"\n") + 1
    for analysis, extra in (("chisq_test", []), ("sync2csv", ["--phen-value-col", "2,3"]), ("chisq_test", ["--n-gpus", "2", "--gpu-ids", "0,0"])):
        r = run([analysis, "-f", sync, "-p", GOLD / "test.csv", "-o", tmp_path / "out.csv", "--sync-parser", "gpu", *extra], ok=False)
        assert f"at line {line}," in r.stderr and "Chromosome1\t77" in r.stderr and "not valid integers" in r.stderr, r.stderr
        assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.sync"], analysis       # no output file, no *.tmp
    text, n, off, reason = sync_corpus.error_texts()["one_pool_more"]
    sync.write_bytes(text)
    r = run(["chisq_test", "-f", sync, "-p", GOLD / "test.csv", "-o", tmp_path / "out.csv", "--sync-parser", "gpu"], ok=False)
    assert "at line 2," in r.stderr and "number of pools" in r.stderr


def test_refusals(tmp_path):
    base = ["-p", GOLD / "test.csv", "-o", tmp_path / "x.csv"]
    r = run(["chisq_test", "-f", GOLD / "test.vcf", *base, "--sync-parser", "gpu"], ok=False)
    assert "--sync-parser gpu" in r.stderr and "*.sync" in r.stderr
    r = run(["vcf2sync", "-f", GOLD / "test.vcf", *base, "--sync-parser", "gpu"], ok=False)
    assert "--sync-parser gpu" in r.stderr
    r = run(["chisq_test", "-f", GOLD / "test.sync", *base, "--sync-parser", "fast"], ok=False)
    assert "`fast`" in r.stderr and "--sync-parser" in r.stderr
    assert not (tmp_path / "x.csv").exists()
    assert "--sync-parser <host|gpu>" in run(["--help"]).stdout
    r = run(["chisq_test", "-f", GOLD / "test.sync", *base, "--sync-parser", "host"], env=dict(PIECES, PGH_TIMING="1"))
    assert (tmp_path / "x.csv").stat().st_size > 1000 and "sync reader on GPU" not in r.stderr
    r = run(["chisq_test", "-f", GOLD / "test.sync", "-p", GOLD / "test.csv", "-o", tmp_path / "y.csv", "--sync-parser", "gpu"], env=dict(PIECES, PGH_TIMING="1"))
    assert "sync reader on GPU 0" in r.stderr                                                 # the flag reaches the reader
