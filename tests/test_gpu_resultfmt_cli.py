"""`poolgen <analysis> --result-writer gpu` end to end: for each of the seven GWAS analyses the file whose rows the GPU formatted is
byte for byte the file of the host writer (every statistic of the fixture is far below 2^53, where the two formatters agree), with
either sync parser, with a VCF and a pileup input, in pieces and with several ranks for the per-locus analyses, for any
--result-slab-rows on the kinship analyses; the refusals, and no file left behind by a run that fails."""
import os
import random
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gwalpha_ref as G

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
SYNC, PHEN = GOLD / "test.sync", GOLD / "test.csv"
GW_PHEN = G.gwalpha_fmt_text("trait", 0.3, 0.5, 6.5, [0.15, 0.4, 0.6, 0.85], [1.0, 2.5, 4.0, 6.0])
ANALYSES = {  # analysis -> its flags beside -f / -p
    "fisher_exact_test": [], "chisq_test": [], "pearson_corr": ["--phen-value-col", "2,3"], "ols_iter": ["--phen-value-col", "2,3"],
    "gwalpha": ["--phen-format", "gwalpha_fmt"], "ols_iter_with_kinship": ["--phen-value-col", "2,3", "-x", "0.5"],
    "mle_iter_with_kinship": ["--phen-value-col", "2,3", "-x", "0.5"],
}


def run(args, ok=True, env=None, cwd=None):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env, cwd=cwd)
    assert (r.returncode == 0) == ok, r.stderr
    return r


@pytest.fixture(scope="module")
def gw_phen(tmp_path_factory):
    p = tmp_path_factory.mktemp("resultfmt_cli") / "phen.py"
    p.write_text(GW_PHEN)
    return p


def base_args(analysis, gw_phen, fname=SYNC):
    return [analysis, "-f", fname, "-p", gw_phen if analysis == "gwalpha" else PHEN, "--n-threads", "3", *ANALYSES[analysis]]


@pytest.fixture(scope="module")
def host_files(tmp_path_factory, gw_phen):
    """the host writer's file per analysis, written once"""
    d = tmp_path_factory.mktemp("resultfmt_cli_host")
    out = {}
    for analysis in ANALYSES:
        f = d / f"{analysis}.csv"
        run([*base_args(analysis, gw_phen), "-o", f])
        out[analysis] = f.read_bytes()
        assert out[analysis].count(b"\n") > 1000, analysis
    return out


@pytest.mark.parametrize("parser", ["host", "gpu"])
@pytest.mark.parametrize("analysis", list(ANALYSES))
def test_gpu_writer_file_equals_host_writer_file(tmp_path, gw_phen, host_files, analysis, parser):
    out = tmp_path / "gpu.csv"
    r = run([*base_args(analysis, gw_phen), "-o", out, "--result-writer", "gpu", "--sync-parser", parser], env=dict(os.environ, PGH_TIMING="1"))
    assert r.stdout.strip().splitlines()[-1] == str(out)
    assert out.read_bytes() == host_files[analysis]
    assert "result writer on the GPU" in r.stderr and "format calls" in r.stderr and "D2H of the text" in r.stderr and "file writes" in r.stderr
    assert not list(tmp_path.glob("*.tmp"))


@pytest.mark.parametrize("analysis", ["ols_iter", "fisher_exact_test", "gwalpha"])
def test_pieces_and_ranks_do_not_change_the_file(tmp_path, gw_phen, host_files, analysis):
    """the text of every piece is appended to the rank's part file: pieces of 50 KB, then two and five ranks sharing GPU 0"""
    env = dict(os.environ, PGH_STREAM_CHUNK_BYTES="50000")
    for tag, extra, e in (("pieces", [], env), ("r2", ["--n-gpus", "2", "--gpu-ids", "0,0"], dict(env, PGH_COMM="host")),
                          ("r5", ["--n-gpus", "5", "--gpu-ids", "0,0,0,0,0"], dict(env, PGH_COMM="host"))):
        out = tmp_path / f"{tag}.csv"
        run([*base_args(analysis, gw_phen), "-o", out, "--result-writer", "gpu", *extra], env=e)
        assert out.read_bytes() == host_files[analysis], tag
        assert not list(tmp_path.glob("*.tmp"))


@pytest.mark.parametrize("analysis", ["ols_iter_with_kinship", "mle_iter_with_kinship"])
def test_result_slab_rows_do_not_change_the_file(tmp_path, analysis):
    """a row, seven rows and the default's worth per turn, on the first 400 loci (a turn is a call that synchronises)"""
    sync = tmp_path / "part.sync"
    sync.write_text("\n".join(SYNC.read_text().splitlines()[:400]) + "\n")
    host = tmp_path / "host.csv"
    run([*base_args(analysis, None, sync), "-o", host])
    assert host.read_bytes().count(b"\n") > 200
    for slab in ("1", "7", None):
        out = tmp_path / f"gpu{slab}.csv"
        run([*base_args(analysis, None, sync), "-o", out, "--result-writer", "gpu", *(["--result-slab-rows", slab] if slab else [])])
        assert out.read_bytes() == host.read_bytes(), slab


def test_streamed_kinship_path(tmp_path):
    """the input sorted by (chromosome, position) and taken in pieces: the coefficients stay on the device until the last piece, then
    the rows are formatted in their trait-major order -- the host writer's file, whatever --result-slab-rows"""
    lines = SYNC.read_text().splitlines()
    rows = [l.split("\t", 2) for l in lines if not l.startswith("#")]
    rows.sort(key=lambda f: (f[0], int(f[1])))
    sync = tmp_path / "sorted.sync"
    sync.write_text("".join(l + "\n" for l in lines if l.startswith("#")) + "".join("\t".join(f) + "\n" for f in rows))
    env = dict(os.environ, PGH_STREAM_CHUNK_BYTES="50000", PGH_TIMING="1")
    host = tmp_path / "host.csv"
    r = run([*base_args("ols_iter_with_kinship", None, sync), "-o", host], env=env)
    assert "partial kinship" in r.stderr                                       # the streamed path ran
    assert host.read_bytes().count(b"\n") > 1000
    for parser, slab in (("host", None), ("gpu", "1000"), ("host", "7777")):
        out = tmp_path / f"gpu_{parser}_{slab}.csv"
        r = run([*base_args("ols_iter_with_kinship", None, sync), "-o", out, "--result-writer", "gpu", "--sync-parser", parser,
                 *(["--result-slab-rows", slab] if slab else [])], env=env)
        assert "partial kinship" in r.stderr and "result writer on the GPU" in r.stderr
        assert out.read_bytes() == host.read_bytes(), (parser, slab)
    # unsorted input with the pieces forced: refused as before, and no file
    r = run([*base_args("ols_iter_with_kinship", None), "-o", tmp_path / "never.csv", "--result-writer", "gpu"], ok=False, env=env)
    assert "sorted" in r.stderr and not (tmp_path / "never.csv").exists()


def test_vcf_and_pileup_inputs(tmp_path):
    import pileup_corpus
    rng = np.random.default_rng(3)
    phen10 = tmp_path / "phen10.csv"
    phen10.write_text("#pop,size,trait1,trait2\n" + "".join(f"Pool{i},10.0,{rng.random():.6f},{rng.random():.6f}\n" for i in range(10)))
    r = random.Random(17)
    pile = tmp_path / "some.pileup"
    pile.write_bytes(b"".join(pileup_corpus.good_line(r, 5) + b"\n" for _ in range(600)))
    for tag, args in (("vcf_ols", ["ols_iter", "-f", GOLD / "test.vcf", "-p", phen10, "--phen-value-col", "2,3"]),
                      ("vcf_kin", ["ols_iter_with_kinship", "-f", GOLD / "test.vcf", "-p", phen10, "-x", "0.5"]),
                      ("pile_fisher", ["fisher_exact_test", "-f", pile, "-p", PHEN]),
                      ("pile_fisher_gpu_parser", ["fisher_exact_test", "-f", pile, "-p", PHEN, "--pileup-parser", "gpu"]),
                      ("pile_ols", ["ols_iter", "-f", pile, "-p", PHEN])):
        host, gpu = tmp_path / f"{tag}_host.csv", tmp_path / f"{tag}_gpu.csv"
        run([*args, "-o", host, "--n-threads", "2"])
        run([*args, "-o", gpu, "--n-threads", "2", "--result-writer", "gpu"])
        assert host.read_bytes() == gpu.read_bytes() and host.read_bytes().count(b"\n") > 20, tag


def test_existing_output_is_refused_and_a_failed_run_leaves_no_file(tmp_path):
    out = tmp_path / "there.csv"
    out.write_text("mine\n")
    for analysis in ("ols_iter", "ols_iter_with_kinship"):
        r = run([*base_args(analysis, None), "-o", out, "--result-writer", "gpu"], ok=False)
        assert out.read_text() == "mine\n" and r.stderr
    lines = SYNC.read_text().splitlines()
    lines[5000] = lines[5000].replace(":", ";", 1)                           # a broken count far behind the first pieces
    bad = tmp_path / "bad.sync"
    bad.write_text("\n".join(lines) + "\n")
    env = dict(os.environ, PGH_STREAM_CHUNK_BYTES="50000")
    for parser in ("host", "gpu"):
        for analysis in ("ols_iter", "fisher_exact_test", "ols_iter_with_kinship"):
            run([*base_args(analysis, None, bad), "-o", tmp_path / "never.csv", "--result-writer", "gpu", "--sync-parser", parser], ok=False, env=env)
            assert sorted(p.name for p in tmp_path.iterdir()) == ["bad.sync", "there.csv"], (parser, analysis)


def test_the_flag_is_refused_where_it_means_nothing(tmp_path, gw_phen):
    out = tmp_path / "x.csv"
    r = run(["ols_iter", "-f", SYNC, "-p", PHEN, "-o", out, "--result-writer", "nonsense"], ok=False)
    assert "Invalid value `nonsense` for --result-writer. Please select: 'host' or 'gpu'" in r.stderr
    for analysis in ("fst", "sync2csv", "heterozygosity", "genomic_prediction_cross_validation"):
        r = run([analysis, "-f", SYNC, "-p", PHEN, "-o", out, "--result-writer", "gpu"], ok=False)
        assert "--result-writer gpu applies to" in r.stderr and f"`{analysis}` writes none" in r.stderr
    for analysis in ("ols_iter_with_kinship", "mle_iter_with_kinship"):
        r = run([*base_args(analysis, None), "-o", out, "--result-writer", "gpu", "--n-gpus", "2", "--gpu-ids", "0,0"], ok=False)
        assert "takes one GPU" in r.stderr and "interleave" in r.stderr
    r = run(["ols_iter", "-f", SYNC, "-p", PHEN, "-o", out, "--result-slab-rows", "5"], ok=False)
    assert "--result-slab-rows needs --result-writer gpu" in r.stderr
    assert not out.exists()
    assert "--result-writer <host|gpu>" in run(["--help"]).stdout and "2^53" in run(["--help"]).stdout
