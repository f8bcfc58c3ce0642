"""`poolgen <analysis> --popgen-writer gpu` end to end on the golden fixture: for fst, heterozygosity, watterson_estimator, tajima_d
and gudmc -- by default and, where the flag applies, with --popgen-as-documented -- the file or files whose text the GPU formatted
are byte for byte the host writer's (every value of the fixture is far below 2^53, where the two formatters agree), for any
--popgen-slab-rows; fst starved of windows; the refusals; no file left behind by a run that fails."""
import os
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "poolgen_amd" / "csrc" / "poolgen"
GOLD = Path(__file__).parent / "golden"
SYNC, PHEN = GOLD / "test.sync", GOLD / "test.csv"
WINDOWS = {"fst": (2000, 1000, 5), "heterozygosity": (2000, 1000, 5), "watterson_estimator": (2000, 1000, 5), "tajima_d": (2000, 1000, 5),
           "gudmc": (100, 50, 20)}                                                        # gudmc: the reference's own test parameters, one stale window
CASES = [("fst", False), ("heterozygosity", False), ("watterson_estimator", False), ("watterson_estimator", True), ("tajima_d", False),
         ("tajima_d", True), ("gudmc", False), ("gudmc", True)]
FIVE = "fst, heterozygosity, watterson_estimator, tajima_d and gudmc"


def run(args, ok=True, env=None):
    r = subprocess.run([str(CLI), *map(str, args)], capture_output=True, text=True, env=env)
    assert (r.returncode == 0) == ok, r.stderr
    return r


def base_args(analysis, documented=False, minl=None):
    win, slide, m = WINDOWS[analysis]
    return [analysis, "-f", SYNC, "-p", PHEN, "--phen-value-col", "2,3", "--n-threads", "2", "--window-size-bp", win, "--window-slide-size-bp", slide,
            "--min-loci-per-window", m if minl is None else minl, *(["--popgen-as-documented"] if documented else [])]


def files_of(d, analysis, stem):
    """the bytes of every file the run wrote, by name"""
    names = [f"{stem}.csv"] + ([f"{stem}-fst-{WINDOWS['fst'][0]}_bp_windows.csv"] if analysis == "fst" else [])
    assert sorted(p.name for p in d.iterdir() if p.name.startswith(stem)) == sorted(names)
    return [(d / n).read_bytes() for n in names]


@pytest.fixture(scope="module")
def host_files(tmp_path_factory):
    """the host writer's files per case, written once"""
    d = tmp_path_factory.mktemp("popgen_writer_host")
    out = {}
    for analysis, documented in CASES:
        stem = f"{analysis}_{int(documented)}"
        run([*base_args(analysis, documented), "-o", d / f"{stem}.csv"])
        out[analysis, documented] = files_of(d, analysis, stem)
    assert out["gudmc", False][0].count(b"\n") == 1 and out["gudmc", True][0].count(b"\n") > 50      # the header alone; rows
    assert all(f.count(b"\n") >= 6 for key, files in out.items() if key[0] != "gudmc" for f in files)   # a header and a line per pool or window
    assert out["fst", False][1].count(b"\n") > 6
    return out


@pytest.mark.parametrize("analysis,documented", CASES)
def test_gpu_writer_files_equal_host_writer_files(tmp_path, host_files, analysis, documented):
    want = host_files[analysis, documented]
    for tag, extra in (("d", []), ("s1", ["--popgen-slab-rows", "1"]), ("s7", ["--popgen-slab-rows", "7"])):
        r = run([*base_args(analysis, documented), "-o", tmp_path / f"{tag}.csv", "--popgen-writer", "gpu", *extra], env=dict(os.environ, PGH_TIMING="1"))
        got = files_of(tmp_path, analysis, tag)
        for g, w in zip(got, want):
            assert g.count(b"\n") >= w.count(b"\n") >= 1                                  # the floor is the host file's: an empty file cannot pass
            assert g == w, (analysis, documented, tag)
        assert str(tmp_path / f"{tag}.csv") in r.stdout.strip().splitlines()[-1]
        if analysis != "gudmc" or documented:
            assert "popgen writer on the GPU" in r.stderr and "format calls" in r.stderr and "D2H of the text" in r.stderr
    run([*base_args(analysis, documented), "-o", tmp_path / "h.csv", "--popgen-writer", "host"])     # the default, spelled out
    assert files_of(tmp_path, analysis, "h") == want


def test_fst_starved_of_windows_behaves_as_the_host_writer_does(tmp_path, host_files):
    """define_sliding_windows keeps its last slot whatever --min-loci-per-window says, so a non-empty input always has a window
    and the CLI cannot reach fst's "no windows" error (the genome-wide file is written before it in both writers' code).  What can
    be run is the most window-starved call: one window, and both writers doing the same."""
    seen = {}
    for writer in ("host", "gpu"):
        out = tmp_path / f"{writer}.csv"
        r = subprocess.run([str(CLI), *map(str, [*base_args("fst", minl=100000), "-o", out, "--popgen-writer", writer])], capture_output=True, text=True)
        seen[writer] = (r.returncode, r.stderr.replace(writer, "W"), files_of(tmp_path, "fst", writer))
    assert seen["gpu"] == seen["host"]
    assert seen["host"][2][0] == host_files["fst", False][0] and seen["host"][2][1].count(b"\n") == 2      # the same means; a header and one window


def test_existing_output_is_refused_and_a_failed_run_leaves_no_file(tmp_path):
    out = tmp_path / "there.csv"
    out.write_text("mine\n")
    for analysis, documented in CASES:
        r = run([*base_args(analysis, documented), "-o", out, "--popgen-writer", "gpu"], ok=False)
        assert "Unable to create file" in r.stderr and out.read_text() == "mine\n"
    assert sorted(p.name for p in tmp_path.iterdir()) == ["there.csv"]
    # --keep-p-minus-1 trips fst's sum-to-one check: neither of its two files is left
    r = run([*base_args("fst"), "--keep-p-minus-1", "-o", tmp_path / "never.csv", "--popgen-writer", "gpu"], ok=False)
    assert "do not sum up to one" in r.stderr and sorted(p.name for p in tmp_path.iterdir()) == ["there.csv"]


def test_the_flags_are_refused_where_they_mean_nothing(tmp_path):
    out = tmp_path / "x.csv"
    r = run(["fst", "-f", SYNC, "-p", PHEN, "-o", out, "--popgen-writer", "nonsense"], ok=False)
    assert "Invalid value `nonsense` for --popgen-writer" in r.stderr and FIVE in r.stderr and "'host' or 'gpu'" in r.stderr
    for analysis in ("ols_iter", "sync2csv", "fisher_exact_test", "genomic_prediction_cross_validation"):
        r = run([analysis, "-f", SYNC, "-p", PHEN, "-o", out, "--popgen-writer", "gpu"], ok=False)
        assert "--popgen-writer gpu applies to " + FIVE in r.stderr and f"`{analysis}` writes none" in r.stderr
    r = run(["fst", "-f", SYNC, "-p", PHEN, "-o", out, "--popgen-slab-rows", "5"], ok=False)
    assert "--popgen-slab-rows needs --popgen-writer gpu" in r.stderr
    r = run(["ols_iter", "-f", SYNC, "-p", PHEN, "-o", out, "--popgen-slab-rows", "5"], ok=False)
    assert FIVE in r.stderr
    for analysis in ("fst", "heterozygosity"):                                            # --result-writer gpu stays refused on them, as before
        r = run([analysis, "-f", SYNC, "-p", PHEN, "-o", out, "--result-writer", "gpu", "--popgen-writer", "gpu"], ok=False)
        assert "--result-writer gpu applies to" in r.stderr and f"`{analysis}` writes none" in r.stderr
    assert not list(tmp_path.iterdir())
    text = run(["--help"]).stdout
    assert "--popgen-writer <host|gpu>" in text and "--popgen-slab-rows <N>" in text
