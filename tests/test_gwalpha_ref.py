"""The Python restatement of GWAlpha (tests/gwalpha_ref.py) against the reference's own test literals (gwas/gwalpha.rs:389-435,
tests/golden/gwalpha_literals.json), and the gwalpha_fmt phenotype parser of the CLI (through `hostcheck gwalpha_phen`) against a
transcription of base/phen.rs:111-158.  No GPU.

The reference prints alpha with six decimals.  The restatement's first LS value is 5.8160675104: it sits on the rounding
boundary of the printed digit, so the four alphas are asked to agree within one unit of that digit (1e-6), not to round alike;
frequencies and the line format are compared exactly."""
import json
import subprocess
from pathlib import Path

import numpy as np
import pytest

import gwalpha_ref as G

ROOT = Path(__file__).resolve().parent.parent
HOSTCHECK = ROOT / "poolgen_amd" / "csrc" / "hostcheck"
GOLD = Path(__file__).parent / "golden" / "gwalpha_literals.json"


def golden_case(oracle):
    g = json.loads(GOLD.read_text())
    counts = np.zeros((5, 6), dtype=np.uint64)
    for j, a in enumerate(g["alleles"]):
        counts[:, G.ALLELES.index(a)] = np.array(g["counts"])[:, j]
    f = g["filter"]
    flt = oracle.filt(f["remove_ns"], f["min_coverage_depth"], f["min_allele_frequency"], f["max_missingness_rate"])
    return g, counts, flt


@pytest.mark.parametrize("method", ["LS", "ML"])
def test_restatement_reproduces_the_reference_literals(oracle, method):
    g, counts, flt = golden_case(oracle)
    rows = G.gwalpha_locus(oracle, counts, g["bins"], g["q"], g["sig"], g["min"], g["max"], flt, method)
    got = G.csv_lines(oracle, g["chromosome"], g["position"], rows).splitlines()
    want = g["expected_ls" if method == "LS" else "expected_ml"].splitlines()
    assert len(got) == len(want) == 2
    for a, b, r in zip(got, want, rows):
        fa, fb = a.split(","), b.split(",")
        assert fa[:5] == fb[:5] and fa[6] == fb[6] == "Unknown", (a, b)   # chr, pos, allele, freq (6 dp), Pheno_0: exact
        print(f"{method} {fa[2]}: alpha {r['alpha']!r} ({r['iters']} iterations), reference prints {fb[5]}")
        assert abs(r["alpha"] - float(fb[5])) <= 1e-6
        assert abs(float(fa[5]) - float(fb[5])) <= 1e-6 + 1e-12


def test_fewer_than_three_pools_are_refused(oracle):
    counts = np.zeros((2, 6), dtype=np.uint64)
    counts[:, 0], counts[:, 1] = (10, 20), (20, 10)
    with pytest.raises(ValueError):
        G.gwalpha_locus(oracle, counts, [0.5, 0.5], [0.0, 0.5], 0.1, 0.0, 1.0, oracle.filt(), "ML")


PHEN_FILES = {
    "min_zero": G.gwalpha_fmt_text("trait", 0.02, 0.0, 0.9, [0.2, 0.4, 0.6, 0.8], [0.1, 0.4, 0.7, 0.9]),
    # MIN != 0, blanks around the numbers, uneven bins, CRLF line ends
    "min_nonzero": 'Pheno_name = "yield (t/ha)" ;\r\nsig= 0.3125 ;\r\nMIN=-1.5;\r\nMAX = 7.25;\r\n'
                   "perc=[0.05, 0.2 ,0.45,0.6,0.85, 0.95];\r\nq=[ -1.0,0.0,1.5, 3.0,5.5,7.0 ];\r\n",
}


@pytest.mark.parametrize("name", sorted(PHEN_FILES))
def test_gwalpha_fmt_parser_equals_the_transcription(tmp_path, name):
    text = PHEN_FILES[name]
    f = tmp_path / "phen.py"
    f.write_bytes(text.encode())
    r = subprocess.run([str(HOSTCHECK), "gwalpha_phen", str(f)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    bins, q_prime, sig, mn, mx, names = G.parse_gwalpha_fmt(text)
    head = lines[0].split()
    assert int(head[0]) == len(bins) and [float(x) for x in head[1:]] == [sig, mn, mx]
    assert lines[1].split() == names
    got = [[float(x) for x in ln.split()] for ln in lines[2:]]
    assert len(got) == len(bins)
    assert [g[0] for g in got] == bins and [g[1] for g in got] == q_prime      # bit for bit (shortest round-trip text)
    if name == "min_nonzero":
        assert mn != 0.0 and q_prime[1] == (-1.0 - mn) / (mx - mn)


def test_gwalpha_fmt_parser_refuses_broken_files(tmp_path):
    for bad in ("sig=1;\n", G.gwalpha_fmt_text("t", 0.1, 0.0, 1.0, [0.5], [0.5]).replace("sig=0.1", "sig=abc"),
                G.gwalpha_fmt_text("t", 0.1, 0.0, 1.0, [0.3, 0.6], [0.1, 0.2, 0.3, 0.4])):
        f = tmp_path / "bad.py"
        f.write_text(bad)
        r = subprocess.run([str(HOSTCHECK), "gwalpha_phen", str(f)], capture_output=True, text=True)
        assert r.returncode == 1 and "hostcheck:" in r.stderr, (bad, r.stdout)
