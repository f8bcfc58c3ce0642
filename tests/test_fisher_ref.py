"""fisher_exact_test without a GPU: the checker (tests/fisher_ref.py) reproduces the reference's literals exactly, its
compacted enumeration equals the literal one, and the library carries the two entry points at every layer of the ABI."""
import json
import re
from pathlib import Path

import numpy as np

import fisher_ref
import rustfmt

ROOT = Path(__file__).resolve().parent.parent
LIT = json.loads((ROOT / "tests" / "golden" / "fisher_literals.json").read_text())


def test_restatement_reproduces_the_reference_literals_and_compaction_holds():
    assert fisher_ref.factorial_log10(LIT["factorial_log10"]["x"]) == LIT["factorial_log10"]["expected"]
    h = LIT["hypergeom_ratio"]
    assert fisher_ref.hypergeom_ratio(np.array(h["counts"], dtype=np.float64), h["log_prod_fac_marginal_sums"]) == h["expected"]
    f = LIT["fisher"]
    po, pv = fisher_ref.fisher(np.array(f["matrix"]))
    assert po == f["p_observed"] and pv == f["pvalue"]
    line = ",".join([f["chromosome"], str(f["position"]), "".join(f["alleles_vector"]), rustfmt.display(po), rustfmt.display(pv)]) + "\n"
    assert line == f["expected_line"]
    # the rounding rule: with total = 833 a cell of 49 reads scales to floor(49 * (34.0 / 833)) = 1, not 49 * 34 / 833 = 2
    s = fisher_ref.scaled(np.array([[49, 98], [392, 294]]))
    assert s.tolist() == [[1.0, 3.0], [15.0, 11.0]]
    # compacted enumeration == literal enumeration on seeded random tables, zeroed first / last rows and columns included
    rng = np.random.default_rng(3)
    worst, cnt = 0.0, 0
    for _ in range(700):
        n, p = int(rng.integers(2, 12)), int(rng.integers(2, 7))
        lam = rng.choice([0.2, 1.0, 5.0, 60.0])
        m = rng.poisson(lam, size=(n, p)) * (rng.random((n, p)) < rng.choice([0.3, 0.9]))
        if rng.random() < 0.3:
            m[-1, :] = 0
        if rng.random() < 0.2:
            m[:, -1] = 0
        if rng.random() < 0.15:
            m[0, :] = 0
        if rng.random() < 0.15:
            m[:, 0] = 0
        if m.sum() == 0:
            continue
        a, b = fisher_ref.fisher(m), fisher_ref.fisher_compact(m)   # (fisher raises where the reference's assert would fire)
        cnt += 1
        worst = max(worst, fisher_ref.rel(b[0], a[0]), fisher_ref.rel(b[1], a[1]))
    print(f"compacted vs literal enumeration: {cnt} tables, worst relative difference {worst:.3g}")
    assert cnt > 500 and worst <= 1e-12


def test_fisher_entry_points_at_every_layer(native):
    names = ["pg_fisher_batch", "pg_fisher_batch_dev"]
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "poolgen_hip.h").read_text(), flags=re.S)
    from poolgen_amd._native import SIGNATURES
    doc = (ROOT / "INTEGRATION.md").read_text()
    for name in names:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} not declared in include/poolgen_hip.h"
        assert name in SIGNATURES, f"{name} missing from poolgen_amd._native.SIGNATURES"
        assert f"fn {name}(" in doc, f"{name} not bound in INTEGRATION.md"
        assert hasattr(native, name), f"{name} not exported by libpoolgen_hip.so"
    assert len(SIGNATURES["pg_fisher_batch"][1]) == len(SIGNATURES["pg_chisq_batch"][1]) == 10
