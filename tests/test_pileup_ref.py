"""tests/pileup_ref.py, the literal restatement of pileup2sync's line rules, against the oracle's (orc_pileup_to_sync2) line by
line -- kept text, dropped, fatal -- on the generator of tests/test_pileup.py and on the reference's own literal; and against the
outcomes worked out by hand in tests/pileup_corpus.py."""
import json
from pathlib import Path

import numpy as np
import pytest

import pileup_corpus
import pileup_ref as R

LIT = json.loads((Path(__file__).parent / "golden" / "reference_literals.json").read_text())


def test_corpus_lines_have_the_outcome_worked_out_by_hand():
    names = [c[0] for c in pileup_corpus.LINES]
    assert len(names) == len(set(names))
    for name, line, sizes, rule, outcome in pileup_corpus.LINES:
        got = R.line_ref(line, sizes, **{**pileup_corpus.BASE, **rule})
        want = pileup_corpus.expected(outcome, line)
        assert got[:-1] == want[:-1] if got[0] == "K" else got == want, (name, got, want)
        if got[0] == "K":
            assert np.array_equal(got[-1], want[-1]), (name, got[-1], want[-1])
    reasons = {o[1] for *_, o in pileup_corpus.LINES if o[0] == "E"} | {e[4] for e in pileup_corpus.error_texts().values()}
    assert reasons == {R.FIELDS, R.POS, R.REF, R.COV, R.RAGGED, R.INDEL, R.MISMATCH}      # (LONG needs a line of 2 GiB)


def test_corpus_lines_against_the_oracle(oracle):
    """where the oracle can take the line (no NUL byte, one pool per pool size checked by both)"""
    for name, line, sizes, rule, outcome in pileup_corpus.LINES:
        if name in pileup_corpus.LIBRARY_LIMITS:
            continue
        r = {**pileup_corpus.BASE, **rule}
        rc, text = oracle.pileup_to_sync(line.decode("latin-1"), sizes, r["remove_ns"], r["max_base_error_rate"], r["min_coverage_depth"],
                                         r["min_coverage_breadth"], r["min_allele_frequency"], keep_lowercase_reference=r["keep_lowercase_reference"])
        got = R.line_ref(line, sizes, **r)
        if got[0] == "K":
            assert rc > 0 and text.rstrip("\n").encode("latin-1") == R.sync_line(line, got), (name, rc, text)
        else:
            assert (rc == 0) == (got[0] == "D") and (rc < 0) == (got[0] == "E"), (name, rc, got)


@pytest.mark.parametrize("k", range(len(pileup_corpus.FILTER_SETS)))
def test_generated_lines_match_oracle(oracle, k):
    sizes, rule, lines, outcomes, _, _ = pileup_corpus.generated(k)
    weird = pileup_corpus.FILTER_SETS[k][6]
    kinds = {"K": 0, "D": 0, "E": 0}
    for line, got in zip(lines, outcomes):
        rc, text = oracle.pileup_to_sync(line.decode("latin-1"), sizes, rule["remove_ns"], rule["max_base_error_rate"], rule["min_coverage_depth"],
                                         rule["min_coverage_breadth"], rule["min_allele_frequency"],
                                         keep_lowercase_reference=rule["keep_lowercase_reference"])
        want = "K" if rc > 0 else ("D" if rc == 0 else "E")
        assert got[0] == want, (line, got, rc)
        if rc > 0:
            assert text.rstrip("\n").encode("latin-1") == R.sync_line(line, got), (line, text)
        kinds[want] += 1
    assert kinds["K"] > 20 and (not weird or (kinds["D"] > 0 and kinds["E"] > 0)), kinds


def test_reference_literal():
    g = LIT["pileup"]; f = g["filter"]
    line = g["line"].encode("latin-1")
    got = R.line_ref(line, f["pool_sizes"], remove_ns=False, max_base_error_rate=1.0, min_coverage_depth=1, min_coverage_breadth=1.0,
                     min_allele_frequency=0.0)
    assert got[0] == "K" and got[1:4] == (len("Chromosome1"), 456527, ord("C")) and got[4].tolist() == g["counts_ATCGDN"]
    got = R.line_ref(line, f["pool_sizes"], remove_ns=f["remove_ns"], max_base_error_rate=f["max_base_error_rate"],
                     min_coverage_depth=f["min_coverage_depth"], min_coverage_breadth=f["min_coverage_breadth"],
                     min_allele_frequency=f["min_allele_frequency"])
    assert got[0] == "K" and got[4].sum(axis=1).tolist() == g["filtered_coverages"]


def test_text_level_rules():
    """line ends, '\\r', the last line without newline; the first bad line wins"""
    for name, text, sizes, rule in pileup_corpus.texts():
        want = R.parse_ref(text, sizes, **rule)
        assert want["error"] is None and want["lines"] == len(R.text_lines(text)), name
    a = {t[0]: R.parse_ref(*t[1:3], **t[3]) for t in pileup_corpus.texts()}
    for k in ("counts", "pos", "ref", "chrom_len"):
        assert np.array_equal(a["crlf"][k], a["no_final_newline"][k]) and np.array_equal(a["crlf_no_final_newline"][k], a["no_final_newline"][k])
    assert len(a["no_final_newline"]["pos"]) > 30
    for name, (text, sizes, rule, off, reason) in pileup_corpus.error_texts().items():
        assert R.parse_ref(text, sizes, **rule)["error"] == (off, reason), name
