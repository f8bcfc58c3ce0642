"""The literal restatement of the reference's vcf2sync (tests/vcf_ref.py) against the reference's own literals and fixture, and
the two short forms the library relies on against the statements as written.  No GPU, no library."""
import json
from pathlib import Path

import pytest

import vcf_corpus
import vcf_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden"


@pytest.fixture(scope="module")
def fixture_text():
    return (GOLDEN / "test.vcf").read_bytes()


def test_restatement_reproduces_the_reference_literal():
    lit = json.loads((GOLDEN / "vcf_literals.json").read_text())
    v = R.lparse(lit["line"])
    assert v == lit["parsed"]
    f1, f2 = lit["filter_stats_1"], lit["filter_stats_2"]
    r = R.vcf_to_sync(v, lit["pool_sizes"], f1["min_coverage_depth"], f1["min_coverage_breadth"], f1["min_allele_frequency"])
    assert f1["kept"] and r[0] == lit["sync_line"]
    assert R.vcf_filter(v, lit["pool_sizes"], f2["min_coverage_depth"], f2["min_coverage_breadth"], f2["min_allele_frequency"]) is f2["kept"]


@pytest.mark.parametrize("depth,breadth,maf,kept", [(1, 1.0, 0.001, 380), (1, 1.0, 0.0, 400), (10, 1.0, 0.0, 61), (5, 0.5, 0.05, 210)])
def test_fixture_loci_kept(fixture_text, depth, breadth, maf, kept):
    """the reference's tests/test.vcf, ten equal pool sizes: 400 loci on 4 chromosomes"""
    r = R.parse_ref(fixture_text, [0.1] * 10, depth, breadth, maf)
    assert r["data_lines"] == 400 and r["n_pools"] == 10
    assert len(r["pos"]) == kept
    chroms = {fixture_text[o:o + l] for o, l in zip(r["line_off"].tolist(), r["chrom_len"].tolist())}
    assert len(chroms) <= 4
    out = R.vcf2sync_bytes(fixture_text, [0.1] * 10, depth, breadth, maf)
    assert out.count(b"\n") == kept + 1
    assert out.startswith(b"#chr\tpos\tref\tEntry-0\tEntry-1\t") and out.split(b"\n")[0].endswith(b"\tEntry-9")


def _data_lines(text):
    for _, raw in R.text_lines(text):
        line = R.strip_eol(raw).decode("latin-1")
        if line and line[0] != "#":
            yield line


def test_collapsed_filter_equals_the_loop_as_written(fixture_text):
    """`while j < m` shrinks m without advancing j, so m collapses to j at the first failing column: the locus stays iff m >= 2
    and column 1 passes.  Every line of the corpus and the fixture, under every threshold set of the corpus."""
    texts = [(t, s, d, b, f) for _, t, s, d, b, f in vcf_corpus.corpus()] + [(fixture_text, [0.1] * 10, 5, 0.5, 0.05)]
    seen = {True: 0, False: 0}
    for text, sizes, d, b, f in texts:
        for line in _data_lines(text):
            v = R.lparse(line)
            for maf in (f, 0.0, 0.05, 0.3):
                a = R.vcf_filter(v, sizes, d, b, maf)
                assert a == R.vcf_filter(v, sizes, d, b, maf, collapsed=True), line[:60]
                seen[a] += 1
    assert seen[True] > 100 and seen[False] > 100


def test_corpus_is_clean_and_covers_its_list():
    """no corpus text panics; the shapes the parser must treat in a way of their own are all there"""
    joined = b""
    kept = 0
    for name, text, sizes, d, b, f in vcf_corpus.corpus():
        assert R.literal_panics(text, sizes, d, b, f) is None, name
        kept += len(R.parse_ref(text, sizes, d, b, f)["pos"])
        joined += text
    assert kept > 50
    for needle in (b"\r\n", b"<NON_REF>", b"\t*\t", b"\t+", b"\t000", b"4294967295", b"\tAD\t", b"\tGT:AD:DP\t", b"\tGT:PL:DP:AD\t", b"Second-0"):
        assert needle in joined, needle
    assert max(len(l) for l in joined.split(b"\n")) > 5000    # an INFO of several KB plus two alleles of about 1000 bytes


def test_error_texts_panic_where_the_contract_says():
    for name, (text, sizes, d, b, f, off, reason) in vcf_corpus.error_texts().items():
        with pytest.raises(R.VcfPanic) as e:
            R.parse_ref(text, sizes, d, b, f)
        assert (e.value.offset, e.value.reason) == (off, reason), name
        if reason not in R.DEVIATIONS:
            assert R.literal_panics(text, sizes, d, b, f) == off, name     # the reference itself panics at that line
        elif reason != R.E_POOLS:   # (more samples than pool sizes panics in the reference too, once its q loop is reached)
            assert R.literal_panics(text, sizes, d, b, f) != off, name     # a deviation: the reference goes on


def test_breadth_rule_comes_before_the_late_panics():
    text, sizes, d, b, f = vcf_corpus.dropped_not_errors()
    assert R.literal_panics(text, sizes, d, b, f) is None
    assert 500 not in R.parse_ref(text, sizes, d, b, f)["pos"].tolist()    # the two lines at position 500 are dropped, not errors
    assert R.literal_panics(text, sizes, 1, b, f) is not None


def test_breadth_threshold_zero_keeps_the_loop_as_written():
    """threshold 0: the loop breaks only on a pool 0 that is NOT covered; a covered pool 0 drops the line"""
    v = {"chromosome": "c", "position": 1, "reference_allele": "A", "alternative_alleles": ["T"], "allele_depths": [[0, 0], [5, 5]]}
    assert R.vcf_filter(v, [0.5, 0.5], 1, 0.0, 0.0) is True
    v["allele_depths"] = [[5, 5], [0, 0]]
    assert R.vcf_filter(v, [0.5, 0.5], 1, 0.0, 0.0) is False


def test_header_comes_from_the_last_chrom_line():
    name, text, sizes, d, b, f = next(c for c in vcf_corpus.corpus() if b"Second-0" in c[1])
    assert R.vcf2sync_bytes(text, sizes, d, b, f).startswith(b"#chr\tpos\tref\tSecond-0")
