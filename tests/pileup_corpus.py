"""Named awkward mpileup lines and error texts for the pileup parser's tests, each with the outcome worked out by hand from
base/pileup.rs.  Lines and expectations only; tests/pileup_ref.py says what they mean in general."""
import functools
import random

import numpy as np

import pileup_ref as R

# the rule of most cases: nothing is dropped for depth or frequency unless the case says so
BASE = dict(remove_ns=True, keep_lowercase_reference=False, max_base_error_rate=0.01, min_coverage_depth=1, min_coverage_breadth=1.0,
            min_allele_frequency=0.0)


def one(reads, quals, cov=None, ref=b"A"):
    """a line of one pool; the coverage is the number of quality bytes unless given"""
    return b"c1\t5\t" + ref + b"\t%d\t" % (len(quals) if cov is None else cov) + reads + b"\t" + quals


def K(*pools):
    return ("K", [list(p) for p in pools])


D = ("D",)


def E(reason):
    return ("E", reason)


# (name, line, pool sizes, rule overrides, outcome): outcome K(six numbers A,T,C,G,D,N per pool), D, or E(reason)
LINES = [
    ("plain", one(b".,TtCcGg*Nn", b"IIIIIIIIIII"), [1.0], dict(remove_ns=False), K([2, 2, 2, 2, 1, 2])),
    ("plain_remove_ns", one(b".,TtCcGg*Nn", b"IIIIIIIIIII"), [1.0], {}, K([2, 2, 2, 2, 1, 0])),
    # '^' drops the byte behind it, whatever it is
    ("caret_plus", one(b"^+.", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("caret_minus", one(b"^-.", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("caret_dollar", one(b"^$.", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("caret_caret", one(b"^^.", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("caret_then_indel", one(b"^x+1T.", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("dollar", one(b".$T$", b"II"), [1.0], {}, K([1, 1, 0, 0, 0, 0])),
    # indel lengths
    ("plus_zero_one", one(b".+01T,", b"II"), [1.0], {}, K([2, 0, 0, 0, 0, 0])),
    ("plus_zero_zero_two", one(b".-002TT,", b"II"), [1.0], {}, K([2, 0, 0, 0, 0, 0])),
    ("two_digits", one(b".+12ACGTACGTACGT,", b"II"), [1.0], {}, K([2, 0, 0, 0, 0, 0])),
    ("two_digits_with_zero", one(b".-10ACGTACGTACT", b"II"), [1.0], {}, K([1, 1, 0, 0, 0, 0])),
    ("skip_swallows_markers", one(b".+3+^.T", b"II"), [1.0], {}, K([1, 1, 0, 0, 0, 0])),
    ("skip_swallows_digit_like", one(b".+2-5C", b"II"), [1.0], {}, K([1, 0, 1, 0, 0, 0])),
    ("skip_clipped_by_field_end", one(b".+5AC", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("field_ends_on_plus", one(b".+", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("field_ends_on_caret", one(b".^", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("field_ends_in_digits", one(b".-12", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("field_ends_in_zeros", one(b".+00", b"I"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("high_byte_after_length", one(b".+1\xe9T", b"II"), [1.0], {}, K([1, 1, 0, 0, 0, 0])),
    # coverage 0: the other two fields are not looked at
    ("cov0_garbage", b"c1\t5\tA\t0\t+x\t\x01\x02\x03\t1\t.\tI", [0.5, 0.5], dict(min_coverage_depth=0), K([0] * 6, [1, 0, 0, 0, 0, 0])),
    ("cov0_garbage_breadth_drops", b"c1\t5\tA\t0\t+x\t\x01\t1\t.\tI", [0.5, 0.5], {}, D),
    ("cov0_half_breadth", b"c1\t5\tA\t0\t*\t*\t1\tT\tI", [0.5, 0.5], dict(min_coverage_breadth=0.5), K([0] * 6, [0, 1, 0, 0, 0, 0])),
    # read bytes
    ("unknown_bytes_kept_as_n", one(b"X\xe9>", b"III"), [1.0], dict(remove_ns=False), K([0, 0, 0, 0, 0, 3])),
    ("unknown_bytes_removed", one(b"X\xe9>", b"III"), [1.0], {}, D),
    # qualities
    ("quality_32", one(b".", b" "), [1.0], {}, D),
    ("quality_32_second_pool", b"c1\t5\tA\t1\t.\tI\t2\t.T\tI\x1f", [0.5, 0.5], {}, D),
    ("quality_high_byte", one(b".", b"\xff"), [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("low_quality_is_n", one(b".T", b"#I"), [1.0], dict(remove_ns=False), K([0, 1, 0, 0, 0, 1])),
    ("low_quality_removed", one(b".T", b"#I"), [1.0], {}, K([0, 1, 0, 0, 0, 0])),
    ("error_rate_one_keeps_all", one(b".T", b"!I"), [1.0], dict(max_base_error_rate=1.0), K([1, 1, 0, 0, 0, 0])),
    # the reference allele
    ("lowercase_ref", one(b".,T", b"III", ref=b"a"), [1.0], {}, K([0, 1, 0, 0, 0, 2])),
    ("lowercase_ref_kept", one(b".,T", b"III", ref=b"a"), [1.0], dict(keep_lowercase_reference=True), K([2, 1, 0, 0, 0, 0])),
    ("star_read_lowercase_kept", one(b"*.", b"II"), [1.0], dict(keep_lowercase_reference=True), K([1, 0, 0, 0, 0, 1])),
    ("ref_n_removed", one(b".", b"I", ref=b"N"), [1.0], {}, D),
    ("ref_n_kept", one(b".T", b"II", ref=b"N"), [1.0], dict(remove_ns=False), K([0, 1, 0, 0, 0, 1])),
    ("ref_star", one(b".", b"I", ref=b"*"), [1.0], {}, K([0, 0, 0, 0, 0, 1])),
    ("ref_star_lowercase_kept", one(b".", b"I", ref=b"*"), [1.0], dict(keep_lowercase_reference=True), K([0, 0, 0, 0, 1, 0])),
    ("ref_d", one(b".", b"I", ref=b"D"), [1.0], {}, K([0, 0, 0, 0, 1, 0])),
    # numbers
    ("plus_position", b"c1\t+5\tA\t+1\t.\tI", [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("nineteen_digits", b"c1\t9999999999999999999\tA\t0000000000000000001\t.\tI", [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    ("empty_chromosome", b"\t5\tA\t1\t.\tI", [1.0], {}, K([1, 0, 0, 0, 0, 0])),
    # pool counts
    ("three_fields", b"c1\t5\tA", [1.0], {}, D),
    ("one_pool_too_many", b"c1\t5\tA\t1\t.\tI\t1\t.\tI", [1.0], {}, D),
    ("one_pool_too_few", b"c1\t5\tA\t1\t.\tI", [0.5, 0.5], {}, D),
    # the frequency rule
    ("all_n_pool_depth_0", b"c1\t5\tA\t1\tN\tI\t1\tT\tI", [0.5, 0.5], dict(min_coverage_depth=0, min_allele_frequency=0.2), K([0] * 6, [0, 1, 0, 0, 0, 0])),
    ("t_below_maf", b"c1\t5\tA\t4\t....\tIIII\t4\t...T\tIIII", [0.5, 0.5], dict(min_allele_frequency=0.2), D),
    ("t_at_maf", b"c1\t5\tA\t4\t...T\tIIII\t4\t...T\tIIII", [0.5, 0.5], dict(min_allele_frequency=0.25), K([3, 1, 0, 0, 0, 0], [3, 1, 0, 0, 0, 0])),
    ("t_above_one_minus_maf", b"c1\t5\tA\t2\tTT\tII\t2\tTT\tII", [0.5, 0.5], dict(min_allele_frequency=0.1), D),
    ("only_c_varies", b"c1\t5\tA\t2\t.C\tII\t2\t.C\tII", [0.5, 0.5], dict(min_allele_frequency=0.1), D),
    # one defect
    ("e_two_fields", b"c1\t5", [1.0], {}, E(R.FIELDS)),
    ("e_no_tab", b"c1", [1.0], {}, E(R.FIELDS)),
    ("e_position", b"c1\t12a\tA\t1\t.\tI", [1.0], {}, E(R.POS)),
    ("e_position_empty", b"c1\t\tA\t1\t.\tI", [1.0], {}, E(R.POS)),
    ("e_position_twenty_digits", b"c1\t10000000000000000000\tA\t1\t.\tI", [1.0], {}, E(R.POS)),
    ("e_ref_two_bytes", b"c1\t5\tAC\t1\t.\tI", [1.0], {}, E(R.REF)),
    ("e_ref_empty", b"c1\t5\t\t1\t.\tI", [1.0], {}, E(R.REF)),
    ("e_ref_high_byte", b"c1\t5\t\xe9\t1\t.\tI", [1.0], {}, E(R.REF)),
    ("e_coverage", b"c1\t5\tA\tx\t.\tI", [1.0], {}, E(R.COV)),
    ("e_coverage_trailing_tab", b"c1\t5\tA\t1\t.\tI\t", [1.0], {}, E(R.COV)),
    ("e_ragged_no_quality", b"c1\t5\tA\t1\t.", [1.0], {}, E(R.RAGGED)),
    ("e_ragged_coverage_only", b"c1\t5\tA\t0", [1.0], {}, E(R.RAGGED)),
    ("e_indel", one(b".+x", b"I"), [1.0], {}, E(R.INDEL)),
    ("e_indel_after_zero", one(b".-0x", b"I"), [1.0], {}, E(R.INDEL)),
    ("e_indel_high_byte", one(b".+\xe9", b"I"), [1.0], {}, E(R.INDEL)),
    ("e_more_reads", one(b"..", b"I"), [1.0], {}, E(R.MISMATCH)),
    ("e_fewer_qualities", one(b"..", b"I", cov=2), [1.0], {}, E(R.MISMATCH)),
    ("e_more_qualities", one(b"..", b"III", cov=2), [1.0], {}, E(R.MISMATCH)),
    ("e_empty_reads", one(b"", b"", cov=1), [1.0], {}, E(R.MISMATCH)),
    ("e_in_the_pool_too_many", b"c1\t5\tA\t1\t.\tI\t1\t.+x\tI", [1.0], {}, E(R.INDEL)),
    ("e_in_a_far_pool_too_many", b"c1\t5\tA\t1\t.\tI" + b"\t1\t.\tI" * 70 + b"\t2\t.\tI", [1.0], {}, E(R.MISMATCH)),
    # two defects: the smallest code of the line, the first of a pool
    ("e2_mismatch_then_coverage", b"c1\t5\tA\t1\t..\tI\tx\t.\tI", [0.5, 0.5], {}, E(R.COV)),
    ("e2_indel_then_position", b"c1\t1e3\tA\t1\t.+x\tI", [1.0], {}, E(R.POS)),
    ("e2_position_and_ref", b"c1\tx\tAC\t1\t.\tI", [1.0], {}, E(R.POS)),
    ("e2_indel_then_ragged", b"c1\t5\tA\t1\t.+x\tI\t1\t.", [0.5, 0.5], {}, E(R.RAGGED)),
    ("e2_coverage_of_a_ragged_pool", b"c1\t5\tA\t1\t.\tI\tx", [0.5, 0.5], {}, E(R.COV)),
    ("e2_indel_before_its_mismatch", one(b"..+x", b"I"), [1.0], {}, E(R.INDEL)),
    ("e2_mismatch_far_then_indel_near", b"c1\t5\tA\t1\t.+x\tI" + b"\t1\t.\tI" * 70 + b"\t2\t.\tI", [1.0 / 72] * 72, {}, E(R.INDEL)),
]

# where the library states a limit of its own and the reference would go on: a number of 20 digits that still fits a u64
LIBRARY_LIMITS = {"e_position_twenty_digits"}


def expected(outcome, line):
    """the outcome of a LINES entry in pileup_ref.line_ref's form"""
    if outcome[0] != "K":
        return outcome
    f = line.split(b"\t")
    return ("K", len(f[0]), int(f[1]), f[2][0], np.array(outcome[1], dtype=np.uint32))


def good_line(rng, n, chrom=None):
    """a sound line of n pools"""
    f = [chrom or "chr%d" % rng.randint(1, 3), str(rng.randint(1, 10 ** 7)), rng.choice("ACGT")]
    for _ in range(n):
        cov = rng.randint(1, 12)
        f += [str(cov), "".join(rng.choice(".,.,ACGTacgt*") for _ in range(cov)), "".join(rng.choice("5?IJ") for _ in range(cov))]
    return "\t".join(f).encode()


def texts(seed=11):
    """(name, text, sizes, rule): whole texts -- every LINES entry that is no error among sound lines, under its own rule; \\r\\n
    lines; a last line without newline"""
    rng = random.Random(seed)
    out = []
    for name, line, sizes, rule, outcome in LINES:
        if outcome[0] == "E":
            continue
        n = len(sizes)
        body = [good_line(rng, n) for _ in range(3)] + [line] + [good_line(rng, n) for _ in range(2)]
        out.append((name, b"\n".join(body) + b"\n", sizes, {**BASE, **rule}))
    lines = [good_line(rng, 3) for _ in range(40)]
    out.append(("crlf", b"\r\n".join(lines) + b"\r\n", [0.2, 0.3, 0.5], dict(BASE)))
    out.append(("crlf_no_final_newline", b"\r\n".join(lines) + b"\r", [0.2, 0.3, 0.5], dict(BASE)))
    out.append(("no_final_newline", b"\n".join(lines), [0.2, 0.3, 0.5], dict(BASE)))
    out.append(("single_line_no_newline", lines[0], [0.2, 0.3, 0.5], dict(BASE)))
    out.append(("default_rule", b"\n".join(lines) + b"\n", [0.2, 0.3, 0.5], dict(R.DEFAULTS)))
    return out


def error_texts(seed=12):
    """name -> (text, sizes, rule, offset of the first bad line, reason): one text per error line of LINES, the bad line behind
    sound ones and in front of another bad one; an empty line; a line that is only '\\r'"""
    rng = random.Random(seed)
    out = {}
    for name, line, sizes, rule, outcome in LINES:
        if outcome[0] != "E":
            continue
        n = len(sizes)
        head = b"".join(good_line(rng, n) + b"\n" for _ in range(rng.randint(0, 9)))
        tail = b"".join(good_line(rng, n) + b"\n" for _ in range(3)) + b"c1\tzz\tA\n" + good_line(rng, n) + b"\n"
        out[name] = (head + line + b"\n" + tail, sizes, {**BASE, **rule}, len(head), outcome[1])
    head = b"".join(good_line(rng, 2) + b"\n" for _ in range(300))       # more than one workgroup of lines in front
    out["e_empty_line"] = (head + b"\n" + good_line(rng, 2) + b"\n", [0.5, 0.5], dict(BASE), len(head), R.FIELDS)
    out["e_cr_only_line"] = (head + b"\r\n" + good_line(rng, 2) + b"\n", [0.5, 0.5], dict(BASE), len(head), R.FIELDS)
    out["e_last_line_without_newline"] = (head + b"c1\t5\tA\t1\t.", [0.5, 0.5], dict(BASE), len(head), R.RAGGED)
    out["e_first_line"] = (b"c1\t5\n" + head, [0.5, 0.5], dict(BASE), 0, R.FIELDS)
    return out


# the filter sets of tests/test_pileup.py: pools, remove_ns, max_base_error_rate, depth, breadth, maf, weird lines, keep_lowercase_reference
FILTER_SETS = [(5, True, 0.01, 1, 1.0, 0.001, False, False), (3, False, 0.005, 2, 0.5, 0.05, True, False),
               (8, True, 0.0005, 1, 0.75, 0.0, True, False), (2, True, 1.0, 3, 1.0, 0.05, True, False),
               (4, True, 0.01, 1, 1.0, 0.001, True, True), (3, False, 0.01, 1, 0.6, 0.02, True, True)]


@functools.lru_cache(maxsize=None)
def generated(k, count=1500):
    """Filter set k on `count` lines of test_pileup's generator (one in a hundred with a pool too many), computed once:
    (sizes, rule, lines, the restatement's outcome of every line, the text of the lines that are no error, its parse_ref)"""
    from test_pileup import _random_line
    n, remove_ns, max_err, depth, breadth, maf, weird, keep_lc = FILTER_SETS[k]
    rng = random.Random(20251003 + k)
    sizes = [1.0 / n] * n
    rule = dict(remove_ns=remove_ns, keep_lowercase_reference=keep_lc, max_base_error_rate=max_err, min_coverage_depth=depth,
                min_coverage_breadth=breadth, min_allele_frequency=maf)
    lines = [_random_line(rng, n if rng.random() > 0.01 else n + 1, weird).encode("latin-1") for _ in range(count)]
    outcomes = [R.line_ref(l, sizes, **rule) for l in lines]
    text = b"".join(l + b"\n" for l, o in zip(lines, outcomes) if o[0] != "E")
    return sizes, rule, lines, outcomes, text, R.parse_ref(text, sizes, **rule)
