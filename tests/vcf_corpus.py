"""A seeded generator of small VCF texts for the vcf2sync parser's tests: every shape of line that vcf.rs treats in a way of
its own, and one text per way in which it panics.  Texts only; what they mean is vcf_ref.py's business."""
import numpy as np

ALLELES = ["A", "T", "C", "G", "N", "D", "a", "t", "*", ".", "AATG", "<NON_REF>", "", "CCT", "GA"]
FORMATS = ["AD", "AD:GT", "GT:AD", "GT:AD:DP", "GT:PL:DP:AD", "GT:DP:AD:PL:GQ"]
HEADER = "##fileformat=VCFv4.2\n##source=vcf_corpus\n"


def chrom_line(n, names=None):
    names = names or [f"Pool-{i}" for i in range(n)]
    return "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + "".join("\t" + x for x in names) + "\n"


def sample_field(fmt, ad, rng):
    other = {"GT": ["0/0", "0/1", "1/1", "./."], "PL": ["0,24,239", "42,0,61", "."], "DP": ["7", "0", "."], "GQ": ["99", "."]}
    return ":".join(",".join(str(v) for v in ad) if k == "AD" else other[k][int(rng.integers(len(other[k])))] for k in fmt.split(":"))


def count(rng):
    """1 to 10 digits, the small ones often, 0 and 4294967295 among them"""
    c = int(rng.integers(0, 12))
    if c == 0:
        return 0
    if c == 11:
        return 4294967295
    if c >= 10:
        return int(rng.integers(10 ** 9, 4294967296))
    if c <= 5:
        return int(rng.integers(0, 40))
    return int(rng.integers(10 ** (c - 1), 10 ** c))


def data_line(rng, n, chrom=None, pos=None, ref=None, alts=None, fmt=None, info=None, short_ad=False, zero_pools=0.15):
    chrom = chrom if chrom is not None else ["chr1", "chrA", "scaffold_12", "X"][int(rng.integers(4))]
    if pos is None:
        p = int(rng.integers(1, 10 ** int(rng.integers(1, 12))))
        pos = [str(p), "+" + str(p), "000" + str(p)][int(rng.choice(3, p=[0.8, 0.1, 0.1]))]
    ref = ref if ref is not None else ALLELES[int(rng.integers(len(ALLELES)))]
    alts = alts if alts is not None else [ALLELES[int(rng.integers(len(ALLELES)))] for _ in range(int(rng.integers(1, 5)))]
    fmt = fmt or FORMATS[int(rng.integers(len(FORMATS)))]
    m = 1 if short_ad else 1 + len(alts) + int(rng.integers(0, 2))           # pool 0's AD values: the columns of the line
    fields = []
    for i in range(n):
        k = m if (i == 0 or short_ad) else m + int(rng.integers(0, 3))        # later pools: as many or more (fewer is an error)
        ad = [0] * k if rng.random() < zero_pools else [count(rng) for _ in range(k)]
        fields.append(sample_field(fmt, ad, rng))
    info = info if info is not None else "DP=%d;AF=0.5;PADDING=xxxxxxxx" % int(rng.integers(1000))
    return "\t".join([chrom, pos, ".", ref, ",".join(alts), "327.237", ".", info, fmt] + fields) + "\n"


def finish(text, crlf, final_newline):
    if crlf:
        text = text.replace("\n", "\r\n")
    if not final_newline:
        text = text[:-2] if crlf else text[:-1]
    return text.encode("latin-1")


def corpus(seed=20240607):
    """[(name, text, pool_sizes, depth, breadth, maf)]"""
    rng = np.random.default_rng(seed)
    out = []
    thresholds = [(1, 1.0, 0.001), (0, 1.0, 0.0), (5, 0.5, 0.05), (10, 1.0, 0.0), (1, 0.0, 0.001), (3, 0.34, 0.01), (1, 0.2, 0.0)]
    for t, n in enumerate([1, 2, 3, 5, 8, 9, 17, 33, 2, 5, 3, 1]):
        lines = [HEADER, chrom_line(n)]
        for r in range(int(rng.integers(15, 45))):
            u = rng.random()
            if u < 0.06:
                lines.append("##a comment in mid-file\n")
            elif u < 0.09:
                lines.append(chrom_line(n, [f"Second-{i}" for i in range(n)]))      # a second #CHROM line: the last one names the pools
            elif u < 0.14:
                lines.append(data_line(rng, n, short_ad=True))                      # one column: dropped after the breadth rule
            elif u < 0.20:
                lines.append(data_line(rng, n, ref="AATG", alts=["CCT", "A"]))      # REF and ALT both indels: the first match
            else:
                lines.append(data_line(rng, n))
        n_sizes = n + (2 if t % 4 == 3 else 0)                                      # a phenotype file with more pools than samples
        sizes = (rng.integers(5, 60, size=n_sizes) * 1.0).tolist() if t % 2 else [1.0 / n_sizes] * n_sizes
        d, b, f = thresholds[t % len(thresholds)]
        out.append((f"random{t}_n{n}", finish("".join(lines), crlf=t % 3 == 1, final_newline=t % 4 != 2), sizes, d, b, f))
    # samples that start many chunks into the line: an INFO of several KB, alleles of about 1000 bytes
    lines = [HEADER, chrom_line(5)]
    for r in range(6):
        lines.append(data_line(rng, 5, info="X=" + "ACGT" * int(rng.integers(800, 1500)), ref="A" * int(rng.integers(900, 1100)),
                               alts=["T", "G" * int(rng.integers(900, 1100))]))
        lines.append(data_line(rng, 5))
    out.append(("long_fields_n5", finish("".join(lines), False, True), [0.2] * 5, 1, 1.0, 0.0))
    # nothing kept / everything kept / only '#' lines
    lines = [HEADER, chrom_line(4)] + [data_line(rng, 4, zero_pools=0.0) for _ in range(20)]
    out.append(("all_dropped_n4", finish("".join(lines), False, True), [0.25] * 4, 1 << 40, 1.0, 0.0))
    lines = [HEADER, chrom_line(4)] + [data_line(rng, 4, ref="A", alts=["T"], zero_pools=1.0) for _ in range(20)]  # q = NaN passes
    out.append(("all_kept_n4", finish("".join(lines), False, True), [0.25] * 4, 0, 1.0, 0.3))
    out.append(("only_comments", finish(HEADER + chrom_line(3) + "##tail\n", False, True), [1.0, 2.0, 3.0], 1, 1.0, 0.001))
    out.append(("only_comments_no_newline", finish(HEADER + chrom_line(3), False, False), [1.0, 2.0, 3.0], 1, 1.0, 0.001))
    # three CRLF data lines, the last one ending in "\r" without its "\n" (crlf_no_final_newline of the sync and pileup corpora):
    # the line index and the line bounds on such a text.  The "\r" is the last byte of the last sample's GT piece, which nobody
    # reads, so this case does not tell whether it was stripped; error_texts()["cr_without_newline_stays"] does
    lines = [data_line(rng, 3, ref="A", alts=["T"], fmt="AD:GT", zero_pools=0.0) for _ in range(3)]
    out.append(("crlf_no_final_newline", "".join(lines).replace("\n", "\r\n")[:-1].encode("latin-1"), [10.0, 20.0, 30.0], 1, 1.0, 0.0))
    return out


def good(n, k, rng):
    return [data_line(rng, n, ref="A", alts=["T"], fmt="GT:AD", pos=str(100 + i)) for i in range(k)]


def bad_line(fields9, samples):
    return "\t".join(fields9 + samples) + "\n"


def error_texts(seed=7):
    """{name: (text, pool_sizes, depth, breadth, maf, offset of the first bad line, reason)}: good lines, the bad line, a good
    line, and a second bad line of another kind behind it (the first one is what must be reported)"""
    import vcf_ref as R
    rng = np.random.default_rng(seed)
    fixed = ["chr1", "500", ".", "A", "T", "30.0", ".", "DP=10;PADDING=xxxxxxxx", "GT:AD"]

    def with_(i, v):
        f = list(fixed)
        f[i] = v
        return f
    two = ["0/1:3,4", "0/0:5,1"]
    cases = {
        "pos_letters": (bad_line(with_(1, "12a"), two), R.E_POS),
        "pos_empty": (bad_line(with_(1, ""), two), R.E_POS),
        "pos_negative": (bad_line(with_(1, "-5"), two), R.E_POS),
        "pos_float": (bad_line(with_(1, "1.0"), two), R.E_POS),
        "pos_plus_only": (bad_line(with_(1, "+"), two), R.E_POS),
        "pos_overflow": (bad_line(with_(1, "18446744073709551616"), two), R.E_POS),
        "no_ad": (bad_line(with_(8, "GT:DP"), two), R.E_AD_KEY),
        "two_ad": (bad_line(with_(8, "AD:GT:AD"), ["1,2:0/1:3,4", "1,2:0/1:3,4"]), R.E_AD_KEY),
        "sample_dot": (bad_line(fixed, ["0/1:3,4", "."]), R.E_SUBFIELDS),
        "sample_gt_only": (bad_line(fixed, ["./.", "0/1:3,4"]), R.E_SUBFIELDS),
        "ad_dot": (bad_line(fixed, ["0/1:3,4", "./.:."]), R.E_AD_VALUE),
        "ad_dot_inside": (bad_line(fixed, ["0/1:3,.", "0/1:3,4"]), R.E_AD_VALUE),
        "ad_overflow_u64": (bad_line(fixed, ["0/1:3,18446744073709551616", "0/1:3,4"]), R.E_AD_VALUE),
        "empty_line": ("\n", R.E_EMPTY),
        "empty_line_crlf": ("\r\n", R.E_EMPTY),
        "short_line": ("c\t1\t.\tA\tT\t.\t.\t.\tAD\n", R.E_SHORT),
        "few_fields": ("chr1\t500\t.\tA\tT\t30.0\t.\tDP=10;PADDING=xxxxxxxx\n", R.E_FIELDS),
        "ad_ragged": (bad_line(fixed, ["0/1:3,4", "0/1:3"]), R.E_AD_RAGGED),
        "allele_oob": (bad_line(with_(4, "G,T"), ["0/1:3,4", "0/1:3,4"]), R.E_ALLELE_OOB),
        # the deviations
        "count_above_u32": (bad_line(fixed, ["0/1:3,4294967296", "0/1:3,4"]), R.E_COUNT32),
        "high_byte_ref": (bad_line(with_(3, "\xe9"), two), R.E_HIGH_BYTE),
        "high_byte_alt": (bad_line(with_(4, "T,\xc3\xa9"), ["0/1:3,4,1", "0/1:3,4,1"]), R.E_HIGH_BYTE),
        "other_pool_count": (bad_line(fixed, ["0/1:3,4"]), R.E_POOLS),
        "more_pools_than_sizes": (bad_line(fixed, two + ["0/1:3,4"]), R.E_POOLS),
        # a line wrong in two ways reports the smaller code
        "pos_and_ad": (bad_line(with_(1, "x"), ["0/1:3,.", "0/1:3,4"]), R.E_POS),
    }
    out = {}
    for name, (bad, reason) in cases.items():
        head = HEADER + chrom_line(2) + "".join(good(2, 3, rng))
        text = head + bad + "".join(good(2, 2, rng)) + bad_line(with_(1, "zzz"), two) + "".join(good(2, 1, rng))
        out[name] = (text.encode("latin-1"), [0.5, 0.5], 1, 1.0, 0.0, len(head.encode("latin-1")), reason)
    # a ragged or out-of-range line that fails the breadth rule is dropped, not an error: the same lines, depth 1000
    # (tests use these through `dropped_not_errors`)
    head = HEADER + chrom_line(2)
    text = head + "chr1\t500\t.\tA\tT\t30.0\t.\tDP=10;PADDING=xxxxxxxx\tGT:AD\n"
    out["no_samples_breadth_0"] = (text.encode(), [0.5, 0.5], 1, 0.0, 0.0, len(head), R.E_NO_SAMPLES)
    # CRLF lines, and the last one ends in "\r" without its "\n": vcf.rs takes a "\r" away only together with the newline
    # (:276-281), so here it stays behind the last allele depth, "5,1\r", which is no u64.  A reader that strips it (as the sync
    # and pileup readers do for their formats) would keep the line.
    head = (HEADER + chrom_line(2) + "".join(good(2, 3, rng))).replace("\n", "\r\n")
    text = head + bad_line(fixed, two).replace("\n", "\r")
    out["cr_without_newline_stays"] = (text.encode("latin-1"), [0.5, 0.5], 1, 1.0, 0.0, len(head.encode("latin-1")), R.E_AD_VALUE)
    return out


def dropped_not_errors(seed=9):
    """texts whose late panics (ragged AD, allele without a column) are never reached because the breadth rule drops the line first"""
    rng = np.random.default_rng(seed)
    fixed = ["chr1", "500", ".", "A", "T", "30.0", ".", "DP=10;PADDING=xxxxxxxx", "GT:AD"]
    g = fixed[:4] + ["G,T"] + fixed[5:]
    text = HEADER + chrom_line(2) + "".join(good(2, 2, rng)) + bad_line(fixed, ["0/1:3,4", "0/1:3"]) + bad_line(g, ["0/1:3,4", "0/1:3,4"]) \
        + "".join(good(2, 2, rng))
    return text.encode(), [0.5, 0.5], 1000, 1.0, 0.0
