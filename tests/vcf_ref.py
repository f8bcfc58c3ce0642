"""The reference's vcf2sync (src/base/vcf.rs), restated literally in Python: the yardstick of pg_host_vcf_parse and
pg_vcf_parse_dev.  Where the reference panics this raises VcfPanic.

Two layers:
  * lparse / vcf_filter / vcf_to_sync / per_chunk / vcf2sync_bytes follow vcf.rs statement by statement (line numbers beside
    them), on text decoded as latin-1 so that a byte is a character;
  * parse_ref is the library's contract on top of them: the same arrays that pg_host_vcf_parse returns, the three documented
    deviations, and for a bad text the offset of the first bad line with the SMALLEST reason code that holds of it.
"""
import math
import re

import numpy as np

# pg_vcf_reason (include/poolgen_hip.h)
E_EMPTY, E_SHORT, E_LONG, E_FIELDS, E_POS, E_HIGH_BYTE, E_AD_KEY, E_POOLS, E_SUBFIELDS, E_AD_VALUE, E_COUNT32, E_NO_SAMPLES, \
    E_AD_RAGGED, E_ALLELE_OOB = range(1, 15)
DEVIATIONS = {E_COUNT32, E_HIGH_BYTE, E_POOLS, E_LONG}


class VcfPanic(Exception):
    def __init__(self, where, offset=-1, reason=0):
        super().__init__(f"{where} (line at byte {offset}, reason {reason})")
        self.where, self.offset, self.reason = where, offset, reason


_U64 = re.compile(r"\+?[0-9]+\Z")


def parse_u64(s):
    """str::parse::<u64>: an optional '+', digits, nothing else, no overflow; None where Rust gives Err"""
    if not _U64.match(s):
        return None
    v = int(s)
    return v if v < 1 << 64 else None


def parse_char_or_d(s):
    return s if len(s) == 1 else "D"


def _index(seq, i, where):
    if i >= len(seq):
        raise VcfPanic(where)
    return seq[i]


def lparse(line):
    """vcf.rs:12-68"""
    raw = line.split("\t")                                                        # :13
    chromosome = raw[0]                                                           # :15
    position = parse_u64(_index(raw, 1, "fields"))                                # :17
    if position is None:
        raise VcfPanic("pos")                                                     # :19, unwrapped by .expect at :287
    reference_allele = parse_char_or_d(_index(raw, 3, "fields"))                  # :22-25
    alternative_alleles = [parse_char_or_d(x) for x in _index(raw, 4, "fields").split(",")]  # :27-33
    idx = [i for i, x in enumerate(_index(raw, 8, "fields").split(":")) if x == "AD"]        # :37-42
    if len(idx) != 1:
        raise VcfPanic("ad_key")                                                  # :46
    idx = idx[0]
    allele_depths = []
    for i in range(9, len(raw)):                                                  # :49
        piece = _index(raw[i].split(":"), idx, "subfields")                       # :51
        row = []
        for x in piece.split(","):
            v = parse_u64(x)
            if v is None:
                raise VcfPanic("ad_value")                                        # :55 unwrap
            row.append(v)
        allele_depths.append(row)
    return {"chromosome": chromosome, "position": position, "reference_allele": reference_allele,
            "alternative_alleles": alternative_alleles, "allele_depths": allele_depths}


def to_counts(v):
    """vcf.rs:73-92"""
    alleles_vector = [v["reference_allele"]] + list(v["alternative_alleles"])
    ad = v["allele_depths"]
    n = len(ad)
    m = len(_index(ad, 0, "no_samples"))                                          # :79
    matrix = [[_index(ad[i], j, "ragged") for j in range(m)] for i in range(n)]   # :81-85
    return alleles_vector, matrix


def to_frequencies(v):
    """vcf.rs:95-112"""
    alleles_vector, matrix = to_counts(v)
    out = []
    for row in matrix:
        s = sum(row)                          # integers: exact
        out.append([(float(c) / float(s)) if s else float("nan") for c in row])   # 0 / 0 = NaN (c <= s)
    return alleles_vector, out


def breadth_threshold(min_coverage_breadth, n_sizes):
    """(x).ceil() as u32: Rust's saturating cast"""
    x = min_coverage_breadth * n_sizes
    if x != x:
        return 0
    t = math.ceil(x) if math.isfinite(x) else (0 if x < 0 else 1 << 32)
    return min(max(int(t), 0), (1 << 32) - 1)


def sequential_sum(xs):
    s = 0.0
    for x in xs:
        s += x
    return s


def _q(freqs, j, pool_sizes):
    q = 0.0
    total = sequential_sum(pool_sizes)
    for i in range(len(freqs)):
        q += freqs[i][j] * _index(pool_sizes, i, "pool_sizes") / total            # :153-154
    return q


def vcf_filter(v, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency, collapsed=False):
    """vcf.rs:117-178; True = Some(self), False = None.  collapsed=True replaces the `while j < m` loop by what it comes to:
    m >= 2 and column 1 passes."""
    thr = breadth_threshold(min_coverage_breadth, len(pool_sizes))                # :119
    pools_covered = 0
    for row in v["allele_depths"]:                                                # :121
        c = sum(row)
        if c >= min_coverage_depth:
            pools_covered += 1
        if pools_covered == thr:
            break
    if pools_covered != thr:                                                      # :130
        return False
    _, freqs = to_frequencies(v)                                                  # :136
    m = len(freqs[0])
    if collapsed:
        if m < 2:
            return False
        q = _q(freqs, 1, pool_sizes)
        return not ((q < min_allele_frequency) | (q > (1.00 - min_allele_frequency)))
    j = 1
    while j < m:                                                                  # :150
        q = _q(freqs, j, pool_sizes)
        if (q < min_allele_frequency) | (q > (1.00 - min_allele_frequency)):      # :157
            m -= 1
        else:
            j += 1
    return m >= 2                                                                 # :174


def vcf_to_sync(v, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency):
    """vcf.rs:182-230: (the sync line, the n x 6 matrix), or None"""
    if not vcf_filter(v, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency):
        return None
    alleles_vector, matrix = to_counts(v)
    n = len(matrix)
    atcgdn = [[0] * 6 for _ in range(n)]
    for i in range(n):
        for j, e in enumerate("ATCGDN"):
            for k in range(len(alleles_vector)):
                if alleles_vector[k] == e:
                    atcgdn[i][j] = _index(matrix[i], k, "oob")                    # :205
                    break
    x = [v["chromosome"], str(v["position"]), v["reference_allele"]] + [":".join(str(w) for w in row) for row in atcgdn]
    return "\t".join(x) + "\n", atcgdn


def text_lines(text):
    """(offset, line with its terminator) as BufRead::read_line gives them"""
    out, s = [], 0
    while s < len(text):
        e = text.find(b"\n", s)
        e = len(text) if e < 0 else e + 1
        out.append((s, text[s:e]))
        s = e
    return out


def strip_eol(raw):
    """vcf.rs:276-281"""
    if raw.endswith(b"\n"):
        raw = raw[:-1]
        if raw.endswith(b"\r"):
            raw = raw[:-1]
    return raw


def per_chunk(text, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency):
    """vcf.rs:268-300 over a whole text: [(offset, parsed line, sync line, matrix)] of the lines written"""
    out = []
    for off, raw in text_lines(text):
        line = strip_eol(raw).decode("latin-1")
        try:
            if len(line) == 0:
                raise VcfPanic("empty")                                           # :283
            if line[0] == "#":
                continue
            if len(line) < 20:
                raise VcfPanic("short")                                           # :291: the message is built before lparse runs
            v = lparse(line)
            r = vcf_to_sync(v, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency)
        except VcfPanic as e:
            raise VcfPanic(e.where, off) from None
        if r is not None:
            out.append((off, v, r[0], r[1]))
    return out


def vcf2sync_bytes(text, pool_sizes, min_coverage_depth=1, min_coverage_breadth=1.0, min_allele_frequency=0.001):
    """read_analyse_write (vcf.rs:306-425) without the files: the bytes of the sync file"""
    pool_names = []
    for _, raw in text_lines(text):
        line = raw.rstrip(b"\n")
        line = line[:-1] if line.endswith(b"\r") and raw.endswith(b"\n") else line   # BufRead::lines strips "\n" and "\r\n"
        if len(line) < 6:
            raise VcfPanic("header_scan")                                         # :346 slices every line
        if line[:6] == b"#CHROM":
            pool_names = line.split(b"\t")[9:]
    if not pool_names:
        raise VcfPanic("pool_names")                                              # :358, unwrapped in main.rs
    rows = per_chunk(text, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency)
    return b"#chr\tpos\tref\t" + b"\t".join(pool_names) + b"\n" + b"".join(r[2].encode("latin-1") for r in rows)


# ---- the library's contract -------------------------------------------------------------------------------------------------
_WHERE = {"no_samples": E_NO_SAMPLES, "ragged": E_AD_RAGGED, "oob": E_ALLELE_OOB}


def _line_codes(line, n_sizes):
    """the reasons that hold of a data line before its filter runs (an empty set: the line parses), and its sample count"""
    if len(line) == 0:
        return {E_EMPTY}, None
    if len(line) < 20:
        return {E_SHORT}, None
    raw = line.split("\t")
    if len(raw) < 9:
        return {E_FIELDS}, None
    n = len(raw) - 9
    codes = set()
    if parse_u64(raw[1]) is None:
        codes.add(E_POS)
    if any(ord(ch) >= 0x80 for ch in raw[3] + raw[4]):
        codes.add(E_HIGH_BYTE)
    keys = raw[8].split(":")
    if keys.count("AD") != 1:
        codes.add(E_AD_KEY)
    if n > n_sizes:
        codes.add(E_POOLS)
    if E_AD_KEY in codes or n > n_sizes:
        return codes, n
    idx = keys.index("AD")
    for f in raw[9:]:
        pieces = f.split(":")
        if idx >= len(pieces):
            codes.add(E_SUBFIELDS)
            continue
        for x in pieces[idx].split(","):
            v = parse_u64(x)
            if v is None:
                codes.add(E_AD_VALUE)
            elif v > 0xFFFFFFFF:
                codes.add(E_COUNT32)
    return codes, n


def parse_ref(text, pool_sizes, min_coverage_depth=1, min_coverage_breadth=1.0, min_allele_frequency=0.001):
    """What pg_host_vcf_parse returns for `text`, from the literal restatement; raises VcfPanic(offset, reason) where it fails."""
    pool_sizes = [float(x) for x in pool_sizes]
    kept, data_lines, chrom_off, first_n = [], 0, -1, None
    for off, raw in text_lines(text):
        line = strip_eol(raw).decode("latin-1")
        if line[:1] == "#":
            if line[:6] == "#CHROM":
                chrom_off = off
            continue
        codes, n = _line_codes(line, len(pool_sizes))
        data_lines += 1 if line else 0
        if n is not None:
            if first_n is None:
                first_n = n
            elif n != first_n:
                codes.add(E_POOLS)
        where = "parse"
        if not codes:   # the reference's own verdict decides between kept, dropped and the three late panics
            try:
                v = lparse(line)
                r = vcf_to_sync(v, pool_sizes, min_coverage_depth, min_coverage_breadth, min_allele_frequency)
            except VcfPanic as e:
                where = e.where
                codes.add(_WHERE[where])
        if codes:
            raise VcfPanic(where, off, min(codes))
        if r is not None:
            kept.append((off, v, r[1]))
    n = first_n or 0
    return {"counts": np.array([k[2] for k in kept], dtype=np.uint32).reshape(len(kept), n, 6),
            "pos": np.array([k[1]["position"] for k in kept], dtype=np.uint64),
            "ref": np.frombuffer("".join(k[1]["reference_allele"] for k in kept).encode("latin-1"), dtype=np.uint8),
            "line_off": np.array([k[0] for k in kept], dtype=np.int64),
            "chrom_len": np.array([len(k[1]["chromosome"]) for k in kept], dtype=np.int32),
            "data_lines": data_lines, "n_pools": n, "chrom_line_off": chrom_off}


def literal_panics(text, pool_sizes, min_coverage_depth=1, min_coverage_breadth=1.0, min_allele_frequency=0.001):
    """the offset of the line at which the literal per_chunk panics, or None"""
    try:
        per_chunk(text, [float(x) for x in pool_sizes], min_coverage_depth, min_coverage_breadth, min_allele_frequency)
    except VcfPanic as e:
        return e.offset
    return None
