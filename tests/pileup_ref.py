"""A literal Python restatement of what pileup2sync makes of mpileup text (base/pileup.rs: String::lparse :11-168 with its
per-byte indel marker, PileupLine::filter :240-334, to_counts :172-215), under the library's stated limits (a number is an
optional '+' and 1-19 digits, the reference allele one byte below 0x80, a byte >= 0x80 is no digit).  Slow and plain: the
yardstick of pg_host_pileup_parse and pg_pileup_parse_dev, itself checked line by line against the oracle
(tests/test_pileup_ref.py).

A pool names the FIRST defect its own walk meets, a line the SMALLEST code among its first three fields' and its pools'."""
import math

import numpy as np

LONG, FIELDS, POS, REF, COV, RAGGED, INDEL, MISMATCH = 1, 2, 3, 4, 5, 6, 7, 8
LEFT_MAX = 4294967295
DEFAULTS = dict(remove_ns=True, keep_lowercase_reference=False, max_base_error_rate=0.01, min_coverage_depth=1,
                min_coverage_breadth=1.0, min_allele_frequency=0.001)


def text_lines(text):
    """(offset, line without its newline and without one trailing '\\r') of every line; the last may lack the newline"""
    out, s = [], 0
    while s < len(text):
        e = text.find(b"\n", s)
        e = len(text) if e < 0 else e
        line = text[s:e]
        if line.endswith(b"\r"):
            line = line[:-1]
        out.append((s, line))
        s = e + 1
    return out


def number(b):
    if b[:1] == b"+":
        b = b[1:]
    if not 1 <= len(b) <= 19 or any(not 48 <= c <= 57 for c in b):
        return None
    return int(b)


def digit(code):
    return code - 48 if 48 <= code <= 57 else None


def read_alleles(reads, ref):
    """lparse's loop over one pool's read codes (:43-129): the allele bytes, or INDEL"""
    alleles = []
    indel, count, left = False, 0, LEFT_MAX
    for code in reads:
        if indel:
            if count == 0 and left == LEFT_MAX:          # the first digit of the length; zeros leave the state as it is
                d = digit(code)
                if d is None:
                    return INDEL
                count = d
                continue
            if count > 0 and left == LEFT_MAX:           # further digits; the first non-digit is the first byte dropped
                d = digit(code)
                if d is not None:
                    count = (count * 10 + d) & 0xFFFFFFFFFFFFFFFF
                else:
                    left = count - 1
                continue
            if left > 0:
                left -= 1
                continue
            indel, count, left = False, 0, LEFT_MAX      # and the byte is looked at as any other
        if code in (43, 45):
            indel, count = True, 0
            continue
        if code in (94, 36):
            if code == 94:
                indel, count, left = True, 1, 1          # the mapping quality behind '^' is dropped
            continue
        if code in (44, 46):
            alleles.append(ref)
        else:
            alleles.append({65: 65, 97: 65, 84: 84, 116: 84, 67: 67, 99: 67, 71: 71, 103: 71, 42: 68}.get(code, 78))
    return alleles


def lparse(line):
    """-> (reason, None) or (0, (chrom_len, pos, ref, coverages, read_codes, read_qualities))"""
    f = line.split(b"\t")
    if len(f) < 3:
        return FIELDS, None
    err = []
    pos = number(f[1])
    if pos is None:
        err.append(POS)
    if len(f[2]) != 1 or f[2][0] >= 0x80:
        err.append(REF)
    ref = f[2][0] if REF not in err else 0
    coverages, codes, quals = [], [], []
    for i in range(3, len(f), 3):
        cov = number(f[i])
        if cov is None:
            err.append(COV)
        elif i + 2 >= len(f):
            err.append(RAGGED)
        elif cov > 0:
            a = read_alleles(f[i + 1], ref)
            if a == INDEL:
                err.append(INDEL)
            elif len(a) != cov or len(f[i + 2]) != cov:
                err.append(MISMATCH)
            else:
                coverages.append(cov); codes.append(a); quals.append(list(f[i + 2]))
                continue
        coverages.append(0); codes.append([]); quals.append([])
    if err:
        return min(err), None
    return 0, (len(f[0]), pos, ref, coverages, codes, quals)


def as_u32(x):
    """Rust's `as u32` of an f64"""
    if not x > 0.0:
        return 0
    return 4294967295 if x >= 4294967295.0 else int(x)


def filter_counts(parsed, sizes, remove_ns, keep_lowercase_reference, max_base_error_rate, min_coverage_depth, min_coverage_breadth,
                  min_allele_frequency):
    """filter + to_counts: the n x 6 counts of a kept line, or None"""
    _, _, _, coverages, codes, quals = parsed
    coverages, codes, quals = list(coverages), [list(c) for c in codes], [list(q) for q in quals]
    if len(coverages) != len(sizes):
        return None
    for i in range(len(quals)):
        j = 0
        while j < len(codes[i]):
            if quals[i][j] < 33:
                return None
            if 10.0 ** (-(float(quals[i][j]) - 33.0) / 10.0) > max_base_error_rate:
                codes[i][j] = 78
            if remove_ns and codes[i][j] == 78:
                del codes[i][j]; del quals[i][j]
                coverages[i] -= 1
            else:
                j += 1
    need = as_u32(math.ceil(min_coverage_breadth * float(len(sizes)))) if not math.isnan(min_coverage_breadth) else 0
    covered = [c for c in coverages if c >= min_coverage_depth][:need]
    if len(covered) != need:
        return None
    if keep_lowercase_reference:
        remap = {65: 65, 97: 65, 84: 84, 116: 84, 67: 67, 99: 67, 71: 71, 103: 71, 42: 68}
        codes = [[remap.get(c, 78) for c in pool] for pool in codes]
    col = {65: 0, 84: 1, 67: 2, 71: 3, 68: 4}
    counts = np.zeros((len(codes), 6), dtype=np.uint32)
    for i, pool in enumerate(codes):
        for c in pool:
            counts[i, col.get(c, 5)] += 1
    n, m, j = len(codes), 6, 1
    while j < m:
        q = 0.0
        for i in range(n):
            s = int(counts[i].sum())
            freq = float(counts[i, j]) / float(s) if s else float("nan")
            q += freq * sizes[i]
        if (q < min_allele_frequency) or (q > (1.00 - min_allele_frequency)):
            m -= 1
        else:
            j += 1
    if m < 2:
        return None
    return counts


def line_ref(line, sizes, **rule):
    """("E", reason) | ("D",) | ("K", chrom_len, pos, ref, counts)"""
    rule = {**DEFAULTS, **rule}
    if len(line) >= 2 ** 31:
        return ("E", LONG)
    reason, parsed = lparse(line)
    if reason:
        return ("E", reason)
    counts = filter_counts(parsed, [float(x) for x in sizes], **rule)
    if counts is None:
        return ("D",)
    return ("K", parsed[0], parsed[1], parsed[2], counts)


def sync_line(line, row):
    """the text pileup_to_sync writes for a kept line"""
    _, clen, pos, ref, counts = row
    return line[:clen] + b"\t%d\t" % pos + bytes([ref]) + b"".join(b"\t" + b":".join(b"%d" % v for v in pool) for pool in counts.tolist())


def parse_ref(text, sizes, **rule):
    """What Engine.pileup_parse / pileup_parse_host return for `text`; with a line the reference panics at, only
    {"error": (offset of the first such line, reason), "lines": ..}"""
    n = len(sizes)
    rows, offs = [], []
    lines = text_lines(text)
    for off, line in lines:
        r = line_ref(line, sizes, **rule)
        if r[0] == "E":
            return {"error": (off, r[1]), "lines": len(lines)}
        if r[0] == "K":
            rows.append(r); offs.append(off)
    k = len(rows)
    return {"error": None, "lines": len(lines), "n_pools": n,
            "counts": np.array([r[4] for r in rows], dtype=np.uint32).reshape(k, n, 6),
            "pos": np.array([r[2] for r in rows], dtype=np.uint64), "ref": np.array([r[3] for r in rows], dtype=np.uint8),
            "line_off": np.array(offs, dtype=np.int64), "chrom_len": np.array([r[1] for r in rows], dtype=np.int32)}
