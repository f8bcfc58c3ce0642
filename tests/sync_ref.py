"""The sync reader's rules (include/poolgen_hip.h), restated literally in Python with regular expressions:
the yardstick of pg_host_sync_parse and pg_sync_parse_dev.  The rules are those of the CLI's parse_range / parse_sync_buffer
(host/host_util.cpp), which `hostcheck parse` prints: test_sync_ref.py holds this restatement against that program too.
Where parse_sync_buffer throws this raises SyncPanic(offset, reason): the first such line in file order, and of that line the
smallest reason."""
import re

import numpy as np

E_EMPTY, E_FIELDS, E_COUNT, E_COUNT32, E_POOLS, E_LONG = 1, 2, 3, 4, 5, 6
MAX_POOLS = 4096
NUMBER = rb"\+?[0-9]{1,19}"
POSITION = re.compile(NUMBER + rb"\Z")
POOL = re.compile(NUMBER + rb"(?::" + NUMBER + rb"){5,}\Z")


class SyncPanic(Exception):
    def __init__(self, offset, reason):
        super().__init__(f"line at byte {offset}: reason {reason}")
        self.offset, self.reason = offset, reason


def text_lines(text):
    """(offset, line) of every line: split at '\\n', one trailing '\\r' dropped; a last line may lack the newline"""
    out, s = [], 0
    while s < len(text):
        e = text.find(b"\n", s)
        if e < 0:
            e = len(text)
        line = text[s:e]
        out.append((s, line[:-1] if line.endswith(b"\r") else line))
        s = e + 1
    return out


def pool_reason(field):
    """0, or why this pool's field fails; the smallest reason"""
    if not POOL.match(field):
        return E_COUNT
    if any(int(x) > 0xFFFFFFFF for x in field.split(b":")[:6]):
        return E_COUNT32
    return 0


def parse_ref(text, expect_n=0):
    lines = text_lines(text)
    errors = []          # (offset, reason)
    first = next(((o, l) for o, l in lines if not l.startswith(b"#")), None)
    n = 0
    if first is not None:
        o, l = first
        tabs = l.count(b"\t")
        if tabs < 3:
            errors.append((o, E_FIELDS))
        else:
            n = tabs - 2
            if n > MAX_POOLS or (expect_n > 0 and n != expect_n):
                errors.append((o, E_POOLS))
    n_ref = expect_n if expect_n > 0 else max(1, min(n, MAX_POOLS))
    counts, pos, off, clen = [], [], [], []
    data_lines = 0
    for o, l in lines:
        if len(l) == 0:
            errors.append((o, E_EMPTY))
            break
        if l.startswith(b"#"):
            continue
        data_lines += 1
        f = l.split(b"\t")
        if len(f) < 3:
            errors.append((o, E_FIELDS))
            break
        if not POSITION.match(f[1]):
            continue                                  # skipped: the position is no number and there is a second tab
        if len(f) < 4:
            errors.append((o, E_FIELDS))
            break
        pools = f[3:]
        reasons = [E_POOLS] if len(pools) != n_ref else []
        reasons += [r for r in (pool_reason(p) for p in pools[:n_ref]) if r]
        if reasons:
            errors.append((o, min(reasons)))
            break
        counts.append([[int(x) for x in p.split(b":")[:6]] for p in pools])
        pos.append(int(f[1]))
        off.append(o)
        clen.append(len(f[0]))
    if errors:
        raise SyncPanic(*min(errors))
    k = len(pos)
    return {"counts": np.array(counts, dtype=np.uint32).reshape(k, n, 6), "pos": np.array(pos, dtype=np.uint64),
            "line_off": np.array(off, dtype=np.int64), "chrom_len": np.array(clen, dtype=np.int32), "data_lines": data_lines, "n_pools": n}


def hostcheck_form(text, r):
    """the result as `hostcheck parse` prints it"""
    k, n = len(r["pos"]), r["n_pools"]
    if n == 0:
        return "0 0\n"
    out = [f"{k} {n}"]
    for i in range(k):
        o = int(r["line_off"][i])
        chrom = text[o:o + int(r["chrom_len"][i])].decode("latin-1")
        out.append(" ".join([chrom, str(int(r["pos"][i]))] + [str(int(x)) for x in r["counts"][i].reshape(-1)]))
    return "\n".join(out) + "\n"
