"""A literal Python restatement of the two row kinds of the popgen writer over tests/rustfmt.py (through tests/f64_corpus.py,
which mends rustfmt's one wrong product): the table of pg_f64_table_dev / pg_host_f64_table and the rows of pg_gudmc_rows_dev /
pg_host_gudmc_rows.  Test infrastructure: plain loops, no NumPy arithmetic on the values."""
import numpy as np

import f64_corpus as FC
import rustfmt

LABEL_MAX = 1 << 22


def cell(x: float, nd: int) -> str:
    return rustfmt.display(x) if nd < 0 else FC.roundup_own(x, nd)


def table(x, labels=None, n_digits=-1, first_col_digits=None, row0=0, n_rows=None) -> bytes:
    """rows [row0, row0 + n_rows) of the 2-D array x (any view): label_r as given, the cells joined by ',', '\\n'"""
    x = np.asarray(x, dtype=np.float64)
    rows, cols = x.shape
    nd0 = n_digits if first_col_digits is None else first_col_digits
    n_rows = rows - row0 if n_rows is None else n_rows
    out = []
    for r in range(row0, row0 + n_rows):
        lab = b"" if labels is None else (labels[r] if isinstance(labels[r], bytes) else str(labels[r]).encode())
        vals = x[r].tolist()
        out.append(lab + ",".join(cell(v, nd0 if c == 0 else n_digits) for c, v in enumerate(vals)).encode() + b"\n")
    return b"".join(out)


def gudmc_rows(res, win_chr, win_ini, win_fin, pool_names, chrom_names, row0=0, rows=None) -> bytes:
    """gudmc's rows (gudmc.rs:433-455) from pg_gudmc_dev's outputs as arrays: res[key] per population, per pair, or per
    (pair, row) with pitch w; chrom_names by chromosome id.  Rows [row0, row0 + rows) of the file."""
    n = len(pool_names)
    r7 = lambda v: FC.roundup_own(float(v), 7)
    D = lambda v: rustfmt.display(float(v))
    per = {k: np.asarray(res[k]).reshape(n * n, -1) for k in ("window", "d", "width", "width_dev", "width_p", "fst_delta", "fst_p")}
    lines = []
    for i in range(n * n):
        a, b = divmod(i, n)
        for j in range(int(res["rows"][b])):
            w = int(per["window"][i][j])
            lines.append(",".join([pool_names[a], pool_names[b], chrom_names[int(win_chr[w])], str(int(win_ini[w])), str(int(win_fin[w])),
                                   r7(res["d_mean"][b]), r7(res["fst_mean"][i]), r7(res["d_sd"][b]), r7(res["fst_sd"][i]),
                                   D(per["d"][i][j]), D(per["width"][i][j]), D(per["width_dev"][i][j]), r7(per["width_p"][i][j]),
                                   r7(per["fst_delta"][i][j]), r7(per["fst_p"][i][j])]) + "\n")
    rows = len(lines) - row0 if rows is None else rows
    return "".join(lines[row0:row0 + rows]).encode()


def padded(res, n, w):
    """the lists per pair of gudmc_ref.gudmc_stage as pg_gudmc_dev's arrays: pitch w, the unspecified tail zero"""
    out = {k: np.asarray(res[k], dtype=np.int64 if k == "rows" else np.float64) for k in ("rows", "d_mean", "d_sd", "fst_mean", "fst_sd")}
    for k in ("window", "d", "width", "width_dev", "width_p", "fst_delta", "fst_p"):
        a = np.zeros((n * n, w), dtype=np.int64 if k == "window" else np.float64)
        for i in range(n * n):
            a[i, :len(res[k][i])] = res[k][i]
        out[k] = a
    return out
